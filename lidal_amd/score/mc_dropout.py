"""MC-dropout: regions and frames scored by how much the predictions of ONE view change with the dropout mask -- the
baseline LiDAL and ReDAL both compare themselves against (Gal & Ghahramani 2016; BALD: Houlsby et al. 2011).

Scoring a frame runs the network in eval mode with its counter dropout kept on (nn.mc_dropout) over `passes` collated
copies of the frame (data.mc_sample: one augmentation repeated, so the copies differ by their masks alone -- an
element's mask depends on its index in the batch); lidal_mc_scores (csrc/score.hip) keeps, beside
the mean prediction, the mutual information between the prediction and the mask (BALD), the mean entropy of the passes
and the number of passes that vote for the predicted class.

  frame_mc_scores    the frame-level BALD / MCENT of frame_level.METRICS and the variation ratio (VOTE's formula)
  mc_sequence        infer + score every frame of a list: score_sequence's output, so collect_sequence, ScoreBoard and
                     select / select_indexed take it as it is

Needs a model with lidal_amd.nn.Dropout (SPVCNN(dropout_seed=...), nn.use_counter_dropout): ValueError otherwise,
MinkUNet included.  What the selection gains from these scores is not measured here.
"""
from .. import backend as B
from .view_level import score_frame_views

__all__ = ['frame_mc_scores', 'mc_sequence']


def frame_mc_scores(bald, ment, agree, reps):
    """(BALD, MCENT, VOTE) of one frame: mean(bald), mean(ment) and the variation ratio 1 - mean(agree) / reps, the
    means in f64, as f32 0-d device tensors.  Larger = the passes disagreed more."""
    B.require_gpu(bald, ment, agree)
    vote = 1.0 - agree.double().mean() / float(reps)
    return bald.double().mean().float(), ment.double().mean().float(), vote.float()


def mc_sequence(model, frames, passes=8, autocast=False, prefetch=True):
    """frames: score_sequence's dicts (coords, feats, inverse of data.mc_sample's batch, world f64 [P, 3], sv_ptr,
    sv_idx), any frames in any order, scored independently.  The model is put under nn.mc_dropout for the pass (its mode
    is the caller's: model.eval()).  Returns score_sequence's list, one (sv_balds f32 [S], sv_ments f32 [S], sv_centers
    f32 [S, 3]) per frame: the per-supervoxel means of the mutual information and of the passes' mean entropy."""
    from ..nn import mc_dropout
    from .pipeline import _Inference
    by_id = dict(enumerate(frames))
    out = []
    with mc_dropout(model):
        infer = _Inference(model, by_id, list(by_id), passes, autocast, prefetch, mc_scores=True)
        for f, d in by_id.items():
            bald, ment, _ = infer(f)
            out.append(score_frame_views(bald, ment, d['world'], d['sv_ptr'], d['sv_idx']))
    return out
