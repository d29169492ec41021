"""Intra-frame inconsistency: regions and frames scored by how much the augmented views of ONE frame disagreed.

Scoring a frame runs the network on `inf_reps` augmented views of it; lidal_view_scores (csrc/score.hip, DESIGN.md
section 17) keeps, beside their mean, the divergence of the mean from every view, the entropy of the mean and the number
of views that vote for the predicted class.  It is the reference's score/sv_level/LiDAL.py:59-81 with the frame's own
fused prediction where the query frame stands and its views where the matched neighbour frames stand -- no poses, no
registration, no neighbour window, no exchange between ranks.

  score_frame_views    per-supervoxel means of one frame (lidal_supervoxel_reduce): score_frame's tuple
  frame_view_scores    the frame-level VIEWD / VIEWE / VOTE of frame_level.METRICS
  view_sequence        infer + score every frame of a list: score_sequence's output, so collect_sequence, ScoreBoard and
                       select / select_indexed take it as it is

Unposed or unordered scans: pass the sensor-frame points (as f64) for `world` and give every frame its OWN seq_index in
ScoreBoard.add_sequence -- the board offsets the centres by seq_index * 1000, so the 5 m rule of the selection
(LiDAL.py:230,252-254) then acts inside a frame only.  Posed sequences: register with lidal_amd.data.register_scan and
keep the sequence's index, as for score_sequence.
"""
import torch

from .. import backend as B

__all__ = ['score_frame_views', 'frame_view_scores', 'view_sequence']


def score_frame_views(viewd, viewe, points_f64, sv_ptr, sv_idx):
    """Per-supervoxel means of view_scores' viewd f64 [P], viewe f32 [P] and the points f64 [P, 3] over the CSR
    (sv_ptr, sv_idx) of interframe.sv_csr: (sv_viewds f32 [S], sv_viewes f32 [S], sv_centers f32 [S, 3])."""
    B.require_gpu(viewd, viewe, points_f64, sv_ptr, sv_idx)
    assert viewd.dtype == torch.float64 and viewe.dtype == torch.float32
    assert points_f64.dtype == torch.float64 and points_f64.shape == (viewd.shape[0], 3)
    assert sv_ptr.dtype == torch.int64 and sv_idx.dtype == torch.int64
    viewd, viewe, points_f64 = viewd.contiguous(), viewe.contiguous(), points_f64.contiguous()
    sv_ptr, sv_idx = sv_ptr.contiguous(), sv_idx.contiguous()
    s = sv_ptr.numel() - 1
    dev = viewd.device
    sv_d = torch.empty(s, dtype=torch.float32, device=dev)
    sv_e = torch.empty(s, dtype=torch.float32, device=dev)
    sv_c = torch.empty((s, 3), dtype=torch.float32, device=dev)
    B.check(B.lib().lidal_supervoxel_reduce(B.ptr(viewd), B.ptr(viewe), B.ptr(points_f64), B.ptr(sv_ptr),
                                            B.ptr(sv_idx), s, B.ptr(sv_d), B.ptr(sv_e), B.ptr(sv_c), B.stream()),
            'supervoxel_reduce')
    return sv_d, sv_e, sv_c


def frame_view_scores(viewd, viewe, agree, reps):
    """(VIEWD, VIEWE, VOTE) of one frame: mean(viewd), mean(viewe) and 1 - mean(agree) / reps, the means in f64, as
    f32 0-d device tensors.  Larger = the views disagreed more."""
    B.require_gpu(viewd, viewe, agree)
    vote = 1.0 - agree.double().mean() / float(reps)
    return viewd.double().mean().float(), viewe.double().mean().float(), vote.float()


def view_sequence(model, frames, inf_reps=8, autocast=False, prefetch=True):
    """frames: score_sequence's dicts (coords, feats, inverse, world f64 [P, 3], sv_ptr, sv_idx), any frames in any
    order: they are scored independently, so a rank passes its frame_range slice and nothing is exchanged.  Returns
    score_sequence's list, one (sv_viewds f32 [S], sv_viewes f32 [S], sv_centers f32 [S, 3]) per frame.
    prefetch: each frame's coordinate tables are built one frame ahead on a second stream (same bytes)."""
    from .pipeline import _Inference
    by_id = dict(enumerate(frames))
    infer = _Inference(model, by_id, list(by_id), inf_reps, autocast, prefetch, view_scores=True)
    out = []
    for f, d in by_id.items():
        viewd, viewe, _ = infer(f)
        out.append(score_frame_views(viewd, viewe, d['world'], d['sv_ptr'], d['sv_idx']))
    return out
