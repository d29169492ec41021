"""One step of /root/reference/score/prob_inference.py:91-113 kept on the GPU.

The reference copies the logits of the 8 collated views to the host (61 MB per frame), gathers
voxel -> point with the inverse indices, soft-maxes, averages the views and arg-maxes in numpy.
Here the model forward and one fused kernel (lidal_view_mean_softmax) do all of it in HBM; only
what the scorer needs next ([P, C] probabilities) stays resident.
"""
import torch

from .. import SparseTensor
from .. import backend as B

__all__ = ['infer_frame', 'view_mean_softmax', 'view_scores', 'mc_scores']


def view_mean_softmax(logits, inverse_indices, inf_reps):
    """logits f32 [sum_v N_v, C]; inverse_indices i64 [inf_reps * P] (collated, offset per view as
    dataset/sk_dataset.py:214-217) -> (prob f32 [P, C], pred i64 [P])."""
    B.require_gpu(logits, inverse_indices)
    logits = logits.contiguous().float()
    inverse_indices = inverse_indices.contiguous()
    assert inverse_indices.dtype == torch.int64
    assert inverse_indices.numel() % inf_reps == 0
    p = inverse_indices.numel() // inf_reps
    c = logits.shape[1]
    prob = torch.empty((p, c), dtype=torch.float32, device=logits.device)
    pred = torch.empty(p, dtype=torch.int64, device=logits.device)
    B.check(B.lib().lidal_view_mean_softmax(B.ptr(logits), B.ptr(inverse_indices), inf_reps, p, c,
                                            B.ptr(prob), B.ptr(pred), B.stream()),
            'view_mean_softmax')
    return prob, pred


def view_scores(logits, inverse_indices, inf_reps):
    """view_mean_softmax plus the disagreement of the views about every point (lidal_view_scores, DESIGN.md section
    17), one launch: (prob f32 [P, C], pred i64 [P] -- view_mean_softmax's bytes --, viewd f64 [P] the mean KL divergence
    of the view mean from each view, viewe f32 [P] the entropy of the view mean, agree i32 [P] the views whose own
    arg-max is pred)."""
    B.require_gpu(logits, inverse_indices)
    logits = logits.contiguous().float()
    inverse_indices = inverse_indices.contiguous()
    assert inverse_indices.dtype == torch.int64
    assert inverse_indices.numel() % inf_reps == 0
    p = inverse_indices.numel() // inf_reps
    c = logits.shape[1]
    dev = logits.device
    prob = torch.empty((p, c), dtype=torch.float32, device=dev)
    pred = torch.empty(p, dtype=torch.int64, device=dev)
    viewd = torch.empty(p, dtype=torch.float64, device=dev)
    viewe = torch.empty(p, dtype=torch.float32, device=dev)
    agree = torch.empty(p, dtype=torch.int32, device=dev)
    B.check(B.lib().lidal_view_scores(B.ptr(logits), B.ptr(inverse_indices), inf_reps, p, c, B.ptr(prob), B.ptr(pred),
                                      B.ptr(viewd), B.ptr(viewe), B.ptr(agree), B.stream()), 'view_scores')
    return prob, pred, viewd, viewe, agree


def mc_scores(logits, inverse_indices, reps):
    """view_mean_softmax plus the MC-dropout scores of every point (lidal_mc_scores), one launch:
    the `reps` rows of a point are the passes of one view under different dropout masks.  (prob f32 [P, C], pred i64 [P]
    -- view_mean_softmax's bytes --, bald f64 [P] the mutual information H(mean) - mean_v H(p_v), ment f32 [P] the mean
    entropy of the passes, agree i32 [P] the passes whose own arg-max is pred.)  No points: nothing is launched."""
    B.require_gpu(logits, inverse_indices)
    logits = logits.contiguous().float()
    inverse_indices = inverse_indices.contiguous()
    assert inverse_indices.dtype == torch.int64
    assert inverse_indices.numel() % reps == 0
    p = inverse_indices.numel() // reps
    c = logits.shape[1]
    dev = logits.device
    prob = torch.empty((p, c), dtype=torch.float32, device=dev)
    pred = torch.empty(p, dtype=torch.int64, device=dev)
    bald = torch.empty(p, dtype=torch.float64, device=dev)
    ment = torch.empty(p, dtype=torch.float32, device=dev)
    agree = torch.empty(p, dtype=torch.int32, device=dev)
    B.check(B.lib().lidal_mc_scores(B.ptr(logits), B.ptr(inverse_indices), reps, p, c, B.ptr(prob), B.ptr(pred),
                                    B.ptr(bald), B.ptr(ment), B.ptr(agree), B.stream()), 'mc_scores')
    return prob, pred, bald, ment, agree


@torch.no_grad()
def infer_frame(model, coords_v_b, feats_v_b, inverse_indices_b, inf_reps=8, autocast=False, return_feat=False,
                geometry=None, return_view_scores=False, return_mc_scores=False):
    """model.eval() forward over the `inf_reps` augmented views of ONE frame, then the fused
    voxel->point gather + softmax + view mean + argmax.  Returns (prob [P,C], pred [P]).
    return_feat (prob_inference.py:103-105,116-118: `outfeat`, saved when r_id == 0 or the metric is
    ReDAL / CSET): also the [P, 96] feature of every point, the view mean of feat[inverse_indices] as the
    reference computes it -- (prob, pred, feat).
    return_view_scores: the triple (viewd, viewe, agree) of view_scores is appended to the result (after feat);
    lidal_view_scores then stands in lidal_view_mean_softmax's place, prob and pred are the same bytes.
    return_mc_scores: the triple (bald, ment, agree) of mc_scores is appended (after the view scores), same prob and pred;
    the caller puts the model under nn.mc_dropout -- without it the passes are identical and bald is 0."""
    x = SparseTensor(feats_v_b, coords_v_b)
    if geometry is not None:        # the frame's coordinate tables, built ahead (lidal_amd.network.GeometryPrefetcher)
        x.geometry = geometry
    with torch.autocast('cuda', dtype=torch.bfloat16, enabled=autocast):
        logits, feat = model(x)
    if return_view_scores:
        prob, pred, *views = view_scores(logits, inverse_indices_b, inf_reps)
        views = (tuple(views),)
    elif not return_mc_scores:
        prob, pred = view_mean_softmax(logits, inverse_indices_b, inf_reps)
        views = ()
    else:
        views = ()
    if return_mc_scores:
        prob, pred, *mc = mc_scores(logits, inverse_indices_b, inf_reps)
        views += (tuple(mc),)
    if not return_feat:
        return (prob, pred) + views
    p = inverse_indices_b.numel() // inf_reps
    feat_p = feat.float()[inverse_indices_b].reshape(inf_reps, p, feat.shape[1]).mean(0)
    return (prob, pred, feat_p) + views
