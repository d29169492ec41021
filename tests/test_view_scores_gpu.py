"""lidal_view_scores (csrc/score.hip) and what stands on it: the per-point disagreement of a
frame's augmented views against the f64 restatement tests/view_ref.py, prob / pred against lidal_view_mean_softmax byte
for byte, the supervoxel and frame means, and infer_frame / view_sequence / frame_sequence end to end.

The bar of viewd and viewe is the one the inter-frame point scores are held to (tests/test_scoring_gpu.py): 1e-4 of the
largest reference value of the case.  agree is an exact integer quantity of the logits and of the GPU's own pred."""
import functools
import math

import numpy as np
import pytest
import torch

import view_ref as V

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def edge_inputs(reps, c, p):
    """The input recipe of test_scoring_edges_gpu.py::test_view_mean_softmax_edges: rows of magnitude 1 / 3 / 30 clipped
    to +-80, all-zero rows, one class at -inf, and (c >= 16) points whose classes 3 and 11 tie for the maximum in every
    view.  (logits f32 [reps * nv, c], inverse i64 [reps * p], tied bool [p])"""
    rs = np.random.RandomState(1000 * reps + 10 * c + p % 10)
    nv = max(2, p // 2)
    logits = (rs.standard_normal((reps * nv, c)) * rs.choice([1.0, 3.0, 30.0], size=(reps * nv, 1))).astype(np.float32)
    logits = np.clip(logits, -80, 80)
    logits[rs.random_sample(reps * nv) < 0.1] *= 0
    if c > 1:
        logits[::7, rs.randint(0, c)] = 80.0
        logits[3::7, rs.randint(0, c)] = -80.0
        logits[:, c // 2][rs.random_sample(reps * nv) < 0.3] = -np.inf
    inverse = np.concatenate([rs.randint(0, nv, size=p) + v * nv for v in range(reps)]).astype(np.int64)
    tied = np.zeros(p, bool)
    if c >= 16:
        tied[::5] = True
        for v in range(reps):
            rows = np.unique(inverse[v * p:(v + 1) * p][tied])
            logits[rows, 3] = logits[rows, 11] = np.float32(81.0)
        tied = np.array([all(logits[inverse[v * p + k], 3] == 81.0 for v in range(reps)) for k in range(p)])
    return logits, inverse, tied


def _run(logits, inverse, reps):
    from lidal_amd.score.prob_inference import view_scores
    out = view_scores(_t(logits), _t(inverse), reps)
    torch.cuda.synchronize()
    return out


def _check_against_definition(out, logits, inverse, reps, what):
    """The bars of the point scores, and agree against the reference's per-view classes and the GPU's own pred."""
    prob, pred, viewd, viewe, agree = (t.cpu().numpy() for t in out)
    ref = V.scores_from_logits(logits, inverse, reps)
    assert viewd.dtype == np.float64 and viewe.dtype == np.float32 and agree.dtype == np.int32
    assert np.isfinite(prob).all() and np.isfinite(viewd).all() and np.isfinite(viewe).all()
    assert np.isfinite(ref['viewd']).all() and np.isfinite(ref['viewe']).all()
    err_d, bar_d = np.abs(viewd - ref['viewd']).max(), 1e-4 * np.abs(ref['viewd']).max()
    err_e, bar_e = np.abs(viewe - ref['viewe']).max(), 1e-4 * np.abs(ref['viewe']).max()
    print('%s: viewd error %.3e (bar %.3e)  viewe error %.3e (bar %.3e)' % (what, err_d, bar_d, err_e, bar_e))
    assert err_d <= bar_d
    assert err_e <= bar_e
    assert np.array_equal(agree, (ref['view_arg'] == pred[None, :]).sum(axis=0))
    assert agree.min() >= 0 and agree.max() <= reps
    return ref


@pytest.mark.parametrize('p', [1, 255, 257])
@pytest.mark.parametrize('c', [1, 16, 19, 32])
@pytest.mark.parametrize('reps', [1, 2, 8])
def test_prob_and_pred_are_the_view_mean_kernels_bytes(reps, c, p):
    from lidal_amd.score.prob_inference import view_mean_softmax
    logits, inverse, _ = edge_inputs(reps, c, p)
    out = _run(logits, inverse, reps)
    prob, pred = view_mean_softmax(_t(logits), _t(inverse), reps)
    assert out[0].shape == (p, c) and torch.equal(out[0], prob) and torch.equal(out[1], pred)


@pytest.mark.parametrize('p', [1, 255, 257])
@pytest.mark.parametrize('c', [1, 16, 19, 32])
@pytest.mark.parametrize('reps', [1, 2, 8])
def test_view_scores_edges(reps, c, p):
    logits, inverse, tied = edge_inputs(reps, c, p)
    out = _run(logits, inverse, reps)
    _check_against_definition(out, logits, inverse, reps, 'reps %d c %d p %d' % (reps, c, p))
    pred, agree = out[1].cpu().numpy(), out[4].cpu().numpy()
    if c >= 16:
        assert tied.any()
    assert np.all(pred[tied] == 3) and np.all(agree[tied] == reps)


@pytest.mark.parametrize('p', [1, 255, 257])
@pytest.mark.parametrize('c', [1, 16, 19, 32])
def test_one_view_and_a_repeated_view_give_exactly_zero(c, p):
    """reps 1: m is p_0.  reps 2 with inverse[P:] = inverse[:P] (no per-view offset: both views read the same rows):
    p + p and / 2 are exact, every KL term is x * log(1) - x + x, and both views vote for pred (soft-max keeps the
    order of a row's logits; no row of these inputs has two unequal logits so close that their probabilities tie)."""
    logits, inverse, _ = edge_inputs(1, c, p)
    out = _run(logits, inverse, 1)
    assert torch.equal(out[2], torch.zeros(p, dtype=torch.float64, device=DEV))
    two = _run(logits, np.concatenate([inverse, inverse]), 2)
    assert torch.equal(two[2], torch.zeros(p, dtype=torch.float64, device=DEV))
    assert torch.equal(two[4], torch.full((p,), 2, dtype=torch.int32, device=DEV))
    assert torch.equal(two[0], out[0]) and torch.equal(two[3], out[3])


@functools.lru_cache(maxsize=None)
def _oracle_shape():
    """The shape of test_scoring_gpu.py::test_view_mean_softmax_matches_oracle, and 20 supervoxels over its points."""
    g = torch.Generator().manual_seed(0)
    reps, p, c, nv = 8, 5000, 19, 3000
    logits = (torch.randn(reps * nv, c, generator=g) * 3).numpy()
    inverse = torch.cat([torch.randint(0, nv, (p,), generator=g) + v * nv for v in range(reps)]).numpy()
    rs = np.random.RandomState(3)
    perm = rs.permutation(p)
    sizes = [1, 255, 257, 1100] + [rs.randint(2, 200) for _ in range(16)]
    groups, at = [], 0
    for n in sizes:
        groups.append(perm[at:at + n])
        at += n
    assert at <= p and len(groups) == 20
    world = rs.uniform(-40, 40, size=(p, 3)) + np.array([1234.5, -2345.25, 17.0])
    return reps, logits, inverse, groups, world


def test_scores_supervoxel_means_and_frame_means_at_the_oracle_shape():
    from lidal_amd.score import frame_view_scores, interframe, score_frame_views
    reps, logits, inverse, groups, world = _oracle_shape()
    out = _run(logits, inverse, reps)
    ref = _check_against_definition(out, logits, inverse, reps, 'oracle shape')
    _, _, viewd, viewe, agree = out
    assert int(agree.min()) < reps                                      # the views do disagree
    ptr, idx, _ = interframe.sv_csr(groups, DEV)
    sv_d, sv_e, sv_c = score_frame_views(viewd, viewe, _t(world), ptr, idx)
    torch.cuda.synchronize()
    for k, g in enumerate(groups):
        assert np.isclose(float(sv_d[k]), math.fsum(ref['viewd'][g]) / len(g), rtol=1e-4, atol=1e-7), k
        assert np.isclose(float(sv_e[k]), math.fsum(ref['viewe'][g]) / len(g), rtol=1e-4, atol=1e-7), k
        for a in range(3):
            assert np.isclose(float(sv_c[k, a]), math.fsum(world[g, a]) / len(g), rtol=1e-5, atol=1e-5), k
    got = [float(t) for t in frame_view_scores(viewd, viewe, agree, reps)]
    votes = (ref['view_arg'] == out[1].cpu().numpy()[None, :]).sum(axis=0)
    want = [ref['viewd'].mean(), ref['viewe'].mean(), 1.0 - votes.mean() / reps]
    assert all(t.dtype == torch.float32 and t.ndim == 0 for t in frame_view_scores(viewd, viewe, agree, reps))
    assert np.allclose(got, want, rtol=1e-4, atol=1e-7)


def test_two_calls_and_a_side_stream_give_identical_bytes():
    from lidal_amd.score.prob_inference import view_scores
    reps, logits, inverse, _, _ = _oracle_shape()
    lg, inv = _t(logits), _t(inverse)
    first = view_scores(lg, inv, reps)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        second = view_scores(lg, inv, reps)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(first, second))


def _scan_frame(seed, world_seed=5):
    from lidal_amd import synth
    from lidal_amd.score import interframe
    rng = np.random.default_rng(seed)
    pts, inten = synth.raycast_scan(synth.make_world(world_seed), (20.0, 0.0), rng, n_beams=16, n_az=128)
    batch = synth.make_score_batch(pts, inten, rng, inf_reps=8)
    ptr, idx, _ = interframe.sv_csr(synth.angular_supervoxels(pts.astype(np.float32), 20), DEV)
    return {'coords': _t(batch['coords_v_b']), 'feats': _t(batch['feats_v_b']), 'inverse': _t(batch['inverse_indices_b']),
            'world': _t(pts[:, :3].astype(np.float64)), 'sv_ptr': ptr, 'sv_idx': idx}


def test_infer_frame_view_sequence_and_frame_sequence_end_to_end():
    """MinkUNet over the frame of test_prob_inference_end_to_end_vs_oracle (16 beams x 128 azimuths, 8 views) and two
    more like it: the default infer_frame is untouched, return_view_scores appends view_scores of the model's logits,
    view_sequence is the per-frame calls with or without the table prefetch, frame_sequence the frame means."""
    import lidal_amd
    from lidal_amd.network import MinkUNet
    from lidal_amd.score import (frame_sequence, frame_view_scores, infer_frame, score_frame_views, view_sequence)
    from lidal_amd.score.prob_inference import view_scores
    from weights import fill_state_dict
    model = fill_state_dict(MinkUNet(19)).eval().to(DEV)
    frames = [_scan_frame(1), _scan_frame(2, 6), _scan_frame(3, 7)]
    d = frames[0]
    prob, pred = infer_frame(model, d['coords'], d['feats'], d['inverse'], 8)
    full = infer_frame(model, d['coords'], d['feats'], d['inverse'], 8, return_view_scores=True)
    assert len(full) == 3 and torch.equal(full[0], prob) and torch.equal(full[1], pred)
    with torch.no_grad():
        logits, _ = model(lidal_amd.SparseTensor(d['feats'], d['coords']))
    direct = view_scores(logits, d['inverse'], 8)
    assert torch.equal(direct[0], prob) and torch.equal(direct[1], pred)
    assert len(full[2]) == 3 and all(torch.equal(a, b) for a, b in zip(full[2], direct[2:]))
    assert float(full[2][0].max()) > 0 and int(full[2][2].min()) < 8          # the views of a real frame disagree
    with_feat = infer_frame(model, d['coords'], d['feats'], d['inverse'], 8, return_feat=True, return_view_scores=True)
    assert len(with_feat) == 4 and with_feat[2].shape == (prob.shape[0], 96)
    assert all(torch.equal(a, b) for a, b in zip(with_feat[3], full[2]))
    each = []
    for f in frames:
        viewd, viewe, agree = infer_frame(model, f['coords'], f['feats'], f['inverse'], 8, return_view_scores=True)[2]
        each.append((score_frame_views(viewd, viewe, f['world'], f['sv_ptr'], f['sv_idx']),
                     frame_view_scores(viewd, viewe, agree, 8)))
    for prefetch in (True, False):
        seq = view_sequence(model, frames, inf_reps=8, prefetch=prefetch)
        torch.cuda.synchronize()
        assert len(seq) == 3
        for got, (want, _) in zip(seq, each):
            assert got[0].shape == (20,) and got[2].shape == (20, 3)
            assert all(torch.equal(a, b) for a, b in zip(got, want))
    out = frame_sequence(model, frames, metrics=('VIEWD', 'VOTE'), inf_reps=8)
    assert set(out) == {'VIEWD', 'VOTE'}
    for k, (_, (vd, _, vote)) in enumerate(each):
        assert torch.equal(out['VIEWD'][k], vd) and torch.equal(out['VOTE'][k], vote)
