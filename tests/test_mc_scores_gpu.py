"""lidal_mc_scores (csrc/score.hip) and what stands on it: the per-point mutual information and
mean entropy of a frame's MC-dropout passes against the f64 definition tests/mc_ref.py, prob / pred against
lidal_view_mean_softmax byte for byte, and infer_frame / mc_sequence / frame_sequence end to end on an SPVCNN with the
counter-based dropout.

The bar of bald and ment is the project's own for point scores (tests/test_view_scores_gpu.py:62-63): 1e-4 of the
largest reference value of the case; tests/test_mc_scores_cpu.py shows that f32 probabilities alone stay two orders of
magnitude inside it.  agree is an exact integer quantity of the logits and of the GPU's own pred."""
import numpy as np
import pytest
import torch

import mc_ref as M

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run(logits, inverse, reps):
    from lidal_amd.score import mc_scores
    out = mc_scores(_t(logits), _t(inverse), reps)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('sigma', M.SIGMAS)
@pytest.mark.parametrize('reps,c,p', M.SHAPES)
def test_scores_against_the_f64_definition(reps, c, p, sigma):
    from lidal_amd.score.prob_inference import view_mean_softmax, view_scores
    logits, inverse = M.inputs(reps, c, p, sigma)
    out = _run(logits, inverse, reps)
    prob, pred, bald, ment, agree = (t.cpu().numpy() for t in out)
    ref = M.scores_from_logits(logits, inverse, reps)
    assert bald.dtype == np.float64 and ment.dtype == np.float32 and agree.dtype == np.int32
    assert bald.shape == ment.shape == agree.shape == (p,) and prob.shape == (p, c)
    assert np.isfinite(prob).all() and np.isfinite(bald).all() and np.isfinite(ment).all()
    err_b, bar_b = np.abs(bald - ref['bald']).max(), 1e-4 * np.abs(ref['bald']).max()
    err_e, bar_e = np.abs(ment - ref['ment']).max(), 1e-4 * np.abs(ref['ment']).max()
    print('reps %d c %d p %d sigma %d: bald error %.3e (bar %.3e)  ment error %.3e (bar %.3e)'
          % (reps, c, p, sigma, err_b, bar_b, err_e, bar_e))
    assert err_b <= bar_b
    assert err_e <= bar_e
    assert np.array_equal(agree, (ref['view_arg'] == pred[None, :]).sum(axis=0))
    assert agree.min() >= 0 and agree.max() <= reps
    if reps > 1:
        assert agree.min() < reps                                   # the passes of these inputs do disagree
    # prob and pred: lidal_view_mean_softmax's bytes; agree: lidal_view_scores'
    vm = view_mean_softmax(_t(logits), _t(inverse), reps)
    assert torch.equal(out[0], vm[0]) and torch.equal(out[1], vm[1])
    assert torch.equal(out[4], view_scores(_t(logits), _t(inverse), reps)[4])


@pytest.mark.parametrize('reps', [1, 2, 4, 8])
def test_a_repeated_row_gives_exactly_zero(reps):
    """Every pass reads the same rows (inverse repeated without the per-pass offset): the mean whose entropy is taken
    is the row and S / reps is H(p), because the kernel takes both sums exactly where they are exact (csrc/score.hip,
    mc_scores_kernel).  prob is lidal_view_mean_softmax's f32 chain all the same, and at reps 8 that chain is NOT the
    row (tests/test_mc_scores_cpu.py::test_why_the_entropy_is_not_taken_of_the_f32_chain)."""
    logits, inverse = M.inputs(1, 19, 257, 3)
    out = _run(logits, np.concatenate([inverse] * reps), reps)
    one = _run(logits, inverse, 1)
    worst = float(out[2].abs().max())
    print('reps %d: max |bald| %.3e, rows whose mean is not the row: %d' % (reps, worst, int((out[0] != one[0]).any(1).sum())))
    assert torch.equal(out[2], torch.zeros(257, dtype=torch.float64, device=DEV))
    from lidal_amd.score.prob_inference import view_mean_softmax
    assert torch.equal(out[3], one[3])
    assert torch.equal(out[0], view_mean_softmax(_t(logits), _t(np.concatenate([inverse] * reps)), reps)[0])
    assert torch.equal(out[0], one[0]) == (reps <= 4)
    assert torch.equal(out[4], torch.full((257,), reps, dtype=torch.int32, device=DEV))


def test_one_hot_rows_one_class_and_no_points():
    from lidal_amd.score import mc_scores
    # logit gaps above 200: every other class underflows to 0, H = 0 without a NaN
    logits = np.full((6, 19), -250.0, np.float32)
    logits[np.arange(6), [0, 5, 18, 7, 7, 3]] = 0.0
    inverse = np.array([0, 1, 2, 3, 4, 5], np.int64)               # 2 passes x 3 points
    prob, pred, bald, ment, agree = _run(logits, inverse, 2)
    assert torch.equal(ment, torch.zeros(3, device=DEV)) and not torch.isnan(bald).any() and not torch.isnan(prob).any()
    # point 0: passes vote 0 and 7 -> m = (.5, .5): bald = log 2; point 1: 5 and 7; point 2: 18 and 3
    assert np.allclose(bald.cpu().numpy(), np.log(2.0), rtol=0, atol=1e-12)
    assert agree.tolist() == [1, 1, 1] and pred.tolist() == [0, 5, 3]
    same = _run(logits, np.array([3, 4, 4, 3], np.int64), 2)       # both passes vote 7
    assert torch.equal(same[2], torch.zeros(2, dtype=torch.float64, device=DEV)) and same[4].tolist() == [2, 2]
    # C = 1: p = 1, everything 0
    lg1, inv1 = M.inputs(4, 1, 65, 3)
    prob, pred, bald, ment, agree = _run(lg1, inv1, 4)
    assert torch.equal(prob, torch.ones(65, 1, device=DEV)) and int(pred.abs().max()) == 0
    assert float(bald.abs().max()) == 0 and float(ment.abs().max()) == 0 and agree.tolist() == [4] * 65
    # P = 0: nothing is launched (the launch of an empty grid would be an error)
    empty = mc_scores(_t(logits), torch.zeros(0, dtype=torch.int64, device=DEV), 2)
    torch.cuda.synchronize()
    assert [tuple(t.shape) for t in empty] == [(0, 19), (0,), (0,), (0,), (0,)]


# ---- end to end: SPVCNN with the counter dropout on three small synthetic frames -------------------------------
def _scan_frame(seed, world_seed=5, passes=8, augment=False):
    from lidal_amd import data, synth
    from lidal_amd.score import interframe
    rng = np.random.default_rng(seed)
    pts, inten = synth.raycast_scan(synth.make_world(world_seed), (20.0, 0.0), rng, n_beams=16, n_az=128)
    batch = data.mc_sample(_t(pts[:, :3].astype(np.float32)), _t(inten.astype(np.float32)), passes=passes,
                           rng=np.random.RandomState(seed), augment=augment)
    ptr, idx, _ = interframe.sv_csr(synth.angular_supervoxels(pts.astype(np.float32), 20), DEV)
    return {'coords': batch['coords_v_b'], 'feats': batch['feats_v_b'], 'inverse': batch['inverse_indices_b'],
            'voxel_ptr': batch['voxel_ptr'], 'world': _t(pts[:, :3].astype(np.float64)), 'sv_ptr': ptr, 'sv_idx': idx}


def test_mc_sample_repeats_one_view_or_draws_each():
    f = _scan_frame(1)
    vp = f['voxel_ptr']
    n = int(vp[1])
    assert len(vp) == 9 and all(int(vp[k + 1] - vp[k]) == n for k in range(8))
    p = f['inverse'].numel() // 8
    for k in range(1, 8):                   # the same voxels, the same features, the same point -> voxel map in every copy
        assert torch.equal(f['coords'][k * n:(k + 1) * n, :3], f['coords'][:n, :3])
        assert torch.equal(f['feats'][k * n:(k + 1) * n], f['feats'][:n])
        assert torch.equal(f['inverse'][k * p:(k + 1) * p] - k * n, f['inverse'][:p])
    assert f['coords'][:, 3].tolist() == [k for k in range(8) for _ in range(n)]
    g = _scan_frame(1, augment=True)
    gp = g['voxel_ptr']                                            # score_sample: every pass its own view
    assert len(gp) == 9 and not any(torch.equal(g['coords'][gp[k]:gp[k + 1], :3], g['coords'][:gp[1], :3]) for k in range(1, 8))


def test_infer_frame_mc_sequence_and_frame_sequence_end_to_end():
    import lidal_amd
    from lidal_amd import nn as spnn
    from lidal_amd.network import MinkUNet, SPVCNN
    from lidal_amd.score import (ScoreBoard, collect_sequence, frame_mc_scores, frame_sequence, infer_frame, mc_scores,
                                 mc_sequence, score_frame_views, view_sequence)
    from weights import fill_state_dict
    model = fill_state_dict(SPVCNN(19, dropout_seed=4)).eval().to(DEV)
    frames = [_scan_frame(1), _scan_frame(2, 6), _scan_frame(3, 7)]
    d = frames[0]
    n, p = int(d['voxel_ptr'][1]), d['inverse'].numel() // 8
    # without mc the copies are the same rows: bald is 0; the default infer_frame is untouched
    prob, pred = infer_frame(model, d['coords'], d['feats'], d['inverse'], 8)
    plain = infer_frame(model, d['coords'], d['feats'], d['inverse'], 8, return_mc_scores=True)
    assert len(plain) == 3 and torch.equal(plain[0], prob) and torch.equal(plain[1], pred)
    assert float(plain[2][0].abs().max()) < 1e-6 and model.dropout.calls == 0
    each = []
    with spnn.mc_dropout(model):
        with torch.no_grad():
            logits, _ = model(lidal_amd.SparseTensor(d['feats'], d['coords']))
        # augment=False: the copies differ by their masks alone -- and they do differ
        rows = logits.float().reshape(8, n, -1)
        assert all(not torch.equal(rows[k], rows[0]) for k in range(1, 8))
        model.dropout.set_rng_state((4, 0))
        full = infer_frame(model, d['coords'], d['feats'], d['inverse'], 8, return_feat=True, return_view_scores=True,
                           return_mc_scores=True)
        direct = mc_scores(logits, d['inverse'], 8)
        assert len(full) == 5 and full[2].shape == (p, 96) and len(full[3]) == 3 and len(full[4]) == 3
        assert torch.equal(full[0], direct[0]) and all(torch.equal(a, b) for a, b in zip(full[4], direct[2:]))
        assert torch.equal(full[3][2], full[4][2])                 # the same agree from either kernel
        # the masks move the predictions: two orders above the rounding floor of identical passes (`plain`, < 1e-6 above)
        assert float(full[4][0].max()) > 1e-5 and float(full[4][0].min()) > -1e-6
        model.dropout.set_rng_state((4, 0))
        for f in frames:
            bald, ment, agree = infer_frame(model, f['coords'], f['feats'], f['inverse'], 8, return_mc_scores=True)[2]
            each.append((score_frame_views(bald, ment, f['world'], f['sv_ptr'], f['sv_idx']),
                         frame_mc_scores(bald, ment, agree, 8), (bald, ment, agree)))
    assert model.dropout.mc is False
    for prefetch in (True, False):
        model.dropout.set_rng_state((4, 0))
        seq = mc_sequence(model, frames, passes=8, prefetch=prefetch)
        torch.cuda.synchronize()
        assert len(seq) == 3 and model.dropout.mc is False and model.dropout.calls == 6
        for got, (want, _, _) in zip(seq, each):
            assert got[0].shape == (20,) and got[1].shape == (20,) and got[2].shape == (20, 3)
            assert all(t.dtype == torch.float32 for t in got)
            assert all(torch.equal(a, b) for a, b in zip(got, want))
    # score_sequence's list: the return leg and the board take it as it is
    rows = collect_sequence(seq, [np.arange(20 * k, 20 * k + 20) for k in range(3)], [f['sv_ptr'] for f in frames], 0, 3)
    board = ScoreBoard(60)
    board.add_sequence(0, rows)
    assert np.array_equal(board.sv_interds, torch.cat([s[0] for s in seq]).cpu().numpy())
    assert np.array_equal(board.sv_interes, torch.cat([s[1] for s in seq]).cpu().numpy())
    assert int(board.sv_pnums.sum()) == sum(f['inverse'].numel() // 8 for f in frames)
    flags = board.select(np.zeros(60, int), 30 * int(board.sv_pnums.sum()))      # (a budget of 30 % of the points)
    assert flags.shape == (60,) and (flags != 0).any()
    # the frame level: f64 means of the point scores, VOTE the variation ratio of the passes
    model.dropout.set_rng_state((4, 0))
    out = frame_sequence(model, frames, metrics=('BALD', 'MCENT', 'VOTE'), inf_reps=8)
    assert set(out) == {'BALD', 'MCENT', 'VOTE'} and model.dropout.mc is False
    for k, (_, got, (bald, ment, agree)) in enumerate(each):
        want = (bald.double().mean().float(), ment.double().mean().float(), (1.0 - agree.double().mean() / 8.0).float())
        for m, a, b in zip(('BALD', 'MCENT', 'VOTE'), got, want):
            assert out[m][k].dtype == torch.float32 and out[m][k].ndim == 0
            assert torch.equal(out[m][k], a) and torch.equal(a, b), (m, k)
    # a model without the counter dropout is refused before anything runs
    for other in (fill_state_dict(MinkUNet(19)).eval().to(DEV), fill_state_dict(SPVCNN(19)).eval().to(DEV)):
        with pytest.raises(ValueError, match='no lidal_amd.nn.Dropout'):
            mc_sequence(other, frames)
        with pytest.raises(ValueError, match='no lidal_amd.nn.Dropout'):
            frame_sequence(other, frames, metrics=('BALD',))
    assert len(view_sequence(model, frames[:1], inf_reps=8)) == 1   # (the view scorer takes the same frames)
