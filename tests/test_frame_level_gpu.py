"""Frame-level selection on the GPU (csrc/frame_level.hip through lidal_amd.score.frame_level) against the numpy
restatement of its orders (tests/frame_ref.py) and the reference's own worker_func values and __main__ flags
(tests/golden/make_golden_frame.py)."""
import os

import numpy as np
import pytest
import torch

import frame_inputs as FI
import frame_ref
from test_frame_level_cpu import ENT_ULPS, SEGENT_ULPS, ulps32, ulps64

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _fixture(golden_dir):
    return np.load(os.path.join(golden_dir, 'frame_small.npz'))


def _same(a, b):
    """bit equality, NaN included"""
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _unc(prob):
    from lidal_amd.score import frame_uncertainty
    return tuple(v.cpu().numpy() for v in frame_uncertainty(torch.from_numpy(prob).to(DEV)))


def test_uncertainty_equals_restatement_and_worker_func(golden_dir):
    g = _fixture(golden_dir)
    worst = 0
    for k, p in enumerate(FI.WORKER_SIZES):
        f = FI.worker_frame(k)
        got = _unc(f['prob'])
        want = frame_ref.uncertainty(f['prob'])
        for m, a, b in zip(('ENT', 'MAR', 'CONF'), got, want):
            assert _same(a, b), (p, m, a, b)
        assert got[1] == g['worker_mar'][k] and got[2] == g['worker_conf'][k], p
        worst = max(worst, int(ulps32(got[0], g['worker_ent'][k])))
    print('ENT vs worker_func: %d ulp' % worst)
    assert worst <= ENT_ULPS


@pytest.mark.parametrize('p', [0, 8191, 8192, 8193, 16383, 16384, 16385, 24575, 24576, 24577])
def test_uncertainty_at_block_edges(p):
    rs = np.random.RandomState(p)
    prob = FI._prob(rs, p, 19) if p else np.zeros((0, 19), np.float32)
    with np.errstate(all='ignore'):
        want = frame_ref.uncertainty(prob)
    got = _unc(prob)
    for a, b in zip(got, want):
        assert _same(a, b), (p, a, b)
    if p == 0:
        assert all(np.isnan(v) for v in got)


def _segent(f, class_num=None):
    from lidal_amd.score import interframe, segment_entropy
    ptr, idx, _ = interframe.sv_csr(f['sv2point'], DEV)
    return float(segment_entropy(torch.from_numpy(f['pred']).to(DEV), ptr, idx,
                                 class_num or f['class_num']).cpu().numpy())


def test_segment_entropy_matches_worker_func(golden_dir):
    """Including a one-point supervoxel in every frame, predictions outside [0, C) (frame 3) and an empty supervoxel
    (NaN, as the reference's 0 / 0)."""
    g = _fixture(golden_dir)
    worst = 0
    for k in range(len(FI.WORKER_SIZES)):
        f = FI.worker_frame(k)
        got = _segent(f)
        want = frame_ref.segment_entropy(f['pred'], f['sv2point'], f['class_num'])
        worst = max(worst, int(ulps64(got, want)), int(ulps64(got, g['worker_segent'][k])))
    print('SEGENT: %d ulp' % worst)
    assert worst <= SEGENT_ULPS
    assert np.isnan(_segent(FI.empty_sv_frame()))
    f = FI.worker_frame(3)
    assert (f['pred'] < 0).any() and (f['pred'] >= f['class_num']).any()


@pytest.mark.parametrize('p,d', [(1, 96), (7, 96), (129, 96), (8193, 96), (120000, 96), (1000, 2), (777, 17),
                                 (1, 1), (8193, 1), (120000, 1), (0, 96)])
def test_frame_feature_bit_equal_to_numpy_mean(p, d):
    from lidal_amd.score import frame_feature
    feat = np.maximum(np.random.RandomState(p + d).normal(size=(p, d)), 0).astype(np.float32)
    got = frame_feature(torch.from_numpy(feat).to(DEV)).cpu().numpy()
    with np.errstate(all='ignore'):
        want = feat.mean(0)
    assert _same(got, want), (p, d)
    assert _same(got, frame_ref.frame_feature(feat))


@pytest.mark.parametrize('share', [0.01, 0.10])
def test_coreset_equals_restatement_at_dataset_size(share):
    from lidal_amd.score import coreset
    n = 19130
    x = FI.large_feats(n, seed=5)
    labeled = np.zeros(n, bool)
    labeled[np.random.RandomState(6).choice(n, int(share * n), replace=False)] = True
    num_add = int(round(0.01 * n))
    picks, flags, md = coreset(torch.from_numpy(x).to(DEV), labeled, return_min_dist=True)
    r_picks, r_md = frame_ref.coreset(x, labeled, num_add)
    assert np.array_equal(picks.cpu().numpy(), r_picks)
    assert _same(md.cpu().numpy(), r_md)
    assert flags.sum() == labeled.sum() + num_add and not labeled[r_picks].any()


def test_coreset_reproduces_reference_main(golden_dir):
    """core_set.py's own flags: frame features by frame_feature on the device, then the greedy loop."""
    from lidal_amd.score import coreset, frame_feature
    g = _fixture(golden_dir)
    seed = int(g['cset_seed'])
    feats = torch.stack([frame_feature(torch.from_numpy(FI.cset_outfeat(seed, s, i)).to(DEV))
                         for s in range(len(FI.SEQS)) for i in range(FI.CSET_FRAMES)])
    assert np.array_equal(feats.cpu().numpy(), FI.cset_feats(seed))
    _, flags = coreset(feats, g['cset_flags_in'])
    assert np.array_equal(flags, g['cset_flags_out'])


def test_coreset_ties_and_refusals():
    from lidal_amd.score import coreset
    rs = np.random.RandomState(2)
    x = rs.uniform(0, 1, size=(500, 96)).astype(np.float32)
    x[[9, 5, 300]] = x[400] + 50.0                     # three identical farthest rows: the first index wins
    labeled = np.zeros(500, bool)
    labeled[0] = True
    picks, _ = coreset(torch.from_numpy(x).to(DEV), labeled, 3)
    assert picks.cpu().numpy()[0] == 5
    assert np.array_equal(picks.cpu().numpy(), frame_ref.coreset(x, labeled, 3)[0])
    same = np.tile(x[:1], (50, 1))                      # every remaining distance 0: the reference asserts
    lab = np.zeros(50, bool)
    lab[0] = True
    with pytest.raises(ValueError, match='selected already'):
        coreset(torch.from_numpy(same).to(DEV), lab, 1)
    with pytest.raises(ValueError, match='no labeled'):
        coreset(torch.from_numpy(x).to(DEV), np.zeros(500, bool), 1)
    with pytest.raises(ValueError, match='unlabeled count'):
        coreset(torch.from_numpy(x).to(DEV), labeled, 500)
    bad = x.copy()
    bad[3, 7] = np.inf
    with pytest.raises(ValueError, match='finite'):
        coreset(torch.from_numpy(bad).to(DEV), labeled, 1)


def test_uncertainty_and_feature_refusals():
    from lidal_amd.score import frame_feature, frame_uncertainty
    prob = torch.full((10, 19), 1.0 / 19, device=DEV)
    prob[3, 2] = float('nan')
    with pytest.raises(ValueError, match='finite'):
        frame_uncertainty(prob)
    with pytest.raises(ValueError, match='margin needs two'):
        frame_uncertainty(torch.ones(10, 1, device=DEV))
    with pytest.raises(ValueError, match='finite'):
        frame_feature(torch.tensor([[1.0, float('inf')]], device=DEV))


def test_frame_sequence_equals_host_restatement():
    """frame_sequence over a small synthetic sequence, every metric: bit-equal to infer_frame followed by the host
    restatement (SEGENT within its bar), then a FrameBoard selection of each metric."""
    from lidal_amd import synth
    from lidal_amd.network import MinkUNet
    from lidal_amd.score import FrameBoard, frame_sequence, infer_frame, interframe
    from lidal_amd.score.frame_level import LARGEST, select_frames
    from weights import fill_state_dict
    frames = synth.make_sequence(4, n_points=None, seed=21, step=0.5, n_beams=12, n_az=96, n_sv=20)
    rng = np.random.default_rng(3)
    model = fill_state_dict(MinkUNet(19)).eval().to(DEV)
    dev_frames = []
    for f in frames:
        sb = synth.make_score_batch(f['points'], f['intensity'], rng, inf_reps=2)
        ptr, idx, _ = interframe.sv_csr(f['sv2point'], DEV)
        dev_frames.append({'coords': torch.from_numpy(sb['coords_v_b']).to(DEV),
                           'feats': torch.from_numpy(sb['feats_v_b']).to(DEV),
                           'inverse': torch.from_numpy(sb['inverse_indices_b']).to(DEV), 'sv_ptr': ptr, 'sv_idx': idx})
    out = frame_sequence(model, dev_frames, metrics=('ENT', 'MAR', 'CONF', 'SEGENT', 'CSET'), inf_reps=2)
    for k, (f, d) in enumerate(zip(frames, dev_frames)):
        prob, pred, feat = (t.cpu().numpy() for t in infer_frame(model, d['coords'], d['feats'], d['inverse'], 2,
                                                                  return_feat=True))
        e, ma, c = frame_ref.uncertainty(prob)
        assert _same(out['ENT'][k].cpu().numpy(), e) and _same(out['MAR'][k].cpu().numpy(), ma)
        assert _same(out['CONF'][k].cpu().numpy(), c)
        assert ulps64(out['SEGENT'][k].cpu().numpy(), frame_ref.segment_entropy(pred, f['sv2point'], 19)) <= SEGENT_ULPS
        assert _same(out['CSET'][k].cpu().numpy(), feat.mean(0))
    assert set(frame_sequence(model, dev_frames[:1], metrics=('CONF',), inf_reps=2)) == {'CONF'}
    with pytest.raises(ValueError):
        frame_sequence(model, dev_frames[:1], metrics=('BALD',))
    board = FrameBoard([np.array([True, False, False, False])], ['00'])
    for m in ('ENT', 'MAR', 'CONF', 'SEGENT', 'CSET'):
        board.add(0, m, out[m])
    assert board.feats.shape == (4, 96)
    for m in ('ENT', 'MAR', 'CONF', 'SEGENT'):
        assert np.array_equal(board.select(m), select_frames(board.flags, board.scores[m], LARGEST[m]))
