"""data.voxelize_batch (lidal_voxelize_batch: a whole batch voxelised and collated from one sort)
against the fixture the reference's own SK_Dataset / collate_fn wrote, bit for bit against the per-scan path
(voxelize_scan per sample + collate), at the ends of the key's fields, in exactly-sized scratch, and composed into the
three loader modes (train_batch, val_batch, score_sample / score_frame_inputs)."""
import os

import numpy as np
import pytest
import torch

import batch_ref as R
from guarded_ws import Guarded

pytestmark = pytest.mark.gpu
DEV = 'cuda'
KEYS = ('coords_v_b', 'feats_v_b', 'inverse_indices_b', 'unique_idxs_b')


def _g(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _ulp_close(a, b):
    return np.all(np.abs(a.astype(np.float64) - b.astype(np.float64)) <= np.spacing(np.abs(b).astype(np.float32)).astype(np.float64))


def _batch(samples, shared=False):
    from lidal_amd import data
    ms, rs = [s[2] for s in samples], [s[3] for s in samples]
    if shared:
        return data.voxelize_batch(_g(samples[0][0]), _g(samples[0][1]), ms, rs)
    return data.voxelize_batch([_g(s[0]) for s in samples], [_g(s[1]) for s in samples], ms, rs)


def _per_scan(samples):
    """The parent path: voxelize_scan per sample, then collate; the first occurrences as rows of the concatenated list."""
    from lidal_amd import data
    parts, uniq, voxel_ptr, point_ptr = [], [], [0], [0]
    for pts, inten, m, r in samples:
        cv, fv, ui, inv = data.voxelize_scan(_g(pts), _g(inten), m, r)
        parts.append({'coords_v': cv, 'feats_v': fv, 'inverse_idxs': inv})
        uniq.append(ui + point_ptr[-1])
        voxel_ptr.append(voxel_ptr[-1] + cv.shape[0])
        point_ptr.append(point_ptr[-1] + pts.shape[0])
    out = data.collate(parts)
    out['unique_idxs_b'] = torch.cat(uniq)
    out['voxel_ptr'], out['point_ptr'] = np.array(voxel_ptr, dtype=np.int64), np.array(point_ptr, dtype=np.int64)
    return out


def _equal(got, want):
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (k, got[k].shape, want[k].shape)
        assert torch.equal(got[k], want[k]), k
    assert got['voxel_ptr'].dtype == np.int64 and np.array_equal(got['voxel_ptr'], want['voxel_ptr'])
    assert np.array_equal(got['point_ptr'], want['point_ptr'])


# ---- 1. the reference's own fixture -----------------------------------------------------------------------------------
def test_golden_batch_in_one_call(golden_dir):
    g = np.load(os.path.join(golden_dir, 'voxelize_small.npz'))
    samples = [(g['points%d' % i], g['intensity%d' % i], g['trans_m%d' % i], g['rnd%d' % i]) for i in range(2)]
    got = _batch(samples)
    assert got['coords_v_b'].dtype == torch.int32 and got['inverse_indices_b'].dtype == torch.int64
    assert np.array_equal(got['coords_v_b'].cpu().numpy(), g['coords_v_b'])
    assert np.array_equal(got['inverse_indices_b'].cpu().numpy(), g['inverse_indices_b'])
    assert _ulp_close(got['feats_v_b'].cpu().numpy(), g['feats_v_b'])       # numpy's matmul may fuse (test_data_gpu.py)
    assert got['labels_v_b'] is None and got['labels_p_b'] is None


# ---- 2. bit-equality with the per-scan path -----------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(R.SIZES))
def test_equals_the_per_scan_path(name):
    samples = R.box_samples(R.SIZES[name], seed=11)
    got = _batch(samples)
    _equal(got, _per_scan(samples))
    ref = R.one_sort(samples)                                   # and the numpy restatement, integers exactly
    for k in ('coords_v_b', 'inverse_indices_b', 'unique_idxs_b'):
        assert np.array_equal(got[k].cpu().numpy(), ref[k]), k


def test_views_of_one_scan_equal_the_per_scan_path():
    samples = R.view_samples(1000, 8, seed=12)
    got = _batch(samples, shared=True)
    _equal(got, _per_scan(samples))
    assert np.array_equal(got['point_ptr'], np.arange(9) * 1000)


# ---- 3. the sample bits separate samples -----------------------------------------------------------------------------------
def test_the_same_scan_twice_gives_two_separate_halves():
    one = R.box_samples([500], seed=15)
    single, both = _batch(one), _batch(one + one)
    n = single['coords_v_b'].shape[0]
    c = both['coords_v_b']
    assert c.shape[0] == 2 * n and list(both['voxel_ptr']) == [0, n, 2 * n]
    assert torch.equal(c[:n, :3], c[n:, :3]) and torch.equal(c[:n], single['coords_v_b'])
    assert bool((c[:n, 3] == 0).all()) and bool((c[n:, 3] == 1).all())
    inv = both['inverse_indices_b']
    assert torch.equal(inv[500:], inv[:500] + n) and torch.equal(inv[:500], single['inverse_indices_b'])
    assert torch.equal(both['feats_v_b'][n:], both['feats_v_b'][:n])


# ---- 4. duplicates -----------------------------------------------------------------------------------------------------
def test_duplicate_points_share_a_voxel_and_the_smallest_row_wins():
    samples = R.duplicate_samples(13)
    got = _batch(samples)
    _equal(got, _per_scan(samples))
    inv, uniq = got['inverse_indices_b'].cpu().numpy(), got['unique_idxs_b'].cpu().numpy()
    assert (np.diff(got['voxel_ptr']) <= 3).all() and (np.diff(got['voxel_ptr']) >= 1).all()
    for run in range(len(uniq)):
        assert uniq[run] == np.nonzero(inv == run)[0].min()
    alike = R.duplicate_samples(14, n_distinct=1)
    got = _batch(alike)
    assert list(got['voxel_ptr']) == [0, 1, 2, 3]
    assert got['unique_idxs_b'].tolist() == [0, 600, 1200]
    _equal(got, _per_scan(alike))


# ---- 5. the 13-bit fields at both ends -----------------------------------------------------------------------------------
def test_voxel_indices_0_and_8191_in_every_axis():
    samples = R.field_end_samples()
    ref = R.one_sort(samples)                                   # the oracle's validity assert holds on this input
    assert ref['coords_v_b'][:, :3].min() == 0 and ref['coords_v_b'][:, :3].max() == 8191
    got = _batch(samples)
    _equal(got, _per_scan(samples))
    c = got['coords_v_b'].cpu().numpy()
    assert np.array_equal(c, ref['coords_v_b'])
    for s in range(2):
        rows = c[got['voxel_ptr'][s]:got['voxel_ptr'][s + 1]]
        assert (rows[:, :3].min(0) == 0).all() and (rows[:, :3].max(0) == 8191).all() and (rows[:, 3] == s).all()


# ---- 6. a sample outside the grid ---------------------------------------------------------------------------------------
def test_a_sample_outside_the_grid_is_named():
    samples = [(p, i, np.eye(3), np.full(6, 0.5)) for p, i in (R.box_points(np.random.default_rng(16 + k), 50) for k in range(3))]
    far = np.concatenate([samples[1][0], np.array([[500.0, 0.0, 0.0]], dtype=np.float32)])       # 500 m * 20 > 8192 voxels
    bad = [samples[0], (far, np.zeros(51, np.float32)) + samples[1][2:], samples[2]]
    with pytest.raises(AssertionError, match=r'not valid.*sample 1\b'):
        _batch(bad)
    got = _batch(samples)
    _equal(got, _per_scan(samples))


# ---- 7. scratch of exactly the size asked for, full of garbage ---------------------------------------------------------------
@pytest.mark.parametrize('case', ['borders', 'duplicates'])
def test_exact_scratch_between_guards(monkeypatch, case):
    from lidal_amd import backend as B
    samples = R.box_samples(R.SIZES['borders'], seed=11) if case == 'borders' else R.duplicate_samples(13)
    want = _batch(samples)
    torch.cuda.synchronize()
    g = Guarded()
    monkeypatch.setattr(B, 'workspace', g)
    got = _batch(samples)
    g.check()
    p_total = int(want['point_ptr'][-1])
    assert [n for _, n in g.bufs] == [B.lib().lidal_voxelize_batch_workspace_bytes(p_total, len(samples))]
    _equal(got, want)


def test_scratch_one_byte_short_is_refused(monkeypatch):
    from lidal_amd import backend as B
    handle = B.lib_handle()

    class Short:
        def __getattr__(self, name):
            fn = getattr(handle, name)
            return (lambda *a: fn(*a) - 1) if name == 'lidal_voxelize_batch_workspace_bytes' else fn
    g = Guarded()
    monkeypatch.setattr(B, 'workspace', g)
    monkeypatch.setattr(B, 'lib', lambda: Short())
    with pytest.raises(RuntimeError, match='too small'):
        _batch(R.box_samples([300], seed=11))
    g.check()


# ---- 8. the composed modes ----------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def scans():
    """Three small raycast scans (about 4 k points each) on the device, with their host copies."""
    from lidal_amd import synth
    world = synth.make_world(5)
    out = []
    for i in range(3):
        pts, inten = synth.raycast_scan(world, (18.0 + 2 * i, 0.0), np.random.default_rng([21, i]), n_beams=16, n_az=256)
        out.append({'points': pts, 'intensity': inten, 'dev': (_g(pts), _g(inten))})
    return out


@pytest.fixture(scope='module')
def model():
    from lidal_amd.network import MinkUNet
    torch.manual_seed(3)
    return MinkUNet(19).to(DEV).eval()


def test_score_sample_feeds_infer_frame(scans, model):
    from lidal_amd import data
    from lidal_amd.score.prob_inference import infer_frame
    pts, inten = scans[0]['dev']
    batch = data.score_sample(pts, inten, inf_reps=2, rng=np.random.RandomState(5))
    rs = np.random.RandomState(5)
    parts = []
    for _ in range(2):
        m, r = data.draw_augmentation(rs)
        cv, fv, _, inv = data.voxelize_scan(pts, inten, m, r)
        parts.append({'coords_v': cv, 'feats_v': fv, 'inverse_idxs': inv})
    want = data.collate(parts)
    for k in ('coords_v_b', 'feats_v_b', 'inverse_indices_b'):
        assert torch.equal(batch[k], want[k]), k
    prob, pred = infer_frame(model, batch['coords_v_b'], batch['feats_v_b'], batch['inverse_indices_b'], inf_reps=2)
    prob_w, pred_w = infer_frame(model, want['coords_v_b'], want['feats_v_b'], want['inverse_indices_b'], inf_reps=2)
    assert prob.shape == (pts.shape[0], 19) and torch.equal(prob, prob_w) and torch.equal(pred, pred_w)


def _label_inputs(scans, n):
    from lidal_amd import data, synth
    from lidal_amd.score.interframe import sv_csr
    table = data.sk_label_map()
    ids = np.nonzero(table != 255)[0]
    rng = np.random.default_rng(22)
    raws, csrs, flags, pseudos = [], [], [], []
    for k, s in enumerate(scans[:n]):
        p = s['points'].shape[0]
        raw = (rng.choice(ids, p) | (rng.integers(1, 65536, p) << 16)).astype(np.uint32)
        raws.append(_g(raw.view(np.int32)))
        csrs.append(sv_csr(synth.angular_supervoxels(s['points'], 4), DEV)[:2])
        flags.append(np.array([[1, 2, 0, 1], [0, 1, 2, 2]][k]))
        pseudos.append(_g(rng.integers(0, 19, p)))
    return table, raws, csrs, flags, pseudos


def test_train_batch_equals_collated_train_samples(scans):
    from lidal_amd import data
    table, raws, csrs, flags, pseudos = _label_inputs(scans, 2)
    pairs = [s['dev'] for s in scans[:2]]
    got = data.train_batch(pairs, raws, table, csrs, flags, pseudos, rng=np.random.RandomState(9))
    rs = np.random.RandomState(9)
    want = data.collate([data.train_sample(pairs[k][0], pairs[k][1], raws[k], table, csrs[k], flags[k], pseudos[k], rng=rs)
                         for k in range(2)])
    for k in ('coords_v_b', 'feats_v_b', 'labels_v_b'):
        assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), k
    assert len(torch.unique(got['labels_v_b'])) > 2 and bool((got['labels_v_b'] == 255).any())
    loose = data.train_batch(pairs, raws, table, csrs, flags, pseudos, rng=np.random.RandomState(9), check=False)
    assert torch.equal(loose['labels_v_b'], want['labels_v_b']) and len(loose['labels_invalid']) == 2
    data.check_labels(loose['labels_invalid'])


def test_val_batch_feeds_evaluate_batches(scans, model):
    from lidal_amd import data
    from lidal_amd.evaluate import evaluate_batches
    table, raws, _, _, _ = _label_inputs(scans, 2)
    batch = data.val_batch([s['dev'] for s in scans[:2]], raws, table, rng=np.random.RandomState(10))
    assert batch['labels_p_b'].shape == batch['inverse_indices_b'].shape
    assert batch['labels_p_b'].shape[0] == sum(s['points'].shape[0] for s in scans[:2])
    want = torch.cat([data.train_labels(raws[k], table)[0] for k in range(2)])
    assert torch.equal(batch['labels_p_b'], want)
    conf, ious, miou = evaluate_batches(model, [batch])
    assert conf.sum() == int((want < 100).sum())


def test_score_frame_inputs_feed_score_sequence(scans, model):
    from lidal_amd import data, synth
    from lidal_amd.score import score_sequence
    rs = np.random.RandomState(11)
    frames = []
    for i, s in enumerate(scans):
        pose = np.eye(4)
        pose[0, 3] = 2.0 * i
        sv2point = synth.angular_supervoxels(s['points'], 4)
        f = data.score_frame_inputs(s['dev'][0], s['dev'][1], pose, sv2point, inf_reps=2, rng=rs)
        assert sorted(f) == ['coords', 'feats', 'inverse', 'sv_idx', 'sv_ptr', 'world']
        assert torch.equal(f['world'], data.register_scan(s['dev'][0], pose))
        assert f['inverse'].shape[0] == 2 * s['points'].shape[0] and f['sv_ptr'].shape[0] == 5
        frames.append(f)
    out = score_sequence(model, frames, 0, 3, nei_num=2, inf_reps=2)
    assert len(out) == 3
    for d, e, c in out:
        assert d.shape == (4,) and e.shape == (4,) and c.shape == (4, 3)
        assert bool(torch.isfinite(d).all()) and bool(torch.isfinite(e).all())
