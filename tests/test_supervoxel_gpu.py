"""The size-constrained k-means supervoxels on the GPU (csrc/supervoxel.hip through lidal_amd.data) against this
project's numpy restatement (tests/supervoxel_ref.py) and the optima HiGHS found for the transportation LPs
(tests/golden/supervoxel_small.npz, tests/golden/make_golden_supervoxel.py).  Everything is compared bit for bit: the
definition is integer arithmetic after the costs, and the costs restate numpy's f64 roundings."""
import os
import zlib

import numpy as np
import pytest
import torch

import supervoxel_inputs as SI
import supervoxel_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'supervoxel_small.npz'))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _assign_and_compare(golden, name, xyz, centers, lo, hi):
    from lidal_amd import data
    assert SI.sha256(xyz, centers) == str(golden['assign_%s_sha' % name]), name
    cost = R.costs(xyz, centers)
    labels, objective = data.balanced_assign(_dev(cost), lo, hi)
    labels = labels.cpu().numpy()
    assert labels.dtype == np.int64
    sizes = np.bincount(labels, minlength=cost.shape[1])
    print('%s: objective %d (LP %d), sizes %d..%d in [%d, %d]' % (name, objective, int(golden['assign_%s_lp' % name]),
                                                                  sizes.min(), sizes.max(), lo, hi))
    assert objective == int(golden['assign_%s_lp' % name]), name
    assert objective == int(cost[np.arange(len(cost)), labels].astype(np.int64).sum())
    assert sizes.min() >= lo and sizes.max() <= hi, name
    assert np.array_equal(labels, golden['assign_%s_labels' % name]), name


def test_costs_equal_numpy_bit_for_bit(golden):
    """The small scan's cost matrices against its seed rows (every column holds a 0: a point that is its own centre)
    and against its updated centres, then distances whose x1000 is exactly a half (62.5 -> 62, 187.5 -> 188), directly
    and through the whole definition."""
    from lidal_amd import data
    xyz = SI.scan(*SI.FRAMES[0][1:])
    seeds = golden['frame_small_seeds']
    cost1 = data.supervoxel_costs(_dev(xyz), _dev(xyz.astype(np.float64)[seeds])).cpu().numpy()
    assert cost1.dtype == np.int32 and np.array_equal(cost1, golden['frame_small_cost1'])
    assert (cost1[seeds, np.arange(20)] == 0).all()
    centers = _dev(R.supervoxel_kmeans(xyz)['centers'])
    assert np.array_equal(data.supervoxel_costs(_dev(xyz), centers).cpu().numpy(), golden['frame_small_cost2'])
    half = np.array([[0.0625, 0, 0], [-0.0625, 0, 0], [0, 0.1875, 0], [0, -0.1875, 0], [3, 4, 12]], dtype=np.float32)
    origin = np.zeros((1, 3))
    got = data.supervoxel_costs(_dev(half), _dev(origin)).cpu().numpy()
    assert got[:, 0].tolist() == [62, 62, 188, 188, 13000] == R.costs(half, origin)[:, 0].tolist()
    # ... and inside the whole definition: the mean of the four symmetric points is exactly the origin
    labels, ptr, idx, d = data.kmeans_supervoxels(_dev(half[:4]), n_clusters=1, slack=0.0, details=True)
    assert np.array_equal(d['centers'].cpu().numpy(), origin)
    assert d['objective'][1] == 62 + 62 + 188 + 188
    assert ptr.tolist() == [0, 4] and idx.tolist() == [0, 1, 2, 3] and labels.tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize('case', range(len(SI.ASSIGN_CASES)), ids=[c[0] for c in SI.ASSIGN_CASES])
def test_balanced_assign_equals_restatement_and_lp(golden, case):
    name, p, k = SI.ASSIGN_CASES[case]
    xyz, centers = SI.assign_case(p, k, 100 + case)
    _assign_and_compare(golden, name, xyz, centers, *R.bounds(p, k))


@pytest.mark.parametrize('name', ['one_centre', 'identical', 'exact_sizes', 'sink_deficit', 'sink_excess'])
def test_balanced_assign_on_shaped_inputs(golden, name):
    xyz, centers, lo, hi = SI.shaped_cases()[name]
    _assign_and_compare(golden, name, xyz, centers, lo, hi)


def test_balanced_assign_batch_equals_single_calls(golden):
    from lidal_amd import data
    costs, los, his = [], [], []
    for i, (name, p, k) in enumerate(SI.ASSIGN_CASES):
        if k != 20:
            continue
        xyz, centers = SI.assign_case(p, k, 100 + i)
        costs.append(_dev(R.costs(xyz, centers)))
        lo, hi = R.bounds(p, k)
        los.append(lo), his.append(hi)
    batch = data.balanced_assign(costs, los, his)
    names = [c[0] for c in SI.ASSIGN_CASES if c[2] == 20]
    for (labels, objective), name in zip(batch, names):
        assert objective == int(golden['assign_%s_lp' % name])
        assert np.array_equal(labels.cpu().numpy(), golden['assign_%s_labels' % name])


@pytest.mark.parametrize('frame', [0, 1], ids=['small', 'medium'])
def test_whole_definition_equals_restatement(golden, frame):
    from lidal_amd import data
    name, beams, az = SI.FRAMES[frame]
    xyz = SI.scan(beams, az)
    assert SI.sha256(xyz) == str(golden['frame_%s_sha' % name])
    x = _dev(xyz)
    labels, sv_ptr, sv_idx, d = data.kmeans_supervoxels(x, details=True)
    assert labels.dtype == torch.int64 and sv_ptr.dtype == torch.int64 and sv_idx.dtype == torch.int64
    assert np.array_equal(d['seeds'].cpu().numpy(), golden['frame_%s_seeds' % name])
    assert np.array_equal(d['labels_first'].cpu().numpy(), golden['frame_%s_labels1' % name])
    assert np.array_equal(d['centers'].cpu().numpy(), golden['frame_%s_centers' % name])
    assert np.array_equal(labels.cpu().numpy(), golden['frame_%s_labels' % name])
    assert d['objective'] == tuple(golden['frame_%s_lp' % name])
    assert d['augmentations'] == tuple(golden['frame_%s_aug' % name])
    lab = labels.cpu().numpy()
    sizes = np.bincount(lab, minlength=20)
    assert (d['size_min'], d['size_max']) == R.bounds(len(xyz), 20)
    assert sizes.min() >= d['size_min'] and sizes.max() <= d['size_max']
    assert np.array_equal(d['counts'].cpu().numpy(), sizes)
    # the CSR: supervoxels in label order, point ids ascending
    assert np.array_equal(sv_ptr.cpu().numpy(), np.concatenate([[0], np.cumsum(sizes)]))
    assert np.array_equal(sv_idx.cpu().numpy(), np.argsort(lab, kind='stable'))
    # two runs are bit-identical
    again = data.kmeans_supervoxels(x)
    assert all(torch.equal(a, b) for a, b in zip(again, (labels, sv_ptr, sv_idx)))


def test_batch_of_three_frames_equals_three_single_calls():
    from lidal_amd import data
    scans = [_dev(SI.scan(beams, az)) for _, beams, az in SI.FRAMES] + [_dev(SI.scan(*SI.BATCH_EXTRA))]
    assert len({s.shape[0] for s in scans}) == 3
    batch = data.kmeans_supervoxels(scans, details=True)
    for s, got in zip(scans, batch):
        one = data.kmeans_supervoxels(s, details=True)
        for a, b in zip(one[:3], got[:3]):
            assert torch.equal(a, b)
        for key in ('seeds', 'labels_first', 'centers', 'counts'):
            assert torch.equal(one[3][key], got[3][key]), key
        assert one[3]['objective'] == got[3]['objective'] and one[3]['augmentations'] == got[3]['augmentations']


def test_full_size_scan(golden):
    """One scan of about 130 k points: sizes inside the bounds, no error word (the call would raise), two runs
    bit-identical, and both objectives, the augmentation counts and the CRC of the labels equal to the numpy
    restatement's, which took about a minute and a half of CPU time when the fixture was made."""
    from lidal_amd import data
    xyz = SI.full_scan()
    assert SI.sha256(xyz) == str(golden['full_sha'])
    x = _dev(xyz)
    labels, sv_ptr, sv_idx, d = data.kmeans_supervoxels(x, details=True)
    lab = labels.cpu().numpy()
    sizes = np.bincount(lab, minlength=20)
    lo, hi = R.bounds(len(xyz), 20)
    print('full scan: P %d, bounds [%d, %d], sizes %d..%d, objectives %s (numpy %s), augmentations %s' % (
        len(xyz), lo, hi, sizes.min(), sizes.max(), d['objective'], tuple(golden['full_objectives']), d['augmentations']))
    assert sizes.min() >= lo and sizes.max() <= hi
    assert d['objective'] == tuple(golden['full_objectives'])
    assert d['augmentations'] == tuple(golden['full_aug'])
    assert zlib.crc32(lab.astype(np.int8).tobytes()) == int(golden['full_labels_crc'])
    again = data.kmeans_supervoxels(x)
    assert torch.equal(again[0], labels) and torch.equal(again[2], sv_idx)


def test_refusals_come_from_python(golden):
    from lidal_amd import backend as B
    from lidal_amd import data
    before = dict(B.HITS)
    with pytest.raises(ValueError, match='size in'):
        data.kmeans_supervoxels(torch.zeros((21, 3), device=DEV), 20)
    with pytest.raises(ValueError, match='points for'):
        data.kmeans_supervoxels(torch.zeros((19, 3), device=DEV), 20)
    bad = torch.randn((400, 3), device=DEV)
    bad[7, 1] = float('nan')
    with pytest.raises(ValueError, match='finite'):
        data.kmeans_supervoxels(bad, 20)
    bad[7, 1] = float('inf')
    with pytest.raises(ValueError, match='finite'):
        data.kmeans_supervoxels(bad, 20)
    with pytest.raises(RuntimeError, match='GPU only'):
        data.kmeans_supervoxels(torch.randn(400, 3), 20)
    with pytest.raises(ValueError, match='n_clusters'):
        data.kmeans_supervoxels(torch.randn((400, 3), device=DEV), 65)
    with pytest.raises(ValueError, match='size in'):
        data.balanced_assign(torch.zeros((44, 4), dtype=torch.int32, device=DEV), 12, 12)
    assert B.HITS == before                                 # nothing reached the library


def test_supervoxels_close_the_loop_to_scoring_and_training(tmp_path):
    """Raw synthetic frames -> kmeans_supervoxels -> its CSR into score_frame and train_labels, against the same
    labels through supervoxel_tables, the pickles on disk and sv_csr: identical results."""
    from lidal_amd import data, io, synth
    from lidal_amd.score import FrameBank, interframe
    frames = synth.make_sequence(3, n_points=None, seed=5, step=0.7, n_beams=12, n_az=192)
    rng = np.random.default_rng(1)
    bank = FrameBank(0.1)
    for f in frames:
        lg = rng.standard_normal((f['world'].shape[0], 19))
        p = np.exp(lg - lg.max(1, keepdims=True))
        bank.add(_dev(f['world']), _dev((p / p.sum(1, keepdims=True)).astype(np.float32)))
    out = data.kmeans_supervoxels([_dev(f['points']) for f in frames])
    names = [('00', '%06d' % i) for i in range(len(frames))]
    tables, id2sv = data.supervoxel_tables([o[0] for o in out], names)
    assert len(id2sv) == 20 * len(frames) and tables[-1][0][-1] == 20 * len(frames) - 1
    label_map = data.sk_label_map()
    for i, (f, (labels, sv_ptr, sv_idx), (sv_id, sv2point)) in enumerate(zip(frames, out, tables)):
        path = os.path.join(str(tmp_path), 'super_voxel', 'KMeans', names[i][0], names[i][1] + '.pickle')
        io.save_supervoxels(path, sv_id, sv2point)
        got_id, got_s2p = io.load_supervoxels(path)
        ptr2, idx2, _ = interframe.sv_csr(got_s2p, DEV)
        assert torch.equal(ptr2, sv_ptr) and torch.equal(idx2, sv_idx)
        a = interframe.score_frame(bank, i, sv_ptr, sv_idx, 2)
        b = interframe.score_frame(bank, i, ptr2, idx2, 2)
        assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))
        raw = _dev(rng.choice([10, 40, 48, 50, 70], size=len(f['points'])).astype(np.int32))
        flags = rng.integers(0, 2, size=len(got_id))
        la = data.train_labels(raw, label_map, (sv_ptr, sv_idx), flags)[0]
        lb = data.train_labels(raw, label_map, (ptr2, idx2), flags)[0]
        assert torch.equal(la, lb)
