"""The size-constrained k-means supervoxels without a GPU: the numpy restatement (tests/supervoxel_ref.py) reaches the
optimum that HiGHS found for every assignment problem of tests/golden/supervoxel_small.npz, the supervoxel tables and
the new on-disk formats round-trip, and the size bounds are the reference's expressions."""
import os

import numpy as np
import pytest
import torch

import supervoxel_inputs as SI
import supervoxel_ref as R


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'supervoxel_small.npz'))


def _check(golden, name, xyz, centers, lo, hi):
    assert SI.sha256(xyz, centers) == str(golden['assign_%s_sha' % name]), name
    cost = R.costs(xyz, centers)
    labels, objective, aug = R.balanced_assign(cost, lo, hi)
    assert objective == int(golden['assign_%s_lp' % name]), name
    assert objective == int(cost[np.arange(len(cost)), labels].astype(np.int64).sum())
    sizes = np.bincount(labels, minlength=cost.shape[1])
    assert sizes.min() >= lo and sizes.max() <= hi, (name, sizes)
    assert np.array_equal(labels, golden['assign_%s_labels' % name]), name
    assert aug == int(golden['assign_%s_aug' % name])


def test_restatement_reaches_the_lp_optimum_on_every_assignment_problem(golden):
    for i, (name, p, k) in enumerate(SI.ASSIGN_CASES):
        xyz, centers = SI.assign_case(p, k, 100 + i)
        assert tuple(golden['assign_%s_bounds' % name]) == R.bounds(p, k)
        _check(golden, name, xyz, centers, *R.bounds(p, k))
    shaped = SI.shaped_cases()
    assert set(shaped) == {'one_centre', 'identical', 'exact_sizes', 'sink_deficit', 'sink_excess'}
    for name, (xyz, centers, lo, hi) in shaped.items():
        _check(golden, name, xyz, centers, lo, hi)
    # the shaped cases are what they say
    assert int(golden['assign_one_centre_aug']) == 2000 - 105
    assert int(golden['assign_identical_aug']) == 600 - 31


def test_whole_definition_on_the_small_frame(golden):
    """Both assignments of the small scan equal the LP optimum; the medium scan's stored labels are checked against
    costs recomputed from its stored seeds and centres (running the restatement on it again takes too long here)."""
    xyz = SI.scan(*SI.FRAMES[0][1:])
    assert SI.sha256(xyz) == str(golden['frame_small_sha'])
    r = R.supervoxel_kmeans(xyz, 20, 0.05, 0)
    assert (r['objective1'], r['objective2']) == tuple(golden['frame_small_lp'])
    assert np.array_equal(r['cost1'], golden['frame_small_cost1'])
    assert np.array_equal(r['cost2'], golden['frame_small_cost2'])
    assert np.array_equal(r['labels'], golden['frame_small_labels'])
    for lab in (r['labels1'], r['labels']):
        sizes = np.bincount(lab, minlength=20)
        assert sizes.min() >= r['lo'] and sizes.max() <= r['hi']
    xyz = SI.scan(*SI.FRAMES[1][1:])
    assert SI.sha256(xyz) == str(golden['frame_medium_sha'])
    lo, hi = R.bounds(len(xyz), 20)
    x64 = xyz.astype(np.float64)
    for centers, labels, lp in ((x64[golden['frame_medium_seeds']], golden['frame_medium_labels1'], 0),
                                (golden['frame_medium_centers'], golden['frame_medium_labels'], 1)):
        cost = R.costs(xyz, centers)
        assert int(cost[np.arange(len(xyz)), labels].astype(np.int64).sum()) == int(golden['frame_medium_lp'][lp])
        sizes = np.bincount(labels, minlength=20)
        assert sizes.min() >= lo and sizes.max() <= hi


def test_costs_round_half_to_even_and_are_zero_at_a_centre():
    """0.0625 m and 0.1875 m are exact in f32 and their x1000 is exactly a half: 62.5 -> 62, 187.5 -> 188."""
    centers = np.array([[0.0, 0.0, 0.0], [1.0, 2.0, 3.0]])
    xyz = np.array([[0.0625, 0, 0], [0, -0.1875, 0], [1, 2, 3], [3, 4, 12]], dtype=np.float32)
    cost = R.costs(xyz, centers)
    assert cost.dtype == np.int32 and cost.shape == (4, 2)
    assert cost[:, 0].tolist() == [62, 188, int(np.rint(1000 * np.sqrt(14.0))), 13000]
    assert cost[2, 1] == 0


def test_size_bounds_are_the_reference_expressions():
    from lidal_amd import data
    for p in (20, 21, 44, 399, 400, 777, 1030, 3000, 12345, 130242):
        for k in (4, 7, 20):
            assert data.supervoxel_bounds(p, k) == (int(p / k * 0.95), int(p / k * 1.05)) == R.bounds(p, k)
    assert data.supervoxel_bounds(130242) == (6186, 6837)
    assert data.supervoxel_bounds(400) == (19, 21) and data.supervoxel_bounds(20) == (0, 1)
    assert data.supervoxel_bounds(1200, 20, 0.0) == (60, 60)


def test_infeasible_combinations_raise_before_any_launch():
    """ValueError comes first, even for CPU tensors; a feasible CPU tensor is then refused as such."""
    from lidal_amd import data
    with pytest.raises(ValueError, match='size in'):
        data.kmeans_supervoxels(torch.zeros(21, 3), 20)                     # size_max = 1: 20 < 21
    with pytest.raises(ValueError, match='size in'):
        data.kmeans_supervoxels(torch.zeros(38, 3), 20)                     # int(38 / 20 * 1.05) is still 1
    with pytest.raises(ValueError, match='points for'):
        data.kmeans_supervoxels(torch.zeros(19, 3), 20)
    for k in (0, 65):
        with pytest.raises(ValueError, match='n_clusters'):
            data.kmeans_supervoxels(torch.zeros(1000, 3), k)
    with pytest.raises(ValueError):
        data.kmeans_supervoxels(torch.zeros(1000, 2), 20)
    with pytest.raises(RuntimeError, match='GPU only'):
        data.kmeans_supervoxels(torch.zeros(400, 3), 20)
    cost = torch.zeros((44, 4), dtype=torch.int32)
    with pytest.raises(ValueError, match='size in'):
        data.balanced_assign(cost, 12, 12)                                  # 4 * 12 > 44
    with pytest.raises(ValueError, match='size in'):
        data.balanced_assign(cost, 0, 10)                                   # 4 * 10 < 44
    with pytest.raises(TypeError):
        data.balanced_assign(cost.long(), 10, 11)
    with pytest.raises(RuntimeError, match='GPU only'):
        data.balanced_assign(cost, 10, 11)
    with pytest.raises(ValueError):
        R.balanced_assign(cost.numpy(), 12, 12)


def test_supervoxel_tables_and_files_round_trip(tmp_path):
    from lidal_amd import data, io
    from lidal_amd.score import interframe
    rng = np.random.RandomState(0)
    names = [('00', '000000'), ('00', '000001'), ('03', '000000')]
    labels = [rng.randint(0, 20, size=500), rng.choice([1, 4, 19], size=77), rng.randint(0, 20, size=1030)]
    tables, id2sv = data.supervoxel_tables(labels, names)
    ref_tables, ref_id2sv = R.sv_tables_script([(s, n, lab) for (s, n), lab in zip(names, labels)])
    assert id2sv == ref_id2sv and len(id2sv) == 20 + 3 + 20
    assert [type(e[2]) for e in id2sv] == [type(e[2]) for e in ref_id2sv]
    for (sv_id, sv2point), (ref_id, ref_s2p), lab in zip(tables, ref_tables, labels):
        assert np.array_equal(sv_id, ref_id) and sv_id.dtype == np.int64
        assert len(sv2point) == len(ref_s2p) == len(np.unique(lab))         # empty clusters dropped
        for a, b in zip(sv2point, ref_s2p):
            assert np.array_equal(a, b) and a.dtype == np.int64
    assert tables[2][0][0] == 23                                             # sv_id runs across the frames
    root = str(tmp_path)
    for (seq, name), lab, (sv_id, sv2point) in zip(names, labels, tables):
        base = os.path.join(root, 'super_voxel', 'KMeans', seq, name)
        io.save_sv_labels(base + '.npy', torch.from_numpy(lab))
        back = io.load_sv_labels(base + '.npy')
        assert back.dtype == np.int64 and np.array_equal(back, lab)
        assert np.load(base + '.npy').dtype == np.int32
        io.save_supervoxels(base + '.pickle', sv_id, sv2point)
        got_id, got_s2p = io.load_supervoxels(base + '.pickle')
        assert np.array_equal(got_id, sv_id)
        assert all(np.array_equal(a, b) for a, b in zip(got_s2p, sv2point))
        # the tables rebuilt from the label file are the same tables
        again, _ = data.supervoxel_tables([back], [(seq, name)])
        assert all(np.array_equal(a, b) for a, b in zip(again[0][1], sv2point))
        ptr, idx, lens = interframe.sv_csr(got_s2p, 'cpu')
        assert np.array_equal(lens, np.bincount(lab)[np.unique(lab)])
        assert np.array_equal(idx.numpy(), np.argsort(lab, kind='stable'))
    path = os.path.join(root, 'super_voxel', 'KMeans', 'id2sv.pickle')
    io.save_id2sv(path, id2sv)
    assert io.load_id2sv(path) == id2sv
    with pytest.raises(ValueError):
        data.supervoxel_tables(labels, names[:2])
