"""CPU tests of the VCCS supervoxels: the numpy restatement (tests/vccs_ref.py) reproduces the
fixture it once wrote (tests/golden/vccs_small.npz) on the small inputs, the ball property holds, the fixtures still
exercise the paths they were made for, what the definition refuses raises before anything is launched, and
data.supervoxel_tables with the new arguments is prepare_supervoxel_VCCS_sk.py:63-89."""
import functools
import os

import numpy as np
import pytest
import torch

import vccs_inputs as VI
import vccs_ref as R


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'vccs_small.npz'))


@functools.lru_cache(maxsize=None)
def _ref(name):
    xyz, kw = VI.fixture(name)
    return xyz, R.vccs(xyz, **kw)


@pytest.mark.parametrize('name', VI.SMALL)
def test_restatement_reproduces_the_fixture_and_the_ball(golden, name):
    xyz, r = _ref(name)
    assert VI.sha256(xyz) == str(golden[name + '_sha'])
    assert np.array_equal(r['labels'], golden[name + '_labels'])
    assert np.array_equal(r['seed_voxels'], golden[name + '_seed_voxels'])
    assert np.array_equal(r['owners'], golden[name + '_owners'])
    assert [len(r['owners']), r['steals'], r['ties'], r['rounds']] == list(golden[name + '_stats'])
    stored = np.unpackbits(golden[name + '_ball'])[:len(r['owners'])].astype(bool)
    mine = R.ball_mask(r['nbr'], r['seed_voxels'], r['rounds'])
    assert np.array_equal(stored, mine) and np.array_equal(r['owners'] != 0, stored)


def test_the_paths_the_fixtures_were_made_for_are_exercised():
    xyz, r = _ref('ground_chain_row')
    assert r['rounds'] == 35 and abs(r['min_seed'] - 15.7) < 0.01
    assert r['steals'] >= 1                                  # an already owned voxel changed hands
    lab = r['labels']
    chain = (xyz[:, 0] > 12.0) & (xyz[:, 0] < 60.0)
    row = xyz[:, 0] > 60.0
    assert chain.sum() == 80 and row.sum() == 8
    assert 1 <= (lab[chain] == 0).sum() < 80                 # beyond the reach of the rounds, and inside it
    assert (lab[row] == 0).all()                             # no seed survives among 8 voxels
    assert (lab[~chain & ~row] != 0).all()
    # the far row's voxels are adjacent to one another and still unlabelled: no seed, not no reach
    assert len(r['seed_voxels']) >= 2 and not (r['cells'][r['seed_voxels'], 0] > 120).any()
    _, plane = _ref('flat_plane')
    assert plane['ties'] >= 1 and np.array_equal(np.bincount(plane['owners']), [0, 400, 400, 400, 400])
    _, wall = _ref('ground_wall')
    assert wall['rounds'] == 13 and len(wall['seed_voxels']) >= 2 and wall['steals'] >= 1


def test_degenerate_inputs():
    _, one = _ref('one_point')
    assert len(one['owners']) == 1 and len(one['seed_voxels']) == 0 and one['labels'].tolist() == [0]
    _, same = _ref('identical')
    assert len(same['owners']) == 1 and same['n'].tolist() == [130] and (same['labels'] == 0).all()
    q = float(np.rint(np.float64(np.float32(-3.3)) * 65536.0)) / 65536.0
    assert same['centroids'][0].tolist() == [q] * 3                                  # the fixed-point mean is exact
    _, two = _ref('two_points')
    assert len(two['owners']) == 2 and not two['normals'].any()                      # |S| < 3: zero normals
    xyz, faces = _ref('faces_negative')
    assert np.array_equal(faces['cells'][faces['point_voxel']], np.floor(xyz.astype(np.float64) / 0.5).astype(np.int64))
    assert faces['cells'][faces['point_voxel'][0]].tolist() == [-1, -1, 0]           # floor, not truncation
    assert faces['cells'][faces['point_voxel'][3]].tolist() == [-2, -2, -2]
    _, line = _ref('three_collinear')
    nrm = line['normals']
    assert np.isfinite(nrm).all() and np.allclose(np.abs(nrm[:, 0]), 0.0) and np.allclose((nrm ** 2).sum(1), 1.0)


def test_parameters_are_the_definitions():
    from lidal_amd import data
    assert data.vccs_parameters() == (R.min_seed_of(0.5, 10.0), 35)
    assert data.vccs_parameters(0.5, 4.0) == (R.min_seed_of(0.5, 4.0), 13)


def test_refusals_raise_before_any_launch():
    from lidal_amd import backend as B
    from lidal_amd import data
    before = dict(B.HITS)
    ok = torch.zeros((4, 3))
    for args, kw in [(([],), {}), ((torch.zeros((0, 3)),), {}), ((torch.zeros((4, 2)),), {}), ((torch.zeros(12),), {}),
                     ((torch.full((4, 3), float('nan')),), {}), ((torch.full((4, 3), float('inf')),), {}),
                     ((torch.full((4, 3), -6e5),), {}), (([ok, torch.zeros((0, 3))],), {}),
                     ((ok,), dict(voxel_resolution=0.0)), ((ok,), dict(voxel_resolution=-1.0)),
                     ((ok,), dict(seed_resolution=0.99)), ((ok,), dict(voxel_resolution=0.25)),
                     ((ok,), dict(spatial_importance=-1.0)), ((ok,), dict(normal_importance=-0.5))]:
        with pytest.raises(ValueError):
            data.vccs_supervoxels(*args, **kw)
    assert B.HITS == before
    with pytest.raises(Exception):                           # valid values on the CPU: no fallback
        data.vccs_supervoxels(ok)


def _vccs_tables_literal(labels_per_frame, names):
    """prepare_supervoxel_VCCS_sk.py:63-89, loop for loop."""
    sv_id_count, id2sv, tables = 0, [], []
    for sv_label, (seq, name) in zip(labels_per_frame, names):
        sv2point = []
        for sv_l in np.unique(sv_label):
            if sv_l != 0:
                p_ids = np.where(sv_label == sv_l)[0]
                if len(p_ids) > 100:
                    sv2point += [p_ids]
        sv_id = np.arange(len(sv2point)) + sv_id_count
        sv_id_count += len(sv2point)
        tables.append((sv_id, sv2point))
        id2sv += [(seq, name, i) for i in np.arange(len(sv2point))]
    return tables, id2sv


def _kmeans_tables_before(labels_per_frame, frame_names):
    """data.supervoxel_tables as it was before it took ignore_label and min_points."""
    tables, id2sv, next_id = [], [], 0
    for lab, (seq, name) in zip(labels_per_frame, frame_names):
        lab = np.asarray(lab).reshape(-1)
        order = np.argsort(lab, kind='stable')
        values, starts = np.unique(lab[order], return_index=True)
        sv2point = [part.astype(np.int64) for part in np.split(order, starts[1:])] if len(values) else []
        sv_id = np.arange(len(sv2point), dtype=np.int64) + next_id
        next_id += len(sv2point)
        tables.append((sv_id, sv2point))
        id2sv.extend((seq, name, local) for local in np.arange(len(sv2point)))
    return tables, id2sv


def _same_tables(got, want):
    (gt, gi), (wt, wi) = got, want
    assert [tuple(x) for x in gi] == [tuple(x) for x in wi] and len(gt) == len(wt)
    for (a_id, a_pts), (b_id, b_pts) in zip(gt, wt):
        assert np.array_equal(a_id, b_id) and len(a_pts) == len(b_pts)
        assert a_id.dtype == np.int64 and all(p.dtype == np.int64 for p in a_pts)
        assert all(np.array_equal(x, y) for x, y in zip(a_pts, b_pts))


def test_supervoxel_tables_with_the_vccs_arguments(golden):
    from lidal_amd import data
    names_in = ('ground_chain_row', 'one_point', 'scan_20k', 'ground_wall')
    labels = [golden[n + '_labels'].astype(np.int64) for n in names_in]
    labels.append(np.repeat(np.arange(4), [150, 100, 101, 300]))         # 100 points are not enough, 101 are
    names = [('00', '%06d' % i) for i in range(len(labels))]
    got = data.supervoxel_tables(labels, names, ignore_label=0, min_points=100)
    _same_tables(got, _vccs_tables_literal(labels, names))
    assert len(got[0][1][1]) == 0 and [len(p) for p in got[0][4][1]] == [101, 300]
    assert [len(p) for p in data.supervoxel_tables(labels[-1:], names[-1:], min_points=100)[0][0][1]] == [150, 101, 300]


def test_supervoxel_tables_defaults_are_unchanged(golden_dir):
    from lidal_amd import data
    g = np.load(os.path.join(golden_dir, 'supervoxel_small.npz'))
    labels = [g['frame_small_labels'], g['frame_medium_labels'], g['assign_p777_k7_labels'], np.zeros(0, dtype=np.int64)]
    names = [('08', '%06d' % i) for i in range(len(labels))]
    _same_tables(data.supervoxel_tables(labels, names), _kmeans_tables_before(labels, names))
    _same_tables(data.supervoxel_tables(labels, names, ignore_label=None, min_points=0),
                 _kmeans_tables_before(labels, names))
