"""GPU tests of the VCCS supervoxels (csrc/vccs.hip) against the numpy restatement's fixture
(tests/golden/vccs_small.npz, tests/golden/make_golden_vccs.py).  Everything is compared bit for bit; no tolerance
appears anywhere.  The fixture's labels, seed voxels, owners and ball masks are stored, not recomputed; the normals are
the restatement's (tests/vccs_ref.py), taken once per fixture."""
import functools
import os

import numpy as np
import pytest
import torch

import vccs_inputs as VI
import vccs_ref as R
from guarded_ws import Guarded

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'vccs_small.npz'))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def _input(name):
    return VI.fixture(name)


@functools.lru_cache(maxsize=None)
def _ref_voxels(name):
    """(cells, centroids, normals, qs, n) of the restatement, computed once and shared."""
    xyz, kw = _input(name)
    cells, inv, qs, n, cen = R.voxelize(xyz, kw.get('voxel_resolution', 0.5))
    nrm = R.normals(cen, R.two_ring(R.adjacency(cells)))
    return cells, cen, nrm, qs, n, inv


@functools.lru_cache(maxsize=None)
def _run(name):
    from lidal_amd import data
    xyz, kw = _input(name)
    out = data.vccs_supervoxels(_dev(xyz), details=True, **kw)
    torch.cuda.synchronize()
    return out


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _check_against_golden(golden, name, item):
    labels, sv_ptr, sv_idx, det = item
    xyz, _ = _input(name)
    assert VI.sha256(xyz) == str(golden[name + '_sha']), name
    assert labels.dtype == torch.int64
    assert np.array_equal(labels.cpu().numpy(), golden[name + '_labels'].astype(np.int64)), name
    assert np.array_equal(det['seed_voxels'].cpu().numpy(), golden[name + '_seed_voxels'].astype(np.int64)), name
    owners = det['owners'].cpu().numpy()
    assert np.array_equal(owners, golden[name + '_owners'].astype(np.int64)), name
    v = int(golden[name + '_stats'][0])
    assert det['rounds'] == int(golden[name + '_stats'][3])
    ball = np.unpackbits(golden[name + '_ball'])[:v].astype(bool)
    assert np.array_equal(owners != 0, ball), name            # the labelled voxels are the ball: no arithmetic enters


@pytest.mark.parametrize('name', VI.ALL)
def test_labels_seeds_owners_and_ball_equal_the_fixture(golden, name):
    _check_against_golden(golden, name, _run(name))


@pytest.mark.parametrize('name', VI.ALL)
def test_voxels_and_normals_equal_the_restatement_bit_for_bit(name):
    det = _run(name)[3]
    cells, cen, nrm, qs, n, inv = _ref_voxels(name)
    assert np.array_equal(det['cells'].cpu().numpy(), cells)
    assert np.array_equal(det['point_voxel'].cpu().numpy(), inv)
    assert np.array_equal(det['qs'].cpu().numpy(), qs) and np.array_equal(det['n'].cpu().numpy(), n)
    assert np.array_equal(_bits(det['centroids'].cpu().numpy()), _bits(cen))
    got = det['normals'].cpu().numpy()
    diff = np.flatnonzero((_bits(got) != _bits(nrm)).any(axis=1))
    print('%s: %d voxels, %d normals differ' % (name, len(nrm), len(diff)))
    assert len(diff) == 0, (name, diff[:5], got[diff[:5]], nrm[diff[:5]])


@pytest.mark.parametrize('p,side', [(2047, 8), (2048, 8), (2049, 8), (524289, 32)])
def test_random_scans_at_the_edges_of_the_scan(p, side):
    """Sizes chosen for the scans of the head flags (8 x 256 = 2048 flags per tile): one tile and its neighbours, and one
    element past 256 tiles.  A seeded random ground patch of 2 side x 2 side metres against the whole restatement, every
    array (the restatement takes about 0.1 s on the small scans and 2 s on the large one: 16 397 voxels, 64 seeds)."""
    from lidal_amd import data
    rng = np.random.RandomState(p)
    xyz = np.stack([rng.uniform(-side, side, p), rng.uniform(-side, side, p), rng.normal(-1.7, 0.05, p)],
                   axis=1).astype(np.float32)
    want = R.vccs(xyz)
    labels, _, _, det = data.vccs_supervoxels(_dev(xyz), details=True)
    assert len(want['seed_voxels']) >= 4 and len(want['cells']) > 800
    assert np.array_equal(labels.cpu().numpy(), want['labels'])
    for key in ('point_voxel', 'cells', 'qs', 'n', 'seed_voxels', 'owners'):
        assert np.array_equal(det[key].cpu().numpy(), want[key]), key
    for key in ('centroids', 'normals'):
        assert np.array_equal(_bits(det[key].cpu().numpy()), _bits(want[key])), key


def test_flat_plane_is_four_supervoxels_of_400_voxels():
    owners = _run('flat_plane')[3]['owners'].cpu().numpy()
    assert np.array_equal(np.bincount(owners), [0, 400, 400, 400, 400])


def test_batch_equals_the_single_calls(golden):
    from lidal_amd import data
    out = data.vccs_supervoxels([_dev(_input(n)[0]) for n in VI.BATCH], details=True)
    assert len(out) == len(VI.BATCH)
    for name, item in zip(VI.BATCH, out):
        _check_against_golden(golden, name, item)
        single = _run(name)
        for a, b in zip(item[:3], single[:3]):
            assert torch.equal(a, b)
        for key in ('cells', 'centroids', 'normals', 'point_voxel', 'qs', 'n', 'seed_voxels', 'owners', 'counts'):
            a, b = item[3][key], single[3][key]
            assert a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)), key


@pytest.mark.parametrize('name', ['ground_chain_row', 'scan_20k'])
def test_two_runs_are_identical(name):
    from lidal_amd import data
    xyz, kw = _input(name)
    again = data.vccs_supervoxels(_dev(xyz), details=True, **kw)
    first = _run(name)
    for a, b in zip(again[:3], first[:3]):
        assert torch.equal(a, b)
    for key in ('normals', 'centroids', 'owners', 'seed_voxels'):
        assert torch.equal(again[3][key].view(torch.int64), first[3][key].view(torch.int64)), key


@pytest.mark.parametrize('name', ['ground_chain_row', 'ground_wall', 'scan_20k', 'identical', 'one_point'])
def test_csr_is_the_reference_lists_and_feeds_scoring_and_training(name):
    """Label order, ascending ids, only labels != 0 with more than 100 points; straight into region_scores and
    train_labels; points outside every list end at 255."""
    from lidal_amd import data
    from lidal_amd.score import redal
    labels, sv_ptr, sv_idx, _ = _run(name)
    lab = labels.cpu().numpy()
    want_ptr, want_idx = R.sv_lists(lab, 100, 0)
    assert sv_ptr.dtype == torch.int64 and sv_idx.dtype == torch.int64
    assert np.array_equal(sv_ptr.cpu().numpy(), want_ptr) and np.array_equal(sv_idx.cpu().numpy(), want_idx)
    for s in range(len(want_ptr) - 1):
        ids = want_idx[want_ptr[s]:want_ptr[s + 1]]
        assert len(ids) > 100 and (np.diff(ids) > 0).all() and lab[ids[0]] != 0 and (lab[ids] == lab[ids[0]]).all()
    p, s = len(lab), len(want_ptr) - 1
    rng = np.random.default_rng(3)
    raw = _dev(rng.choice([10, 40, 48, 50, 70], size=p).astype(np.int32))
    label_map = data.sk_label_map()
    got = data.train_labels(raw, label_map, (sv_ptr, sv_idx), np.ones(s, dtype=np.int64))[0].cpu().numpy()
    covered = np.zeros(p, dtype=bool)
    covered[want_idx] = True
    assert (got[~covered] == 255).all()
    plain = data.train_labels(raw, label_map)[0].cpu().numpy()
    assert np.array_equal(got[covered], plain[covered])
    if s:
        prob = rng.random((p, 19)).astype(np.float32)
        prob /= prob.sum(1, keepdims=True)
        scores, feats, pnums = redal.region_scores(_dev(prob), _dev(rng.random((p, 8)).astype(np.float32)),
                                                   _dev(rng.random(p).astype(np.float32)), sv_ptr, sv_idx)
        assert np.array_equal(pnums.cpu().numpy(), np.diff(want_ptr)) and bool(torch.isfinite(scores).all())


@pytest.mark.parametrize('names', [('one_point',), ('three_collinear',), ('ground_wall',), VI.BATCH])
def test_workspace_is_exact(monkeypatch, golden, names):
    """In scratch of exactly lidal_vccs_workspace_bytes bytes that arrives full of garbage, between untouched guards:
    the same results; with one byte less: refused before any launch."""
    from lidal_amd import backend as B
    from lidal_amd import data
    scans = [_dev(_input(n)[0]) for n in names]
    kw = _input(names[0])[1]
    g = Guarded()
    monkeypatch.setattr(B, 'workspace', g)
    out = data.vccs_supervoxels(scans, details=True, **kw)
    g.check()
    assert g.bufs[0][1] == B.lib_handle().lidal_vccs_workspace_bytes(sum(len(s) for s in scans), len(scans))
    for name, item in zip(names, out):
        _check_against_golden(golden, name, item)
        assert torch.equal(item[3]['normals'].view(torch.int64), _run(name)[3]['normals'].view(torch.int64))

    class Short:
        def __getattr__(self, attr):
            fn = getattr(B.lib_handle(), attr)
            return (lambda *a: fn(*a) - 1) if attr == 'lidal_vccs_workspace_bytes' else fn

    monkeypatch.setattr(B, 'lib', lambda: Short())
    with pytest.raises(RuntimeError, match='too small'):
        data.vccs_supervoxels(scans, **kw)
    g.check()


def test_refusals_launch_nothing():
    from lidal_amd import backend as B
    from lidal_amd import data
    before = dict(B.HITS)
    ok = torch.zeros((4, 3), device=DEV)
    bad = [((torch.full((4, 3), float('nan'), device=DEV),), {}), ((torch.full((4, 3), 6e5, device=DEV),), {}),
           ((torch.zeros((0, 3), device=DEV),), {}), ((torch.zeros((4, 2), device=DEV),), {}), (([],), {}),
           ((ok,), dict(voxel_resolution=0.0)), ((ok,), dict(seed_resolution=0.9)), ((ok,), dict(voxel_resolution=0.25)),
           ((ok,), dict(spatial_importance=-1.0)), ((ok,), dict(normal_importance=-0.5))]
    for args, kw in bad:
        with pytest.raises(ValueError):
            data.vccs_supervoxels(*args, **kw)
    assert B.HITS == before
