"""data.euclidean_clusters (lidal_euclidean_clusters) against the numpy restatement
tests/cluster_ref.py: every output array equal, no tolerance anywhere -- on the scene of the CPU test, on a chain that
crosses hundreds of cells, at the rounded root and at the cell borders, on one dense cell, across classes, scans and size
filters, under a permutation of the rows, twice, in exactly-sized scratch between guards -- and the pastes by instance
of mix_scans(paste_masks=...)."""
import numpy as np
import pytest
import torch

import cluster_ref as C
import mix_ref as R
from guarded_ws import Guarded

pytestmark = pytest.mark.gpu
DEV = 'cuda'
F0 = np.float32(0)
KEYS = ('inst', 'inst_ptr', 'cls', 'member_ptr', 'members', 'bbox', 'sizes')


def _g(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _host(v):
    return v.cpu().numpy() if torch.is_tensor(v) else np.asarray(v)


def _run(scans, labels=None, **kw):
    from lidal_amd import data
    return data.euclidean_clusters([_g(np.asarray(x, np.float32).reshape(-1, 3)) for x in scans],
                                   None if labels is None else [_g(np.asarray(l, np.int64)) for l in labels], **kw)


def _same(got, want):
    for k in KEYS:
        g, w = _host(getattr(got, k)), want[k]
        assert g.dtype == w.dtype and g.shape == w.shape, (k, g.dtype, g.shape, w.dtype, w.shape)
        assert np.array_equal(g.view(np.uint32) if g.dtype == np.float32 else g,
                              w.view(np.uint32) if w.dtype == np.float32 else w), k


def _check(scans, labels=None, tolerance=0.5, min_points=1, max_points=None):
    """One call over the scans against the reference -> (Instances, the reference's dict)."""
    scans = [np.asarray(x, np.float32).reshape(-1, 3) for x in scans]
    ptr = np.concatenate([[0], np.cumsum([len(x) for x in scans])]).astype(np.int64)
    got = _run(scans, labels, tolerance=tolerance, min_points=min_points, max_points=max_points)
    want = C.clusters_ref(np.concatenate(scans), ptr, None if labels is None else np.concatenate(labels), tolerance,
                          min_points, max_points)
    _same(got, want)
    return got, want


@pytest.fixture(scope='module')
def scene():
    xyz, ptr, lab = C.scene()
    want = C.clusters_ref(xyz, ptr, lab, C.SCENE_TOL, C.SCENE_MIN, C.SCENE_MAX)
    cut = int(ptr[1])
    return dict(scans=[xyz[:cut], xyz[cut:]], labels=[lab[:cut], lab[cut:]], want=want)


def _run_scene(scene):
    return _run(scene['scans'], scene['labels'], tolerance=C.SCENE_TOL, min_points=C.SCENE_MIN, max_points=C.SCENE_MAX)


def test_the_scene(scene):
    from lidal_amd import backend as B
    before = B.HITS.get('euclidean_clusters', 0)
    got = _run_scene(scene)
    assert B.HITS['euclidean_clusters'] == before + 1                     # one library call
    _same(got, scene['want'])
    assert len(got) == len(scene['want']['cls']) >= 20
    ptr, rows = got.as_csr(1)                                             # scan-local rows of the second scan's instances
    k0 = int(got.inst_ptr[1])
    assert ptr.dtype == torch.int64 and rows.dtype == torch.int64 and ptr[0] == 0 and len(ptr) == len(got) - k0 + 1
    local = got.inst[len(scene['scans'][0]):].long()
    assert torch.equal(local[rows], torch.repeat_interleave(torch.arange(k0, len(got), device=DEV), ptr[1:] - ptr[:-1]))


def _chain(gap_at, second):
    """1 000 points on the x axis, 0.45 m apart (0.9 of the tolerance 0.5), one link set by hand: 225 -> `second`."""
    x = np.float32(0.45) * np.arange(1000, dtype=np.float32)
    x[gap_at] = np.float32(225.0)
    x[gap_at + 1:] = np.float32(second) + np.float32(0.45) * np.arange(999 - gap_at, dtype=np.float32)
    xyz = np.zeros((1000, 3), np.float32)
    xyz[:, 0] = x
    return xyz[np.random.RandomState(31).permutation(1000)]


def test_a_chain_across_hundreds_of_cells():
    """One component through some 900 cells of 0.5 m, rows shuffled; a link of exactly the tolerance opens it, a link one
    ulp shorter does not."""
    got, _ = _check([_chain(500, 225.45)])
    assert len(got) == 1 and int(got.sizes[0]) == 1000
    got, _ = _check([_chain(500, 225.5)])
    assert len(got) == 2 and sorted(got.sizes.tolist()) == [499, 501]
    got, _ = _check([_chain(500, np.nextafter(np.float32(225.5), F0))])
    assert len(got) == 1


def test_the_rounded_root_decides_at_the_tolerance():
    """From (0,0,0) at tol 5: (3,4,0) is at 5.0; (3, 4-, 0) has a squared distance below 25 whose rounded root is 5.0 --
    not joined either; one step nearer it is.  Repeated shifted across a cell border and on the other axes: 21 scans of
    two points in one call."""
    four = np.nextafter(np.float32(4), F0)
    ends = np.array([[3, 4, 0], [3, four, 0], [3, np.nextafter(four, F0), 0]], np.float32)
    assert float(np.square(ends[1]).sum()) < 25.0
    scans = []
    for shift in ([0.0, 0.0, 0.0], [5.0, 4.0, -3.0], [-11.0, -12.0, 7.0]):
        for perm in ([0, 1, 2], [2, 0, 1], [1, 2, 0]):
            if shift == [0.0, 0.0, 0.0] and perm != [0, 1, 2]:
                continue
            for e in ends:
                scans.append((np.stack([np.zeros(3, np.float32), e]) + np.float32(shift))[:, perm])
    assert len(scans) == 21
    got, _ = _check(scans, tolerance=5.0)
    assert np.diff(got.inst_ptr).tolist()[:3] == [2, 2, 1]                # (shifted, the ends round: the reference decides)


def test_either_side_of_cell_borders():
    """Coordinates at, just below and just above the borders of the 1 m cells at 0, +-1, +-2, with a tolerance (0.7) that
    is no power of two: the cell is wider than the radius."""
    vals = []
    for b in (-2.0, -1.0, 0.0, 1.0, 2.0):
        b = np.float32(b)
        vals += [b, np.nextafter(b, np.float32(-100)), np.nextafter(b, np.float32(100)), b - np.float32(0.0625),
                 b + np.float32(0.0625), b - np.float32(0.59375), b + np.float32(0.3125)]
    vals = np.array(vals + [-0.0], np.float32)
    rs = np.random.RandomState(21)
    _check([vals[rs.randint(0, vals.size, (700, 3))]], tolerance=0.7)
    for axis in range(3):                               # all on one axis: pairs straddle the border cell by cell
        line = np.zeros((vals.size, 3), np.float32)
        line[:, axis] = vals
        _check([line], tolerance=0.7)


def test_a_dense_blob_in_one_cell():
    """2 000 points in a 0.2 m cube at tol 0.5: every pair is an edge, one cell run is longer than a workgroup, every
    hook lands on one root."""
    xyz = np.random.RandomState(32).uniform(0.1, 0.3, (2000, 3)).astype(np.float32)
    got, _ = _check([xyz])
    assert len(got) == 1 and torch.equal(got.members, torch.arange(2000, dtype=torch.int32, device=DEV))
    assert not bool((got.inst != 0).any())


def test_classes():
    rs = np.random.RandomState(33)
    blob = rs.uniform(0, 0.25, (20, 3)).astype(np.float32)
    # identical coordinates in two classes: two instances
    got, _ = _check([np.concatenate([blob, blob])], [np.repeat([1, 2], 20)])
    assert len(got) == 2 and got.cls.tolist() == [1, 2]
    # a class without a tolerance, labels outside 0..63: no instance
    lab = np.array([1] * 5 + [2] * 5 + [255, 64, -1, 63, 63], np.int64)
    got, _ = _check([blob[:15]], [lab], tolerance={1: 0.5, 63: 0.5})
    assert got.inst.tolist() == [0] * 5 + [-1] * 8 + [1, 1]
    # two blobs 0.8 m apart; between them a NaN point, an infinite one and a finite one of an ignored class
    a = np.array([[0, 0, 0], [0.1, 0, 0]], np.float32)
    between = np.array([[0.45, np.nan, 0], [0.45, np.inf, 0], [-np.inf, 0, 0], [0.45, 0, 0]], np.float32)
    xyz = np.concatenate([a, between, a + np.float32([0.8, 0, 0])])
    got, _ = _check([xyz], [np.array([1, 1, 1, 1, 1, 255, 1, 1])])
    assert got.inst.tolist() == [0, 0, -1, -1, -1, -1, 1, 1]
    got, _ = _check([xyz[[0, 1, 5, 6, 7]]], [np.ones(5, np.int64)])               # the same point, live: it bridges
    assert len(got) == 1
    # tolerances per class: two pairs 0.4 m apart; the class at 0.5 joins, the class at 0.3 does not
    pair = np.array([[0, 0, 0], [0, 0.4, 0]], np.float32)
    got, _ = _check([np.concatenate([pair, pair + np.float32(10)])], [np.array([1, 1, 2, 2])], tolerance={1: 0.5, 2: 0.3})
    assert got.inst.tolist() == [0, 0, 1, 2] and got.cls.tolist() == [1, 2, 2]


def test_scans():
    rs = np.random.RandomState(34)
    blob = rs.uniform(0, 0.25, (30, 3)).astype(np.float32)
    far = blob + np.float32(50)
    # the same coordinates in two scans: two instances, no edge across scans; an empty scan between them
    got, _ = _check([blob, np.zeros((0, 3), np.float32), blob])
    assert got.inst_ptr.tolist() == [0, 1, 1, 2] and got.sizes.tolist() == [30, 30]
    ptr, rows = got.as_csr(2)
    assert ptr.tolist() == [0, 30] and rows.tolist() == list(range(30))
    assert [t.numel() for t in got.as_csr(1)] == [1, 0]
    # a scan without live points between two with; labels=None is class 0
    dead = np.full(30, 255, np.int64)
    live = np.zeros(30, np.int64)
    got, _ = _check([np.concatenate([blob, far]), blob, far], [np.concatenate([live, live]), dead, live])
    assert got.inst_ptr.tolist() == [0, 2, 2, 3]
    got, _ = _check([np.concatenate([blob, far]), blob], None)
    assert got.inst_ptr.tolist() == [0, 2, 3] and got.cls.tolist() == [0, 0, 0]
    # a batch in which nothing is live, and one without points: no instance, no launch
    for scans, labels in (([blob], [dead]), ([np.zeros((0, 3), np.float32)], None)):
        got, _ = _check(scans, labels)
        assert len(got) == 0 and got.member_ptr.tolist() == [0]
    got = _run([blob], tolerance={5: 0.5})
    assert len(got) == 0 and got.inst.tolist() == [-1] * 30


def test_size_filters():
    """Components of min - 1, min, max and max + 1 points (min 3, max 6), their rows interleaved over two scans: the
    numbering skips the dropped ones and inst_ptr counts the kept ones."""
    rs = np.random.RandomState(35)
    def scan(order):
        parts = [np.float32([10 * j, 0, 0]) + rs.uniform(0, 0.2, (n, 3)).astype(np.float32) for j, n in enumerate(order)]
        xyz, comp = np.concatenate(parts), np.repeat(np.arange(len(order)), order)
        perm = rs.permutation(len(xyz))
        return xyz[perm], comp[perm]
    (xa, ca), (xb, cb) = scan([2, 3, 6, 7]), scan([7, 6, 2, 3, 3])
    got, want = _check([xa, xb], min_points=3, max_points=6)
    assert got.inst_ptr.tolist() == [0, 2, 5] and sorted(got.sizes.tolist()[:2]) == [3, 6]
    inst = got.inst.cpu().numpy()
    assert (inst[:18][np.isin(ca, (0, 3))] == -1).all() and (inst[:18][np.isin(ca, (1, 2))] >= 0).all()
    assert (inst[18:][np.isin(cb, (0, 2))] == -1).all() and set(inst[18:][np.isin(cb, (1, 3, 4))]) == {2, 3, 4}
    got, _ = _check([xa, xb], min_points=7, max_points=7)
    assert got.inst_ptr.tolist() == [0, 1, 2]


@pytest.mark.parametrize('p', [2047, 2048, 2049, 524289, 2097153])
def test_pairs_on_a_lattice_at_the_edges_of_the_scan(p):
    """Sizes chosen for the scan of the kept-root flags (8 x 256 = 2048 flags per tile): one tile and its neighbours, one
    element past 256 tiles and one past 1024.  Sites on a 1 m lattice, 1024 to a row; a site holds two points 0.1 m
    apart, every third site a single point; rows in site order, cut at p.  One class, tolerance 0.25 m, min_points 2:
    the flags run 1, 0, 1, 0, 0, ... and instance k is the k-th whole pair, so every table is index arithmetic."""
    i = np.arange(p, dtype=np.int64)
    r = i % 5                                           # rows 0, 1 and 2, 3 of a period are pairs, row 4 stands alone
    site = 3 * (i // 5) + np.array([0, 0, 1, 1, 2])[r]
    xyz = np.stack([(site % 1024).astype(np.float32) + np.where((r == 1) | (r == 3), np.float32(0.1), F0),
                    (site // 1024).astype(np.float32), np.zeros(p, np.float32)], axis=1).astype(np.float32)
    first = np.flatnonzero(((r == 0) | (r == 2)) & (i + 1 < p))
    k = len(first)
    inst = np.full(p, -1, np.int32)
    inst[first] = inst[first + 1] = np.arange(k, dtype=np.int32)
    want = dict(inst=inst, inst_ptr=np.array([0, k], np.int64), cls=np.zeros(k, np.int32),
                member_ptr=2 * np.arange(k + 1, dtype=np.int64),
                members=np.stack([first, first + 1], axis=1).reshape(-1).astype(np.int32),
                bbox=np.concatenate([xyz[first], xyz[first + 1]], axis=1), sizes=np.full(k, 2, np.int64))
    _same(_run([xyz], tolerance=0.25, min_points=2), want)


def test_order_permutation_and_repetition(scene):
    got = _run_scene(scene)
    first = got.members[got.member_ptr[:-1]]
    assert bool((first[1:] > first[:-1]).all())                           # ids ascend with the smallest member row
    assert torch.equal(first, torch.stack([got.members[a:b].min() for a, b in
                                           zip(got.member_ptr[:-1].tolist(), got.member_ptr[1:].tolist())]))
    again = _run_scene(scene)
    for k in KEYS:                                                        # two runs: the same bits
        a, b = _host(getattr(got, k)), _host(getattr(again, k))
        assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a,
                              b.view(np.uint32) if b.dtype == np.float32 else b), k
    # the rows of each scan permuted: the same partition and the same boxes, mapped back through the permutation
    rs = np.random.RandomState(36)
    perms = [rs.permutation(len(x)) for x in scene['scans']]
    moved = _run([x[p] for x, p in zip(scene['scans'], perms)], [l[p] for l, p in zip(scene['labels'], perms)],
                 tolerance=C.SCENE_TOL, min_points=C.SCENE_MIN, max_points=C.SCENE_MAX)
    assert np.array_equal(moved.inst_ptr, got.inst_ptr)
    inst, inst_m, bbox, bbox_m = (_host(v) for v in (got.inst, moved.inst, got.bbox, moved.bbox))
    back = np.empty_like(inst_m)
    off = 0
    for p in perms:
        back[off + p] = inst_m[off:off + len(p)]                          # the moved call's id of every original row
        off += len(p)
    assert np.array_equal(back >= 0, inst >= 0)
    pairs = np.unique(np.stack([inst[inst >= 0], back[inst >= 0]]), axis=1)
    assert pairs.shape[1] == len(got) and len(set(pairs[0])) == len(set(pairs[1])) == len(got)     # a bijection of ids
    assert np.array_equal(bbox[pairs[0]].view(np.uint32), bbox_m[pairs[1]].view(np.uint32))
    assert np.array_equal(_host(got.cls)[pairs[0]], _host(moved.cls)[pairs[1]])


def test_a_live_point_out_of_the_key_range_is_refused():
    xyz = np.random.RandomState(37).uniform(0, 1, (50, 3)).astype(np.float32)
    xyz[17, 1] = 1e9
    lab = np.ones(50, np.int64)
    with pytest.raises(ValueError, match='cell key'):
        _run([xyz], [lab], tolerance=0.5)
    lab[17] = 255                                                         # not live: never an error
    _check([xyz], [lab])
    lab[17] = 2
    _check([xyz], [lab], tolerance={1: 0.5})


def test_scratch_is_what_the_library_says(scene, monkeypatch):
    """Scratch of exactly lidal_euclidean_clusters_workspace_bytes between guards, filled with 0xA5: the guards are
    intact and the result is the reference's (a word of scratch read before it was written would change it)."""
    from lidal_amd import backend as B
    g = Guarded()
    monkeypatch.setattr(B, 'workspace', g)
    got = _run_scene(scene)
    g.check()
    assert [n for _, n in g.bufs] == [B.lib().lidal_euclidean_clusters_workspace_bytes(len(got.inst), 2)]
    _same(got, scene['want'])


# ---- pastes by instance ----------------------------------------------------------------------------------------------------
def _paste_scans():
    """Two scans of blobs (classes 1, 2, 3) on a ground of class 9, with intensities."""
    rs = np.random.RandomState(38)
    out = []
    for s in range(2):
        parts, labs = [np.concatenate([rs.uniform(-30, 30, (300, 2)), np.full((300, 1), -1.7)], axis=1)], [np.full(300, 9)]
        for b in range(9):
            centre = np.concatenate([rs.uniform(-25, 25, 2), [-1.0]])
            n = int(rs.randint(8, 40))
            parts.append(centre + rs.uniform(-0.3, 0.3, (n, 3)))
            labs.append(np.full(n, 1 + b % 3))
        xyz, lab = np.concatenate(parts).astype(np.float32), np.concatenate(labs).astype(np.int64)
        perm = rs.permutation(len(xyz))
        out.append((xyz[perm], rs.uniform(0, 1, len(xyz)).astype(np.float32), lab[perm]))
    return out


def _mix(scans, mixes, **kw):
    from lidal_amd import data
    return data.mix_scans([_g(s[0]) for s in scans], [_g(s[1]) for s in scans], [_g(s[2]) for s in scans], mixes, **kw)


def test_all_true_masks_change_nothing():
    from lidal_amd import data
    scans = _paste_scans()
    mixes = list(data.draw_polarmix(0, 1, np.random.RandomState(5), paste_classes=(1, 3), n_rot=2))
    want = _mix(scans, mixes)
    assert want['parts'][:, 2:4].all()
    for masks in ([torch.ones(len(s[0]), dtype=torch.bool, device=DEV) for s in scans],
                  [None, torch.ones(len(scans[1][0]), dtype=torch.bool, device=DEV)], [None, None]):
        got = _mix(scans, mixes, paste_masks=masks)
        for k in ('points', 'intensity', 'labels', 'src'):
            assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), k
        assert np.array_equal(got['point_ptr'], want['point_ptr']) and np.array_equal(got['parts'], want['parts'])
    with pytest.raises(ValueError):
        _mix(scans, mixes, paste_masks=[None])
    with pytest.raises(ValueError):
        _mix(scans, mixes, paste_masks=[None, torch.ones(3, dtype=torch.bool, device=DEV)])


def test_pastes_hold_the_chosen_instances():
    from lidal_amd import data
    scans = _paste_scans()
    ins = data.euclidean_clusters([_g(s[0]) for s in scans], [_g(s[2]) for s in scans], tolerance={1: 0.5, 2: 0.5, 3: 0.5},
                                  min_points=5)
    ptr = np.array([0, len(scans[0][0]), len(scans[0][0]) + len(scans[1][0])])
    _same(ins, C.clusters_ref(np.concatenate([s[0] for s in scans]), ptr, np.concatenate([s[2] for s in scans]),
                              {1: 0.5, 2: 0.5, 3: 0.5}, 5))
    rs = np.random.RandomState(6)
    masks = [data.draw_instance_paste(ins, s, rs, classes=(1, 3), n_inst=2) for s in range(2)]
    assert all(m.dtype == torch.bool and m.is_cuda and m.any() for m in masks)
    mixes = list(data.draw_polarmix(0, 1, rs, paste_classes=(1, 3), n_rot=2))
    got = _mix(scans, mixes, paste_masks=masks)
    lab = np.concatenate([s[2] for s in scans])
    mask = np.concatenate([m.cpu().numpy() for m in masks])
    want = R.mix_scans(np.concatenate([s[0] for s in scans]), np.concatenate([s[1] for s in scans]),
                       np.where(mask, lab, 255), ptr, mixes)                # the rotation as mix_ref takes it
    assert np.array_equal(got['point_ptr'], want['point_ptr']) and np.array_equal(got['parts'], want['parts'])
    assert np.array_equal(got['points'].cpu().numpy().view(np.uint32), want['points'].view(np.uint32))
    assert np.array_equal(got['intensity'].cpu().numpy().view(np.uint32), want['intensity'].view(np.uint32))
    src = got['src'].cpu().numpy()
    assert np.array_equal(src, want['src'])
    assert np.array_equal(got['labels'].cpu().numpy(), lab[src])              # the labels behind the steering key
    inst = ins.inst.cpu().numpy()
    for j, m in enumerate(mixes):                                           # mix j pastes from scan m.b, twice
        chosen = np.nonzero(mask & (np.arange(len(mask)) >= ptr[m.b]) & (np.arange(len(mask)) < ptr[m.b + 1]))[0]
        assert len(chosen) and len(np.unique(inst[chosen])) == 2 and (inst[chosen] >= 0).all()
        assert np.isin(lab[chosen], (1, 3)).all()
        assert got['parts'][j, 2:].tolist() == [len(chosen), len(chosen), 0, 0]
        at = int(got['point_ptr'][j]) + int(got['parts'][j, :2].sum())
        for k in range(2):
            assert np.array_equal(src[at + k * len(chosen):at + (k + 1) * len(chosen)], chosen)      # in source order


def test_mixed_train_batch_without_masks_is_unchanged():
    from lidal_amd import data
    from test_mix_gpu import _label_inputs, _raycast
    host = _raycast([900, 700], [4, 5])
    pairs = [(_g(p), _g(w)) for p, w in host]
    table, raws, csrs, flags, pseudos = _label_inputs([h[0] for h in host], 26)
    def batch(**kw):
        rs = np.random.RandomState(7)
        mixes = list(data.draw_polarmix(0, 1, rs, paste_classes=(1, 6, 7, 17), n_rot=3))
        return data.mixed_train_batch(pairs, raws, table, mixes, csrs, flags, pseudos, rng=rs, **kw)
    want = batch()
    assert want['parts'][:, 2:5].all()
    ones = [torch.ones(len(h[0]), dtype=torch.bool, device=DEV) for h in host]
    for got in (batch(paste_masks=None), batch(paste_masks=ones)):
        assert set(got) == set(want)
        for k, v in want.items():
            if torch.is_tensor(v):
                assert got[k].dtype == v.dtype and torch.equal(got[k], v), k
            elif isinstance(v, np.ndarray):
                assert np.array_equal(got[k], v), k
