"""Every builder whose scratch has more than one region, run in a buffer of EXACTLY the size its size query returns.

backend.workspace() never hands out less than 16 MiB, and at test shapes these builders ask for about 2 MiB, so a size
query that reports less than its entry point carves would go unseen.  Here the scratch is the middle of a buffer with a
4096-byte guard on either side, all of it filled with 0xA5: after the call the guards must be untouched, and the outputs
must equal, bit for bit, those of the same call in the ordinary workspace -- the scratch arrives full of garbage, so a
builder that relies on a clean buffer fails the comparison too.  And given one byte less than it asked for, every entry
point must refuse ("... too small") before it launches anything.

How the calls are made.  The Python wrappers marshal the operands, so that every pointer is valid and every output is
allocated in full; the library call is the one backend.lib() returns.  For the refusals the size query of the builder
under test answers one byte less (_OneByteShort), so the wrapper allocates and passes exactly that.  FrameBank.grid and
kmeans_single allocate their scratch with torch.empty rather than backend.workspace, so their exact-fit cases call the
entry point with a guarded buffer and compare with the wrapper's results (k-means with 1 local trial is not reachable
through the wrapper at all, which draws 2 + log k of them).

Shapes: n in {1, 33, 65, 1024, 1025} -- the 256-byte rounding of 4-, 8- and 24-byte elements (33 * 8 and 65 * 4 cross a
256-byte line, 1 * 24 does not fill one) and the 1024-element tile of the scans (one block, and one more).  Two builders
have no call with n = 1: knn needs k + 1 points and the core-set needs an unlabeled frame to add; there the n = 1 case
checks what the wrapper does instead (the refusal, num_add = 0) under the same guards.
"""

import numpy as np
import pytest
import torch

import frame_inputs as FI
import geometry_ref as G
import interframe_ref as IR
from guarded_ws import Guarded

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SIZES = [1, 33, 65, 1024, 1025]
K27, K8 = ((3, 3, 3), 1), ((2, 2, 2), 2)          # 27 offsets, symmetric; 8 offsets, strided


def _B():
    from lidal_amd import backend
    return backend


def _g(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _flat(x):
    if torch.is_tensor(x):
        return [x]
    if isinstance(x, (list, tuple)):
        return [t for v in x for t in _flat(v)]
    return [torch.as_tensor(x)]


def _same(got, want):
    got, want = _flat(got), _flat(want)
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
        a, b = a.contiguous().cpu().reshape(-1), b.contiguous().cpu().reshape(-1)
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))       # bit for bit (NaN included)


def _exact(monkeypatch, call):
    """call() in the ordinary workspace, then in guarded scratch of exactly the requested size."""
    want = call()
    torch.cuda.synchronize()
    g = Guarded()
    monkeypatch.setattr(_B(), 'workspace', g)
    got = call()
    g.check()
    _same(got, want)


class _OneByteShort:
    """backend.lib() whose size queries `names` answer one byte less than the library does."""

    def __init__(self, handle, names):
        self._handle, self._names = handle, names

    def __getattr__(self, name):
        fn = getattr(self._handle, name)
        if name in self._names:
            return lambda *a: fn(*a) - 1
        return fn


def _refused(monkeypatch, size_query, call):
    B = _B()
    short = _OneByteShort(B.lib_handle(), (size_query,))
    g = Guarded()
    monkeypatch.setattr(B, 'workspace', g)
    monkeypatch.setattr(B, 'lib', lambda: short)
    with pytest.raises(RuntimeError, match='too small'):
        call()
    assert 'too small' in B.lib_handle().lidal_last_error().decode()
    if g.bufs:
        g.check()
    torch.cuda.synchronize()


# ---------------------------------------------------------------- inputs (seeded; shared, read only)
def _keys(n):
    k = np.random.default_rng(n).integers(0, G.INT64_MAX, size=n, dtype=np.int64)
    k[n // 2:] = k[:n - n // 2]                                   # duplicates
    return k


def _coords(n):
    return G.sheet_rows(n, 1, seed=n, batch=n % 3)


def _points(n, frame=0):
    """f64 [n, 3]; the frames of one n are the same cloud moved by a few centimetres (inter-frame matches exist)."""
    base = np.random.RandomState(100 + n).uniform(-4.0, 4.0, size=(n, 3))
    return base if frame == 0 else base + np.random.RandomState(frame).normal(0.0, 0.03, size=(n, 3))


def _kmap(n, shape):
    conv = _conv()
    ks, st = shape
    with torch.enable_grad():
        km, oc = conv.build_kernel_map(_g(_coords(n)), (1, 1, 1), ks, (st,) * 3)
    return km, oc


def _conv():
    from lidal_amd.nn.functional import conv
    return conv


def _F():
    from lidal_amd.nn import functional as F
    return F


def _map_outputs(km, oc):
    return [oc, km.nbr_out, km.nbsizes, km.koff, km.nbmaps]


def _order_outputs(o):
    n = o.n_rows
    return [o.perm[:n], o.table, o.tile_masks[:-(-n // 128)]]


# ---------------------------------------------------------------- kmap.hip
def _unique(n):
    return lambda: _F().unique_sorted(_g(_keys(n)))


def _downsample(n):
    return lambda: _F().spdownsample(_g(_coords(n)), 2, 2, 1)


def _pyramid(n, levels):
    return lambda: _F().downsample_pyramid(_g(_coords(n)), levels, 1)


def _build_map(n, shape, grad):
    def call():
        ks, st = shape
        with torch.set_grad_enabled(grad):
            km, oc = _conv().build_kernel_map(_g(_coords(n)), (1, 1, 1), ks, (st,) * 3)
        return _map_outputs(km, oc)           # (under no_grad the rule lists are built here, by a second call)
    return call


def _build_maps(n, grad):
    """Four jobs of both volumes, the second without rows."""
    def call():
        jobs = []
        for rows, (ks, st) in ((n, K27), (0, K27), (n, K8), (65, K8)):
            c = _coords(rows)
            oc = c if st == 1 else G.downsample(c, (st,) * 3)
            jobs.append((_g(c), (1, 1, 1), ks, (st,) * 3, _g(oc)))
        with torch.set_grad_enabled(grad):
            maps = _conv().build_kernel_maps(jobs, {})
        return [_map_outputs(km, job[4]) for km, job in zip(maps, jobs)]
    return call


def _order(n, shape):
    km, _ = _kmap(n, shape)
    return lambda: _order_outputs(_conv().RowOrder(km.nbr_out))


def _order_many(n, shape):
    """Three tables of one volume through one sort, the second without rows."""
    tabs = [_kmap(n, shape)[0].nbr_out, _kmap(0, shape)[0].nbr_out, _kmap(65, shape)[0].nbr_out]
    return lambda: [_order_outputs(o) for o in _conv().RowOrder.build_many(tabs)]


def _voxelize(n):
    def call():
        from lidal_amd import data
        pts = _points(n).astype(np.float32)
        inten = np.random.RandomState(n).uniform(0, 1, size=n).astype(np.float32)
        return list(data.voxelize_scan(_g(pts), _g(inten), np.eye(3), np.full(6, 0.5)))
    return call


@pytest.mark.parametrize('n', SIZES)
def test_unique_sorted_in_exact_scratch(monkeypatch, n):
    _exact(monkeypatch, _unique(n))


@pytest.mark.parametrize('n', SIZES)
def test_spdownsample_in_exact_scratch(monkeypatch, n):
    _exact(monkeypatch, _downsample(n))


@pytest.mark.parametrize('levels', [1, 4])
@pytest.mark.parametrize('n', SIZES)
def test_downsample_pyramid_in_exact_scratch(monkeypatch, n, levels):
    _exact(monkeypatch, _pyramid(n, levels))


@pytest.mark.parametrize('grad', [True, False])
@pytest.mark.parametrize('shape', [K27, K8], ids=['k27', 'k8'])
@pytest.mark.parametrize('n', SIZES)
def test_kernel_map_in_exact_scratch(monkeypatch, n, shape, grad):
    _exact(monkeypatch, _build_map(n, shape, grad))


@pytest.mark.parametrize('grad', [True, False])
@pytest.mark.parametrize('n', SIZES)
def test_batched_kernel_maps_in_exact_scratch(monkeypatch, n, grad):
    _exact(monkeypatch, _build_maps(n, grad))


@pytest.mark.parametrize('shape', [K27, K8], ids=['k27', 'k8'])
@pytest.mark.parametrize('n', SIZES)
def test_row_order_in_exact_scratch(monkeypatch, n, shape):
    _exact(monkeypatch, _order(n, shape))


@pytest.mark.parametrize('shape', [K27, K8], ids=['k27', 'k8'])
@pytest.mark.parametrize('n', SIZES)
def test_batched_row_orders_in_exact_scratch(monkeypatch, n, shape):
    _exact(monkeypatch, _order_many(n, shape))


@pytest.mark.parametrize('n', SIZES)
def test_voxelize_scan_in_exact_scratch(monkeypatch, n):
    _exact(monkeypatch, _voxelize(n))


# ---------------------------------------------------------------- voxel.hip
def _invlist(n):
    def call():
        from lidal_amd.nn.functional.invlist import inverse_lists
        m = n // 3 + 1
        idx = _g(np.random.RandomState(n).randint(0, m, size=n).astype(np.int32))
        return list(inverse_lists(idx, m))
    return call


@pytest.mark.parametrize('n', SIZES)
def test_inverse_lists_in_exact_scratch(monkeypatch, n):
    _exact(monkeypatch, _invlist(n))


# ---------------------------------------------------------------- score.hip
def _grid_by_wrapper(n):
    from lidal_amd.score.interframe import FrameBank
    bank = FrameBank(dis_thresh=0.1)
    bank.add(_g(_points(n)), _g(IR.softmax_rows(np.random.RandomState(n), n, 19)))
    return bank.grid(0)


@pytest.mark.parametrize('n', SIZES)
def test_neighbour_grid_in_exact_scratch(n):
    from lidal_amd.score.interframe import FrameBank
    B = _B()
    want = _grid_by_wrapper(n)
    pts = _g(_points(n))
    nbytes = B.lib().lidal_nn_grid_bytes(n)
    ws_bytes = B.lib().lidal_nn_grid_workspace_bytes(n)
    assert want.numel() == nbytes
    g = Guarded()
    grid, ws = g(nbytes), g(ws_bytes)                             # (the grid buffer is guarded too: it is carved as well)
    B.check(B.lib().lidal_nn_grid_build(B.ptr(pts), n, FrameBank.CELL * 0.1, B.ptr(grid), nbytes, B.ptr(ws), ws_bytes,
                                        B.stream()), 'nn_grid_build')
    g.check()
    # what a query reads: the header, the slots and their values, the occupancy bits, the sorted keys / ids / points.
    # Bytes the build never writes (padding between the regions) keep whatever the allocation held, so the two
    # buffers are compared through a query rather than byte for byte.
    _same(_score_with_grid(n, grid), _score_with_grid(n, want))


def _score_with_grid(n, grid):
    from lidal_amd.score.interframe import FrameBank, score_points
    rs = np.random.RandomState(n)
    bank = FrameBank(dis_thresh=0.1)
    bank.add(_g(_points(n, 1)), _g(IR.softmax_rows(rs, n, 19)))
    bank.add(_g(_points(n)), _g(IR.softmax_rows(rs, n, 19)))
    bank.add(_g(_points(n, 2)), _g(IR.softmax_rows(rs, n, 19)))
    bank._grid[1] = grid
    return list(score_points(bank, 0, nei_num=2))


# ---------------------------------------------------------------- redal.hip
def _knn(n, what):
    def call():
        from lidal_amd.score import knn, surface_variation
        xyz = _g(_points(n).astype(np.float32))
        return knn(xyz, 4) if what == 'knn' else surface_variation(xyz, k=4)
    return call


@pytest.mark.parametrize('what', ['knn', 'surface_variation'])
@pytest.mark.parametrize('n', SIZES)
def test_knn_in_exact_scratch(monkeypatch, n, what):
    if n == 1:                # no valid call: one point has no neighbour.  The refusal, under the same guards
        g = Guarded()
        monkeypatch.setattr(_B(), 'workspace', g)
        with pytest.raises(RuntimeError, match='need at least k \\+ 1'):
            _knn(n, what)()
        g.check()
        return
    _exact(monkeypatch, _knn(n, what))


def _kmeans_direct(x, k, first, u, trials, ws, ws_bytes, max_iter=5):
    B = _B()
    n, d = x.shape
    seeds = torch.empty(k, dtype=torch.int32, device=DEV)
    labels = torch.empty(n, dtype=torch.int32, device=DEV)
    centers = torch.empty((k, d), dtype=torch.float64, device=DEV)
    inertia, n_iter = np.zeros(1, dtype=np.float64), np.zeros(1, dtype=np.int32)
    rc = B.lib().lidal_kmeans(B.ptr(x), n, d, k, first, B.ptr(u), trials, max_iter, 0.0, B.ptr(seeds), B.ptr(labels),
                              B.ptr(centers), inertia.ctypes.data, n_iter.ctypes.data, B.ptr(ws), ws_bytes, B.stream())
    torch.cuda.synchronize()
    return rc, [labels, centers, seeds, torch.from_numpy(inertia.copy()), torch.from_numpy(n_iter.copy())]


@pytest.mark.parametrize('trials', [1, 3])
@pytest.mark.parametrize('n', [256, 257])
def test_kmeans_in_exact_scratch(n, trials):
    """n = 256 | 257: one chunk of the potential scan, and one more; 1 and 3 local trials."""
    B = _B()
    d, k = 8, 4
    rs = np.random.RandomState(n + trials)
    x = _g((rs.normal(size=(n, d)) + 3.0 * rs.randint(0, k, size=(n, 1))).astype(np.float32))
    u = _g(rs.random_sample((k - 1) * trials))
    nbytes = B.lib().lidal_kmeans_workspace_bytes(n, d, k, trials)
    roomy = torch.zeros(nbytes + (1 << 20), dtype=torch.uint8, device=DEV)
    rc, want = _kmeans_direct(x, k, 7, u, trials, roomy, roomy.numel())
    B.check(rc, 'kmeans')
    g = Guarded()
    rc, got = _kmeans_direct(x, k, 7, u, trials, g(nbytes), nbytes)
    B.check(rc, 'kmeans')
    g.check()
    _same(got, want)
    rc, _ = _kmeans_direct(x, k, 7, u, trials, g(nbytes), nbytes - 1)
    assert rc != 0 and 'too small' in B.lib().lidal_last_error().decode()
    g.check()


def test_kmeans_wrapper_agrees_with_the_direct_call():
    from lidal_amd.score.redal import kmeans_draws, kmeans_single
    B = _B()
    n, d, k = 257, 8, 4
    rs = np.random.RandomState(5)
    x = _g((rs.normal(size=(n, d)) + 3.0 * rs.randint(0, k, size=(n, 1))).astype(np.float32))
    first, u, trials = kmeans_draws(n, k, 9)
    assert trials == 3
    labels, centers, inertia, n_iter, seeds = kmeans_single(x, k, 9, max_iter=5)
    nbytes = B.lib().lidal_kmeans_workspace_bytes(n, d, k, trials)
    g = Guarded()
    rc, got = _kmeans_direct(x, k, first, _g(u.reshape(-1)), trials, g(nbytes), nbytes)
    B.check(rc, 'kmeans')
    g.check()
    _same(got[:3], [labels, centers, seeds])
    assert float(got[3][0]) == inertia and int(got[4][0]) == n_iter


# ---------------------------------------------------------------- frame_level.hip
def _uncertainty(n):
    def call():
        from lidal_amd.score.frame_level import frame_uncertainty
        return list(frame_uncertainty(_g(FI._prob(np.random.RandomState(n), n, 19))))
    return call


def _coreset(n, num_add):
    def call():
        from lidal_amd.score.frame_level import coreset
        flags = np.zeros(n, dtype=bool)
        flags[::11] = True                                        # 1, 3, 6, 94, 94 labeled frames
        picks, out, md = coreset(_g(FI.large_feats(n, seed=n)), flags, num_add, return_min_dist=True)
        return [picks, torch.from_numpy(out), md]
    return call


@pytest.mark.parametrize('n', SIZES)
def test_frame_uncertainty_in_exact_scratch(monkeypatch, n):
    _exact(monkeypatch, _uncertainty(n))


@pytest.mark.parametrize('num_add', [1, 5])
@pytest.mark.parametrize('n', SIZES)
def test_coreset_in_exact_scratch(monkeypatch, n, num_add):
    _exact(monkeypatch, _coreset(n, 0 if n == 1 else num_add))    # one frame, labeled: nothing can be added


# ---------------------------------------------------------------- one byte short
REFUSALS = {
    'unique': ('lidal_unique_workspace_bytes', lambda: _unique(65)),
    'downsample': ('lidal_downsample_workspace_bytes', lambda: _downsample(65)),
    'downsample_pyramid': ('lidal_downsample_pyramid_workspace_bytes', lambda: _pyramid(65, 4)),
    'kmap_build': ('lidal_kmap_workspace_bytes', lambda: _build_map(65, K27, True)),
    'kmap_build_table_only': ('lidal_kmap_workspace_bytes', lambda: _build_map(65, K27, False)),
    'kmap_build_batch': ('lidal_kmap_build_batch_workspace_bytes', lambda: _build_maps(65, True)),
    'kmap_order': ('lidal_kmap_order_workspace_bytes', lambda: _order(65, K27)),
    'kmap_order_batch': ('lidal_kmap_order_workspace_bytes', lambda: _order_many(65, K8)),
    'voxelize_points': ('lidal_voxelize_points_workspace_bytes', lambda: _voxelize(65)),
    'invlist_build': ('lidal_invlist_workspace_bytes', lambda: _invlist(65)),
    'nn_grid_build': ('lidal_nn_grid_workspace_bytes', lambda: (lambda: _grid_by_wrapper(65))),
    'knn': ('lidal_knn_workspace_bytes', lambda: _knn(65, 'knn')),
    'surface_variation': ('lidal_knn_workspace_bytes', lambda: _knn(65, 'surface_variation')),
    'frame_uncertainty': ('lidal_frame_uncertainty_workspace_bytes', lambda: _uncertainty(65)),
    'coreset': ('lidal_coreset_workspace_bytes', lambda: _coreset(65, 5)),
}


@pytest.mark.parametrize('builder', sorted(REFUSALS))
def test_one_byte_less_is_refused(monkeypatch, builder):
    """(k-means: test_kmeans_in_exact_scratch.)  'kmap_build' is the call that makes table and rule lists at once,
    'kmap_build_table_only' the one build_kernel_map makes under no_grad."""
    size_query, make = REFUSALS[builder]
    call = make()                                                 # (inputs that need a build of their own: made unpatched)
    _refused(monkeypatch, size_query, call)
