"""The ReDAL kernels (csrc/redal.hip) at their edges, against plain numpy restatements (tests/redal_ref.py):
region scores of supervoxels past numpy's 8192-value reduce blocks, empty supervoxels and unusual widths; the
k-nearest-neighbour list bit for bit against brute force on ties, duplicates, tail blocks, outliers and every cell size;
surface variation against f64 eigenvalues on degenerate neighbourhoods; k-means seeds, labels, centres, n_iter and
inertia over a grid of widths, sizes and cluster counts, and with a tolerance.  All inputs come from fixed seeds."""
import warnings

import numpy as np
import pytest
import torch

import redal_inputs as RI
import redal_ref

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SCORE_ULPS = 4          # as test_redal_gpu.py: the one step not restated is numpy's f32 log2
SIZES = (1, 7, 8, 9, 127, 128, 129, 1254, 8191, 8192, 8193, 16384, 16385, 100000)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _csr(groups):
    ptr = np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.int64)
    idx = np.concatenate([np.asarray(g, np.int64) for g in groups]) if groups else np.zeros(0, np.int64)
    return _t(ptr), _t(idx)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ------------------------------------------------------------------------------------------------ region scores
def test_region_scores_bit_exact_past_numpy_reduce_blocks():
    """One class with prob = 1 makes every point score f32(gamma) * curvature exactly (log2(1 + 1e-12f) = 0), so the
    supervoxel mean is pinned bit for bit: numpy's pairwise trees over blocks of 8192, added in order.  Four supervoxels
    of every size in SIZES, listed in a shuffled order, drawing shared point ids in permuted order.  (One tree over the
    whole supervoxel gives other bits at 8193, 16385 and 100000 here; 16384 splits into the same two trees.)"""
    from lidal_amd.score import region_scores
    rs = np.random.RandomState(11)
    p = 120000
    curv = rs.uniform(1e-3, 0.1, p).astype(np.float32)              # in (0, 0.1]: no signed zero anywhere
    feat = rs.normal(size=(p, 8)).astype(np.float32)
    sizes = [m for m in SIZES for _ in range(4)]
    groups = [rs.permutation(p)[:sizes[j]] for j in rs.permutation(len(sizes))]
    ptr, idx = _csr(groups)
    sc, ft, pn = region_scores(_t(np.ones((p, 1), np.float32)), _t(feat), _t(curv), ptr, idx, alpha=1.0, gamma=0.05)
    sc, ft, pn = sc.cpu().numpy(), ft.cpu().numpy(), pn.cpu().numpy()
    ps = np.float32(0.05) * curv
    bad = []
    for j, g in enumerate(groups):
        want = ps[g].mean()
        assert redal_ref.np_mean_f32(ps[g]) == want
        if _bits(sc[j]) != _bits(want):
            bad.append((len(g), sc[j], want))
        assert np.array_equal(_bits(ft[j]), _bits(feat[g].mean(0))), len(g)
        assert pn[j] == len(g)
    assert not bad, sorted(bad)


def _worker_func(prob, feat, curv, groups, alpha=1.0, gamma=0.05):
    uncertain = np.mean(-prob * np.log2(prob + 1e-12), axis=1)
    ps = alpha * uncertain + gamma * curv
    sc = np.array([ps[g].mean() for g in groups], np.float32)
    ft = np.stack([feat[g].mean(0) for g in groups]).astype(np.float32)
    return sc, ft, np.array([len(g) for g in groups])


@pytest.mark.parametrize('c', [1, 19, 32])
def test_region_scores_classes_and_widths_match_worker_func(c):
    """C in {1, 19, 32} (the class sum's leaf with and without a tail), d in {1, 96, 129, 300} (d = 1 is reduced by
    numpy as a contiguous column; d > 128 takes the lane loop); prob with exact 0s and 1s."""
    from lidal_amd.score import region_scores
    rs = np.random.RandomState(20 + c)
    p = 9000
    logit = rs.normal(0, 2, size=(p, c))
    prob = (np.exp(logit) / np.exp(logit).sum(1, keepdims=True)).astype(np.float32)
    hot = rs.randint(0, p, size=p // 5)
    prob[hot] = 0.0
    prob[hot, rs.randint(0, c, size=hot.size)] = 1.0
    curv = rs.uniform(0, 0.1, p).astype(np.float32)
    groups = [rs.permutation(p)[:m] for m in (1, 9, 200, 1254, 8193, 3)]
    ptr, idx = _csr(groups)
    for d in (1, 96, 129, 300):
        feat = rs.normal(size=(p, d)).astype(np.float32)
        sc, ft, pn = region_scores(_t(prob), _t(feat), _t(curv), ptr, idx)
        r_sc, r_ft, r_pn = _worker_func(prob, feat, curv, groups)
        assert np.array_equal(pn.cpu().numpy(), r_pn)
        assert np.array_equal(_bits(ft.cpu().numpy()), _bits(r_ft)), d
        ulps = np.abs(_bits(sc.cpu().numpy()).astype(np.int64) - _bits(r_sc).astype(np.int64))
        assert ulps.max() <= SCORE_ULPS, (d, ulps)


def test_region_scores_empty_supervoxels_and_refusals():
    from lidal_amd.score import region_scores
    rs = np.random.RandomState(31)
    p, c, d = 50, 19, 4
    prob = rs.dirichlet(np.ones(c), size=p).astype(np.float32)
    feat = rs.normal(size=(p, d)).astype(np.float32)
    curv = rs.uniform(0, 0.1, p).astype(np.float32)
    groups = [np.arange(5), np.zeros(0, np.int64), np.array([7, 3, 9]), np.zeros(0, np.int64)]
    sc, ft, pn = (t.cpu().numpy() for t in region_scores(_t(prob), _t(feat), _t(curv), *_csr(groups)))
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)          # numpy's "Mean of empty slice"
        r_sc, r_ft, r_pn = _worker_func(prob, feat, curv, groups)
    assert np.array_equal(pn, r_pn) and pn[1] == pn[3] == 0
    assert np.isnan(sc[[1, 3]]).all() and np.isnan(ft[[1, 3]]).all()         # numpy's mean of nothing
    assert np.array_equal(_bits(ft[[0, 2]]), _bits(r_ft[[0, 2]]))
    assert not np.isnan(sc[[0, 2]]).any()
    # no points at all, only empty supervoxels
    sc, ft, pn = region_scores(_t(np.zeros((0, c), np.float32)), _t(np.zeros((0, d), np.float32)),
                               _t(np.zeros(0, np.float32)), *_csr([np.zeros(0, np.int64)] * 3))
    assert np.isnan(sc.cpu().numpy()).all() and np.isnan(ft.cpu().numpy()).all() and (pn.cpu().numpy() == 0).all()
    ptr, idx = _csr([np.arange(5)])
    prob33 = rs.dirichlet(np.ones(33), size=p).astype(np.float32)
    with pytest.raises(RuntimeError, match='classes'):
        region_scores(_t(prob33), _t(feat), _t(curv), ptr, idx)
    with pytest.raises(RuntimeError, match='feature width'):
        region_scores(_t(prob), _t(np.zeros((p, 0), np.float32)), _t(curv), ptr, idx)


# ------------------------------------------------------------------------------------------------ knn
_KNN_QUERIES = [0]


def _check_knn(xyz, k, cell=0.5, want=None):
    from lidal_amd.score import knn
    got = knn(_t(xyz.astype(np.float32)), k, cell=cell).cpu().numpy()
    if want is None:
        want = redal_ref.knn_brute(xyz, k)
    bad = np.flatnonzero((got != want).any(1))
    assert bad.size == 0, (k, cell, bad[:5], got[bad[:1]], want[bad[:1]])
    _KNN_QUERIES[0] += len(xyz)
    return got


def _lattice(rs, n=16, h=0.25):
    g = (np.arange(n) - n // 2) * h
    lat = np.stack(np.meshgrid(g, g, g, indexing='ij'), -1).reshape(-1, 3)
    return lat[rs.permutation(len(lat))].astype(np.float32)


def test_knn_lattice_ties_cell_faces_and_negative_coordinates():
    """A 0.25 lattice centred on the origin at cell 0.5: every distance ties many times, half the points lie on cell
    faces, half the coordinates are negative.  The same lattice moved by +1e4 (still exact in f32)."""
    rs = np.random.RandomState(41)
    lat = _lattice(rs)
    for k in (50, 64):
        _check_knn(lat, k)
    _check_knn(lat + np.float32(1e4), 50)


def test_knn_coincident_block_in_a_cloud():
    """70 copies of one point (more than k at distance 0) among 4000 random points, at shuffled indices."""
    rs = np.random.RandomState(42)
    cloud = rs.uniform(-5, 5, size=(4000, 3)).astype(np.float32)
    xyz = np.concatenate([cloud, np.repeat(cloud[17:18], 70, axis=0)])
    xyz = xyz[rs.permutation(len(xyz))]
    for k in (50, 64):
        _check_knn(xyz, k)


@pytest.mark.parametrize('k', [1, 2, 50, 64])
def test_knn_sizes_and_tail_blocks(k):
    """P = k + 1 (every other point is a neighbour), 65 and 4097 (a tail workgroup of one query)."""
    rs = np.random.RandomState(43 + k)
    for p in sorted({k + 1, 65, 4097}):
        _check_knn(rs.normal(0, 2, size=(p, 3)).astype(np.float32), k)


def _scan_with_outliers(rs):
    ground = np.c_[rs.uniform(-15, 15, size=(5000, 2)), rs.normal(-1.7, 0.03, 5000)]
    blobs = np.concatenate([rs.normal(c, 0.4, size=(600, 3)) for c in ([4, 2, 0], [-6, -3, 0.5], [1, -8, -0.5])])
    ang = rs.uniform(0, 2 * np.pi, 5)
    r = rs.uniform(20, 40, 5)
    far = np.c_[15 * np.sign(np.cos(ang)) + r * np.cos(ang), r * np.sin(ang), rs.uniform(-3, 3, 5)]
    xyz = np.concatenate([ground, blobs, far]).astype(np.float32)
    return xyz[rs.permutation(len(xyz))]


def test_knn_outliers_and_every_cell_size_give_one_list():
    """A clustered scan with five outliers 20-40 m away: the list is the brute-force list at cell 0.1, 0.5, 3 and 1000
    (one cell holds the whole scan), so it does not depend on the cell."""
    rs = np.random.RandomState(44)
    xyz = _scan_with_outliers(rs)
    want = redal_ref.knn_brute(xyz, 50)
    lists = [_check_knn(xyz, 50, cell, want) for cell in (0.1, 0.5, 3.0, 1000.0)]
    for other in lists[1:]:
        assert np.array_equal(lists[0], other)
    print('knn: %d queries compared bit for bit with brute force' % _KNN_QUERIES[0])


def test_knn_refusals():
    from lidal_amd.score import knn, surface_variation
    xyz = torch.rand(100, 3, device=DEV)
    for k in (0, 65):
        with pytest.raises(RuntimeError, match='k must be in'):
            knn(xyz, k)
    for bad in (float('nan'), float('inf')):
        pts = np.random.RandomState(45).uniform(0, 1, size=(100, 3)).astype(np.float32)
        pts[37, 1] = bad
        for f in (lambda a: knn(a, 10), lambda a: surface_variation(a)):
            with pytest.raises(ValueError, match='finite'):
                f(pts)
            with pytest.raises(ValueError, match='finite'):
                f(_t(pts))


def test_knn_refuses_points_outside_the_search_grid():
    """A finite coordinate beyond 2^20 cells: the grid build parks it where no query looks (csrc/grid.h), so the wrapper
    refuses it instead of returning lists that silently lack it."""
    from lidal_amd.score import knn, surface_variation
    pts = np.random.RandomState(46).uniform(0, 1, size=(100, 3)).astype(np.float32)
    far = pts.copy()
    far[37, 2] = -6e5                                   # 1.2e6 cells of 0.5
    for f in (lambda a: knn(a, 10), lambda a: surface_variation(a), lambda a: knn(a, 10, cell=0.5)):
        with pytest.raises(ValueError, match='outside the search grid'):
            f(_t(far))
    assert np.array_equal(knn(_t(pts), 10).cpu().numpy(), redal_ref.knn_brute(pts, 10))      # a valid call after the refusals


# ------------------------------------------------------------------------------------------------ surface variation
def _sigma(xyz, k=50, threshold=0.1):
    from lidal_amd.score import surface_variation
    return surface_variation(_t(xyz.astype(np.float32)), k=k, threshold=threshold).cpu().numpy()


def _sigma_ref(xyz, k=50):
    from lidal_amd.score import knn
    nb = knn(_t(xyz.astype(np.float32)), k).cpu().numpy()
    return redal_ref.surface_variation_f64(xyz, nb)


def test_surface_variation_random_clouds_against_f64_eigenvalues():
    rs = np.random.RandomState(51)
    for xyz in (rs.normal(0, 1, size=(3000, 3)), rs.normal(0, 1, size=(3000, 3)) * [5.0, 2.0, 0.05],
                _scan_with_outliers(rs)):
        xyz = xyz.astype(np.float32)
        raw = _sigma(xyz, threshold=None)
        ref = _sigma_ref(xyz)
        err = np.abs(raw.astype(np.float64) - ref)
        print('surface variation, random cloud: max |d sigma| %.3g' % err.max())
        assert err.max() <= 1e-6
        assert np.array_equal(_sigma(xyz), np.minimum(raw, np.float32(0.1)))


def test_surface_variation_degenerate_neighbourhoods():
    rs = np.random.RandomState(52)
    # on a line along an axis: lambda_min is exactly 0
    line = np.zeros((300, 3), np.float32)
    line[:, 1] = rs.uniform(-20, 20, 300)
    s = _sigma(line, threshold=None)
    print('surface variation, line: max |sigma| %.3g' % np.abs(s).max())
    assert (s == 0).all()
    # a tilted plane
    uv = rs.uniform(-3, 3, size=(2000, 2))
    plane = np.c_[uv, 0.3 * uv[:, 0] - 0.2 * uv[:, 1] + 1.0].astype(np.float32)
    s = _sigma(plane, threshold=None).astype(np.float64)
    err = np.abs(s - _sigma_ref(plane))
    print('surface variation, tilted plane: max sigma %.3g, max |d sigma| %.3g' % (s.max(), err.max()))
    assert s.max() <= 1e-9 and err.max() <= 1e-9
    # isotropic: the 32 nearest lattice points of an interior point are the closed shells at 1, sqrt 2, sqrt 3 and 2
    g = np.arange(-4, 5)
    cube = np.stack(np.meshgrid(g, g, g, indexing='ij'), -1).reshape(-1, 3).astype(np.float32)
    inner = (np.abs(cube) <= 2).all(1)
    s = _sigma(cube, k=32, threshold=None)
    ref = _sigma_ref(cube, k=32)
    print('surface variation, isotropic: max |d sigma| %.3g (the f32 rounding of 1/3)'
          % np.abs(s[inner] - ref[inner]).max())
    assert np.abs(ref[inner] - 1 / 3).max() <= 1e-12
    assert (s[inner] == np.float32(1 / 3)).all()
    assert (_sigma(cube, k=32)[inner] == np.float32(0.1)).all()
    # k neighbours that all coincide: 0 / 0, which passes the clip
    dup = np.concatenate([np.repeat([[1.5, -2.0, 0.25]], 60, axis=0), rs.uniform(5, 9, size=(200, 3))])
    dup = dup[rs.permutation(len(dup))].astype(np.float32)
    copies = (dup == np.float32([1.5, -2.0, 0.25])).all(1)
    for thr in (None, 0.1):
        s = _sigma(dup, threshold=thr)
        assert np.isnan(s[copies]).all() and not np.isnan(s[~copies]).any()


def _jacobi_cases():
    """(name, xyz, k): the least k on k + 1 points, one full workgroup's worth short of one, a second, partial 64-lane
    workgroup, distance ties, and neighbours that all coincide (0 / 0)."""
    rs = np.random.RandomState(53)
    g = np.arange(3.0)
    return [('k3_on_4', rs.normal(0, 1, size=(4, 3)), 3), ('k8_on_9', rs.normal(0, 1, size=(9, 3)), 8),
            ('70_random', rs.normal(0, 2, size=(70, 3)) * [3.0, 1.0, 0.2], 8),
            ('lattice_3x3x3', np.stack(np.meshgrid(g, g, g, indexing='ij'), -1).reshape(-1, 3) * 0.25, 8),
            ('5_coincident', np.repeat([[1.5, -2.0, 0.25]], 5, axis=0), 4)]


@pytest.mark.parametrize('case', _jacobi_cases(), ids=lambda c: c[0])
def test_surface_variation_equals_the_jacobi_restatement_bit_for_bit(case):
    """The sweep that redal.hip and vccs.hip share (csrc/sym3.h), pinned on this side too: sigma equals, bit for bit,
    the restatement that sums mean and covariance in neighbour order and runs the numpy Jacobi the VCCS normals are
    checked with (tests/jacobi_ref.py), unclipped and clipped at 0.1.  NaN compares as NaN.  (On these inputs the
    restatement agrees with LAPACK's f64 eigenvalues, redal_ref.surface_variation_f64, to 5.3e-9, the f32 rounding of
    its result: far inside the 1e-6 of test_surface_variation_random_clouds_against_f64_eigenvalues.)"""
    from lidal_amd.score import knn
    name, xyz, k = case
    xyz = xyz.astype(np.float32)
    nb = knn(_t(xyz), k).cpu().numpy()
    assert np.array_equal(nb, redal_ref.knn_brute(xyz, k))
    for thr in (None, 0.1):
        got = _sigma(xyz, k=k, threshold=thr)
        want = redal_ref.surface_variation_jacobi(xyz, nb, threshold=thr)
        nan = np.isnan(want)
        print('%s, threshold %s: %d values, %d NaN, %d differ' % (name, thr, len(want), nan.sum(),
                                                                 (_bits(got)[~nan] != _bits(want)[~nan]).sum()))
        assert np.array_equal(np.isnan(got), nan)
        assert np.array_equal(_bits(got)[~nan], _bits(want)[~nan])
    assert nan.all() == (name == '5_coincident')


# ------------------------------------------------------------------------------------------------ k-means
def _km_data(n, d, seed):
    """Normal rows, the last third copies of rows of the first third: clusters seeded on a repeated row are empty."""
    rs = np.random.RandomState(seed)
    x = rs.normal(size=(n, d)).astype(np.float32)
    x[n - n // 3:] = x[rs.randint(0, n // 3, size=n // 3)]
    return x


def test_kmeans_grid_bit_exact_with_inertia():
    """Seeds, labels, centres, n_iter and inertia equal the restatement bit for bit for d in {1, 7, 8, 9, 96, 127, 128}
    (km_d2's short, tail and full paths), n around the 256-row chunk borders, k in {1, 2, 3, n} and max_iter in
    {0, 1, 300}.  At k = n the repeated rows leave many clusters empty in one iteration."""
    from lidal_amd.score.redal import kmeans_single
    cases, most_empty = 0, 0
    for d in (1, 7, 8, 9, 96, 127, 128):
        for n in (255, 256, 257, 769):
            x = _km_data(n, d, 1000 * n + d)
            x64 = x.astype(np.float64)
            xd = _t(x)
            for k in (1, 2, 3, n):
                s = 17 + k
                seeds = redal_ref.seed(x, k, s)
                lab0, _ = redal_ref.assign(x64, x64[seeds])
                most_empty = max(most_empty, int((np.bincount(lab0, minlength=k) == 0).sum()))
                for max_iter in (0, 1, 300):
                    labels, centers, inertia, n_iter, dseeds = kmeans_single(xd, k, s, max_iter=max_iter, tol=0.0)
                    r_labels, r_centers, r_it, r_inertia = redal_ref.lloyd(x, seeds, max_iter)
                    what = (d, n, k, max_iter)
                    assert np.array_equal(dseeds.cpu().numpy(), seeds), what
                    assert np.array_equal(labels.cpu().numpy(), r_labels), what
                    assert np.array_equal(centers.cpu().numpy(), r_centers), what
                    assert n_iter == r_it, (what, n_iter, r_it)
                    assert inertia == r_inertia, (what, inertia, r_inertia)
                    cases += 1
    print('kmeans grid: %d runs bit-equal, up to %d empty clusters in the first assignment' % (cases, most_empty))
    assert most_empty >= 2


def test_kmeans_with_tolerance_restarts_equal_restatement():
    """kmeans()'s ten restart seeds at tol = 1e-4 * mean variance, the same absolute tol on both sides: every restart
    and the winner match the restatement (the shift is restated in the device's lane-and-tree order).  Clusters of
    ~1600 rows make the shift of a few relabelled rows fall below tol, so the tolerance ends the runs."""
    from lidal_amd.score import kmeans
    from lidal_amd.score.redal import kmeans_single
    x = np.ascontiguousarray(RI.overlapping()[:, :8])
    xd = _t(x)
    k = 5
    tol = float(np.var(x.astype(np.float64), axis=0).mean()) * 1e-4
    restarts = np.random.RandomState(0).randint(2 ** 31 - 1, size=10)
    results = []
    for s in restarts:
        labels, centers, inertia, n_iter, seeds = kmeans_single(xd, k, int(s), tol=tol)
        r_labels, r_centers, r_it, r_seeds, r_inertia = redal_ref.kmeans_single(x, k, int(s), tol=tol)
        assert np.array_equal(seeds.cpu().numpy(), r_seeds)
        assert np.array_equal(labels.cpu().numpy(), r_labels)
        assert np.array_equal(centers.cpu().numpy(), r_centers)
        assert (n_iter, inertia) == (r_it, r_inertia)
        results.append((r_labels, r_inertia, r_it, r_seeds))
    # the tolerance decided: without it the first restart runs longer
    assert redal_ref.lloyd(x, results[0][3], 300, 0.0)[2] > results[0][2]
    best = min(range(len(results)), key=lambda i: results[i][1])            # the first on ties
    labels, _, inertia, _ = kmeans(xd, n_clusters=k, random_state=0, n_init=10)
    assert inertia == results[best][1]
    assert np.array_equal(labels, results[best][0])


def test_kmeans_refusals():
    from lidal_amd.score.redal import kmeans_single
    x = _t(np.random.RandomState(61).normal(size=(40, 129)).astype(np.float32))
    with pytest.raises(RuntimeError, match='feature width'):
        kmeans_single(x, 3, 0)
    for k in (0, 41):
        with pytest.raises(ValueError, match='n_clusters'):
            kmeans_single(x[:, :8].contiguous(), k, 0)
