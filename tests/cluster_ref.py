"""Brute-force numpy restatement of lidal_amd.data.euclidean_clusters (csrc/cluster.hip).

A point is live iff its coordinates are finite, 0 <= label < 64 and tol[label] > 0.  Two live points i != j of one scan
and one class c are joined iff the expression of pairs_ref.within holds with radius = tol[c] on the f32 rows,

    np.sqrt(np.square(xyz[i] - xyz[j]).sum()) < np.float32(tol[c])

A component is a connected component of that graph, kept iff min_points <= size <= max_points; the kept ones are
numbered in ascending order of their smallest row.  The union below is a plain one over the true pairs: joining two
components renames the rows of both to the smaller of their smallest rows."""
import numpy as np

import pairs_ref

N_CLASSES = 64


def tolerance_table(tolerance):
    """A float for every class, or {class: metres} -> f32 [64]."""
    tol = np.zeros(N_CLASSES, dtype=np.float32)
    if isinstance(tolerance, dict):
        for c, t in tolerance.items():
            tol[int(c)] = t
    else:
        tol[:] = tolerance
    return tol


def live_mask(xyz, labels, tol):
    lab = np.zeros(len(xyz), dtype=np.int64) if labels is None else np.asarray(labels, dtype=np.int64)
    ok = np.isfinite(xyz).all(axis=1) & (lab >= 0) & (lab < N_CLASSES)
    ok[ok] = tol[lab[ok]] > 0
    return ok, lab


def components(xyz, point_ptr, labels, tol):
    """root i64 [P]: the smallest row of the component of every live point, -1 for a point that is not live."""
    xyz = np.asarray(xyz)
    assert xyz.dtype == np.float32 and xyz.ndim == 2 and xyz.shape[1] == 3, (xyz.dtype, xyz.shape)
    p = len(xyz)
    live, lab = live_mask(xyz, labels, tol)
    scan = np.searchsorted(np.asarray(point_ptr), np.arange(p), side='right') - 1
    root = np.arange(p, dtype=np.int64)             # the smallest row of the component so far, kept up to date for every row
    for s in range(len(point_ptr) - 1):
        for c in np.unique(lab[live & (scan == s)]):
            rows = np.nonzero(live & (scan == s) & (lab == c))[0]
            pts = xyz[rows]
            for a in range(len(rows)):
                hit = pairs_ref.within(pts, a, np.float32(tol[c]))
                hit[a:] = False                     # every pair once, from its larger row
                if hit.any():
                    joined = np.append(np.unique(root[rows[hit]]), root[rows[a]])
                    root[rows[np.isin(root[rows], joined)]] = joined.min()
    root[~live] = -1
    return root


def clusters_ref(xyz, point_ptr, labels=None, tolerance=0.5, min_points=1, max_points=None):
    """dict of inst i32 [P], inst_ptr i64 [S+1], cls i32 [K], member_ptr i64 [K+1], members i32, bbox f32 [K,6],
    sizes i64 [K]."""
    xyz = np.asarray(xyz)
    point_ptr = np.asarray(point_ptr, dtype=np.int64)
    p = len(xyz)
    max_points = max(p, min_points) if max_points is None else max_points
    tol = tolerance_table(tolerance)
    root = components(xyz, point_ptr, labels, tol)
    _, lab = live_mask(xyz, labels, tol)
    size = np.bincount(root[root >= 0], minlength=p) if p else np.zeros(0, dtype=np.int64)
    kept = np.nonzero((root == np.arange(p)) & (size >= min_points) & (size <= max_points))[0]     # ascending roots
    ident = np.full(p, -1, dtype=np.int64)
    ident[kept] = np.arange(len(kept))
    inst = np.where(root >= 0, ident[np.maximum(root, 0)], -1).astype(np.int32)
    groups = [np.nonzero(inst == k)[0].astype(np.int32) for k in range(len(kept))]
    member_ptr = np.zeros(len(kept) + 1, dtype=np.int64)
    if len(kept):
        member_ptr[1:] = np.cumsum([len(g) for g in groups])
    members = np.concatenate(groups).astype(np.int32) if len(kept) else np.zeros(0, dtype=np.int32)
    bbox = np.zeros((len(kept), 6), dtype=np.float32)
    for k, g in enumerate(groups):
        bbox[k, :3], bbox[k, 3:] = xyz[g].min(axis=0), xyz[g].max(axis=0)
    inst_ptr = np.searchsorted(kept, point_ptr, side='left').astype(np.int64)
    return dict(inst=inst, inst_ptr=inst_ptr, cls=lab[kept].astype(np.int32), member_ptr=member_ptr, members=members,
                bbox=bbox, sizes=np.diff(member_ptr))


def scene(seed=3):
    """The scene of the tests: two scans, together about 3 000 points -- 40 Gaussian blobs of four classes plus clutter.
    Returns (xyz f32 [P,3], point_ptr i64 [3], labels i64 [P])."""
    rng = np.random.RandomState(seed)
    parts, labs = [], []
    for b in range(40):
        centre = np.concatenate([rng.uniform(-40, 40, 2), rng.uniform(-1, 1, 1)])
        n = int(rng.randint(3, 130))
        sigma = rng.uniform(0.1, 0.6)
        parts.append(centre + rng.randn(n, 3) * sigma * np.array([1.0, 1.0, 0.4]))
        labs.append(np.full(n, 1 + b % 4))
    n_clutter = 400
    parts.append(np.concatenate([rng.uniform(-45, 45, (n_clutter, 2)), rng.uniform(-1.5, 1.5, (n_clutter, 1))], axis=1))
    labs.append(rng.randint(0, 6, n_clutter))                          # classes 0 and 5 are not clustered
    xyz = np.concatenate(parts).astype(np.float32)
    lab = np.concatenate(labs).astype(np.int64)
    order = rng.permutation(len(xyz))
    xyz, lab = xyz[order], lab[order]
    cut = len(xyz) * 11 // 20
    return xyz, np.array([0, cut, len(xyz)], dtype=np.int64), lab


SCENE_TOL = {1: 0.5, 2: 0.5, 3: 0.7, 4: 0.3}
SCENE_MIN, SCENE_MAX = 5, 400
