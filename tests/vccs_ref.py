"""numpy restatement of the VCCS supervoxels as this project defines them (csrc/vccs.hip): test
infrastructure, the CPU side of the bit-for-bit checks.  Not the PCL library's algorithm and not its labels.

f64 throughout, on the widened f32 coordinates; every product and sum is a separate numpy element-wise operation or a
Python float operation, so each is rounded on its own, and sums the definition orders ("summed in that order") are
loops, never np.sum.  Integer sums use whatever order numpy likes.

The tie rules, restated here as the kernels have them:
  voxel ids          ascending (x, y, z) of the cell, inside one scan
  two-ring           ascending (dx + 2) * 25 + (dy + 2) * 5 + (dz + 2)
  normal             the eigenvector column of the smallest diagonal entry, the lowest index among equals
  seed candidate     least squared distance to the seed cell's centre, the lowest voxel among equals
  labels             1..S in ascending (x, y, z) of the seed cell
  a round            the least (D, label) among the neighbours' owners of the round's start, taken if D is strictly
                     below the voxel's own distance; all voxels switch at once
"""
import math

import numpy as np

from jacobi_ref import jacobi3

BIAS = 1 << 20
OFF27 = np.array([(o // 9 - 1, (o // 3) % 3 - 1, o % 3 - 1) for o in range(27)], dtype=np.int64)


def min_seed_of(voxel_resolution, seed_resolution):
    """Python floats, as the host computes it: 15.7 at the defaults."""
    return 0.05 * (0.5 * seed_resolution) ** 2 * math.pi / voxel_resolution ** 2


def rounds_of(voxel_resolution, seed_resolution):
    return int(1.8 * seed_resolution / voxel_resolution) - 1


def _pack(cell):
    b = cell + BIAS
    ok = ((b >= 0) & (b < (1 << 21))).all(axis=-1)
    return (b[..., 0] << 42) | (b[..., 1] << 21) | b[..., 2], ok


def voxelize(xyz, rv):
    """cells i64 [V,3] in (x, y, z) order, voxel of each point, qs i64 [V,3], n i64 [V], centroids f64 [V,3]."""
    x = np.asarray(xyz, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    cell = np.floor(x / rv).astype(np.int64)
    cells, inv = np.unique(cell, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    q = np.rint(x * 65536.0).astype(np.int64)
    qs = np.zeros(cells.shape, dtype=np.int64)
    np.add.at(qs, inv, q)
    n = np.bincount(inv, minlength=len(cells)).astype(np.int64)
    cen = qs.astype(np.float64) / n.astype(np.float64)[:, None] / 65536.0
    return cells, inv, qs, n, cen


def adjacency(cells):
    """nbr i64 [27, V]: the voxel at cell + offset o = (dx + 1) * 9 + (dy + 1) * 3 + (dz + 1), or -1."""
    keys, _ = _pack(cells)
    nbr = np.full((27, len(cells)), -1, dtype=np.int64)
    for o in range(27):
        k, ok = _pack(cells + OFF27[o])
        pos = np.minimum(np.searchsorted(keys, k), len(keys) - 1)
        hit = ok & (keys[pos] == k)
        nbr[o, hit] = pos[hit]
    return nbr


def two_ring(nbr):
    """mem i64 [125, V]: the voxel at offset idx = (dx + 2) * 25 + (dy + 2) * 5 + (dz + 2) if it is within two
    adjacency steps, else -1."""
    v = nbr.shape[1]
    mem = np.full((125, v), -1, dtype=np.int64)
    for o1 in range(27):
        u = nbr[o1]
        has = u >= 0
        for o2 in range(27):
            w = np.where(has, nbr[o2][np.maximum(u, 0)], -1)
            d = OFF27[o1] + OFF27[o2] + 2
            idx = d[0] * 25 + d[1] * 5 + d[2]
            mem[idx] = np.where(w >= 0, w, mem[idx])
    return mem


def _jacobi_normal(a, c):
    """a: 3x3 list (symmetric), c: the voxel's centroid.  The cyclic Jacobi of sym3.h (tests/jacobi_ref.py)."""
    e = jacobi3(a)
    m = 0
    if a[1][1] < a[m][m]:
        m = 1
    if a[2][2] < a[m][m]:
        m = 2
    n = [e[0][m], e[1][m], e[2][m]]
    if (n[0] * c[0] + n[1] * c[1]) + n[2] * c[2] > 0.0:
        n = [-n[0], -n[1], -n[2]]
    return n


def normals(cen, mem):
    """f64 [V,3]: zero for |S| < 3, else the Jacobi normal turned toward the origin."""
    v = cen.shape[0]
    count = (mem >= 0).sum(axis=0)
    mean = np.zeros((v, 3))
    for idx in range(125):
        w = mem[idx]
        has = (w >= 0)[:, None]
        mean = np.where(has, mean + cen[np.maximum(w, 0)], mean)
    inv = 1.0 / np.maximum(count, 1).astype(np.float64)
    mean = mean * inv[:, None]
    acc = np.zeros((v, 6))
    pairs = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
    for idx in range(125):
        w = mem[idx]
        has = w >= 0
        d = cen[np.maximum(w, 0)] - mean
        for j, (p, q) in enumerate(pairs):
            acc[:, j] = np.where(has, acc[:, j] + d[:, p] * d[:, q], acc[:, j])
    acc = acc * inv[:, None]
    out = np.zeros((v, 3))
    for i in range(v):
        if count[i] < 3:
            continue
        a00, a01, a02, a11, a12, a22 = (float(t) for t in acc[i])
        out[i] = _jacobi_normal([[a00, a01, a02], [a01, a11, a12], [a02, a12, a22]], [float(t) for t in cen[i]])
    return out


def seeds(cen, rs, min_seed):
    """Voxels of the surviving seeds in label order (label = position + 1)."""
    sc = np.floor(cen / rs).astype(np.int64)
    d = cen - (sc.astype(np.float64) + 0.5) * rs
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    cells, inv = np.unique(sc, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    r2 = (0.5 * rs) * (0.5 * rs)
    out = []
    for g in range(len(cells)):
        members = np.flatnonzero(inv == g)                      # ascending: argmin returns the lowest voxel among equals
        cand = int(members[np.argmin(d2[members])])
        e = cen - cen[cand]
        near = int(((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2] <= r2).sum())
        if float(near) > min_seed:
            out.append(cand)
    return np.array(out, dtype=np.int64)


def _centres(owner, qv, qn, n_sv, svc, svn):
    live = owner > 0
    s = owner[live] - 1
    sums = np.zeros((n_sv, 6), dtype=np.int64)
    np.add.at(sums, s, np.concatenate([qv[live], qn[live]], axis=1))
    k = np.bincount(s, minlength=n_sv)
    for l in range(n_sv):
        if k[l] == 0:
            continue
        svc[l] = sums[l, :3].astype(np.float64) / float(k[l]) / 65536.0
        sx, sy, sz = (float(t) for t in sums[l, 3:])
        length = math.sqrt((sx * sx + sy * sy) + sz * sz)
        svn[l] = [sx / length, sy / length, sz / length] if length > 0.0 else [0.0, 0.0, 0.0]


def grow(cen, nrm, nbr, seed_voxels, rounds, rs, w_s, w_n, stats=None):
    """owner i64 [V] after `rounds` synchronous rounds."""
    v, n_sv = cen.shape[0], len(seed_voxels)
    qv = np.rint(cen * 65536.0).astype(np.int64)
    qn = np.rint(nrm * 1073741824.0).astype(np.int64)
    owner = np.zeros(v, dtype=np.int64)
    dist = np.full(v, np.inf)
    owner[seed_voxels] = np.arange(1, n_sv + 1)
    dist[seed_voxels] = 0.0
    svc, svn = np.zeros((n_sv, 3)), np.zeros((n_sv, 3))
    _centres(owner, qv, qn, n_sv, svc, svn)
    steals = ties = 0
    for _ in range(rounds):
        best = np.full(v, np.inf)
        best_l = np.zeros(v, dtype=np.int64)
        for o in range(27):
            if o == 13 or n_sv == 0:
                continue
            u = nbr[o]
            l = np.where(u >= 0, owner[np.maximum(u, 0)], 0)
            cand = (l != 0) & (l != owner)
            s = np.maximum(l - 1, 0)
            e = svc[s] - cen
            dot = (svn[s, 0] * nrm[:, 0] + svn[s, 1] * nrm[:, 1]) + svn[s, 2] * nrm[:, 2]
            dd = w_n * (1.0 - np.abs(dot)) + w_s * (np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]) / rs)
            ties += int((cand & (best_l != 0) & (dd == best) & (l != best_l)).sum())
            take = cand & ((best_l == 0) | (dd < best) | ((dd == best) & (l < best_l)))
            best = np.where(take, dd, best)
            best_l = np.where(take, l, best_l)
        switch = (best_l != 0) & (best < dist)
        steals += int((switch & (owner != 0)).sum())
        owner = np.where(switch, best_l, owner)
        dist = np.where(switch, best, dist)
        _centres(owner, qv, qn, n_sv, svc, svn)
    if stats is not None:
        stats.update(steals=steals, ties=ties)
    return owner


def vccs(xyz, voxel_resolution=0.5, seed_resolution=10.0, spatial_importance=0.4, normal_importance=1.0):
    """The whole definition for one scan: a dict with labels i64 [P], point_voxel, cells, qs, n, centroids, normals,
    nbr, seed_voxels, owners, rounds, min_seed, steals, ties."""
    rv, rs = float(voxel_resolution), float(seed_resolution)
    cells, inv, qs, n, cen = voxelize(xyz, rv)
    nbr = adjacency(cells)
    nrm = normals(cen, two_ring(nbr))
    min_seed, rounds = min_seed_of(rv, rs), rounds_of(rv, rs)
    sv = seeds(cen, rs, min_seed)
    stats = {}
    owner = grow(cen, nrm, nbr, sv, rounds, rs, float(spatial_importance), float(normal_importance), stats)
    return dict(labels=owner[inv], point_voxel=inv, cells=cells, qs=qs, n=n, centroids=cen, normals=nrm, nbr=nbr,
                seed_voxels=sv, owners=owner, rounds=rounds, min_seed=min_seed, **stats)


def ball_mask(nbr, seed_voxels, rounds):
    """Voxels within `rounds` adjacency steps of a seed voxel, by plain breadth-first steps (no arithmetic)."""
    v = nbr.shape[1]
    inside = np.zeros(v, dtype=bool)
    inside[seed_voxels] = True
    for _ in range(rounds):
        grown = inside.copy()
        for o in range(27):
            u = nbr[o]
            grown |= (u >= 0) & inside[np.maximum(u, 0)]
        if (grown == inside).all():
            break
        inside = grown
    return inside


def sv_lists(labels, min_points=100, ignore_label=0):
    """(sv_ptr, sv_idx): labels != ignore_label with strictly more than min_points points, ascending label, ascending
    point ids (prepare_supervoxel_VCCS_sk.py:72-77)."""
    labels = np.asarray(labels).reshape(-1)
    ptr, idx = [0], []
    for l in np.unique(labels):
        if l == ignore_label:
            continue
        pts = np.flatnonzero(labels == l)
        if len(pts) > min_points:
            idx.append(pts)
            ptr.append(ptr[-1] + len(pts))
    return np.array(ptr, dtype=np.int64), (np.concatenate(idx) if idx else np.zeros(0, dtype=np.int64)).astype(np.int64)
