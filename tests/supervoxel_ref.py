"""numpy restatement of the size-constrained k-means supervoxels (csrc/supervoxel.hip): test
infrastructure, the CPU side of the bit-for-bit checks.  Everything after the costs is integer arithmetic.

The tie rules, restated here as the kernel has them:
  initial label      the cluster of least cost, the lowest cluster on ties
  arc a -> b         M[a][b] = min over the points p of cluster a of cost[p][b] - cost[p][a]; among equal deltas the
                     lowest point is the arc's point
  Bellman-Ford       synchronous rounds over the K + 1 nodes (clusters 0..K-1, then the sink T = K): every node v takes
                     the least dist[u] + w(u, v) over the nodes u = 0..K in ascending order (strict `<`, so the lowest u
                     among equals) computed from the distances of the round before, and replaces its own distance and
                     parent only if that is strictly less; the rounds stop when one changes nothing
  target             the deficit node of least distance, the lowest node among equals
"""
import numpy as np

import redal_ref

INF = np.iinfo(np.int64).max


def bounds(p, k, slack=0.05):
    """(size_min, size_max) as prepare_supervoxel_kmeans_sk.py:17 computes them (slack 0.05: `* 0.95` and `* 1.05`)."""
    return int(p / k * (1 - slack)), int(p / k * (1 + slack))


def seed_of(random_state):
    """The seed of the one restart (n_init = 1)."""
    return int(np.random.RandomState(random_state).randint(2 ** 31 - 1, size=1)[0])


def costs(xyz, centers):
    """i32 [P,K]: rint(1000 * sqrt((dx*dx + dy*dy) + dz*dz)) in f64, the f32 point widened against the f64 centre."""
    x = np.asarray(xyz, dtype=np.float32).astype(np.float64)
    e = x[:, None, :] - np.asarray(centers, dtype=np.float64)[None, :, :]
    d2 = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
    return np.rint(1000.0 * np.sqrt(d2)).astype(np.int32)


def _row(cost, labels, a):
    """(M[a][:], points) of cluster a: the least delta to every cluster and the lowest point that has it."""
    k = cost.shape[1]
    members = np.flatnonzero(labels == a)                  # ascending: argmin returns the lowest point among equals
    if members.size == 0:
        return np.full(k, INF), np.full(k, -1)
    delta = cost[members].astype(np.int64) - cost[members, a].astype(np.int64)[:, None]
    arg = np.argmin(delta, axis=0)
    return delta[arg, np.arange(k)], members[arg]


def balanced_assign(cost, lo, hi):
    """The exact least-cost labels with every cluster size in [lo, hi]: (labels i64 [P], objective, augmentations).
    Successive shortest paths on the K + 1 node cluster graph from the unconstrained optimum."""
    cost = np.asarray(cost)
    p, k = cost.shape
    if not (k * lo <= p <= k * hi):
        raise ValueError('no assignment of %d points to %d clusters has every size in [%d, %d]' % (p, k, lo, hi))
    t = k
    labels = np.argmin(cost, axis=1)
    count = np.bincount(labels, minlength=k).astype(np.int64)
    take = np.clip(count, lo, hi)
    m = np.full((k, k), INF)
    arg = np.full((k, k), -1)
    for a in range(k):
        m[a], arg[a] = _row(cost, labels, a)

    def excess():
        return np.concatenate([count - take, [take.sum() - p]])

    exc = excess()
    n_aug = int(np.maximum(exc, 0).sum())
    for _ in range(n_aug):
        # arc weights of this state, w[u][v]
        w = np.full((k + 1, k + 1), INF)
        w[:k, :k] = m
        w[np.arange(k + 1), np.arange(k + 1)] = INF
        w[:k, t] = np.where(take < hi, 0, INF)
        w[t, :k] = np.where(take > lo, 0, INF)
        dist = np.where(exc > 0, 0, INF)
        parent = np.full(k + 1, -1)
        for _round in range(k + 1):
            ok = (dist[:, None] != INF) & (w != INF)
            cand = np.where(ok, np.where(ok, dist[:, None], 0) + np.where(ok, w, 0), INF)      # [u][v]
            best_u = np.argmin(cand, axis=0)                   # the lowest u among equals
            best = cand[best_u, np.arange(k + 1)]
            upd = best < dist
            if not upd.any():
                break
            dist = np.where(upd, best, dist)
            parent = np.where(upd, best_u, parent)
        else:
            raise RuntimeError('balanced_assign: the distances did not settle (a negative cycle)')
        deficit = np.flatnonzero((exc < 0) & (dist != INF))
        if deficit.size == 0:
            raise RuntimeError('balanced_assign: no deficit node can be reached')
        target = int(deficit[np.argmin(dist[deficit])])        # the lowest node among equals
        path = [target]
        while parent[path[-1]] >= 0:
            path.append(int(parent[path[-1]]))
            if len(path) > k + 1:
                raise RuntimeError('balanced_assign: the path walk does not end')
        path.reverse()
        assert exc[path[0]] > 0
        touched = set()
        moves = []
        for u, v in zip(path[:-1], path[1:]):
            if u == t:
                take[v] -= 1
            elif v == t:
                take[u] += 1
            else:
                moves.append((int(arg[u][v]), u, v))
        for q, u, v in moves:
            assert labels[q] == u
            labels[q] = v
            count[u] -= 1
            count[v] += 1
            touched.update((u, v))
        for a in sorted(touched):
            m[a], arg[a] = _row(cost, labels, a)
        exc = excess()
    assert not exc.any()
    objective = int(cost[np.arange(p), labels].astype(np.int64).sum())
    return labels.astype(np.int64), objective, n_aug


def lp_optimum(cost, lo, hi):
    """The optimum of the transportation LP (x[p][c] >= 0, rows sum to 1, column sums in [lo, hi]) by HiGHS: the
    independent check.  The constraint matrix is totally unimodular, so the optimum is an integer."""
    from scipy.optimize import linprog
    from scipy.sparse import coo_matrix
    cost = np.asarray(cost)
    p, k = cost.shape
    n = p * k
    var = np.arange(n)
    rows_eq = coo_matrix((np.ones(n), (var // k, var)), shape=(p, n)).tocsr()
    cols = coo_matrix((np.ones(n), (var % k, var)), shape=(k, n)).tocsr()
    from scipy.sparse import vstack
    r = linprog(cost.reshape(-1).astype(np.float64), A_ub=vstack([cols, -cols]).tocsr(),
                b_ub=np.concatenate([np.full(k, float(hi)), np.full(k, -float(lo))]), A_eq=rows_eq, b_eq=np.ones(p),
                bounds=(0, None), method='highs')
    assert r.status == 0, r.message
    assert abs(r.fun - round(r.fun)) < 1e-3, r.fun
    return int(round(r.fun))


def supervoxel_kmeans(xyz, k=20, slack=0.05, random_state=0):
    """The whole definition for one frame: dict of seeds, centers0, cost1, labels1, objective1, centers, cost2, labels,
    objective2, augmentations (first, second), lo, hi."""
    xyz = np.asarray(xyz, dtype=np.float32)
    p = len(xyz)
    lo, hi = bounds(p, k, slack)
    seeds = redal_ref.seed(xyz, k, seed_of(random_state))
    x64 = xyz.astype(np.float64)
    centers0 = x64[seeds].copy()
    cost1 = costs(xyz, centers0)
    labels1, obj1, aug1 = balanced_assign(cost1, lo, hi)
    centers = redal_ref.update(x64, labels1, centers0)
    cost2 = costs(xyz, centers)
    labels, obj2, aug2 = balanced_assign(cost2, lo, hi)
    return dict(seeds=seeds.astype(np.int32), centers0=centers0, cost1=cost1, labels1=labels1, objective1=obj1,
                centers=centers, cost2=cost2, labels=labels, objective2=obj2, augmentations=(aug1, aug2), lo=lo, hi=hi)


def sv_tables_script(label_files):
    """prepare_supervoxel_kmeans_sk.py:54-80 written out for a list of (sequence, frame name, labels): per frame
    (sv_id, sv2point), and the id2sv list."""
    tables, id2sv, first_id = [], [], 0
    for seq, name, frame_labels in label_files:
        frame_labels = np.asarray(frame_labels)
        groups = [np.flatnonzero(frame_labels == value) for value in sorted(set(frame_labels.tolist()))]
        tables.append((first_id + np.arange(len(groups)), groups))
        id2sv.extend((seq, name, local) for local in np.arange(len(groups)))
        first_id += len(groups)
    return tables, id2sv
