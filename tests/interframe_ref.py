"""A plain restatement of the inter-frame scorer and the small scoring kernels (csrc/score.hip).  TEST INFRASTRUCTURE.

numpy only in the matching step: chunked brute force in f64, the nearest point chosen by (d2, index) -- the tie rule the
kernel states, which sklearn's KDTree (oracle/scoring_ref.py) does not follow.  The accumulation is LiDAL.py:61-81 as
oracle/scoring_ref.py restates it, with scipy's kl_div / entropy on f32 arrays.  tests/test_scoring_cpu.py pins this file
against the reference's own fixtures and against KDTree; tests/test_scoring_edges_gpu.py holds the kernels to it."""
import math

import numpy as np
from scipy.special import kl_div
from scipy.stats import entropy

EPSILON = 0.00001          # LiDAL.py:58


def nearest(query, pts, chunk=1024):
    """For every row of query f64 [Q,3]: (index i64 [Q], d2 f64 [Q]) of the point of pts f64 [N,3] with the smallest
    (d2, index), d2 = (ex*ex + ey*ey) + ez*ez, e = point - query.  N = 0 gives index -1 and d2 = inf; so does a query
    whose every d2 is NaN."""
    query = np.asarray(query, np.float64).reshape(-1, 3)
    pts = np.asarray(pts, np.float64).reshape(-1, 3)
    q, n = query.shape[0], pts.shape[0]
    idx = np.full(q, -1, np.int64)
    d2 = np.full(q, np.inf)
    if n == 0 or q == 0:
        return idx, d2
    px, py, pz = pts[:, 0][None, :], pts[:, 1][None, :], pts[:, 2][None, :]
    with np.errstate(invalid='ignore', over='ignore'):
        for s in range(0, q, chunk):
            c = query[s:s + chunk]
            ex, ey, ez = px - c[:, 0:1], py - c[:, 1:2], pz - c[:, 2:3]
            d = (ex * ex + ey * ey) + ez * ez
            d = np.where(np.isnan(d), np.inf, d)
            a = np.argmin(d, axis=1)                     # the first minimum: the lowest index of a tie
            m = d[np.arange(c.shape[0]), a]
            idx[s:s + chunk] = np.where(np.isfinite(m), a, -1)
            d2[s:s + chunk] = m
    return idx, d2


def match(query, pts, dis_thresh):
    """(ids i64 [Q], d2 f64 [Q]): nearest() where sqrt(d2) <= dis_thresh, -1 elsewhere."""
    idx, d2 = nearest(query, pts)
    with np.errstate(invalid='ignore'):
        ok = (idx >= 0) & (np.sqrt(d2) <= dis_thresh)
    return np.where(ok, idx, -1), d2


def score_points(query_world, query_prob, nei_worlds, nei_probs, dis_thresh):
    """LiDAL.py:61-81 for one query frame against its neighbour frames, given in the reference's order.  Returns a dict:
    ids        list of i64 [P], the matched point of each neighbour frame or -1
    map_count  i64 [P]
    interd     f64 [P]
    intere     f32 [P]
    kl_abs     f64 [P], sum over the matched neighbours of sum_k |f32 KL term_k|
    entr_abs   f64 [P], sum_k |f32 entropy term_k| of the mean row"""
    query_prob = np.ascontiguousarray(query_prob, np.float32)
    query_points = np.asarray(query_world, np.float64).reshape(-1, 3)
    p = query_prob.shape[0]
    map_count = np.ones(p)
    interd_points = np.zeros(p)
    kl_abs = np.zeros(p)
    sum_prob = query_prob.copy()
    ids = []
    for world, n_prob in zip(nei_worlds, nei_probs):
        j, _ = match(query_points, world, dis_thresh)
        ids.append(j)
        m = j >= 0
        picked = np.ascontiguousarray(n_prob, np.float32)[j[m]]
        sum_prob[m] += picked
        terms = kl_div(query_prob[m] + EPSILON, picked + EPSILON)
        assert terms.dtype == np.float32
        interd_points[m] += np.sum(terms, axis=1)
        kl_abs[m] += np.abs(terms).astype(np.float64).sum(axis=1)
        map_count[m] += 1
    sum_prob /= np.expand_dims(map_count, 1)
    with np.errstate(invalid='ignore', divide='ignore'):
        intere_points = entropy(sum_prob, axis=1) if p else np.zeros(0, np.float32)
        pk = sum_prob / np.sum(sum_prob, axis=1, keepdims=True) if p else sum_prob
        entr_abs = np.where(pk > 0, np.abs(pk.astype(np.float64) * np.log(pk.astype(np.float64))), 0.0).sum(axis=1)
    map_count = map_count - 1
    mm = map_count > 0
    interd_points[mm] /= map_count[mm]
    return {'ids': ids, 'map_count': map_count.astype(np.int64), 'interd': interd_points,
            'intere': np.asarray(intere_points, np.float32), 'kl_abs': kl_abs, 'entr_abs': entr_abs}


def score_frame_points(i, probs, worlds, nei_ids, dis_thresh):
    return score_points(worlds[i], probs[i], [worlds[n] for n in nei_ids], [probs[n] for n in nei_ids], dis_thresh)


def interd_bound(ref, ulps=4):
    """|delta interd| allowed per point: `ulps` * 2^-24 * (sum of |KL term|) / max(cnt, 1)."""
    return ulps * 2.0 ** -24 * ref['kl_abs'] / np.maximum(ref['map_count'], 1)


def intere_bound(ref, ulps=4):
    return ulps * 2.0 ** -24 * ref['entr_abs']


def supervoxel_means(interd, intere, world, groups):
    """LiDAL.py:91-98 in f64: exactly rounded sums (math.fsum) divided by the size, as f64 [S], [S], [S,3].  An empty
    supervoxel gives NaN."""
    interd, intere = np.asarray(interd, np.float64), np.asarray(intere, np.float64)
    world = np.asarray(world, np.float64)
    s = len(groups)
    d, e, c = np.full(s, np.nan), np.full(s, np.nan), np.full((s, 3), np.nan)
    for k, g in enumerate(groups):
        g = np.asarray(g, np.int64)
        if g.size == 0:
            continue
        d[k] = math.fsum(interd[g]) / g.size
        e[k] = math.fsum(intere[g]) / g.size
        for a in range(3):
            c[k, a] = math.fsum(world[g, a]) / g.size
    return d, e, c


def view_mean_softmax(logits, inverse, reps):
    """prob_inference.py:100-113 in f64: (prob f64 [P,C], pred i64 [P], the first maximum)."""
    logits = np.asarray(logits, np.float64)
    p = inverse.shape[0] // reps
    x = logits[np.asarray(inverse)].reshape(reps, p, logits.shape[1])
    with np.errstate(invalid='ignore'):
        x = np.exp(x - x.max(axis=2, keepdims=True))
    prob = (x / x.sum(axis=2, keepdims=True)).mean(axis=0)
    return prob, prob.argmax(axis=1)


def confusion(logits, inverse, labels, c):
    """evaluate.py:100-109 + utils/iou_sk.py:14-19: bincount of pred * c + gt over the points with 0 <= gt < min(c, 100);
    rows = prediction (the first maximum), columns = ground truth."""
    logits, labels = np.asarray(logits), np.asarray(labels)
    pred = logits[np.asarray(inverse)].reshape(-1, c).argmax(axis=1) if labels.size else np.zeros(0, np.int64)
    keep = (labels >= 0) & (labels < min(c, 100))
    return np.bincount(pred[keep] * c + labels[keep], minlength=c * c).reshape(c, c).astype(np.int32)


def register(points, pose):
    """prepare_kdtree_sk.py:76-80."""
    points = np.asarray(points)
    hcoords = np.hstack((points[:, :3], np.ones_like(points[:, :1])))
    return np.sum(np.expand_dims(hcoords, 2) * np.asarray(pose).T, axis=1)[:, :3]


def lattice(pitch=0.05, keep=0.08, seed=0):
    """The tie input: every node of the lattice of `pitch` over [-1, 1]^2 x [-0.2, 0.2] as integer multiples of the pitch
    (so nodes sit exactly on multiples of 0.1 and 0.2 where the index allows, negative ones included, and the zero of the
    negative side is -0.0), and a seeded subset of about `keep` of them.  Returns (query f64 [Q,3], neighbour f64 [N,3])."""
    n_xy, n_z = int(round(1.0 / pitch)), int(round(0.2 / pitch))
    ax = np.arange(-n_xy, n_xy + 1)
    az = np.arange(-n_z, n_z + 1)
    g = np.stack(np.meshgrid(ax, ax, az, indexing='ij'), axis=-1).reshape(-1, 3).astype(np.float64)
    q = g * pitch
    q[(g == 0) & (np.arange(q.shape[0])[:, None] % 2 == 1)] = -0.0
    rs = np.random.RandomState(seed)
    return q, q[rs.random_sample(q.shape[0]) < keep].copy()


def margin_pairs(r=0.1, cell=0.05, per_axis=4):
    """The input that needs the margin of the probed cube.  Where neighbour - query is exact, e <= r gives
    neighbour <= fl(query + r) by the monotonicity of rounding, and the cube [q - r, q + r] holds the neighbour's cell
    without any margin: lattices and random clouds are of that kind.  Here it is not: the neighbour sits exactly on the
    cell face `cell` (index 1), in a lower binade than r, and the query one ulp beyond cell - r, so that
    fl(neighbour - query) rounds (to even) DOWN to r -- a match -- while fl(query + r) = cell - ulp lies in cell 0.
    Returns (query f64 [2 * 3 * per_axis, 3], neighbour f64 [3 * per_axis, 3]): query k of the first half matches
    neighbour k at exactly r; query k of the second half is one ulp farther from the same neighbour, at r + ulp(r), and
    matches nothing.  The other two coordinates of a pair are equal, and pairs are >= 0.5 apart."""
    near = np.nextafter(cell - r, -np.inf)
    far = np.nextafter(near, -np.inf)
    q1, q2, nb = [], [], []
    for a in range(3):
        for m in range(per_axis):
            rest = [0.7 + 0.5 * m, 2.0 + 0.5 * a]
            for lst, v in ((q1, near), (q2, far), (nb, cell)):
                row = list(rest)
                row.insert(a, v)
                lst.append(row)
    return np.array(q1 + q2, np.float64), np.array(nb, np.float64)


def softmax_rows(rs, n, c, scale=2.0):
    lg = rs.standard_normal((n, c)) * scale
    e = np.exp(lg - lg.max(axis=1, keepdims=True))
    return (e / e.sum(axis=1, keepdims=True)).astype(np.float32)
