"""numpy restatement of the project's k-means definition (csrc/kmeans.hip), of worker_func's
per-region reductions and of the k-nearest-neighbour list and surface variation: test infrastructure, the CPU side of
the bit-for-bit checks."""
import numpy as np

from jacobi_ref import jacobi3

CHUNK = 256
NP_BUFSIZE = 8192       # numpy's ufunc buffer size: an add-reduce sees blocks of at most this many values
SHIFT_LANES = 256       # km_shift_kernel's workgroup


def np_pairwise_f32(a):
    """numpy's pairwise_sum of f32 values a [n]: n < 8 summed in order from 0; n <= 128 a leaf with 8 accumulators over
    whole blocks of 8, combined ((0+1)+(2+3))+((4+5)+(6+7)), then the rest in order; else the two halves split at
    n/2 - (n/2) % 8."""
    f = np.float32
    n = a.size
    if n < 8:
        r = f(0)
        for v in a:
            r = f(r + v)
        return r
    if n <= 128:
        n8 = n - n % 8
        r = a[:8].copy()
        for i in range(8, n8, 8):
            r = r + a[i:i + 8]
        res = f(f(f(r[0] + r[1]) + f(r[2] + r[3])) + f(f(r[4] + r[5]) + f(r[6] + r[7])))
        for v in a[n8:]:
            res = f(res + v)
        return res
    n2 = n // 2
    n2 -= n2 % 8
    return f(np_pairwise_f32(a[:n2]) + np_pairwise_f32(a[n2:]))


def np_mean_f32(values):
    """numpy's mean of a contiguous f32 array, written out: the pairwise tree over each block of 8192 values, the block
    sums added in order to 0, divided by f32(n).  (Not one tree over the whole array: numpy's reduce iterator hands its
    inner loop at most one buffer of 8192 values at a time.)"""
    a = np.ascontiguousarray(values, dtype=np.float32).reshape(-1)
    total = np.float32(0)
    for b in range(0, a.size, NP_BUFSIZE):
        total = np.float32(total + np_pairwise_f32(a[b:b + NP_BUFSIZE]))
    return np.float32(total / np.float32(a.size))


def d2(x64, c):
    """f64 squared distance of every row of x64 [N,D] to c [D] (or [..., D], broadcast): numpy's pairwise order over the
    D terms, written out (8 accumulators over whole blocks of 8, combined ((0+1)+(2+3))+((4+5)+(6+7)), then the rest in
    order)."""
    sq = (x64 - c) ** 2
    d = sq.shape[-1]
    if d < 8:
        r = np.zeros(sq.shape[:-1])
        for f in range(d):
            r = r + sq[..., f]
        return r
    d8 = d - d % 8
    r = sq[..., :8].copy()
    for i in range(8, d8, 8):
        r = r + sq[..., i:i + 8]
    res = ((r[..., 0] + r[..., 1]) + (r[..., 2] + r[..., 3])) + ((r[..., 4] + r[..., 5]) + (r[..., 6] + r[..., 7]))
    for f in range(d8, d):
        res = res + sq[..., f]
    return res


def scan(rows):
    """rows f64 [R,N] -> (pot [R], cs [R,N]): sequential inclusive scans inside chunks of 256, chunk offsets by a
    sequential exclusive scan of the chunk totals; pot = the last offset + the last total."""
    r, n = rows.shape
    nc = -(-n // CHUNK)
    pad = np.zeros((r, nc * CHUNK))
    pad[:, :n] = rows
    loc = np.cumsum(pad.reshape(r, nc, CHUNK), axis=2)
    tot = loc[:, :, -1]
    inc = np.cumsum(tot, axis=1)
    off = np.concatenate([np.zeros((r, 1)), inc[:, :-1]], axis=1)
    cs = (off[:, :, None] + loc).reshape(r, nc * CHUNK)[:, :n]
    return inc[:, -1], cs


def seed(x, k, seed_):
    """greedy k-means++ from numpy.random.RandomState(seed_): the k seed rows."""
    x64 = x.astype(np.float64)
    n = len(x64)
    trials = 2 + int(np.log(k))
    rs = np.random.RandomState(seed_)
    seeds = [int(rs.randint(n))]
    closest = d2(x64, x64[seeds[0]])
    pot, cs = scan(closest[None])
    pot, cs = pot[0], cs[0]
    for _ in range(1, k):
        u = rs.random_sample(trials)
        cand = np.minimum(np.searchsorted(cs, u * pot), n - 1)
        dist = np.stack([np.minimum(closest, d2(x64, x64[c])) for c in cand])
        pots, css = scan(dist)
        b = int(np.argmin(pots))
        seeds.append(int(cand[b]))
        closest, pot, cs = dist[b], pots[b], css[b]
    return np.array(seeds)


def assign(x64, centers):
    step = max(1, (1 << 22) // max(1, x64.size))
    dist = np.concatenate([d2(x64[:, None, :], centers[None, j:j + step]) for j in range(0, len(centers), step)],
                          axis=1)
    labels = np.argmin(dist, axis=1)
    return labels, dist[np.arange(len(x64)), labels]


def relocate(labels, mind2, k):
    counts = np.bincount(labels, minlength=k)
    empty = np.where(counts == 0)[0]
    if len(empty):
        far = np.lexsort((np.arange(len(mind2)), -mind2))[:len(empty)]
        labels = labels.copy()
        labels[far] = empty
    return labels


def update(x64, labels, centers):
    """Sequential f64 sum of each cluster's rows in row order, divided by the count; an empty cluster keeps its
    centre."""
    out = centers.copy()
    order = np.argsort(labels, kind='stable')
    counts = np.bincount(labels, minlength=len(centers))
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]])
    rows = x64[order]
    for j in np.flatnonzero(counts):
        out[j] = np.cumsum(rows[starts[j]:starts[j] + counts[j]], axis=0)[-1] / counts[j]
    return out


def shift_sum(new, old):
    """km_shift_kernel's sum of (new - old)^2 over the k x d values (row-major): lane t of 256 sums the values t,
    t + 256, ... in order from 0, then the fixed tree red[t] += red[t + w] for w = 128, 64, ..., 1."""
    sq = ((new - old) ** 2).reshape(-1)
    m = sq.size
    pad = np.zeros(-(-m // SHIFT_LANES) * SHIFT_LANES)
    pad[:m] = sq                                  # (+0.0 leaves a lane sum unchanged: every term is >= 0)
    red = np.zeros(SHIFT_LANES)
    for row in pad.reshape(-1, SHIFT_LANES):
        red = red + row
    w = SHIFT_LANES // 2
    while w > 0:
        red = np.concatenate([red[:w] + red[w:2 * w], red[w:]])
        w //= 2
    return float(red[0])


def inertia_of(x64, labels, centers):
    """The chunked (256) scan total of every row's d2 to its centre."""
    pot, _ = scan(d2(x64, centers[labels])[None])
    return float(pot[0])


def lloyd(x, seeds, max_iter=300, tol=0.0):
    """Lloyd iterations from the seed rows: (labels, centers, n_iter, inertia)."""
    x64 = x.astype(np.float64)
    k = len(seeds)
    centers = x64[seeds].copy()
    old = np.full(len(x64), -1)
    strict, it = False, 0
    labels = None
    while it < max_iter:
        labels, mind2 = assign(x64, centers)
        labels = relocate(labels, mind2, k)
        new = update(x64, labels, centers)
        shift = shift_sum(new, centers)
        centers = new
        it += 1
        if np.array_equal(labels, old):
            strict = True
            break
        if shift <= tol:
            break
        old = labels
    if not strict:
        labels, _ = assign(x64, centers)
    return labels, centers, it, inertia_of(x64, labels, centers)


def kmeans_single(x, k, seed_, max_iter=300, tol=0.0):
    """(labels, centers, n_iter, seeds, inertia) of one restart; tol is absolute."""
    seeds = seed(x, k, seed_)
    labels, centers, it, inertia = lloyd(x, seeds, max_iter, tol)
    return labels, centers, it, seeds, inertia


def kmeans(x, k, random_state=0, n_init=10, max_iter=300, tol=1e-4):
    """(labels, inertia) of the restart of least inertia, the first on ties."""
    tol_abs = float(np.var(x.astype(np.float64), axis=0).mean()) * tol
    best = None
    for s in np.random.RandomState(random_state).randint(2 ** 31 - 1, size=n_init):
        labels, _, _, _, inertia = kmeans_single(x, k, int(s), max_iter, tol_abs)
        if best is None or inertia < best[1]:
            best = (labels, inertia)
    return best


def knn_brute(xyz, k, block=256):
    """The k nearest OTHER points of every point of xyz f32 [P,3] as the kernel defines them: coordinates widened to
    f64, d2 = (dx*dx + dy*dy) + dz*dz with every product and sum rounded, ordered by (d2, index).  i32 [P,k]."""
    x = np.asarray(xyz, dtype=np.float32).astype(np.float64)
    p = len(x)
    out = np.empty((p, k), np.int32)
    for b in range(0, p, block):
        q = x[b:b + block]
        e = x[None, :, :] - q[:, None, :]
        dist = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
        dist[np.arange(len(q)), np.arange(b, b + len(q))] = np.inf          # the query itself
        kth = np.partition(dist, k - 1, axis=1)[:, k - 1]
        for r in range(len(q)):
            cand = np.flatnonzero(dist[r] <= kth[r])                     # ascending index
            out[b + r] = cand[np.argsort(dist[r, cand], kind='stable')[:k]]
    return out


def surface_variation_f64(xyz, nb):
    """lambda_min / (l0 + l1 + l2) of the population covariance of each point's neighbours nb [P,k] (f64, LAPACK)."""
    x = np.asarray(xyz, dtype=np.float32).astype(np.float64)[nb]
    e = x - x.mean(axis=1, keepdims=True)
    cov = np.einsum('pki,pkj->pij', e, e) / nb.shape[1]
    lam = np.linalg.eigvalsh(cov)
    return lam[:, 0] / lam.sum(axis=1)


def surface_variation_jacobi(xyz, nb, threshold=0.1):
    """The surface variation as knn_kernel computes it, bit for bit: the mean and the population covariance of each
    point's neighbours nb [P,k] summed in neighbour order (f64, every product and sum rounded), the eigenvalues by the
    shared cyclic Jacobi (tests/jacobi_ref.py), f32(min / (l0 + l1 + l2)), then the kernel's clip: a value above
    f32(threshold) becomes it, NaN (a neighbourhood of one repeated point: 0 / 0) passes.  f32 [P]."""
    x = np.asarray(xyz, dtype=np.float32).astype(np.float64)
    k = nb.shape[1]
    inv = 1.0 / float(k)
    thr = np.float32(np.inf if threshold is None else threshold)
    out = np.empty(len(nb), np.float32)
    for i, row in enumerate(nb):
        pts = [[float(v) for v in x[j]] for j in row]
        m = [0.0, 0.0, 0.0]
        for q in pts:
            m = [m[0] + q[0], m[1] + q[1], m[2] + q[2]]
        m = [m[0] * inv, m[1] * inv, m[2] * inv]
        a00 = a01 = a02 = a11 = a12 = a22 = 0.0
        for q in pts:
            dx, dy, dz = q[0] - m[0], q[1] - m[1], q[2] - m[2]
            a00 += dx * dx; a01 += dx * dy; a02 += dx * dz
            a11 += dy * dy; a12 += dy * dz; a22 += dz * dz
        a = [[a00 * inv, a01 * inv, a02 * inv], [a01 * inv, a11 * inv, a12 * inv], [a02 * inv, a12 * inv, a22 * inv]]
        jacobi3(a)
        l0, l1, l2 = a[0][0], a[1][1], a[2][2]
        lmin = min(l0, l1, l2)                                      # (finite inputs: no NaN reaches the fmin)
        with np.errstate(invalid='ignore', divide='ignore'):
            sigma = np.float32(np.float64(lmin) / np.float64(l0 + l1 + l2))
        out[i] = thr if sigma > thr else sigma
    return out


def same_partition(a, b):
    """a and b split the rows the same way (up to renaming the clusters)."""
    a, b = np.asarray(a), np.asarray(b)
    pairs = set(zip(a.tolist(), b.tolist()))
    return len(pairs) == len(set(a.tolist())) == len(set(b.tolist()))
