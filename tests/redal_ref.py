"""numpy restatement of the project's k-means definition (csrc/redal.hip) and of worker_func's
per-region reductions: test infrastructure, the CPU side of the bit-for-bit checks."""
import numpy as np

CHUNK = 256


def d2(x64, c):
    """f64 squared distance of every row of x64 [N,D] to c [D]: numpy's pairwise order over the D terms, written out
    (8 accumulators over whole blocks of 8, combined ((0+1)+(2+3))+((4+5)+(6+7)), then the rest in order)."""
    sq = (x64 - c) ** 2
    d = sq.shape[1]
    if d < 8:
        r = np.zeros(sq.shape[0])
        for f in range(d):
            r = r + sq[:, f]
        return r
    d8 = d - d % 8
    r = sq[:, :8].copy()
    for i in range(8, d8, 8):
        r = r + sq[:, i:i + 8]
    res = ((r[:, 0] + r[:, 1]) + (r[:, 2] + r[:, 3])) + ((r[:, 4] + r[:, 5]) + (r[:, 6] + r[:, 7]))
    for f in range(d8, d):
        res = res + sq[:, f]
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
    dist = np.stack([d2(x64, c) for c in centers], axis=1)
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
    out = centers.copy()
    for j in range(len(centers)):
        rows = x64[labels == j]
        if len(rows):
            out[j] = np.cumsum(rows, axis=0)[-1] / len(rows)
    return out


def kmeans_single(x, k, seed_, max_iter=300, tol=0.0):
    """(labels, centers, n_iter, seeds) of one restart."""
    x64 = x.astype(np.float64)
    seeds = seed(x, k, seed_)
    centers = x64[seeds].copy()
    old = np.full(len(x64), -1)
    strict, it = False, 0
    labels = None
    while it < max_iter:
        labels, mind2 = assign(x64, centers)
        labels = relocate(labels, mind2, k)
        new = update(x64, labels, centers)
        shift = ((new - centers) ** 2).sum()
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
    return labels, centers, it, seeds


def kmeans(x, k, random_state=0, n_init=10, max_iter=300, tol=1e-4):
    tol_abs = float(np.var(x.astype(np.float64), axis=0).mean()) * tol
    best = None
    for s in np.random.RandomState(random_state).randint(2 ** 31 - 1, size=n_init):
        labels, centers, it, _ = kmeans_single(x, k, int(s), max_iter, tol_abs)
        inertia = float(((x.astype(np.float64) - centers[labels]) ** 2).sum())
        if best is None or inertia < best[1]:
            best = (labels, inertia)
    return best


def same_partition(a, b):
    """a and b split the rows the same way (up to renaming the clusters)."""
    a, b = np.asarray(a), np.asarray(b)
    pairs = set(zip(a.tolist(), b.tolist()))
    return len(pairs) == len(set(a.tolist())) == len(set(b.tolist()))
