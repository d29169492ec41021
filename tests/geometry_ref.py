"""Plain restatement of the integer geometry (csrc/hash.hip, csrc/kmap.hip, csrc/common.h) in numpy and Python dicts,
and the input families the geometry edge tests share.  TEST INFRASTRUCTURE.

Nothing here is keyed by the 60-bit hash: kernel maps and look-ups go through dicts of coordinate TUPLES / Python ints,
so a collision of the hash, a bitmap alias or a probe chain cannot hide in the reference.  The table arithmetic
(mix_key, slot_of, sbit_of, table_capacity, table_spatial_dims) is restated only so that the tests can CONSTRUCT
colliding and aliasing inputs and prove that they are what they claim (tests/test_geometry_ref_cpu.py)."""
import numpy as np

M64 = (1 << 64) - 1
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
INT64_MIN, INT64_MAX = -2 ** 63, 2 ** 63 - 1


# ---------------------------------------------------------------- hashing and the table layout
def fnv60(coords):
    """FNV-1a-64 over the four u32 words of each (x, y, z, b) row, folded to 60 bits.  i32 [n, 4] -> i64 [n]."""
    w = np.ascontiguousarray(coords, dtype=np.int32).reshape(-1, 4).view(np.uint32).astype(np.uint64)
    with np.errstate(over='ignore'):
        h = np.full(w.shape[0], 14695981039346656037, dtype=np.uint64)
        for j in range(4):
            h = (h ^ w[:, j]) * np.uint64(1099511628211)
        h = (h >> np.uint64(60)) ^ (h & np.uint64(0x0FFFFFFFFFFFFFFF))
    return h.astype(np.int64)


def sphash(coords, offsets=None):
    """F.sphash: [n] without offsets, [k, n] with i32 [k, 3] offsets added to (x, y, z) in wrapping int32."""
    c = np.ascontiguousarray(coords, dtype=np.int32).reshape(-1, 4)
    if offsets is None:
        return fnv60(c)
    o = np.asarray(offsets, dtype=np.int32).reshape(-1, 3)
    cur = np.repeat(c[None], o.shape[0], 0)
    with np.errstate(over='ignore'):
        cur[:, :, :3] += o[:, None, :]
    return fnv60(cur.reshape(-1, 4)).reshape(o.shape[0], c.shape[0])


def mix_key(key):
    """murmur3 finaliser of common.h, on u64 arrays (any i64 input is taken as its two's complement)."""
    k = np.asarray(key).astype(np.int64).view(np.uint64).copy()
    with np.errstate(over='ignore'):
        k ^= k >> np.uint64(33)
        k *= np.uint64(0xff51afd7ed558ccd)
        k ^= k >> np.uint64(33)
    return k


def table_capacity(n):
    cap = 1024
    while cap < 2 * n:
        cap <<= 1
    return cap


def table_spatial_dims(cap):
    """(x bits, y bits) of the spatial bitmap of a table of capacity cap (z: 5 bits, batch: 2 bits)."""
    sbytes = max(cap, 16384)
    lg = sbytes.bit_length() - 1
    xy = lg + 3 - 7
    return (xy + 1) // 2, xy // 2


def slot_of(key, cap):
    return (mix_key(key) & np.uint64(cap - 1)).astype(np.int64)


def sbit_of(coords, shift, xb, yb, batch_mask=3):
    """Bit of each (x, y, z, b) row in the spatial bitmap; arithmetic shift, as `>>` of a C int."""
    c = np.asarray(coords, dtype=np.int64).reshape(-1, 4)
    xi = (c[:, 0] >> shift) & ((1 << xb) - 1)
    yi = (c[:, 1] >> shift) & ((1 << yb) - 1)
    zi = (c[:, 2] >> shift) & 31
    bi = c[:, 3] & batch_mask
    return ((((bi << 5) | zi) << yb | yi) << xb) | xi


def hash_edge_coords():
    """Negative coordinates, INT32_MIN / INT32_MAX (offsets wrap there), negative batch ids."""
    rng = np.random.default_rng(1)
    c = rng.integers(-5000, 5000, size=(1500, 4)).astype(np.int32)
    c[:, 3] = rng.integers(-3, 4, size=1500)
    lim = np.array([[INT32_MIN, INT32_MAX, 0, 0], [INT32_MAX, INT32_MIN, INT32_MAX, -1],
                    [INT32_MIN, INT32_MIN, INT32_MIN, INT32_MIN], [-1, -1, -1, -1],
                    [INT32_MAX, INT32_MAX, INT32_MAX, INT32_MAX], [0, -1, INT32_MIN + 1, -32768]],
                   dtype=np.int32)
    return np.concatenate([c, lim])


def hashquery(queries, references, last_wins=False):
    """F.sphashquery: index of the FIRST occurrence of each query among the references, or -1.  Python ints in a dict."""
    first = {}
    for i, r in enumerate(np.asarray(references, dtype=np.int64).reshape(-1).tolist()):
        if last_wins:
            first[r] = i
        else:
            first.setdefault(r, i)
    q = np.asarray(queries, dtype=np.int64)
    return np.array([first.get(v, -1) for v in q.reshape(-1).tolist()], dtype=np.int64).reshape(q.shape)


# ---------------------------------------------------------------- kernel maps
def kernel_offsets(kernel_size, stride):
    """get_kernel_offsets: odd volume x fastest, even volume z fastest; offsets in units of the tensor stride."""
    ax = [[(v - (kernel_size[d] - 1) // 2) * stride[d] for v in range(kernel_size[d])] for d in range(3)]
    if (kernel_size[0] * kernel_size[1] * kernel_size[2]) % 2 == 1:
        off = [[x, y, z] for z in ax[2] for y in ax[1] for x in ax[0]]
    else:
        off = [[x, y, z] for x in ax[0] for y in ax[1] for z in ax[2]]
    return np.asarray(off, dtype=np.int32).reshape(-1, 3)


def _distinct_rows(a):
    """Number of distinct rows of an i32 [m, 4] array."""
    if a.shape[0] == 0:
        return 0
    u = np.ascontiguousarray(a, dtype=np.int32).view(np.uint32).astype(np.uint64)
    p, q = (u[:, 0] << np.uint64(32)) | u[:, 1], (u[:, 2] << np.uint64(32)) | u[:, 3]
    o = np.lexsort((q, p))
    p, q = p[o], q[o]
    return 1 + int(np.count_nonzero((p[1:] != p[:-1]) | (q[1:] != q[:-1])))


class KMap:
    pass


def kernel_map(coords, in_stride, kernel_size, stride, out_coords=None):
    """The kernel map of torchsparse's conv3d, keyed by coordinate tuples: results[k][j] = row of
    out_coords[j] + offset_k (wrapping int32) among `coords`, first row wins, -1 if absent.  Raises if two distinct
    coordinates among the inputs and the probed ones share a 60-bit hash (the kernels key by the hash, as torchsparse
    does: on such an input they and this reference may legitimately differ)."""
    c = np.ascontiguousarray(coords, dtype=np.int32).reshape(-1, 4)
    off = kernel_offsets(kernel_size, in_stride)
    if out_coords is None:
        out_coords = c
        if any(s > 1 for s in stride):
            out_coords = downsample(c, [in_stride[d] * stride[d] for d in range(3)])
    oc = np.ascontiguousarray(out_coords, dtype=np.int32).reshape(-1, 4)
    K, n_in, n_out = off.shape[0], c.shape[0], oc.shape[0]
    probed = np.repeat(oc[None], K, 0)
    with np.errstate(over='ignore'):
        probed[:, :, :3] += off[:, None, :]
    every = np.concatenate([c, probed.reshape(-1, 4)])
    if _distinct_rows(every) != np.unique(fnv60(every)).size:
        raise ValueError('two distinct coordinates of this input share a 60-bit hash')
    first = {}
    for i, t in enumerate(map(tuple, c.tolist())):
        first.setdefault(t, i)
    res = np.array([first.get(t, -1) for t in map(tuple, probed.reshape(-1, 4).tolist())],
                   dtype=np.int32).reshape(K, n_out)
    m = KMap()
    m.offsets, m.results, m.out_coords, m.sizes = off, res, oc, (n_in, n_out)
    kk, jj = np.nonzero(res >= 0)                                 # row-major: grouped by k, ascending out row
    m.nbmaps = np.stack([res[kk, jj], jj.astype(np.int32)], 1).astype(np.int32).reshape(-1, 2)
    m.nbsizes = (res >= 0).sum(1).astype(np.int32)
    m.koff = np.concatenate([[0], np.cumsum(m.nbsizes, dtype=np.int64)]).astype(np.int64)
    m.total = int(m.koff[-1])
    m.nbr_in = invert(res, n_in)
    return m


def invert(nbr_out, n_in):
    """nbr_in[k][i] = j  <=>  nbr_out[k][j] = i (unique rows: one j per (k, i))."""
    nbr_in = np.full((nbr_out.shape[0], n_in), -1, dtype=np.int32)
    kk, jj = np.nonzero(nbr_out >= 0)
    nbr_in[kk, nbr_out[kk, jj]] = jj
    return nbr_in


def symmetric_probe_model(coords, ts, kernel_size, results, shift_probe=None, insert_batch_mask=3, swap_xy=False,
                          mirror_shift=0):
    """Model of the symmetric probe through the spatial bitmap, for the sensitivity list: the first K/2 offsets are
    answered by `results` (the true map) only where the probed voxel's bit is set, every hit writes its mirror entry,
    the centre is the identity.  Defaults = the kernel; each argument is one mutation."""
    c = np.ascontiguousarray(coords, dtype=np.int32).reshape(-1, 4)
    n = c.shape[0]
    off = kernel_offsets(kernel_size, (ts,) * 3)
    K, half = off.shape[0], off.shape[0] // 2
    shift = ts.bit_length() - 1
    xb, yb = table_spatial_dims(table_capacity(n))
    bits = np.zeros(1 << (xb + yb + 7), dtype=bool)
    bits[sbit_of(c, shift, xb, yb, insert_batch_mask)] = True
    pxb, pyb = (yb, xb) if swap_xy else (xb, yb)
    nbr = np.full((K, n), -1, dtype=np.int32)
    nbr[half] = np.arange(n)
    for k in range(half):
        p = c.copy()
        with np.errstate(over='ignore'):
            p[:, :3] += off[k]
        sb = sbit_of(p, shift if shift_probe is None else shift_probe, pxb, pyb)
        r = np.where(bits[sb % bits.size], results[k], -1)
        nbr[k] = r
        j = np.nonzero(r >= 0)[0]
        mk = K - 1 - k + mirror_shift
        if mk < K:
            nbr[mk, r[j]] = j
    return nbr


# ---------------------------------------------------------------- downsampling
def downsample(coords, factors, trunc=False):
    """F.spdownsample: floor (x, y, z) to multiples of `factors`, then the unique rows in (b, x, y, z) order."""
    c = np.ascontiguousarray(coords, dtype=np.int64).reshape(-1, 4).copy()
    f = np.asarray(factors, dtype=np.int64).reshape(1, 3)
    if trunc:
        c[:, :3] = np.trunc(c[:, :3] / f).astype(np.int64) * f
    else:
        c[:, :3] = c[:, :3] // f * f
    if c.shape[0] == 0:
        return c.astype(np.int32)
    u = np.unique(c[:, [3, 0, 1, 2]], axis=0)
    return np.ascontiguousarray(u[:, [1, 2, 3, 0]]).astype(np.int32)


def pyramid(coords, levels, ts):
    """F.downsample_pyramid as the chain of stride-2 downsamplings from tensor stride ts."""
    out, cur, s = [], coords, np.asarray(ts, dtype=np.int64).reshape(-1) * np.ones(3, dtype=np.int64)
    for _ in range(levels):
        s = s * 2
        cur = downsample(cur, s)
        out.append(cur)
    return out


# ---------------------------------------------------------------- occupancy row order
def bit_rank(K):
    """to_key[k]: key bit of offset k.  K = 27: rarest offsets (largest L1 norm of the offset) most significant."""
    to_key = list(range(32))
    if K != 27:
        return to_key
    pos = 26
    for want in (3, 2, 1, 0):
        for k in range(27):
            a, b, c = k % 3, (k // 3) % 3, k // 9
            if (a != 1) + (b != 1) + (c != 1) == want:
                to_key[k] = pos
                pos -= 1
    return to_key


def row_masks(nbr):
    """Occupancy mask of each row in offset bits: bit k set iff nbr[k][j] >= 0.  u32 [n]."""
    K = nbr.shape[0]
    m = np.zeros(nbr.shape[1], dtype=np.uint64)
    for k in range(K):
        m |= (nbr[k] >= 0).astype(np.uint64) << np.uint64(k)
    return m.astype(np.uint32)


def row_keys(nbr):
    """Sort key of each row: the mask with its bits re-ranked (bit_rank), then its Gray rank (prefix xor)."""
    K = nbr.shape[0]
    to_key = bit_rank(K)
    m = np.zeros(nbr.shape[1], dtype=np.uint64)
    for k in range(K):
        m |= (nbr[k] >= 0).astype(np.uint64) << np.uint64(to_key[k])
    for s in (1, 2, 4, 8, 16):
        m ^= m >> np.uint64(s)
    return m.astype(np.uint32)


def row_order(nbr, tile_rows=128, stable=True):
    """-> (perm, nbr[:, perm], tile masks): stable sort of the rows by row_keys; mask of a tile = OR of the offset
    masks of its `tile_rows` sorted rows."""
    nbr = np.asarray(nbr, dtype=np.int32)
    n = nbr.shape[1]
    keys = row_keys(nbr)
    if stable:
        perm = np.argsort(keys, kind='stable')
    else:                                       # a legal unstable sort: ties in descending row order
        perm = np.lexsort((-np.arange(n), keys))
    perm = perm.astype(np.int32)
    masks = row_masks(nbr)[perm]
    tiles = -(-n // tile_rows)
    tm = np.zeros(tiles, dtype=np.uint32)
    for t in range(tiles):
        tm[t] = np.bitwise_or.reduce(masks[t * tile_rows:(t + 1) * tile_rows])
    return perm, nbr[:, perm], tm


# ---------------------------------------------------------------- input families
def _shuffle(c, seed):
    c = np.unique(np.asarray(c, dtype=np.int32).reshape(-1, 4), axis=0)
    return np.ascontiguousarray(c[np.random.default_rng(seed).permutation(c.shape[0])])


def sheet_origin(ts, seed=0):
    """Two wavy sheets straddling the origin in x, y and z (-40 .. 40 cells, z about -8 .. 8), at tensor stride ts."""
    x, y = np.meshgrid(np.arange(-40, 41), np.arange(-40, 41), indexing='ij')
    out = []
    for b in range(2):
        z = np.floor(4 * np.sin(x / 7.0 + b) + 3 * np.cos(y / 5.0) + 0.5 * b).astype(np.int64)
        out.append(np.stack([x * ts, y * ts, z * ts, np.full_like(x, b)], -1).reshape(-1, 4))
    return _shuffle(np.concatenate(out), seed)


def sheet_rows(n, ts=1, seed=0, batch=0):
    """Exactly n rows of a wavy sheet with x in 0 .. 127 cells: every y row is an x-run that crosses x' = 31|32 and 63|64
    (the word boundaries of the spatial bitmap) and 127|0 wraps for xb < 7.  n = 0 gives an empty [0, 4] array."""
    if n == 0:
        return np.zeros((0, 4), dtype=np.int32)
    ny = -(-n // 128)
    y, x = np.meshgrid(np.arange(ny), np.arange(128), indexing='ij')           # y-major: trimming cuts the last run
    z = np.floor(3 * np.sin(x / 9.0) + 2 * np.cos(y / 5.0)).astype(np.int64) + 6
    c = np.stack([x * ts, y * ts, z * ts, np.full_like(x, batch)], -1).reshape(-1, 4)[:n]
    return _shuffle(c, seed)


def batches8():
    """Batch ids 0 .. 7 on small sheets; the column (5, 5, 5) is present in batches 0 and 4 -- which the bitmap cannot
    tell apart (it keeps b & 3) -- with different neighbourhoods: +x only in batch 0, -x and +y only in batch 4."""
    rows = []
    for b in range(8):
        x, y = np.meshgrid(np.arange(20, 30), np.arange(20, 30), indexing='ij')
        z = (x + b * y) % 3 + 9
        rows.append(np.stack([x, y, z, np.full_like(x, b)], -1).reshape(-1, 4))
    rows.append(np.array([[5, 5, 5, 0], [6, 5, 5, 0], [5, 5, 5, 4], [4, 5, 5, 4], [5, 6, 5, 4]]))
    return _shuffle(np.concatenate(rows), 8)


def aliased(ts):
    """Voxel triples that share ONE bit of the spatial bitmap of this input's table (xb = yb = 5): A, A + 32 ts in z and
    A + 2^xb ts in x, plus a pair A, A + 2^yb ts in y.  One member of each pair has a neighbour the other lacks, so a
    set bit that belongs to the alias must be resolved by the slots.  Returns (coords, list of aliased row pairs)."""
    rows, pairs = [], []
    for i in range(12):
        a = np.array([(3 + 2 * i) - 20, 7 * (i % 3) - 5, (i % 5) - 2, i % 2]) * np.array([ts, ts, ts, 1])
        az = a + np.array([0, 0, 32 * ts, 0])
        ax = a + np.array([32 * ts, 0, 0, 0])
        ay = a + np.array([0, 32 * ts, 0, 0])
        rows += [a, az, ax, ay,
                 a + np.array([ts, 0, 0, 0]),               # A's +x neighbour: az, ax, ay have none
                 az + np.array([0, ts, 0, 0]),              # az's +y neighbour: a has none
                 ax + np.array([-ts, 0, ts, 0]),            # ax's (-x, +z) neighbour
                 ay + np.array([0, -ts, -ts, 0])]           # ay's (-y, -z) neighbour
        pairs += [(a, az), (a, ax), (a, ay)]
    return _shuffle(np.stack(rows), 3), pairs


def dense_block(lo=-6):
    g = np.arange(lo, lo + 12)
    x, y, z = np.meshgrid(g, g, g, indexing='ij')
    return _shuffle(np.stack([x, y, z, np.zeros_like(x)], -1).reshape(-1, 4), 12)


ISOLATED = np.array([[-7, 3, -2, 5]], dtype=np.int32)

SHAPES = [((3, 3, 3), 1), ((5, 5, 5), 1), ((3, 1, 1), 1), ((1, 3, 3), 1), ((1, 1, 1), 1), ((2, 2, 2), 2)]


def kmap_cases():
    """name -> (coords maker, tensor stride, list of (kernel_size, stride)).  Strided shapes only on families without
    negative coordinates (spdownsample refuses them)."""
    k3, all_s = [SHAPES[0]], SHAPES
    cases = {}
    for ts in (1, 2, 4, 8):
        cases['sheet_origin_ts%d' % ts] = (lambda ts=ts: sheet_origin(ts, seed=ts), ts, k3)
    cases['batches8'] = (batches8, 1, all_s)
    for ts in (1, 4):
        cases['aliased_ts%d' % ts] = (lambda ts=ts: aliased(ts)[0], ts, SHAPES[:5])
    for n in (8192, 8193, 16384, 16385):
        cases['rows_%d' % n] = (lambda n=n: sheet_rows(n, 1, seed=n), 1, [SHAPES[0], SHAPES[5]])
    cases['rows_8193_ts2'] = (lambda: sheet_rows(8193, 2, seed=5), 2, [SHAPES[0], SHAPES[5]])
    for n in (0, 1, 2, 1023, 1024, 1025):
        cases['rows_%d' % n] = (lambda n=n: sheet_rows(n, 1, seed=n, batch=n % 3), 1, all_s)
    cases['isolated'] = (lambda: ISOLATED.copy(), 1, SHAPES[:5])
    cases['dense12'] = (dense_block, 1, SHAPES[:5])
    cases['dense12_pos'] = (lambda: dense_block(3), 1, all_s)
    return cases


def kmap_case_ids():
    return [(name, ks, st) for name, (_, _, shapes) in kmap_cases().items() for ks, st in shapes]


_CACHE = {}


def case_coords(name):
    if ('c', name) not in _CACHE:
        _CACHE[('c', name)] = kmap_cases()[name][0]()
    return _CACHE[('c', name)]


def case_map(name, ks, st):
    """The reference map of a case, computed once per process and shared (read only)."""
    key = ('m', name, ks, st)
    if key not in _CACHE:
        ts = kmap_cases()[name][1]
        _CACHE[key] = kernel_map(case_coords(name), (ts,) * 3, ks, (st,) * 3)
    return _CACHE[key]


def end_of_table_chain(n_keys=64, cap=1024, seed=0):
    """(keys, absent): n_keys distinct i64 keys -- of either sign -- whose slot is the LAST one of a table of `cap`
    slots, so their probe chain wraps to slot 0; and absent keys that start in that chain (the last slot or one of the
    first n_keys - 1) without being among them."""
    rng = np.random.default_rng(seed)
    cand = rng.integers(INT64_MIN, INT64_MAX, size=400 * cap, dtype=np.int64)
    s = slot_of(cand, cap)
    cand, first = np.unique(cand, return_index=True)
    cand = cand[np.argsort(first)]                              # distinct, in the order drawn: both signs
    s = slot_of(cand, cap)
    keys = cand[s == cap - 1][:n_keys]
    absent = np.concatenate([cand[s == cap - 1][n_keys:n_keys + 20], cand[s < n_keys - 1][:180]])
    assert keys.size == n_keys and absent.size == 200
    return rng.permutation(keys), absent
