"""Exact-operand cases and the f64 reference of the point-voxel sums (csrc/voxel.hip), for test_voxel_ref_cpu.py and
test_voxel_exact_gpu.py.

The oracle.  Rows and upstream gradients are integers in [-8, 8], devoxelize weights are k / 64, voxelize counts are
powers of two up to 64: every term of a sum is a multiple of 2^-6 of magnitude at most 8, so every product and every
partial sum of a list of L < 2^24 / 512 entries is an f32 number.  Whatever the association -- lane groups, waves, parts,
the fold -- an ordered sum then holds the exact value, and the result must EQUAL the f64 sum rounded once to the output
type.  One entry dropped, doubled or taken from a neighbour's list changes an output element.

The cases.  Which kernel an ordered sum runs follows the average list length alone; `lidal_segment_form` tells which.  A
case names the form it wants; its lists are the `ladder` of lengths on the edges of the kernels' loops and splits, once
each on a random voxel, and a filler length F on every other voxel -- the smallest F for which the query answers the
wanted form.  A threshold that moves changes F, never the form under test."""
import collections

import numpy as np
import torch

F32, BF16 = 0, 1                      # include/lidal_amd.h LIDAL_F32 / LIDAL_BF16
TORCH = {F32: torch.float32, BF16: torch.bfloat16}
GROUP, WAVE, WG1, WG2, WG4 = 0, 1, 11, 12, 14       # what lidal_segment_form answers
BIG = 5000                            # the one long list some cases carry

Case = collections.namedtuple('Case', 'form dtype c m big avg')


def _case(form, dtype, c, m, big=False, avg=None):
    return Case(form, dtype, c, m, big, avg)


# (form; type, channels; voxels) -- avg: the band the average list length must lie in, where the form depends on it
CASES = [
    _case(GROUP, F32, 32, 200), _case(GROUP, F32, 4, 200), _case(GROUP, F32, 100, 200),     # 100: 25 of 32 lanes live
    _case(GROUP, BF16, 256, 200), _case(GROUP, BF16, 12, 200),                              # 12: 8-byte accesses
    _case(GROUP, BF16, 32, 65536, avg=(13, 32)),                                            # the many-voxels rule
    _case(WAVE, F32, 32, 200, big=True), _case(WAVE, BF16, 96, 200),
    _case(WAVE, BF16, 4, 65536, avg=(128, 319)),                                            # a wave only because m >= 65536
    _case(WG1, F32, 256, 120), _case(WG1, BF16, 256, 120, big=True), _case(WG1, F32, 100, 120),
    _case(WG2, F32, 96, 120, big=True), _case(WG2, BF16, 256, 120),
    _case(WG4, F32, 256, 120), _case(WG4, BF16, 512, 120, big=True), _case(WG4, BF16, 32, 120),
]
FORM_NAME = {GROUP: 'group', WAVE: 'wave', WG1: 'wg1', WG2: 'wg2', WG4: 'wg4'}


def case_id(case):
    return '%s-%s-c%d-m%d' % (FORM_NAME[case.form], 'f32' if case.dtype == F32 else 'bf16', case.c, case.m)


# one small case per form (the CPU order-freedom check, the per-element test with true counts)
SMALL = {GROUP: (CASES[1], CASES[3]), WAVE: (CASES[6], CASES[7]), WG1: (CASES[11], CASES[10]), WG2: (CASES[12], CASES[13]),
         WG4: (CASES[14], CASES[15])}


def lib():
    from lidal_amd import backend as B
    return B.lib_handle()


def lanes_per_row(form, dtype, c):
    """Lanes that cover a row in the kernel of `form`: 16-byte steps for f32 and for bf16 rows of whole 8-element steps,
    8-byte steps for other bf16 rows; a power of two, at least 4 (8 in the wave and workgroup kernels on 4-element steps)."""
    vec = 8 if dtype == BF16 and c % 8 == 0 else 4
    need = -(-c // vec)
    lanes = 4 if form == GROUP or vec == 8 else 8
    while lanes < need:
        lanes *= 2
    return min(lanes, 64)


def ladder(rpw, parts):
    """List lengths on the edges of segment_wave_sum's loops (batches of 64 entries, unrolled steps of 4 * rpw, the
    guarded tail) and of the splits (4 * parts waves, `parts` partial rows)."""
    s = {0, 1, 2, 3, 4, 5, 7, 8, 9, rpw - 1, rpw, rpw + 1, 4 * rpw - 1, 4 * rpw, 4 * rpw + 1, 63, 64, 65,
         64 + 4 * rpw - 1, 64 + 4 * rpw + 1, 127, 128, 129, 255, 256, 257}
    if parts > 0:
        s |= {4 * parts - 1, 4 * parts, 4 * parts + 1, 256 * parts - 1, 256 * parts, 256 * parts + 1}
    return sorted(s)


def _dead(live):
    return 3 * max(2, live // 24)


def _n_entries(live, op):
    n = live + _dead(live)
    return n if op == 'vox' else 8 * (-(-n // 8))


Layout = collections.namedtuple('Layout', 'lengths filler n_entries form rpw')


def layout(case, op):
    """The list length of every voxel of `case` for op 'vox' (lidal_voxelize_fwd_sorted, n_entries = points) or 'devox'
    (lidal_devoxelize_bwd_sorted, n_entries = 8 * points).  Needs the library (the query), no GPU."""
    L = lib()
    rpw = 64 // lanes_per_row(case.form, case.dtype, case.c)
    special = ladder(rpw, case.form - 10 if case.form > 10 else 0) + ([BIG] if case.big else [])
    rng = np.random.default_rng(1000 * case.c + case.m + 7 * case.form + case.dtype + (0 if op == 'vox' else 50000))
    ids = rng.permutation(case.m)[:len(special)]
    for filler in range(0, 1 << 13):
        ne = _n_entries(sum(special) + (case.m - len(special)) * filler, op)
        if case.avg is not None and ne // case.m < case.avg[0]:
            continue
        if L.lidal_segment_form(ne, case.m, case.c, case.dtype) == case.form:
            break
    else:
        raise AssertionError('no filler length gives form %d for %s' % (case.form, case_id(case)))
    assert case.avg is None or ne // case.m <= case.avg[1], (case_id(case), ne // case.m)
    lengths = np.full(case.m, filler, dtype=np.int64)
    lengths[ids] = special
    # the exactness precondition: 64 * (largest term) * (longest list) is an integer below 2^24
    assert 64 * 8 * int(lengths.max()) < 2 ** 24
    return Layout(lengths, filler, ne, case.form, rpw)


def _rows(rng, n, c, dtype):
    return torch.from_numpy(rng.integers(-8, 9, size=(n, c), dtype=np.int8)).to(TORCH[dtype])


def _scatter(rng, lengths, m, n_slots):
    """Voxel ids for n_slots entries in a random order: the lists of `lengths`, then dead entries of kind 0 (-1), 1
    (>= m), 2 (caller's choice: a valid voxel).  Returns (ids, kind) with kind -1 for live entries."""
    live = int(lengths.sum())
    nd = n_slots - live
    assert nd >= 6
    ids = np.empty(n_slots, dtype=np.int32)
    ids[:live] = np.repeat(np.arange(m, dtype=np.int32), lengths)
    kind = np.full(n_slots, -1, dtype=np.int8)
    kind[live:] = np.arange(nd) % 3
    ids[live:] = np.where(kind[live:] == 0, -1,
                          np.where(kind[live:] == 1, m + rng.integers(0, 3, size=nd) * (2 ** 29), rng.integers(0, m, size=nd)))
    perm = rng.permutation(n_slots)
    return ids[perm], kind[perm]


def build_voxelize(m, c, dtype, lengths, seed, true_counts=False, normal=False):
    """Operands of lidal_voxelize_fwd_sorted over lists of `lengths`: rows [n, c], idx i32 [n] (also -1 and >= m),
    counts i32 [m] -- powers of two that are NOT the list lengths (the kernels divide by counts[v], whatever it is),
    or with true_counts the real lengths; normal: N(0, 1) rows instead of the exact integers (true_counts cases)."""
    rng = np.random.default_rng(seed)
    n = _n_entries(int(lengths.sum()), 'vox')
    ids, kind = _scatter(rng, lengths, m, n)
    ids[kind == 2] = m + 1                       # (voxelize has no third kind of dead entry)
    if normal:
        rows = torch.from_numpy(rng.standard_normal((n, c), dtype=np.float32)).to(TORCH[dtype])
    else:
        rows = _rows(rng, n, c, dtype)
    counts = lengths.astype(np.int32) if true_counts else (1 << rng.integers(0, 7, size=m)).astype(np.int32)
    return dict(rows=rows, idx=torch.from_numpy(ids), counts=torch.from_numpy(counts), m=m, c=c, n_entries=n)


def build_devoxelize(m, c, dtype, lengths, seed):
    """Operands of lidal_devoxelize_bwd_sorted: gout [n, c], idx8 i32 [n, 8], w8 f32 [n, 8] = k / 64; the live entries
    (valid voxel, weight > 0) form the lists of `lengths`, dealt into the 8 n corner slots at random among entries of
    -1, >= m and weight 0."""
    rng = np.random.default_rng(seed)
    slots = _n_entries(int(lengths.sum()), 'devox')
    ids, kind = _scatter(rng, lengths, m, slots)
    k = np.where(kind == -1, rng.integers(1, 65, size=slots), np.where(kind == 2, 0, rng.integers(0, 65, size=slots)))
    w8 = (k.astype(np.float32) / 64.0).reshape(-1, 8)
    n = slots // 8
    return dict(rows=_rows(rng, n, c, dtype), idx=torch.from_numpy(ids).view(n, 8), w=torch.from_numpy(w8), m=m, c=c,
                n_entries=slots)


def build_case(case, op, lay=None):
    lay = lay or layout(case, op)
    seed = 77 + 1000 * case.c + case.m + 7 * case.form + case.dtype
    if op == 'vox':
        return build_voxelize(case.m, case.c, case.dtype, lay.lengths, seed)
    return build_devoxelize(case.m, case.c, case.dtype, lay.lengths, seed + 1)


CELLS = [(F32, 16), (F32, 256), (BF16, 32), (BF16, 128), (BF16, 512)]        # 4 and 64 lanes; 4, 16 and 64 lanes


def build_cells(dtype, c, seed=5):
    """The structured index of lidal_devoxelize_bwd_cells: m = 120 cells, cell v has corner 0 = v and corners 1..7 drawn
    from [0, m) and -1; its point count comes from ladder(rpw, 1) (every length at least once), several cells are
    empty, the last one among them; every point of a cell has the cell's corner row.  Returns the devoxelize operands
    plus `points` (per cell)."""
    m = 120
    rng = np.random.default_rng(seed + 31 * c + dtype)
    lad = ladder(64 // (c // (4 if dtype == F32 else 8)), 1)
    assert len(lad) + 4 <= m - 1
    points = rng.choice(lad, size=m).astype(np.int64)
    ids = rng.permutation(m - 1)
    points[ids[:len(lad)]] = lad
    points[ids[len(lad):len(lad) + 3]] = 0
    points[m - 1] = 0
    corners = rng.integers(0, m, size=(m, 8)).astype(np.int32)
    corners[rng.random((m, 8)) < 0.2] = -1
    corners[:, 0] = np.arange(m)
    n = int(points.sum())
    cell = np.repeat(np.arange(m), points)[rng.permutation(n)]
    k = rng.integers(0, 65, size=(n, 8))
    k[rng.random((n, 8)) < 0.15] = 0
    idx8 = corners[cell]
    # exactness: a voxel's sum has at most this many terms
    live = (idx8 >= 0) & (k > 0)
    longest = int(np.bincount(idx8[live], minlength=m).max())
    assert 64 * 8 * longest < 2 ** 24
    return dict(rows=_rows(rng, n, c, dtype), idx=torch.from_numpy(idx8).contiguous(),
                w=torch.from_numpy(k.astype(np.float32) / 64.0), m=m, c=c, n_entries=8 * n, points=points)


# ---- the definitions, in f64 (torch, on whatever device the operands are) -------------------------------------------
def ref_voxelize(rows, idx, counts, m):
    """out[v] = sum over the points i with idx[i] == v of rows[i] / counts[v]  (f64; counts 0 divides by 1)."""
    idx = idx.long()
    ok = (idx >= 0) & (idx < m)
    v = idx[ok]
    div = counts.double().clamp_min(1.0)[v].unsqueeze(1)
    out = torch.zeros((m, rows.shape[1]), dtype=torch.float64, device=rows.device)
    return out.index_add_(0, v, rows[ok].double() / div)


def ref_devoxelize_bwd(gout, idx8, w8, m):
    """gin[v] = sum over the entries (i, k) with idx8[i, k] == v of w8[i, k] * gout[i]  (f64)."""
    flat = idx8.reshape(-1).long()
    e = torch.nonzero((flat >= 0) & (flat < m) & (w8.reshape(-1) != 0)).view(-1)
    out = torch.zeros((m, gout.shape[1]), dtype=torch.float64, device=gout.device)
    return out.index_add_(0, flat[e], gout.double()[e >> 3] * w8.reshape(-1).double()[e].unsqueeze(1))


def ref_devoxelize_fwd(feat, idx8, w8):
    """out[i] = sum over k of w8[i, k] * feat[idx8[i, k]], corners outside [0, m) or with weight 0 left out  (f64)."""
    m = feat.shape[0]
    out = torch.zeros((idx8.shape[0], feat.shape[1]), dtype=torch.float64, device=feat.device)
    fd = feat.double()
    for k in range(8):
        v = idx8[:, k].long()
        ok = (v >= 0) & (v < m) & (w8[:, k] != 0)
        out[ok] += w8[ok, k].double().unsqueeze(1) * fd[v[ok]]
    return out


def ref_voxelize_bwd(gout, idx, counts, residual=None):
    """gin[i] = gout[idx[i]] / counts[idx[i]] (0 for idx outside [0, m) or a count of 0), + residual[i]  (f64)."""
    m = gout.shape[0]
    idx = idx.long()
    ok = (idx >= 0) & (idx < m)
    ok[ok.clone()] = counts[idx[ok]] > 0
    out = torch.zeros((idx.shape[0], gout.shape[1]), dtype=torch.float64, device=gout.device)
    out[ok] = gout.double()[idx[ok]] / counts.double()[idx[ok]].unsqueeze(1)
    return out if residual is None else out + residual.double()
