"""BatchNorm over the rows of a [N, C] matrix, restated in f64, with the error bounds the kernel forms of
csrc/bn.hip are held to (tests/test_batchnorm_edges_gpu.py) and that the reference alone is shown to respect
(tests/test_batchnorm_ref_cpu.py).

Every bound is derived from the kernel's expressions, never from what a kernel returns.  u = 2^-24 is the unit
roundoff of f32, ub = 2^-8 that of bf16.  A bound counts one u per f32 operation of the uncontracted expression; a
contracted (fma) evaluation skips a rounding and so stays inside the same bound.  The functions work on numpy arrays
(xp = NP) and on torch tensors (xp = TH: the GPU tests keep the f64 arithmetic on the device); all arithmetic is f64.
"""
import math

import numpy as np
import torch

U = 2.0 ** -24
UB = 2.0 ** -8
AMBIGUOUS_CAP = 1e-5          # share of a case's elements whose ReLU mask may be ambiguous, at most
EPS = float(np.float32(1e-5))       # the kernels take eps as a float and widen it
MOMENTUM = 0.1

# ---- the launch geometry of csrc/bn.hip, restated ------------------------------------------------------------------
NT = 256
BN_WGS = 256
MIN_ROWS_PER_WG = 32
EW_WIDE_BYTES = 12 << 20
SLOT_CH = 2048
TILE = 128
VEC = {'f32': 4, 'bf16': 8}
ESIZE = {'f32': 4, 'bf16': 2}


def rows_per_wg(n):
    return max(MIN_ROWS_PER_WG, -(-n // BN_WGS))


def rows_per_wg_ew(n, row_bytes):
    wgs = 2 * BN_WGS if n * row_bytes >= EW_WIDE_BYTES else BN_WGS
    return max(MIN_ROWS_PER_WG, -(-n // wgs))


def nparts(n):
    return -(-max(n, 1) // rows_per_wg(n))


def nslabs_ew(n, row_bytes):
    return -(-max(n, 1) // rows_per_wg_ew(n, row_bytes))


def workspace_bytes(n, c):
    return nparts(n) * c * 3 * 8 + 256


def rows_per_sweep(c, dt):
    return NT // (c // VEC[dt])


def chain_length(rpw, rpi):
    """The longest chain of f32 additions behind one slab sum: a lane adds ceil(rpw / rpi) terms to its accumulator,
    the LDS tree over the rpi lanes is ceil(log2 rpi) deep."""
    return -(-rpw // rpi) + (int(math.ceil(math.log2(rpi))) if rpi > 1 else 0)


# ---- shapes: the smallest at which each path of the row loop changes ------------------------------------------------
CHANNELS = {'f32': [4, 24, 96, 128, 256, 516, 1024], 'bf16': [8, 48, 96, 256, 1032, 2048]}
ROWS = [2, 31, 32, 33, 63, 64, 65, 8191, 8192, 8193]
WIDE = {'f32': [(262145, 4), (16385, 256)], 'bf16': [(262145, 8), (16385, 512)]}


def shapes(dt, with_one_row=False):
    """(n, c): every channel count at n in {2, 33, 8193}, every row count at c = 96 and 256, the two wide cases; and
    n = 1 (C entry points only) on request."""
    s = [(n, c) for c in CHANNELS[dt] for n in (2, 33, 8193)]
    s += [(n, c) for c in (96, 256) for n in ROWS]
    s += WIDE[dt]
    if with_one_row:
        s += [(1, 96), (1, 256)]
    out = []
    for p in s:
        if p not in out:
            out.append(p)
    return out


def all_cases(with_one_row=False):
    return [(dt, n, c) for dt in ('f32', 'bf16') for n, c in shapes(dt, with_one_row)]


def case_id(v):
    return '%s-%dx%d' % v if isinstance(v, tuple) and len(v) == 3 else str(v)


# ---- namespaces: the few array functions the reference needs, for numpy and for torch -------------------------------
class NP:
    where, maximum, minimum, sqrt, frexp, exp2, abs = np.where, np.maximum, np.minimum, np.sqrt, np.frexp, np.exp2, np.abs

    @staticmethod
    def f64(a):
        return np.asarray(a).astype(np.float64)

    @staticmethod
    def zeros_like(a):
        return np.zeros_like(a)


class TH:
    where, maximum, minimum, sqrt, frexp, exp2, abs = (torch.where, torch.maximum, torch.minimum, torch.sqrt, torch.frexp,
                                                      torch.exp2, torch.abs)

    @staticmethod
    def f64(a):
        return a.double()

    @staticmethod
    def zeros_like(a):
        return torch.zeros_like(a)


def round_bf16(a):
    """f32 -> nearest bf16 (ties to even), returned as f32."""
    b = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    return ((b + (((b >> 16) & 1) + 0x7FFF)) & 0xFFFF0000).astype(np.uint32).view(np.float32)


def quantise(a, dt):
    a = np.asarray(a, dtype=np.float32)
    return round_bf16(a) if dt == 'bf16' else a


def ulp32(v, xp=NP):
    """Spacing of f32 at |v| (v in f64), never below the smallest subnormal step."""
    _, e = xp.frexp(xp.abs(v))
    e = xp.f64(e)
    e = xp.where(v == 0, xp.zeros_like(e) - 125.0, xp.maximum(e, xp.zeros_like(e) - 125.0))
    return xp.exp2(e - 24.0)


def _ratio(err, bound, xp):
    """max(err / bound); an error where the bound is zero counts as infinite."""
    big = xp.zeros_like(err) + float('inf')
    r = xp.where(bound > 0, err / xp.where(bound > 0, bound, bound + 1.0), xp.where(err > 0, big, xp.zeros_like(err)))
    return float(r.max()) if int(np.prod(tuple(r.shape))) else 0.0


# ---- seeded operands ------------------------------------------------------------------------------------------------
# a case whose reference exceeded the ambiguity cap gets another seed here (never a wider cap)
SEED_BUMP = {}


class Case:
    """The operands of one (dtype, n, c), each generated on first use from its own stream of the case's seed; matrix
    operands are rounded to the case's dtype and returned as f32 arrays."""
    _ORDER = ('x', 'dy', 'dyi', 'res', 'out', 'xb', 'gamma', 'beta', 'rm0', 'rv0')

    def __init__(self, dt, n, c):
        self.dt, self.n, self.c = dt, n, c
        self.seed = (1000003 if dt == 'bf16' else 0) + 4099 * n + c + SEED_BUMP.get((dt, n, c), 0)
        self._made = {}

    def __getitem__(self, name):
        if name not in self._made:
            self._made[name] = self._make(name)
        return self._made[name]

    def _make(self, name):
        n, c, dt = self.n, self.c, self.dt
        rng = np.random.default_rng([self.seed, self._ORDER.index(name)])

        def randn(*s):
            return rng.standard_normal(s, dtype=np.float32)
        if name == 'x':
            x = randn(n, c) * np.float32(1.5) + np.float32(0.3)
            x[:, 1] = x[:, 1] * np.float32(0.05) + np.float32(10.0)       # |mean| >> std
            return quantise(x, dt)
        if name == 'xb':
            return quantise(randn(n, c) * np.float32(0.7) - np.float32(0.2), dt)
        if name in ('dy', 'res', 'out'):
            return quantise(randn(n, c), dt)
        if name == 'dyi':
            return rng.integers(-8, 9, size=(n, c)).astype(np.float32)
        if name == 'gamma':
            return randn(c) + np.float32(0.25)
        if name == 'beta':
            return randn(c) * np.float32(0.5)
        if name == 'rm0':
            return rng.random(c, dtype=np.float32) * np.float32(0.5) + np.float32(0.1)
        if name == 'rv0':
            return rng.random(c, dtype=np.float32) + np.float32(0.5)
        raise KeyError(name)


# ---- forward --------------------------------------------------------------------------------------------------------
def batch_stats(x, eps=EPS, xp=NP):
    """-> (mean, biased var, unbiased var (the biased one for n = 1), invstd) of the columns of x, f64."""
    n = x.shape[0]
    mean = x.sum(0) / n
    m2 = ((x - mean) ** 2).sum(0)
    var = m2 / n
    return mean, var, (m2 / (n - 1) if n > 1 else var), 1.0 / xp.sqrt(var + eps)


def tile_merge(triples, c, eps=EPS, xp=NP):
    """The f64 merge N, S1 = sum n m, S2 = sum (M2 + n m^2) of f32 (count, mean, M2) triples laid out [c][tiles][3]
    -> (mean, var, unbiased var, invstd)."""
    t = xp.f64(triples).reshape(c, -1, 3)
    pn, pm, pq = t[:, :, 0], t[:, :, 1], t[:, :, 2]
    n = pn.sum(1)
    mean = (pn * pm).sum(1) / n
    m2 = xp.maximum((pq + pn * pm * pm).sum(1) - n * mean * mean, xp.zeros_like(mean))
    var = m2 / n
    unb = xp.where(n > 1, m2 / xp.maximum(n - 1, xp.zeros_like(n) + 0.5), var)
    return mean, var, unb, 1.0 / xp.sqrt(var + eps)


def stats_ulps(save_mean, save_invstd, mean, invstd, xp=NP):
    """Errors of the saved f32 statistics in f32 ulps of the f64 values.  The kernel accumulates in f64 and rounds
    once: half an ulp plus what f64 leaves (1 ulp asked for the mean); invstd is the rounding of 1 / sqrt(var + eps)
    of an f64 variance (2 ulp asked)."""
    em = xp.abs(xp.f64(save_mean) - mean) / ulp32(mean, xp)
    ei = xp.abs(xp.f64(save_invstd) - invstd) / ulp32(invstd, xp)
    return float(em.max()), float(ei.max())


def running_ref(r0, value, momentum=MOMENTUM):
    """(1 - momentum) * r0 + momentum * (float)value: the kernel's f32 expression in numpy.  -> (f32 result, f32 ulp
    at the larger of the two products and the result: each product is rounded at its own magnitude, so a cancelling
    sum is not asked for more than its terms carry)."""
    m = np.float32(momentum)
    r0 = np.asarray(r0, dtype=np.float32)
    v = np.asarray(value, dtype=np.float64).astype(np.float32)
    a, b = (np.float32(1) - m) * r0, m * v
    res = a + b
    mag = np.maximum(np.maximum(np.abs(a), np.abs(b)), np.abs(res)).astype(np.float64)
    return res, ulp32(mag)


def running_ulps(got, r0, value, momentum=MOMENTUM):
    """Three roundings (two products, the sum) and the half ulp by which the kernel's (float)value may differ from the
    reference's, scaled by the momentum: at most 2 ulp."""
    res, ulp = running_ref(r0, value, momentum)
    return float((np.abs(np.asarray(got, dtype=np.float64) - res.astype(np.float64)) / ulp).max())


def forward_ratio(y, x, mu, sigma, gamma, beta, relu, res, dt, xp=NP, var_in=False):
    """max |y - ref| / bound per element.  ref = (x - mu) * (sigma * gamma) + beta in f64 with the kernel's own saved
    f32 mu and sigma; relu bit 0: ReLU on that; res: + residual (after a rounding to the dtype), relu bit 1: ReLU on
    the sum.

    Bound: 4 roundings (the difference, sigma * gamma, the product, the sum), each at most u of a value no larger
    than |x - mu| |sigma gamma| + |beta|: e = 4u (|x - mu| |sigma gamma| + |beta|).  var_in (the eval form,
    sigma = 1 / sqrt(var + eps) in f32): the sum var + eps, the square root and the division add 3 roundings of sigma
    (the issue counts two; the addition is a third), so 7u on the product term.  ReLU is 1-Lipschitz: e is unchanged.
    Residual: the intermediate v is rounded to the dtype (bf16: ub |v| + the (1 + ub) that the rounding of a perturbed
    value adds to e; f32: nothing) and one f32 addition rounds u |v + r|.  bf16 output: the value that is rounded is
    off by e already, so e (1 + ub) + ub |y|."""
    sg = sigma * gamma
    v = (x - mu) * sg + beta
    k = 7.0 if var_in else 4.0
    e = k * U * xp.abs(x - mu) * xp.abs(sg) + 4.0 * U * xp.abs(beta) + xp.zeros_like(x)
    zero = xp.zeros_like(v)
    if relu & 1:
        v = xp.maximum(v, zero)
    if res is not None:
        if dt == 'bf16':
            e = e * (1.0 + UB) + UB * xp.abs(v)
        v = v + res
        e = e + U * (xp.abs(v) + e)
        if relu & 2:
            v = xp.maximum(v, zero)
    if dt == 'bf16':
        e = e * (1.0 + UB) + UB * xp.abs(v)
    return _ratio(xp.abs(y - v), e, xp), v


# ---- backward -------------------------------------------------------------------------------------------------------
class Backward:
    """The f64 terms of one backward pass with the kernel's saved f32 statistics: xhat, the masked gradient dy', the
    ambiguous elements of the ReLU mask (|xhat gamma + beta| <= 4u (|xhat gamma| + |beta|): the f32 evaluation
    (two roundings in xhat, the product, the sum) may land on either side of zero), the two column sums with their
    sums of magnitudes and what the ambiguous elements may add to them."""

    def __init__(self, x, dy, mu, sigma, gamma, beta, relu, xp=NP):
        self.xp, self.n = xp, x.shape[0]
        self.gamma, self.sigma = gamma, sigma
        self.xhat = (x - mu) * sigma
        zero = xp.zeros_like(x)
        self.dy_raw = dy
        if relu:
            z = self.xhat * gamma + beta
            self.amb = xp.abs(z) <= 4.0 * U * (xp.abs(self.xhat * gamma) + xp.abs(beta))
            self.dyp = xp.where(z > 0, dy, zero)
            amb_dy = xp.where(self.amb, xp.abs(dy), zero)
            self.n_amb = int(self.amb.sum())
            self.slack_b = amb_dy.sum(0)
            self.slack_g = (amb_dy * xp.abs(self.xhat)).sum(0)
        else:
            self.amb, self.dyp, self.n_amb = None, dy + zero, 0
            self.slack_b = self.slack_g = xp.zeros_like(gamma + mu)
        self.tb, self.tg = self.dyp, self.dyp * self.xhat
        self.sum_b, self.sum_g = self.tb.sum(0), self.tg.sum(0)
        self.mag_b, self.mag_g = xp.abs(self.tb).sum(0), xp.abs(self.tg).sum(0)

    def ambiguous_share(self):
        return self.n_amb / float(self.dyp.shape[0] * self.dyp.shape[1])

    def sums_ratio_f64(self, gb, gg):
        """f64-sum forms: |err| <= 3u sum|terms| + u |sum|.  A term dy * xhat carries the two roundings of
        xhat = (x - mu) * sigma (2u); the products and sums are f64 (2^-53 each, inside the third u); the result is
        rounded to f32 once (u |sum|).  sum dy has exact terms and is held to the same bound."""
        xp = self.xp
        rb = _ratio(xp.abs(gb - self.sum_b), 3 * U * self.mag_b + U * xp.abs(self.sum_b) + self.slack_b, xp)
        rg = _ratio(xp.abs(gg - self.sum_g), 3 * U * self.mag_g + U * xp.abs(self.sum_g) + self.slack_g, xp)
        return rb, rg

    def sums_ratio_f32(self, gb, gg, k):
        """f32 slab forms: (k + 3) u sum|terms|, k the longest chain of f32 additions (chain_length): every addition
        rounds at most u of a partial sum no larger than sum|terms| (k u), the term carries 3 roundings (xhat twice,
        the product), the slabs are merged in f64 and rounded once (inside the bound: |sum| <= sum|terms| and the
        first addition of a chain, to zero, is exact)."""
        xp = self.xp
        rb = _ratio(xp.abs(gb - self.sum_b), (k + 3) * U * self.mag_b + self.slack_b, xp)
        rg = _ratio(xp.abs(gg - self.sum_g), (k + 3) * U * self.mag_g + self.slack_g, xp)
        return rb, rg

    def dx_ref(self, gb, gg, d=None):
        """gamma sigma (dy' - sum dy' / n - xhat sum dy' xhat / n)"""
        d = self.dyp if d is None else d
        return self.gamma * self.sigma * (d - gb / self.n - self.xhat * (gg / self.n))

    def dx_ratio(self, dx, gb, gg, dt):
        """dx against gamma sigma (dy' - k1 - xhat k2) with k1, k2 from the kernel's own f32 sums.  8 roundings at
        most u each of a value no larger than |gamma sigma| (|dy'| + |k1| + |xhat k2|): xhat (2), k1, k2 (the products
        with 1 / n, itself rounded: 2 each, counted once per term they enter), xhat k2, the two differences,
        gamma sigma and the last product -- 8u |gamma sigma| (|dy'| + |k1| + |xhat k2|); bf16 adds ub |dx| and the
        (1 + ub) of rounding a perturbed value.  An ambiguous element may take either branch of the mask."""
        xp = self.xp
        gs = self.gamma * self.sigma
        k1, k2 = gb / self.n, gg / self.n

        def one(d):
            ref = self.dx_ref(gb, gg, d)
            e = 8 * U * xp.abs(gs) * (xp.abs(d) + xp.abs(k1) + xp.abs(self.xhat * k2))
            if dt == 'bf16':
                e = e * (1.0 + UB) + UB * xp.abs(ref)
            err = xp.abs(dx - ref)
            return xp.where(e > 0, err / xp.where(e > 0, e, e + 1.0), xp.where(err > 0, err + float('inf'), err))
        r = one(self.dyp)
        if self.amb is not None and self.n_amb:
            other = xp.where(self.dyp == 0, self.dy_raw, xp.zeros_like(self.dyp))
            r = xp.where(self.amb, xp.minimum(r, one(other)), r)
        return float(r.max())


def tile_sums_ref(tb, tg, tile=TILE):
    """f32 (sum dy', sum dy' xhat) per tile of rows, laid out [c][tiles][2] as a data-gradient launch leaves them
    (numpy, f64 sums rounded once)."""
    n, c = tb.shape
    tiles = -(-n // tile)
    out = np.zeros((c, tiles, 2), dtype=np.float32)
    idx = np.arange(0, n, tile)
    out[:, :, 0] = np.add.reduceat(tb, idx, axis=0).T
    out[:, :, 1] = np.add.reduceat(tg, idx, axis=0).T
    return out


def merged_ulps(got, tiles, which, xp=NP):
    """A merge of given f32 pairs in f64, rounded once: at most 1 ulp of the f64 sum of the same pairs; the ulp is
    taken at sum|pairs| 2^-28 at least, which is what f64 sums in another order may differ by at most (2^-52 n)."""
    t = xp.f64(tiles)[:, :, which]
    s = t.sum(1)
    floor = ulp32(xp.abs(t).sum(1) * 2.0 ** -28, xp)
    return float((xp.abs(xp.f64(got) - s) / xp.maximum(ulp32(s, xp), floor)).max())


# ---- the kernel's expressions in numpy f32 (what test_batchnorm_ref_cpu.py holds to the same bounds) ----------------
def emulate_forward(x, mu32, sig32, gamma, beta, relu, res, dt, var_in=False, eps=EPS):
    f = np.float32
    x, gamma, beta = x.astype(f), gamma.astype(f), beta.astype(f)
    if var_in:
        sig32 = f(1) / np.sqrt(sig32.astype(f) + f(eps))
    sc = sig32.astype(f) * gamma
    y = (x - mu32.astype(f)) * sc + beta
    if relu & 1:
        y = np.maximum(y, f(0))
    if res is not None:
        y = quantise(y, dt) + res.astype(f)
        if relu & 2:
            y = np.maximum(y, f(0))
    return quantise(y, dt)


def emulate_terms(x, dy, mu32, sig32, gamma, beta, relu):
    f = np.float32
    xhat = (x.astype(f) - mu32.astype(f)) * sig32.astype(f)
    d = dy.astype(f)
    if relu:
        d = np.where(xhat * gamma.astype(f) + beta.astype(f) > 0, d, f(0))
    return xhat, d


def emulate_sums_f64(xhat, d):
    """bn_bwd_partial_kernel + bn_bwd_final_kernel: f32 terms, f64 products and sums, one rounding."""
    return d.astype(np.float64).sum(0).astype(np.float32), (d.astype(np.float64) * xhat.astype(np.float64)).sum(0).astype(np.float32)


def emulate_sums_f32(xhat, d, rpw, rpi):
    """bn_bwd_slab_sums_kernel / tail_tile_sums_kernel: lane rl of a slab adds rows rl, rl + rpi, ... in f32 in row
    order, an LDS tree (halving spans, as tree_sum_rows) adds the lanes; the slabs are merged in f64 and rounded."""
    f = np.float32
    n, c = d.shape
    slabs = -(-n // rpw)
    steps = -(-rpw // rpi)

    def run(t):
        pad = np.zeros((slabs, steps * rpi, c), dtype=f)
        flat = np.zeros((slabs * rpw, c), dtype=f)
        flat[:n] = t
        pad[:, :rpw] = flat.reshape(slabs, rpw, c)
        pad = pad.reshape(slabs, steps, rpi, c)
        acc = np.zeros((slabs, rpi, c), dtype=f)
        for s in range(steps):
            acc = acc + pad[:, s]
        span = 1
        while span < rpi:
            span <<= 1
        s = span >> 1
        while s >= 1:
            hi = min(rpi - s, s)
            if hi > 0:
                acc[:, :hi] = acc[:, :hi] + acc[:, s:s + hi]
            s >>= 1
        return acc[:, 0].astype(np.float64).sum(0).astype(f)
    return run(d), run(d * xhat)


def emulate_dx(xhat, d, sig32, gamma, gb32, gg32, n, dt):
    f = np.float32
    inv_n = f(1) / f(n)
    k1, k2 = gb32.astype(f) * inv_n, gg32.astype(f) * inv_n
    return quantise(gamma.astype(f) * sig32.astype(f) * (d - k1 - xhat * k2), dt)


def _tile_triples(x, tile=128):
    """(count, mean, M2) per 128-row tile and channel, what a convolution's epilogue leaves: f32, laid out
    [c][tiles][3] (csrc/conv_img.hip store_tile) -- returned with that buffer's shape recorded as (tiles, c, 3)."""
    n, c = x.shape
    xf = x.float()
    out = []
    for r in range(0, n, tile):
        blk = xf[r:r + tile]
        m = blk.mean(0)
        out.append(torch.stack([torch.full_like(m, blk.shape[0]), m, ((blk - m) ** 2).sum(0)], 1))
    t = torch.stack(out, 0)                                     # [tiles, c, 3]
    return t.permute(1, 0, 2).contiguous().view(t.shape[0], t.shape[1], 3)     # the bytes of [c][tiles][3]
