"""A numpy restatement of the counter-based dropout (csrc/dropout.hip).  TEST INFRASTRUCTURE.

Philox4x32-10 with Random123's constants; element e = first + i takes word e & 3 of the generator under key
(seed lo, seed hi) and counter (g lo, g hi, call lo, call hi), g = e >> 2, and is kept iff that word is below
thr = min(floor((1 - p) * 2^32), 0xffffffff); the result is rn_dtype(f32(x) * m), m = f32(1 / (1 - p)) or 0.0f.
bf16 tensors travel as their uint16 bit patterns."""
import math

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter: four uint32 values or arrays, key: two ints -> the four output words (uint64 arrays holding 32 bits)."""
    c0, c1, c2, c3 = (np.atleast_1d(np.asarray(c, dtype=np.uint64)) for c in counter)
    k0, k1 = int(key[0]) & MASK32, int(key[1]) & MASK32
    m32 = np.uint64(MASK32)
    s32 = np.uint64(32)
    for _ in range(10):
        p0 = np.uint64(M0) * c0                 # (32 x 32 bits: fits 64)
        p1 = np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ np.uint64(k0), p1 & m32, (p0 >> s32) ^ c3 ^ np.uint64(k1), p0 & m32
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return c0, c1, c2, c3


def words(n, seed, call, first=0):
    """The 32-bit word of each of n elements starting at element `first` (uint64 array)."""
    e = np.uint64(first) + np.arange(n, dtype=np.uint64)
    g = e >> np.uint64(2)
    g0 = int(g[0]) if n else 0
    groups = np.arange(g0, g0 + (int(g[-1]) - g0 + 1 if n else 0), dtype=np.uint64)
    m32, s32 = np.uint64(MASK32), np.uint64(32)
    out = philox4x32_10((groups & m32, groups >> s32, np.full(groups.shape, call & MASK32, np.uint64),
                         np.full(groups.shape, (call >> 32) & MASK32, np.uint64)), (seed & MASK32, (seed >> 32) & MASK32))
    table = np.stack(out, axis=1)               # [groups, 4]
    return table[(g - np.uint64(g0)).astype(np.int64), (e & np.uint64(3)).astype(np.int64)]


def constants(p):
    """(thr, scale f32) as the host forms them."""
    thr = min(int(math.floor((1.0 - float(p)) * 2.0 ** 32)), MASK32)
    scale = np.float32(1.0 / (1.0 - float(p))) if p < 1 else np.float32(np.inf)
    return thr, scale


def keep(n, p, seed, call, first=0):
    thr, _ = constants(p)
    return words(n, seed, call, first) < np.uint64(thr)


def multiplier(n, p, seed, call, first=0):
    """m f32 [n]: scale where kept, 0.0 where dropped."""
    _, scale = constants(p)
    return np.where(keep(n, p, seed, call, first), scale, np.float32(0)).astype(np.float32)


def apply_f32(x, p, seed, call, first=0):
    x = np.ascontiguousarray(x, np.float32).reshape(-1)
    with np.errstate(invalid='ignore', over='ignore'):
        return x * multiplier(x.size, p, seed, call, first)


def bf16_to_f32(bits):
    return (np.ascontiguousarray(bits, np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def f32_to_bf16(x):
    """Round to nearest even; a NaN stays a NaN (0x7fc0: the tests compare NaN-ness, not payloads)."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    r = ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)
    return np.where(np.isnan(x), np.uint16(0x7FC0), r)


def apply_bf16(bits, p, seed, call, first=0):
    """bits uint16 [n] -> uint16 [n]: rn_bf16(f32(x) * m)."""
    x = bf16_to_f32(np.asarray(bits).reshape(-1))
    with np.errstate(invalid='ignore', over='ignore'):
        return f32_to_bf16(x * multiplier(x.size, p, seed, call, first))
