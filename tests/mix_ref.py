"""numpy restatement of the mixed samples (lidal_mix_scans).  TEST CODE: the definition is the
project's own (no mixing exists in the reference, and the LaserMix / PolarMix papers' code is not reproduced), written
here once more in numpy so that the kernels can be pinned bit for bit.

Every f32 operation is rounded on its own: numpy's f32 products, sums, differences and square root are correctly
rounded, which is what csrc/mix.hip computes with __fmul_rn / __fadd_rn / __fsub_rn / sqrtf.  No atan, no atan2.

A mix is any record with the fields of lidal_amd.data.Mix (a, b, tans, wedge, take_a, take_b, paste_classes, paste_rot).
"""
import numpy as np

PARTS = 6
F = np.float32


def cells(xyz, tans, wedge):
    """xyz f32 [P,3] -> (band, in_sector, cell) per point, as the kernel evaluates them."""
    with np.errstate(all='ignore'):
        x, y, z = (np.ascontiguousarray(xyz[:, k], dtype=F) for k in range(3))
        r = np.sqrt(x * x + y * y)                              # f32 throughout: each operation rounds once
        assert r.dtype == F
        band = np.zeros(len(x), dtype=np.int64)
        for t in np.asarray(tans, dtype=F):
            band += z >= t * r                                  # NaN compares false
        inw = np.zeros(len(x), dtype=bool)
        if wedge is not None:
            d0x, d0y, d1x, d1y = (F(v) for v in wedge)
            inw = (d0x * y - d0y * x >= F(0)) & (d1x * y - d1y * x < F(0))
    return band, inw, band + (len(tans) + 1) * inw


def _bits(mask, idx):
    """bit idx[i] of the 64-bit mask, per element."""
    table = np.array([(int(mask) >> c) & 1 for c in range(64)], dtype=bool)
    return table[idx]


def mix_one(xyz, intensity, labels, point_ptr, m):
    """One mix -> (xyz, intensity, labels or None, src, parts i64 [6])."""
    a0, a1, b0, b1 = (int(point_ptr[i]) for i in (m.a, m.a + 1, m.b, m.b + 1))
    rows_a, rows_b = np.arange(a0, a1, dtype=np.int64), np.arange(b0, b1, dtype=np.int64)
    wedge = None if m.wedge is None else np.asarray(m.wedge, dtype=F)
    keep_a = _bits(m.take_a, cells(xyz[a0:a1], m.tans, wedge)[2])
    keep_b = _bits(m.take_b, cells(xyz[b0:b1], m.tans, wedge)[2])
    src = [rows_a[keep_a], rows_b[keep_b]]
    out = [xyz[src[0]], xyz[src[1]]]
    rot = np.asarray(m.paste_rot, dtype=F).reshape(-1, 2)
    if len(rot):
        lab_b = labels[b0:b1]
        ok = (lab_b >= 0) & (lab_b < 64)
        pasted = rows_b[ok & _bits(m.paste_classes, np.where(ok, lab_b, 0))]
        for c, s in rot:
            p = xyz[pasted].copy()
            x, y = p[:, 0].copy(), p[:, 1].copy()
            with np.errstate(all='ignore'):
                p[:, 0] = c * x - s * y
                p[:, 1] = s * x + c * y
            src.append(pasted)
            out.append(p)
    parts = np.zeros(PARTS, dtype=np.int64)
    parts[:len(src)] = [len(s) for s in src]
    src = np.concatenate(src)
    return (np.concatenate(out).astype(F).reshape(-1, 3), intensity[src], None if labels is None else labels[src], src,
            parts)


def mix_scans(xyz, intensity, labels, point_ptr, mixes):
    """The concatenated input (xyz f32 [P,3], intensity f32 [P], labels i64 [P] or None, point_ptr i64 [S+1]) and a list of
    mixes -> the dict of data.mix_scans as numpy arrays."""
    xyz = np.ascontiguousarray(xyz, dtype=F).reshape(-1, 3)
    intensity = np.ascontiguousarray(intensity, dtype=F).reshape(-1)
    labels = None if labels is None else np.ascontiguousarray(labels, dtype=np.int64).reshape(-1)
    outs = [mix_one(xyz, intensity, labels, point_ptr, m) for m in mixes]
    ptr = np.concatenate([[0], np.cumsum([len(o[3]) for o in outs])]).astype(np.int64)
    return {'points': np.concatenate([o[0] for o in outs]).reshape(-1, 3),
            'intensity': np.concatenate([o[1] for o in outs]),
            'labels': None if labels is None else np.concatenate([o[2] for o in outs]),
            'src': np.concatenate([o[3] for o in outs]), 'point_ptr': ptr,
            'parts': np.stack([o[4] for o in outs]).astype(np.int64)}
