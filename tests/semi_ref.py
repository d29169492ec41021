"""numpy restatement of lidal_amd.semi (csrc/semi.hip): the EMA update, the pseudo labels and the
consistency term with its gradient.  Every function takes the float type to compute in: np.float32 restates the
kernels operation by operation (bit for bit wherever no expf / logf is involved), np.float64 is the reference the
tolerances are measured against."""
import numpy as np

F32 = np.float32
KINDS = ('mse', 'kl')


# ---- EMA -------------------------------------------------------------------------------------------------------
def ema_alpha(alpha, updates, warmup=True):
    return min(float(alpha), 1.0 - 1.0 / (updates + 1)) if warmup else float(alpha)


def ema_update(t, s, alpha_eff, copy=False):
    """t + (s - t) * oma in f32, oma = (float)(1.0 - alpha_eff) formed in double; alpha_eff == 0, `copy` or a tensor
    that is not f32: the copy."""
    t, s = np.asarray(t), np.asarray(s)
    if alpha_eff == 0.0 or copy or t.dtype != np.float32:
        return s.copy()
    oma = F32(1.0 - float(alpha_eff))
    with np.errstate(all='ignore'):
        return (t + (s - t) * oma).astype(np.float32)


# ---- rows ------------------------------------------------------------------------------------------------------
def bf16_round(x):
    """f32 -> the nearest bf16 (ties to even) as f32: what a bf16 tensor holds."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16
    out = r.astype(np.uint32).view(np.float32)
    return np.where(np.isnan(x), x, out).astype(np.float32)


def row_softmax(x, ft=F32):
    """(e [n, c] = exp(x - mx), s [n] = their running sum in class order, mx [n], arg [n] = the first maximum)."""
    x = np.asarray(x).astype(ft)
    n, c = x.shape
    mx = np.full(n, -np.inf, ft)
    arg = np.zeros(n, np.int64)
    with np.errstate(all='ignore'):
        for j in range(c):
            up = x[:, j] > mx
            arg[up] = j
            mx = np.fmax(mx, x[:, j])
        e = np.exp(x - mx[:, None]).astype(ft)
        s = np.zeros(n, ft)
        for j in range(c):
            s = (s + e[:, j]).astype(ft)
    return e, s, mx, arg


def np_sum_rows(a):
    """numpy's pairwise add-reduce of every row of a [n, c <= 128] (csrc/npsum.h np_sum_f32), in a's own float type."""
    a = np.asarray(a)
    n, c = a.shape
    ft = a.dtype.type
    with np.errstate(all='ignore'):
        if c < 8:
            r = np.zeros(n, ft)
            for j in range(c):
                r = (r + a[:, j]).astype(ft)
            return r
        r = [a[:, j].copy() for j in range(8)]
        i = 8
        while i < c - (c % 8):
            for j in range(8):
                r[j] = (r[j] + a[:, i + j]).astype(ft)
            i += 8
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
        while i < c:
            res = (res + a[:, i]).astype(ft)
            i += 1
        return res.astype(ft)


# ---- pseudo labels ---------------------------------------------------------------------------------------------------
def confidence(logits, ft=F32):
    """(arg, conf) of every row: the first maximum and the softmax there."""
    e, s, _, arg = row_softmax(logits, ft)
    with np.errstate(all='ignore'):
        conf = (e[np.arange(len(arg)), arg] / s).astype(ft) if len(arg) else np.zeros(0, ft)
    return arg, conf


def pseudo_labels(logits, thresholds, inverse=None, labels=None, ignore_index=255, ft=F32):
    """(out i64 [p], stats i64 [c + 2], conf [p])."""
    logits = np.asarray(logits)
    nv, c = logits.shape
    thr = np.broadcast_to(np.asarray(thresholds, dtype=np.float32), (c,)).astype(ft)
    arg_v, conf_v = confidence(logits, ft)
    rows = np.arange(nv, dtype=np.int64) if inverse is None else np.asarray(inverse, dtype=np.int64)
    p = len(rows)
    inside = (rows >= 0) & (rows < nv)
    safe = np.where(inside, rows, 0)
    arg = np.where(inside, arg_v[safe], 0) if nv else np.zeros(p, np.int64)
    conf = np.where(inside, conf_v[safe], ft(0)).astype(ft) if nv else np.zeros(p, ft)
    human = np.full(p, ignore_index, np.int64) if labels is None else np.asarray(labels, dtype=np.int64)
    is_human = human != ignore_index
    with np.errstate(invalid='ignore'):
        accept = inside & ~is_human & (conf >= thr[arg])
    reject = inside & ~is_human & ~accept
    bad = ~inside & ~is_human
    out = np.full(p, ignore_index, np.int64)
    out[accept] = arg[accept]
    out[is_human] = human[is_human]
    stats = np.zeros(c + 2, np.int64)
    stats[:c] = np.bincount(arg[accept], minlength=c)
    stats[c] = reject.sum()
    stats[c + 1] = bad.sum()
    return out, stats, conf


# ---- consistency -----------------------------------------------------------------------------------------------
def _pair(zs, zt, kind, probs, ft):
    """ps, pt, conf of the teacher, dl = lt - ls (kl) per row."""
    zs, zt = np.asarray(zs).astype(ft), np.asarray(zt).astype(ft)
    n, c = zs.shape
    if probs:
        return zs, zt, np.fmax.reduce(zt, axis=1, initial=ft(-np.inf)).astype(ft), None
    es, ss, mxs, _ = row_softmax(zs, ft)
    et, st, mxt, arg = row_softmax(zt, ft)
    with np.errstate(all='ignore'):
        conf = (et[np.arange(n), arg] / st).astype(ft)
        ps = (es / ss[:, None]).astype(ft)
        pt = (et / st[:, None]).astype(ft)
        dl = None
        if kind == 'kl':
            ls = ((zs - mxs[:, None]).astype(ft) - np.log(ss).astype(ft)[:, None]).astype(ft)
            lt = ((zt - mxt[:, None]).astype(ft) - np.log(st).astype(ft)[:, None]).astype(ft)
            dl = (lt - ls).astype(ft)
    return ps, pt, conf, dl


def consistency(zs, zt, kind='mse', min_conf=0.0, probs=False, ft=F32):
    """(loss as a Python float (the rows summed exactly, math.fsum), per_row [n] masked, mask [n])."""
    import math
    assert kind in KINDS
    ps, pt, conf, dl = _pair(zs, zt, kind, probs, ft)
    n, c = ps.shape
    with np.errstate(all='ignore'):
        mask = conf >= ft(F32(min_conf))
        if kind == 'mse':
            d = (ps - pt).astype(ft)
            terms = (d * d).astype(ft)
        else:
            terms = np.where(pt == 0, ft(0), (pt * dl).astype(ft)).astype(ft)
        r = np.where(mask, np_sum_rows(terms), ft(0)).astype(ft)
    denom = float(n) * c if kind == 'mse' else float(n)
    loss = math.fsum(float(v) for v in r) / denom if n else 0.0
    return loss, r, mask


def consistency_grad(zs, zt, g=1.0, kind='mse', min_conf=0.0, probs=False, ft=F32):
    """d loss / d student * g, [n, c] in `ft`, the roundings of consistency_bwd_kernel."""
    ps, pt, conf, _ = _pair(zs, zt, kind, probs, ft)
    n, c = ps.shape
    with np.errstate(all='ignore'):
        mask = conf >= ft(F32(min_conf))
        d = (ps - pt).astype(ft)
        if kind == 'kl':
            coef = ft(ft(g) * ft(1.0 / float(n)))
            dz = (coef * d).astype(ft)
        elif probs:
            coef = ft(ft(g) * ft(2.0 / (float(n) * c)))
            dz = (coef * d).astype(ft)
        else:
            coef = ft(ft(g) * ft(1.0 / (float(n) * c)))
            a = (ft(2) * d).astype(ft)
            dot = np.zeros(n, ft)
            for j in range(c):
                dot = (dot + (ps[:, j] * a[:, j]).astype(ft)).astype(ft)
            dz = (coef * (ps * (a - dot[:, None]).astype(ft)).astype(ft)).astype(ft)
        return np.where(mask[:, None], dz, ft(0)).astype(ft)


# ---- inputs and thresholds the CPU and GPU tests share --------------------------------------------------------------
def logits_grid(n, c, seed, dtype='f32'):
    """Rows of magnitude 1 / 3 / 30 clipped to +-80, with tied maxima, a class at -inf, an all-equal row and (pseudo labels
    only: `nan_row`) a NaN row where n allows; f32 values, rounded to bf16 for dtype 'bf16'."""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(n, c)) * rng.choice([1.0, 3.0, 30.0], size=(n, 1))
    x = np.clip(x, -80.0, 80.0).astype(np.float32)
    if dtype == 'bf16':
        x = bf16_round(x)
    if n >= 8 and c >= 2:
        x[1, :] = x[1, 0]                       # an all-equal row
        x[2, c - 1] = x[2].max()                # tied maxima: the first wins
        x[2, 0] = x[2, c - 1]
        x[3, c // 2] = -np.inf                  # a class at -inf
    return x


def gap_threshold(conf64, lo=0.3, hi=0.99):
    """The midpoint of the widest gap between the sorted f64 confidences inside [lo, hi] (the bounds count as
    confidences), and that gap: a threshold no confidence is near."""
    v = np.asarray(conf64, dtype=np.float64)
    v = np.sort(np.concatenate([[lo, hi], v[np.isfinite(v) & (v > lo) & (v < hi)]]))
    gaps = np.diff(v)
    k = int(np.argmax(gaps))
    return float(v[k] + gaps[k] / 2), float(gaps[k])
