"""A plain restatement of the view-disagreement scores (csrc/score.hip view_scores_kernel).  TEST
INFRASTRUCTURE.

LiDAL.py:59-81 with a frame's own view mean where the query frame stands and its `reps` augmented views where the
matched neighbour frames stand.  scores_from_logits is the definition in f64 throughout, what the GPU tests hold the
kernel to; scores_from_view_probs restates the kernel's number widths on given f32 view probabilities, and
tests/test_view_scores_cpu.py pins it against scipy's kl_div and entropy applied as LiDAL.py:71,76 applies them."""
import numpy as np

EPSILON = np.float32(0.00001)          # LiDAL.py:64, as the f32 the kernel adds


def scores_from_logits(logits, inverse, reps):
    """logits [NV, C], inverse i64 [reps * P] -> dict, everything in f64:
    prob [P, C], pred i64 [P] (first maximum), viewd [P], viewe [P], view_arg i64 [reps, P] (the first-maximum class of
    every view's logits row)."""
    logits = np.asarray(logits, np.float64)
    p, c = np.asarray(inverse).shape[0] // reps, logits.shape[1]
    rows = logits[np.asarray(inverse)].reshape(reps, p, c)
    view_arg = rows.argmax(axis=2)
    with np.errstate(invalid='ignore'):
        e = np.exp(rows - rows.max(axis=2, keepdims=True))
    pv = e / e.sum(axis=2, keepdims=True)
    m = pv.mean(axis=0)
    eps = float(EPSILON)
    x, y = (m + eps)[None], pv + eps
    viewd = (x * np.log(x / y) - x + y).sum(axis=2).mean(axis=0)
    q = m / m.sum(axis=1, keepdims=True)
    with np.errstate(divide='ignore', invalid='ignore'):
        viewe = np.where(q > 0, -q * np.log(q), 0.0).sum(axis=1)
    return {'prob': m, 'pred': m.argmax(axis=1), 'viewd': viewd, 'viewe': viewe, 'view_arg': view_arg}


def scores_from_view_probs(pv):
    """pv f32 [reps, P, C], the soft-max rows of every view -> (m f32 [P, C], viewd f64 [P], viewe f32 [P]) with the
    kernel's widths: m = p_0, f32 adds in view order, / f32(reps); a KL term is the f64 expression of f32 (m + eps) and
    (p_v + eps) rounded to f32; numpy's f32 sum over the classes; an f64 accumulator over the views, / f64(reps); the
    entropy terms of m / sum(m) likewise f64 expressions rounded to f32, summed in f32."""
    pv = np.ascontiguousarray(pv, np.float32)
    reps = pv.shape[0]
    m = pv[0].copy()
    for v in range(1, reps):
        m = m + pv[v]
    m = m / np.float32(reps)
    assert m.dtype == np.float32
    viewd = np.zeros(pv.shape[1], np.float64)
    x = (m + EPSILON).astype(np.float64)
    for v in range(reps):
        y = (pv[v] + EPSILON).astype(np.float64)
        terms = (x * np.log(x / y) - x + y).astype(np.float32)
        viewd += np.sum(terms, axis=1)
    viewd /= float(reps)
    q = m / np.sum(m, axis=1, keepdims=True)
    q64 = q.astype(np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        ent = np.where(q > 0, (-q64 * np.log(q64)).astype(np.float32), np.float32(0))
    viewe = np.sum(ent, axis=1)
    assert viewe.dtype == np.float32
    return m, viewd, viewe
