"""A plain restatement of the MC-dropout point scores (csrc/score.hip mc_scores_kernel).  TEST
INFRASTRUCTURE.

With p_v the soft-max row of pass v, m their mean and H(q) = sum_k (q_k > 0 ? -q_k log q_k : 0):
    ment = (1 / reps) sum_v H(p_v)          the mean entropy of the passes
    bald = H(m) - ment                      the mutual information between the prediction and the mask
scores_from_logits is the definition in f64 throughout, what the GPU tests hold the kernel to; scores_from_pass_probs
restates the kernel's number widths on given f32 rows."""
import numpy as np

# (reps, classes, points) of the GPU tests against the definition; the logits of case k are N(0, k + 1)
SHAPES = ((8, 19, 257), (3, 2, 65), (8, 32, 64), (2, 19, 300), (1, 19, 64))
SIGMAS = (1, 2, 3, 4, 5, 6)


def inputs(reps, c, p, sigma, seed=0):
    """(logits f32 [reps * nv, c], inverse i64 [reps * p]): every pass has its own block of nv rows, as the collated
    batch of a frame has."""
    rs = np.random.RandomState(7000 + 100 * reps + 10 * c + p + 1000 * int(sigma) + seed)
    nv = max(2, p // 2)
    logits = (rs.standard_normal((reps * nv, c)) * sigma).astype(np.float32)
    inverse = np.concatenate([rs.randint(0, nv, size=p) + v * nv for v in range(reps)]).astype(np.int64)
    return logits, inverse


def entropy(q):
    q = np.asarray(q, np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(q > 0, -q * np.log(q), 0.0).sum(axis=-1)


def scores_from_logits(logits, inverse, reps):
    """logits [NV, C], inverse i64 [reps * P] -> dict in f64: prob [P, C], pred i64 [P] (first maximum), bald [P],
    ment [P], view_arg i64 [reps, P]."""
    logits = np.asarray(logits, np.float64)
    p, c = np.asarray(inverse).shape[0] // reps, logits.shape[1]
    rows = logits[np.asarray(inverse)].reshape(reps, p, c)
    e = np.exp(rows - rows.max(axis=2, keepdims=True))
    pv = e / e.sum(axis=2, keepdims=True)
    m = pv.mean(axis=0)
    ment = entropy(pv).mean(axis=0)
    return {'prob': m, 'pred': m.argmax(axis=1), 'bald': entropy(m) - ment, 'ment': ment, 'view_arg': rows.argmax(axis=2)}


def _entropy_in_class_order(q):
    """H of f32 rows [P, C]: every term an f64 expression of the f32 q_k, summed in f64 in class order."""
    q = np.asarray(q, np.float32)
    h = np.zeros(q.shape[0], np.float64)
    for k in range(q.shape[1]):
        qk = q[:, k].astype(np.float64)
        with np.errstate(divide='ignore', invalid='ignore'):
            h = h + np.where(q[:, k] > 0, -qk * np.log(qk), 0.0)
    return h


def scores_from_pass_probs(pv):
    """pv f32 [reps, P, C] -> (prob f32 [P, C], bald f64 [P], ment f32 [P], m f32 [P, C]) with the kernel's widths:
    prob = p_0, f32 adds in pass order, / f32(reps) (lidal_view_mean_softmax's chain); m, the mean whose entropy is
    taken, = f32(the f64 sum of the rows in pass order / reps); S = the f64 sum of H(p_v) in pass order with the rounding
    error of every add kept (two-sum) and added at the end; ment = f32(S / reps), bald = H(m) - S / reps."""
    pv = np.ascontiguousarray(pv, np.float32)
    reps = pv.shape[0]
    prob = pv[0].copy()
    md = pv[0].astype(np.float64)
    for v in range(1, reps):
        prob = prob + pv[v]
        md = md + pv[v].astype(np.float64)
    prob = prob / np.float32(reps)
    assert prob.dtype == np.float32
    m = (md / float(reps)).astype(np.float32)
    s = np.zeros(pv.shape[1], np.float64)
    err = np.zeros(pv.shape[1], np.float64)
    for v in range(reps):
        h = _entropy_in_class_order(pv[v])
        t = s + h
        hh = t - s
        err = err + ((s - (t - hh)) + (h - hh))
        s = t
    mean = (s + err) / float(reps)
    return prob, _entropy_in_class_order(m) - mean, mean.astype(np.float32), m


def softmax_f32(rows):
    """Soft-max rows in f32 arithmetic (numpy's expf; the kernel's is the device's: not the same bits)."""
    rows = np.asarray(rows, np.float32)
    e = np.exp(rows - rows.max(axis=-1, keepdims=True))
    return (e / e.sum(axis=-1, keepdims=True, dtype=np.float32)).astype(np.float32)
