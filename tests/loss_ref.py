"""Restatements of the objectives of lidal_amd/csrc/loss.hip for the tests (test_loss_cpu.py, test_loss_gpu.py).

Lovasz-softmax (Berman et al., CVPR 2018, lovasz_softmax_flat) on the rows whose label is not ignore_index, p [n, c]:
  per class k: fg = (label == k), e = |fg - p[:, k]|; rows by e descending, ties by ascending row (a stable argsort);
  gts = sum fg; at rank r: inter = gts - cumsum(fg), union = gts + cumsum(1 - fg) (integers), jac = 1 - inter / union,
  g[r] = jac[r] - jac[r - 1], g[0] = jac[0];  L_k = sum_r e[r] g[r] in f64;
  loss = mean of L_k over the classes with gts > 0 ('present') or over all classes ('all'); 0 without a valid row.
  dL_k/dp = -g[rank] where fg = 1, +g[rank] where fg = 0, 0 where e == 0 (torch's abs at 0).
  dL/dz[i, k] = p[i, k] (a_k - sum_j a_j p[i, j]), a_k = dL_k/dp[i, k] s_k, j ascending, s_k = 1 / (classes that
  count) on the classes that count, times the incoming gradient.
`ft` is the type of e, jac and the softmax.  np.float32 on given probabilities (lovasz_flat) restates the kernels bit
for bit; np.float64 is the all-f64 reference.  On logits the kernels are between the two -- softmax in f64, e rounded
once to f32, jac in f32 -- and are held to the all-f64 reference with measured bars."""
import numpy as np
import torch


def softmax(z, ft):
    z = z.astype(ft)
    x = np.exp(z - z.max(axis=1, keepdims=True))
    return (x / x.sum(axis=1, keepdims=True)).astype(ft)


def lovasz_flat(p, labels, ignore_index=255, classes='present', ft=np.float32):
    """-> dict(loss f64, per_class f64 [c], gts i64 [c], present, counts bool [c], scale f64 [c], n_valid,
               grad ft [n, c] = dL_k/dp (not scaled), ranks i32 [n, c] (-1 on ignored rows))"""
    p = np.asarray(p).astype(ft)
    labels = np.asarray(labels)
    n, c = p.shape
    rows = np.nonzero(labels != ignore_index)[0]
    nv = rows.size
    pv, lv = p[rows], labels[rows]
    grad = np.zeros((n, c), ft)
    ranks = np.full((n, c), -1, np.int32)
    per_class = np.zeros(c, np.float64)
    gts_all = np.zeros(c, np.int64)
    for k in range(c):
        if nv == 0:
            break
        fg = lv == k
        e = np.abs(fg.astype(ft) - pv[:, k])
        order = np.argsort(-e, kind='stable')
        es, fs = e[order], fg[order].astype(np.int64)
        cum = np.cumsum(fs)
        gts = int(fs.sum())
        r = np.arange(nv, dtype=np.int64)
        inter = (gts - cum).astype(ft)
        union = (gts + (r + 1 - cum)).astype(ft)
        jac = (ft(1) - inter / union).astype(ft)
        g = jac.copy()
        g[1:] = jac[1:] - jac[:-1]
        per_class[k] = np.sum(es.astype(np.float64) * g.astype(np.float64))
        gts_all[k] = gts
        grad[rows[order], k] = np.where(es == 0, ft(0), np.where(fs == 1, -g, g))
        ranks[rows[order], k] = r
    present = int((gts_all > 0).sum())
    counts = (gts_all > 0) if classes == 'present' else np.full(c, nv > 0)
    denom = int(counts.sum())
    loss = float(per_class[counts].sum() / denom) if denom > 0 else 0.0
    scale = np.where(counts, 1.0 / max(denom, 1), 0.0)
    return dict(loss=loss, per_class=per_class, gts=gts_all, present=present, counts=counts, scale=scale, n_valid=nv,
                grad=grad, ranks=ranks)


def lovasz_logits(z, labels, ignore_index=255, classes='present', ft=np.float32, upstream=1.0):
    """The same with the softmax inside, and dL/dz: the dict of lovasz_flat plus p and dz (both `ft`)."""
    p = softmax(np.asarray(z), ft)
    out = lovasz_flat(p, labels, ignore_index, classes, ft)
    a = (out['grad'] * (out['scale'] * upstream).astype(ft)[None, :]).astype(ft)
    dot = np.zeros(p.shape[0], ft)
    for k in range(p.shape[1]):                        # ascending, one rounding per product and per sum
        dot = (dot + (a[:, k] * p[:, k]).astype(ft)).astype(ft)
    dz = (p * (a - dot[:, None])).astype(ft)
    dz[np.asarray(labels) == ignore_index] = 0
    out.update(p=p, dz=dz)
    return out


# ---- the well-known torch formulation, written out (one sort, one gather, two cumsums and a dot per class) ----
def torch_lovasz_grad(fg_sorted):
    gts = fg_sorted.sum()
    inter = gts - fg_sorted.cumsum(0)
    union = gts + (1 - fg_sorted).cumsum(0)
    jac = 1 - inter / union
    if fg_sorted.numel() > 1:
        jac[1:] = jac[1:] - jac[:-1]
    return jac


def torch_lovasz_softmax_flat(probas, labels, classes='present', ignore_index=255):
    valid = labels != ignore_index
    probas, labels = probas[valid], labels[valid]
    if probas.numel() == 0:
        return probas.sum() * 0.0
    losses = []
    for k in range(probas.shape[1]):
        fg = (labels == k).to(probas.dtype)
        if classes == 'present' and fg.sum() == 0:
            continue
        errors = (fg - probas[:, k]).abs()
        errors_sorted, perm = torch.sort(errors, 0, descending=True)
        losses.append(torch.dot(errors_sorted, torch_lovasz_grad(fg[perm])))
    if not losses:
        return probas.sum() * 0.0
    return torch.stack(losses).mean()


def torch_lovasz_softmax(logits, labels, classes='present', ignore_index=255):
    return torch_lovasz_softmax_flat(torch.softmax(logits, 1), labels, classes, ignore_index)


# ---- inputs whose per-class errors are separated by construction ------------------------------------------------
GAP = 1e-3


def separated_logits(n, c, seed, bf16=False, n_ignored=2, ignore_index=255):
    """Logits f32 [n, c] (rounded to bf16 values if asked) and labels whose errors |fg - p| differ by at least GAP
    between any two valid rows of one class, so no rank can depend on f32 against f64 rounding.  Row i gets its own
    t_i from a shuffled linspace(0.5, 0.98); its label's probability is 1 - t_i and the other classes share t_i
    evenly: the foreground errors of a class are t_i (apart by the linspace's step), its background errors
    t_i / (c - 1) <= 0.49 (apart by step / (c - 1), and below every foreground error); with c = 2 both are t_i.
    The construction is verified on the (rounded) logits in f64 before they are returned."""
    assert c >= 2
    rng = np.random.RandomState(seed)
    t = np.linspace(0.5, 0.98, n)
    rng.shuffle(t)
    labels = rng.randint(0, c, n).astype(np.int64)
    labels[:c] = np.arange(c)[:n]                      # every class occurs when n allows it
    p = np.repeat((t / (c - 1))[:, None], c, axis=1)
    p[np.arange(n), labels] = 1.0 - t
    z = np.log(p).astype(np.float32)
    if bf16:
        z = torch.from_numpy(z).bfloat16().float().numpy()
    if n_ignored:
        labels[rng.choice(n, min(n_ignored, max(n - c, 0)), replace=False) + 0] = ignore_index
        labels[:c] = np.arange(c)[:n]
    p64 = softmax(z, np.float64)
    valid = labels != ignore_index
    for k in range(c):
        e = np.sort(np.abs((labels[valid] == k) - p64[valid, k]))
        assert e.size < 2 or np.diff(e).min() >= GAP, (n, c, k, np.diff(e).min())
    return z, labels


# ---- cross-entropy with class weights, f64 ------------------------------------------------------------------------
def weighted_cross_entropy(z, labels, weight, ignore_index=255, upstream=1.0):
    """-> (loss, dz): sum_i w[y_i] * -log p[i, y_i] / sum_i w[y_i] over the non-ignored rows, and its gradient."""
    z = np.asarray(z, np.float64)
    labels = np.asarray(labels)
    w = np.asarray(weight, np.float64)
    p = softmax(z, np.float64)
    valid = labels != ignore_index
    y = np.where(valid, labels, 0)
    wy = np.where(valid, w[y], 0.0)
    with np.errstate(invalid='ignore', divide='ignore'):
        loss = float((wy * -np.log(p[np.arange(len(y)), y])).sum() / wy.sum())
        onehot = np.zeros_like(p)
        onehot[np.arange(len(y)), y] = 1.0
        dz = wy[:, None] * (p - onehot) * upstream / wy.sum()
    return loss, dz
