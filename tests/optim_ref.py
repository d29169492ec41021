"""numpy restatement of what lidal_amd.optim adds beside Adam (csrc/optim.hip): torch's single-tensor SGD and AdamW with
every operation rounded separately in f32, and the global gradient norm of clip_grad_norm_ in the kernel's summation order.
No torch in here: tests/test_optim_family_cpu.py checks THIS against torch in f64, and tests/test_optim_family_gpu.py
checks the kernels against this bit for bit.

The scalars are computed in Python floats (f64) and rounded once to f32, as the C-ABI does with its `double` arguments."""
import numpy as np

import adam_ref

F = np.float32
NORM_THREADS = 256          # threads of a block of the norm; element e of a block belongs to thread (e // 4) % 256


def clipped(g, coef):
    """g * coef, rounded: what every update rule sees of a clipped gradient (coef None: no clipping, g itself)."""
    if coef is None:
        return g
    with np.errstate(all='ignore'):
        return g * F(coef)


def sgd_step(p, g, buf, lr=1e-3, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, coef=None):
    """One step on f32 arrays.  `buf` None: this parameter's first step (or momentum 0).  Returns the new (p, buf); buf stays
    None with momentum 0.  The inputs are not written."""
    assert p.dtype == g.dtype == np.float32 and (buf is None or buf.dtype == np.float32)
    with np.errstate(all='ignore'):
        g = clipped(g, coef)
        if weight_decay != 0:
            g = g + F(weight_decay) * p
        if momentum != 0:
            if buf is None:
                buf = g.copy()
            else:
                buf = buf * F(momentum) + F(1 - dampening) * g
            g = g + F(momentum) * buf if nesterov else buf
        else:
            buf = None
        p = p + F(-lr) * g
    assert p.dtype == np.float32 and (buf is None or buf.dtype == np.float32)
    return p, buf


def adamw_step(p, g, m, v, t, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-2, coef=None):
    """Step number t (1-based) of AdamW: the decay on p first, then Adam's five lines on the (clipped) gradient."""
    with np.errstate(all='ignore'):
        p = p * F(1 - lr * weight_decay)
    return adam_ref.adam_step(p, clipped(g, coef), m, v, t, lr=lr, beta1=beta1, beta2=beta2, eps=eps)


def adam_step(p, g, m, v, t, coef=None, **kw):
    """adam_ref.adam_step (coupled weight decay) behind a clipped gradient."""
    return adam_ref.adam_step(p, clipped(g, coef), m, v, t, **kw)


def block_sum(g, block):
    """The f64 sum of g * g over ONE block (len(g) <= block) in the kernel's order: thread t adds the squares of its
    elements in ascending element index, elements behind the end count +0; then sum[t] += sum[t + s] for s = 128 .. 1."""
    assert g.dtype == np.float32 and g.size <= block and block % (4 * NORM_THREADS) == 0
    sq = np.zeros(block, np.float64)
    g64 = g.astype(np.float64)
    with np.errstate(all='ignore'):
        sq[:g.size] = g64 * g64
        per_thread = sq.reshape(-1, NORM_THREADS, 4).transpose(1, 0, 2).reshape(NORM_THREADS, -1)
        acc = np.zeros(NORM_THREADS, np.float64)
        for c in range(per_thread.shape[1]):
            acc = acc + per_thread[:, c]
        s = NORM_THREADS // 2
        while s >= 1:
            acc[:s] = acc[:s] + acc[s:2 * s]
            s //= 2
    return acc[0]


def norm_slots(numels, block):
    """sum(ceil(n_r / block)) over every record, with a gradient or not: the f64 slots of the partials workspace."""
    return sum(-(-n // block) for n in numels)


def grad_norm(records, block):
    """The f32 total norm of `records` (per tensor its flattened f32 gradient, or None where it has none): the blocks of a
    tensor in ascending order, the tensors in ascending order, one f64 running sum; total = f32(sqrt_f64(sum))."""
    total = np.float64(0.0)
    with np.errstate(all='ignore'):
        for g in records:
            if g is None:
                continue
            g = np.ascontiguousarray(g, dtype=np.float32).reshape(-1)
            for e0 in range(0, g.size, block):
                total = total + block_sum(g[e0:e0 + block], block)
        return F(np.sqrt(total))


def clip_coef(total, max_norm):
    """min(f32(max_norm) / (total + 1e-6f), 1) in f32; a NaN stays a NaN (torch.clamp keeps it)."""
    with np.errstate(all='ignore'):
        q = F(max_norm) / (F(total) + F(1e-6))
    return F(1.0) if q > F(1.0) else q
