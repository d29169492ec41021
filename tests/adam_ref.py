"""numpy restatement of lidal_amd.optim.Adam's arithmetic (csrc/optim.hip): torch's single-tensor Adam with every operation
rounded separately in f32.  No torch in here: tests/test_optim_cpu.py checks THIS against torch.optim.Adam in f64, and
tests/test_optim_gpu.py checks the kernel against this bit for bit.

The scalars are computed in Python floats (f64) and rounded once to f32, as the C-ABI does with its `double` arguments."""
import math

import numpy as np

F = np.float32


def adam_step(p, g, m, v, t, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0):
    """Step number t (1-based) on f32 arrays: returns the new (p, m, v); the inputs are not written."""
    assert p.dtype == g.dtype == m.dtype == v.dtype == np.float32
    with np.errstate(all='ignore'):
        if weight_decay != 0:
            g = g + F(weight_decay) * p
        m = m + (g - m) * F(1 - beta1)
        v = v * F(beta2) + (F(1 - beta2) * g) * g
        den = np.sqrt(v) / F(math.sqrt(1 - beta2 ** t)) + F(eps)
        p = p + F(-(lr / (1 - beta1 ** t))) * (m / den)
    assert p.dtype == m.dtype == v.dtype == np.float32
    return p, m, v


def wide_gradients(rng, steps, n, lo=-6.0, hi=3.0):
    """`steps` f32 gradients of n elements with magnitudes 10^lo .. 10^hi and random signs; every seventh step's gradient is
    one-third exact zeros."""
    out = []
    for s in range(steps):
        g = (10.0 ** rng.uniform(lo, hi, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
        if s % 7 == 6:
            g[rng.permutation(n)[:n // 3]] = 0
        out.append(g)
    return out


def bits(a):
    """The bit patterns of an f32 array (so that -0.0 != 0.0 and NaNs compare by payload)."""
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
