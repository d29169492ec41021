"""Counter-based dropout (csrc/dropout.hip): the mask of an application is a pure function of
(seed, call, element index) -- Philox4x32-10, one word per element -- so nothing is stored for the backward pass, a
training run is reproducible from two integers per module, and a launch plan carries the operation like any other
(network/plan.py).  Opt-in: a model built as before keeps torch's nn.Dropout and torch's generator.

  Dropout               the module (no parameters, no buffers: state_dict keys are nn.Dropout's, i.e. none)
  use_counter_dropout   swap it in for the nn.Dropout at `model.dropout`
  mc_dropout            with mc_dropout(model): the masks stay on in eval mode (MC-dropout scoring, score/mc_dropout.py)
"""
import contextlib
import math

import numpy as np
import torch
from torch import nn

from .. import backend as B

__all__ = ['Dropout', 'use_counter_dropout', 'mc_dropout', 'mask_constants', 'dropout_apply_']


def mask_constants(p):
    """(thr, scale) of drop probability p as lidal_dropout_apply takes them: an element is kept iff its 32-bit word is
    below thr = min(floor((1 - p) * 2^32), 0xffffffff) (formed in f64), and then multiplied by scale = f32(1 / (1 - p))
    (p == 1 keeps nothing: its scale is never used)."""
    p = float(p)
    if not 0.0 <= p <= 1.0:
        raise ValueError('dropout probability has to be between 0 and 1, but got %r' % p)
    thr = min(int(math.floor((1.0 - p) * 4294967296.0)), 0xffffffff)
    scale = float(np.float32(1.0 / (1.0 - p))) if p < 1.0 else float('inf')
    return thr, scale


def _i64(v):
    """An unsigned 64-bit seed / call id as the signed word the C ABI (and a plan) carries: the same bits."""
    v = int(v)
    if not 0 <= v < (1 << 64):
        raise ValueError('lidal_amd.nn.Dropout: seed and call ids are 64-bit unsigned integers (got %d)' % v)
    return v - (1 << 64) if v >= (1 << 63) else v


def dropout_apply_(x, p, seed, call, first=0):
    """x (contiguous, f32 or bf16, on the GPU) scaled IN PLACE by the mask of (seed, call); element i of x is element
    first + i of the mask (first % 8 == 0).  p == 0 launches nothing.  The backward pass is the same call on the gradient."""
    B.require_gpu(x)
    if not x.is_contiguous():
        raise ValueError('lidal_amd.nn.Dropout: the in-place form needs a contiguous tensor')
    code = B.dtype_code(x.dtype)
    thr, scale = mask_constants(p)
    if p == 0 or x.numel() == 0:
        return x
    B.check(B.lib().lidal_dropout_apply(B.ptr(x), x.numel(), code, int(first), _i64(seed), _i64(call), thr, scale,
                                        B.stream()), 'dropout_apply')
    return x


class _DropoutFn(torch.autograd.Function):
    """Forward and backward are the same kernel with the same (seed, call): grad_in = grad_out * m, bit for bit."""

    @staticmethod
    def forward(ctx, x, p, seed, call, inplace):
        ctx.mask = (p, seed, call)
        if inplace:
            ctx.mark_dirty(x)
            return dropout_apply_(x, p, seed, call)
        return dropout_apply_(x.clone(memory_format=torch.contiguous_format), p, seed, call)

    @staticmethod
    def backward(ctx, g):
        p, seed, call = ctx.mask
        # (a copy: autograd may hand the same gradient tensor to another consumer)
        return dropout_apply_(g.clone(memory_format=torch.contiguous_format), p, seed, call), None, None, None, None


class Dropout(nn.Module):
    """nn.Dropout's contract -- y = x * m / (1 - p), m ~ Bernoulli(1 - p) per element -- with the counter-based mask.
    `seed` names the module's stream of masks, `calls` counts its applications: application number `calls` uses call id
    `calls`, whatever the tensor's size.  `mc` keeps the module active in eval mode (mc_dropout).  Ranks of a
    data-parallel run have to be given different seeds by the caller."""

    def __init__(self, p=0.5, inplace=False, seed=0):
        super().__init__()
        mask_constants(p)
        _i64(seed)
        self.p = float(p)
        self.inplace = bool(inplace)
        self.seed = int(seed)
        self.calls = 0
        self.mc = False

    def extra_repr(self):
        return 'p=%g, inplace=%s, seed=%d' % (self.p, self.inplace, self.seed)

    def active(self):
        return (self.training or self.mc) and self.p > 0

    def draw(self):
        """The call id of the next application (and the counter moves on)."""
        call = self.calls
        self.calls += 1
        return call

    def rng_state(self):
        return self.seed, self.calls

    def set_rng_state(self, state):
        seed, calls = state
        _i64(seed)
        _i64(calls)
        self.seed, self.calls = int(seed), int(calls)

    def forward(self, x):
        B.require_gpu(x)
        if not self.active():
            return x
        if self.inplace and not x.is_contiguous():
            raise ValueError('lidal_amd.nn.Dropout(inplace=True) needs a contiguous tensor')
        B.dtype_code(x.dtype)
        return _DropoutFn.apply(x, self.p, self.seed, self.draw(), self.inplace)


def use_counter_dropout(model, seed=0):
    """Replace the nn.Dropout at `model.dropout` (SPVCNN's) by the counter form with the same p and inplace, in the same
    mode; returns the new module.  A model that already has the counter form gets the new seed and a counter of 0."""
    old = getattr(model, 'dropout', None)
    if isinstance(old, Dropout):
        old.set_rng_state((seed, 0))
        return old
    if not isinstance(old, nn.Dropout):
        raise ValueError('use_counter_dropout: %s has no nn.Dropout at .dropout' % type(model).__name__)
    new = Dropout(old.p, old.inplace, seed)
    new.train(old.training)
    model.dropout = new
    return new


@contextlib.contextmanager
def mc_dropout(model):
    """with mc_dropout(model): every counter dropout of `model` stays active whatever the mode (BatchNorm keeps its
    eval behaviour: call model.eval() as for any inference).  ValueError for a model without one (MinkUNet; an SPVCNN
    that kept nn.Dropout)."""
    mods = [m for m in model.modules() if isinstance(m, Dropout)]
    if not mods:
        raise ValueError('mc_dropout: %s has no lidal_amd.nn.Dropout (build SPVCNN with dropout_seed=..., or call '
                         'use_counter_dropout)' % type(model).__name__)
    saved = [m.mc for m in mods]
    for m in mods:
        m.mc = True
    try:
        yield model
    finally:
        for m, was in zip(mods, saved):
            m.mc = was
