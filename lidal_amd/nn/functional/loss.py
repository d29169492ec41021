"""Training objectives beside the plain cross-entropy (csrc/loss.hip): the Lovasz-softmax loss of Berman et al.
(CVPR 2018), the surrogate of the mIoU that lidal_amd.evaluate reports, and the cross-entropy with class weights.
All opt-in: train_step's default objective is fused.cross_entropy, unchanged.

Bad labels.  A label outside [0, c) that is not ignore_index makes the Lovasz kernels raise a status word, which
travels in the same 8 * (4 + 2 c) bytes as the loss (`LovaszOutputs.stats`).  With check_labels=True (the default of
lovasz_softmax, lovasz_softmax_flat and lovasz_forward) the wrapper reads those bytes back after the forward launches --
one synchronisation -- and raises ValueError.  With check_labels=False (the default of combined_loss, which is meant as
train_step's criterion: the read-back costs the single-scan step 1.5 ms) nothing is read back: the rows are left out
like ignored ones, and the caller may inspect `lovasz_forward(...).stats[2]` where it synchronises anyway.
The two cross-entropies have no status word: both leave a row whose label is outside [0, c) out like an ignored one,
where torch raises a device assertion."""
import collections

import torch
from torch.autograd import Function

from ... import backend as B
from . import fused

__all__ = ['lovasz_softmax', 'lovasz_softmax_flat', 'lovasz_forward', 'cross_entropy', 'combined_loss',
           'LovaszOutputs', 'MAX_CLASSES']

MAX_CLASSES = 32

# stats f64 [4 + 2 c] = {loss, present classes, status, valid rows, L_k [c], gts_k [c]};  grad f32 [n, c] = dL_k / dp;
# ranks i32 [n, c] (None unless asked for): the rank of row i in class k's order, -1 on ignored rows
LovaszOutputs = collections.namedtuple('LovaszOutputs', ['stats', 'grad', 'ranks'])


def _mode(classes):
    if classes not in ('present', 'all'):
        raise ValueError("classes must be 'present' or 'all', got %r" % (classes,))
    return 1 if classes == 'all' else 0


def _operands(x, labels, probs):
    B.require_gpu(x, labels)
    if x.dim() != 2 or labels.dim() != 1 or labels.shape[0] != x.shape[0]:
        raise ValueError('expected [n, c] scores and [n] labels, got %s and %s' % (tuple(x.shape), tuple(labels.shape)))
    if labels.dtype != torch.int64:
        raise TypeError('labels must be int64, got %s' % labels.dtype)
    ok = (torch.float32,) if probs else (torch.float32, torch.bfloat16)
    if x.dtype not in ok:
        raise TypeError('%s must be %s, got %s' % ('probabilities' if probs else 'logits',
                                                    ' or '.join(str(d) for d in ok), x.dtype))
    return x.contiguous(), labels.contiguous()


def lovasz_forward(x, labels, ignore_index=255, classes='present', probs=False, want_ranks=False, check_labels=True):
    """The forward launches on logits (probs=False: softmax inside, e = |fg - p| rounded once to f32) or on probabilities (probs=True, f32):
    LovaszOutputs(stats, grad, ranks), everything the loss, the tests and the backward pass need.  A shape outside
    c in 1..32, n * c < 2^30 is refused before anything is launched."""
    x, labels = _operands(x, labels, probs)
    n, c = x.shape
    mode = _mode(classes)
    L = B.lib()
    dev = x.device
    stats = torch.empty(4 + 2 * c, dtype=torch.float64, device=dev)
    nbytes = L.lidal_lovasz_workspace_bytes(n, c)
    if nbytes > 0:                      # (0: a refused shape -- the entry point says why, and nothing is allocated)
        grad = torch.empty((n, c), dtype=torch.float32, device=dev)
        ranks = torch.empty((n, c), dtype=torch.int32, device=dev) if want_ranks else None
        ws = B.workspace(nbytes, dev)
    else:
        grad = ranks = ws = None
    B.check(L.lidal_lovasz_fwd(B.ptr(x), B.dtype_code(x.dtype), 1 if probs else 0, B.ptr(labels), n, c,
                               int(ignore_index), mode, B.ptr(stats), B.ptr(grad), B.ptr(ranks), B.ptr(ws), nbytes,
                               B.stream()), 'lovasz_fwd')
    if check_labels and float(stats[2]) != 0.0:
        raise ValueError('lovasz_softmax: a label is outside [0, %d) and is not ignore_index (%d)'
                         % (c, int(ignore_index)))
    return LovaszOutputs(stats, grad, ranks)


class _Lovasz(Function):
    @staticmethod
    def forward(ctx, x, labels, ignore_index, mode_all, probs, check_labels):
        out = lovasz_forward(x, labels, ignore_index, 'all' if mode_all else 'present', probs, False, check_labels)
        x, labels = _operands(x, labels, probs)
        ctx.save_for_backward(x, labels, out.stats, out.grad)
        ctx.args = (int(ignore_index), int(mode_all), int(probs))
        ctx.set_materialize_grads(False)          # an output nobody used sends None, not zeros
        c = x.shape[1]
        return out.stats[0].to(torch.float32), out.stats[4:4 + c].to(torch.float32)

    @staticmethod
    def backward(ctx, g_loss, g_class):
        x, labels, stats, grad = ctx.saved_tensors
        ignore_index, mode_all, probs = ctx.args
        n, c = x.shape
        dx = torch.empty_like(x)
        gs = g_loss.reshape(1).float().contiguous() if g_loss is not None else None
        gc = g_class.reshape(c).float().contiguous() if g_class is not None else None
        B.check(B.lib().lidal_lovasz_bwd(B.ptr(x), B.dtype_code(x.dtype), probs, B.ptr(labels), n, c, ignore_index,
                                         mode_all, B.ptr(stats), B.ptr(grad), B.ptr(gs), B.ptr(gc), B.ptr(dx),
                                         B.stream()), 'lovasz_bwd')
        return dx, None, None, None, None, None


def _lovasz(x, labels, ignore_index, classes, per_class, probs, check_labels):
    loss, lk = _Lovasz.apply(x, labels, int(ignore_index), _mode(classes), probs, bool(check_labels))
    return (loss, lk) if per_class else loss


def lovasz_softmax(logits, labels, ignore_index=255, classes='present', per_class=False, check_labels=True):
    """Lovasz-softmax of logits [n, c] (f32 or bf16; the softmax runs inside) against labels i64 [n]: Berman's
    lovasz_softmax_flat on the rows whose label is not ignore_index.  Per class k: e = |[label == k] - p_k|, rows by e
    descending (ties: ascending row), L_k = <e, gradient of the Lovasz extension of the Jaccard loss>; the loss is the
    mean of L_k over the classes that occur ('present') or over all c ('all'); 0 when no row is valid.
    per_class=True returns (loss, L_k f32 [c]) -- L_k of every class, whether it counts in the mean or not.  Both are
    differentiable with respect to the logits."""
    return _lovasz(logits, labels, ignore_index, classes, per_class, False, check_labels)


def lovasz_softmax_flat(probas, labels, ignore_index=255, classes='present', per_class=False, check_labels=True):
    """The same on given probabilities f32 [n, c], differentiable with respect to `probas`."""
    return _lovasz(probas, labels, ignore_index, classes, per_class, True, check_labels)


class _WeightedCrossEntropy(Function):
    @staticmethod
    def forward(ctx, logits, labels, ignore_index, weight):
        n, c = logits.shape
        out2 = torch.empty(2, dtype=torch.float32, device=logits.device)
        nbytes = B.lib().lidal_ce_weighted_workspace_bytes(n)
        ws = B.workspace(nbytes, logits.device)
        B.check(B.lib().lidal_ce_weighted_fwd(B.ptr(logits), B.dtype_code(logits.dtype), B.ptr(labels), n, c,
                                              int(ignore_index), B.ptr(weight), B.ptr(out2), B.ptr(ws), nbytes,
                                              B.stream()), 'ce_weighted_fwd')
        ctx.save_for_backward(logits, labels, weight, out2)
        ctx.ignore_index = int(ignore_index)
        return out2[0]

    @staticmethod
    def backward(ctx, g):
        logits, labels, weight, out2 = ctx.saved_tensors
        n, c = logits.shape
        d = torch.empty_like(logits)
        gs = g.reshape(1).float().contiguous()
        B.check(B.lib().lidal_ce_weighted_bwd(B.ptr(logits), B.dtype_code(logits.dtype), B.ptr(labels), n, c,
                                              ctx.ignore_index, B.ptr(weight), B.ptr(out2), B.ptr(gs), B.ptr(d),
                                              B.stream()), 'ce_weighted_bwd')
        return d, None, None, None


def cross_entropy(logits, labels, ignore_index=255, weight=None):
    """torch.nn.functional.cross_entropy(logits, labels, weight=weight, ignore_index=..., reduction='mean'):
    sum_i w[y_i] * -log p[i, y_i] / sum_i w[y_i] over the non-ignored rows (nan when that sum of weights is 0, as
    torch).  weight=None is fused.cross_entropy itself, bit for bit.  A label outside [0, c) that is not ignore_index
    is not reported: the row is left out like an ignored one, as in fused.cross_entropy (torch asserts on the device)."""
    B.require_gpu(logits, labels, weight)
    if weight is None:
        return fused.cross_entropy(logits, labels, ignore_index)
    logits, labels = _operands(logits, labels, False)
    c = logits.shape[1]
    if not 1 <= c <= MAX_CLASSES:
        raise ValueError('cross_entropy: classes must be in 1..%d, got %d' % (MAX_CLASSES, c))
    if weight.shape != (c,):
        raise ValueError('weight must have shape (%d,), got %s' % (c, tuple(weight.shape)))
    return _WeightedCrossEntropy.apply(logits, labels, int(ignore_index), weight.detach().float().contiguous())


def combined_loss(logits, labels, ce_weight=1.0, lovasz_weight=1.0, class_weight=None, ignore_index=255,
                  classes='present', check_labels=False):
    """ce_weight * cross_entropy(weight=class_weight) + lovasz_weight * lovasz_softmax, the usual pair for LiDAR
    segmentation.  Each term runs its own softmax: they are 2 of the Lovasz form's ~14 launches, and sharing the
    probabilities would store an [n, c] f32 matrix that neither term needs otherwise.  As a criterion of train_step it
    does not synchronise: check_labels=True adds lovasz_softmax's read-back of the label status (ValueError)."""
    B.require_gpu(logits, labels, class_weight)
    return (ce_weight * cross_entropy(logits, labels, ignore_index, class_weight)
            + lovasz_weight * lovasz_softmax(logits, labels, ignore_index, classes, check_labels=check_labels))
