"""The counter-based dropout on the GPU (csrc/dropout.hip, lidal_amd/nn/dropout.py): the kernel
bit for bit against tests/dropout_ref.py, the identities of the mask, and SPVCNN with the dropout as an operation of its
launch plans -- the plan against the per-operator path, one plan per pass, reproducibility from (seed, calls), the
inference plan under nn.mc_dropout.

A NaN is compared as a NaN, not by its payload (inf * 0.0f and a dropped NaN are NaNs of the multiplier's making)."""
import copy
import functools

import numpy as np
import pytest
import torch

import dropout_ref as D

pytestmark = pytest.mark.gpu
DEV = 'cuda'

# csrc/dropout.hip: 256 threads per workgroup, at most 2048 workgroups; a thread takes one 16-byte vector per trip
FULL_GRID_VECTORS = 2048 * 256
VEC = {torch.float32: 4, torch.bfloat16: 8}


def _bits(t):
    if t.dtype == torch.float32:
        return t.detach().contiguous().view(torch.int32).cpu().numpy().view(np.uint32).reshape(-1)
    return t.detach().contiguous().view(torch.int16).cpu().numpy().view(np.uint16).reshape(-1)


def _tensor(n, dtype, seed, special=False):
    x = np.random.RandomState(seed).standard_normal(n).astype(np.float32)
    if special:
        x[::5] = np.tile(np.array([-0.0, np.inf, -np.inf, np.nan, 0.0], np.float32), n // 25 + 1)[:x[::5].size]
    return torch.from_numpy(x).to(DEV).to(dtype)


def _want(x, p, seed, call, first=0):
    """(expected bit patterns, where they are NaN)"""
    if x.dtype == torch.float32:
        want = D.apply_f32(x.detach().cpu().numpy().reshape(-1), p, seed, call, first)
        return want.view(np.uint32), np.isnan(want)
    want = D.apply_bf16(_bits(x), p, seed, call, first)
    return want, np.isnan(D.bf16_to_f32(want))


def _check(got, want_bits, want_nan, what=''):
    bits = _bits(got)
    val = got.detach().float().cpu().numpy().reshape(-1)
    assert np.array_equal(np.isnan(val), want_nan), what
    assert np.array_equal(bits[~want_nan], want_bits[~want_nan]), what


def _apply(x, p, seed, call, first=0):
    from lidal_amd.nn.dropout import dropout_apply_
    y = dropout_apply_(x.clone(), p, seed, call, first)
    torch.cuda.synchronize()
    return y


@pytest.mark.parametrize('p', [0.3, 1.0])
@pytest.mark.parametrize('n', [1, 3, 4, 5, 7, 8, 9, 257 * 128, 'second trip'])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_kernel_is_the_restatement_bit_for_bit(dtype, n, p):
    """Sizes below, at and above one vector, the coarsest-level block of the model tests (257 x 128), and one vector and
    three elements past a full grid: the grid-stride loop takes a second trip and the scalar tail follows it."""
    if n == 'second trip':
        n = (FULL_GRID_VECTORS + 1) * VEC[dtype] + 3
    x = _tensor(n, dtype, n % 1000)
    seed, call = 0x123456789abcdef1, 3 + (1 << 40)
    want, nan = _want(x, p, seed, call)
    got = _apply(x, p, seed, call)
    _check(got, want, nan)
    if p == 1.0:
        assert not got.float().abs().max().item() > 0            # every element dropped: +-0
    elif n >= 64:
        kept = (got != 0).float().mean().item()
        assert abs(kept - 0.7) <= 6 * (0.21 / n) ** 0.5 + 1e-3, kept


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_group_index_crosses_two_to_the_32(dtype):
    first = 2 ** 34 - 8
    x = _tensor(16, dtype, 1)
    want, nan = _want(x, 0.3, 11, 2, first)
    _check(_apply(x, 0.3, 11, 2, first), want, nan)
    lo = _apply(x, 0.3, 11, 2, 0)
    assert not torch.equal(lo, _apply(x, 0.3, 11, 2, 2 ** 34))


@pytest.mark.parametrize('p', [0.3, 1.0])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_signed_zero_infinities_and_nan(dtype, p):
    x = _tensor(203, dtype, 2, special=True)
    want, nan = _want(x, p, 9, 0)
    got = _apply(x, p, 9, 0)
    _check(got, want, nan)
    src = x.float().cpu().numpy()
    out = got.float().cpu().numpy()
    assert np.isnan(out[np.isnan(src)]).all()                      # a dropped NaN stays NaN
    if p == 1.0:
        assert np.isnan(out[np.isinf(src)]).all()                  # inf * 0.0f
        neg_zero = (src == 0) & np.signbit(src)
        assert neg_zero.any() and np.signbit(out[neg_zero]).all()  # -0.0 * 0.0f = -0.0


def test_p_zero_launches_nothing_and_leaves_the_bytes():
    from lidal_amd import backend as B
    from lidal_amd import nn as spnn
    x = _tensor(1000, torch.float32, 3, special=True)
    B.HITS.clear()
    y = _apply(x, 0.0, 1, 0)
    assert 'dropout_apply' not in B.HITS and np.array_equal(_bits(y), _bits(x))
    d = spnn.Dropout(0.0, True, 1).train()
    z = x.clone()
    assert d(z) is z and d.calls == 0 and 'dropout_apply' not in B.HITS and np.array_equal(_bits(z), _bits(x))


@pytest.mark.parametrize('inplace', [False, True])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_backward_mask_is_the_forward_mask(dtype, inplace):
    """grad == g * m exactly: the same kernel with the saved call id, whatever the counter has moved to since."""
    from lidal_amd import nn as spnn
    n = 37 * 24 + 5
    d = spnn.Dropout(0.3, inplace, seed=21).train()
    d.set_rng_state((21, 4))
    x = _tensor(n, dtype, 4).requires_grad_(True)
    z = x * 1 if inplace else x
    before = z.detach().clone()
    y = d(z)
    assert (y is z) == inplace and d.calls == 5
    want, nan = _want(before, 0.3, 21, 4)
    _check(y, want, nan)
    if not inplace:
        assert torch.equal(x.detach(), before)
    d(torch.ones(8, device=DEV))                                    # the counter moves on before the backward pass
    g = _tensor(n, dtype, 5)
    y.backward(g)
    torch.cuda.synchronize()
    want_g, nan_g = _want(g, 0.3, 21, 4)
    _check(x.grad, want_g, nan_g)
    m = D.multiplier(n, 0.3, 21, 4)
    assert np.array_equal((x.grad.float().cpu().numpy() != 0), (m != 0) & (g.float().cpu().numpy() != 0))


def test_same_seed_and_call_same_bytes_on_any_stream_and_other_ids_other_masks():
    x = _tensor(257 * 128, torch.bfloat16, 6)
    first = _apply(x, 0.3, 5, 7)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        second = _apply(x, 0.3, 5, 7)
    torch.cuda.synchronize()
    assert torch.equal(first, second) and torch.equal(first, _apply(x, 0.3, 5, 7))
    assert not torch.equal(first, _apply(x, 0.3, 5, 8))
    assert not torch.equal(first, _apply(x, 0.3, 6, 7))
    assert not torch.equal(first, _apply(x, 0.3, 5 + (1 << 32), 7))        # the high key word counts
    assert not torch.equal(first, _apply(x, 0.3, 5, 7 + (1 << 32)))        # ... and the high call word


def test_module_modes_counters_and_layouts():
    from lidal_amd import nn as spnn
    d = spnn.Dropout(0.5, False, seed=2)
    x = _tensor(64 * 6, torch.float32, 7).reshape(64, 6)
    d.eval()
    assert d(x) is x and d.calls == 0
    with pytest.raises(RuntimeError, match='GPU only'):
        d(x.cpu())
    d.train()
    y0 = d(x)
    y1 = d(x)
    assert d.calls == 2 and d.rng_state() == (2, 2) and not torch.equal(y0, y1)
    d.set_rng_state((2, 0))
    assert torch.equal(d(x), y0) and torch.equal(d(x), y1)
    # out of place: a non-contiguous input is made contiguous (the mask follows the contiguous result's element order)
    xt = x.t()
    assert not xt.is_contiguous()
    d.set_rng_state((2, 9))
    yt = d(xt)
    d.set_rng_state((2, 9))
    assert yt.is_contiguous() and torch.equal(yt, d(xt.contiguous()))
    with pytest.raises(ValueError, match='contiguous'):
        spnn.Dropout(0.5, True).train()(xt)
    with pytest.raises(TypeError):
        d(x.double())
    # mc: active in eval mode
    d.eval()
    d.mc = True
    d.set_rng_state((2, 0))
    assert torch.equal(d(x), y0)


# ---- SPVCNN with the dropout inside its launch plans ------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _batch():
    from lidal_amd import synth
    b = synth.make_train_batch(n_frames=1, n_points=5000, seed=321)
    return tuple(torch.from_numpy(b[k]).to(DEV) for k in ('feats_v_b', 'coords_v_b', 'labels_v_b'))


def _model(seed=5):
    from lidal_amd.network import SPVCNN
    torch.manual_seed(0)
    return SPVCNN(19, dropout_seed=seed).to(DEV).train()


class _Planned:
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        from lidal_amd.network import plan
        self.saved = plan.ENABLED, plan.TALLY
        plan.ENABLED, plan.TALLY = self.on, False

    def __exit__(self, *exc):
        from lidal_amd.network import plan
        plan.ENABLED, plan.TALLY = self.saved
        return False


def _step(model, autocast, planned=True):
    """One forward + backward pass: (loss, logits, gradients, plans of the forward pass, plans of the backward pass)."""
    import lidal_amd
    from lidal_amd.network import plan
    from lidal_amd.nn.functional.fused import cross_entropy
    feats, coords, labels = _batch()
    model.zero_grad(set_to_none=True)
    with _Planned(planned):
        c0 = plan.COUNTERS['plans']
        with torch.autocast('cuda', dtype=torch.bfloat16, enabled=autocast):
            logits, _ = model(lidal_amd.SparseTensor(feats, coords))
        c1 = plan.COUNTERS['plans']
        loss = cross_entropy(logits, labels, ignore_index=255)
        loss.backward()
        c2 = plan.COUNTERS['plans']
    torch.cuda.synchronize()
    return loss.detach().clone(), logits.detach().clone(), [p.grad.clone() for p in model.parameters()], c1 - c0, c2 - c1


def _same_step(a, b):
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for k, (p, q) in enumerate(zip(a[2], b[2])):
        assert torch.equal(p, q), k


@pytest.mark.parametrize('autocast', [False, True])
def test_plan_is_the_per_operator_path_bitwise_and_one_plan_per_pass(autocast):
    from torch import nn
    a = _model()
    b, c, e = copy.deepcopy(a), copy.deepcopy(a), copy.deepcopy(a)      # (copies before anything is cached on a model)
    ra = _step(a, autocast, planned=False)
    rb = _step(b, autocast, planned=True)
    assert ra[3:] == (0, 0)
    assert rb[3:] == (1, 1), rb[3:]                 # the whole forward pass one plan, the whole backward pass one plan
    assert a.dropout.calls == 2 and b.dropout.calls == 2            # the same call ids, in the same order
    _same_step(ra, rb)
    names = [k for k, _ in a.named_parameters()]
    assert len(names) == len(ra[2]) and float(ra[0]) > 0
    for (k, p), q in zip(a.state_dict().items(), b.state_dict().values()):      # every BatchNorm buffer
        assert torch.equal(p, q), k
    # ... and what it was: the same model with nn.Dropout cuts either pass in three
    c.dropout = nn.Dropout(0.3, True)
    assert _step(c, autocast, planned=True)[3:] == (3, 3)
    # the masks did drop something: p = 0 gives other logits
    e.dropout.p = 0.0
    assert not torch.equal(_step(e, autocast)[1], rb[1]) and e.dropout.calls == 0


@pytest.mark.parametrize('autocast', [False, True])
def test_a_step_is_a_function_of_seed_and_calls_not_of_torchs_generator(autocast):
    model = _model(seed=77)
    torch.manual_seed(1)
    first = _step(model, autocast)
    assert model.dropout.rng_state() == (77, 2)
    torch.manual_seed(2)
    model.dropout.set_rng_state((77, 0))
    second = _step(model, autocast)
    _same_step(first, second)
    third = _step(model, autocast)                                  # calls 2, 3: other masks
    assert not torch.equal(third[1], first[1])
    model.dropout.set_rng_state((77, 2))                            # a checkpoint's state replays the step
    _same_step(third, _step(model, autocast))
    model.dropout.set_rng_state((78, 0))
    assert not torch.equal(_step(model, autocast)[1], first[1])


def _eval_logits(model, autocast, planned):
    import lidal_amd
    from lidal_amd import backend as B
    feats, coords, _ = _batch()
    with _Planned(planned), torch.no_grad():
        B.HITS.clear()
        with torch.autocast('cuda', dtype=torch.bfloat16, enabled=autocast):
            logits, _ = model(lidal_amd.SparseTensor(feats, coords))
        runs = B.HITS.get('plan_run', 0)
    torch.cuda.synchronize()
    return logits.clone(), runs


@pytest.mark.parametrize('autocast', [False, True])
def test_inference_plan_without_and_with_mc_dropout(autocast):
    from torch import nn
    from lidal_amd import nn as spnn
    model = _model(seed=3).eval()
    for m in model.modules():               # non-trivial running statistics
        if isinstance(m, nn.BatchNorm1d):
            m.running_mean.normal_(0, 0.3)
            m.running_var.uniform_(0.5, 2.0)
    plain = copy.deepcopy(model)
    plain.dropout = nn.Dropout(0.3, True).eval()
    off, runs = _eval_logits(model, autocast, True)
    assert runs == 1 and model.dropout.calls == 0
    assert torch.equal(off, _eval_logits(plain, autocast, True)[0])             # eval without mc: nn.Dropout's bytes
    with spnn.mc_dropout(model) as same:
        assert same is model and model.dropout.mc
        on, runs = _eval_logits(model, autocast, True)
        assert runs == 1 and model.dropout.calls == 2                           # one plan, both sites inside it
        model.dropout.set_rng_state((3, 0))
        per_op, runs = _eval_logits(model, autocast, False)
        assert runs == 0 and model.dropout.calls == 2
    assert model.dropout.mc is False
    assert torch.equal(on, per_op)
    assert not torch.equal(on, off)
    with pytest.raises(KeyError):
        with spnn.mc_dropout(model):
            raise KeyError('x')
    assert model.dropout.mc is False
    assert torch.equal(_eval_logits(model, autocast, True)[0], off)


def test_use_counter_dropout_after_a_first_planned_forward():
    from torch import nn
    from lidal_amd import nn as spnn
    from lidal_amd.network import SPVCNN
    torch.manual_seed(0)
    model = SPVCNN(19).to(DEV).train()
    assert type(model.dropout) is nn.Dropout
    ref = copy.deepcopy(model)
    assert _step(model, True)[3:] == (3, 3)
    d = spnn.use_counter_dropout(model, seed=9)
    assert model.dropout is d and (d.p, d.inplace, d.training) == (0.3, True, True)
    got = _step(model, True)
    assert got[3:] == (1, 1) and d.calls == 2
    spnn.use_counter_dropout(ref, seed=9)
    _same_step(got, _step(ref, True, planned=False))
