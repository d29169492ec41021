"""lidal_amd.optim.AdamW / SGD and the gradient-norm clipping of all three optimizers, without a GPU: the arithmetic they
restate (tests/optim_ref.py) against torch's optimizers and clip_grad_norm_ in f64, the norm's summation against
math.fsum, what is refused, and the state_dicts against torch's on the reference's parameter names."""
import copy
import json
import math
import os

import numpy as np
import pytest
import torch

import adam_ref
import optim_ref

MAX_NORM = 10.0


def _block():
    from lidal_amd import backend as B
    return int(B.lib_handle().lidal_grad_norm_block_elems())


# ---- the restatement against torch in f64 -------------------------------------------------------------------------------
_CASES = {
    'sgd_plain': ('sgd', dict(lr=1e-3)),
    'sgd_momentum': ('sgd', dict(lr=1e-3, momentum=0.9)),
    'sgd_nesterov_wd': ('sgd', dict(lr=1e-3, momentum=0.9, nesterov=True, weight_decay=1e-4)),
    'sgd_dampening_wd': ('sgd', dict(lr=1e-3, momentum=0.9, dampening=0.1, weight_decay=1e-4)),
    'adamw_lr1e-3_wd0.01': ('adamw', dict(lr=1e-3, weight_decay=0.01)),
    'adamw_lr8e-3_wd0.05': ('adamw', dict(lr=8e-3, weight_decay=0.05)),
}


def _errors(run, ref):
    """max |run - ref| over the elements, per quantity, in f64"""
    return [float(np.abs(np.asarray(a, np.float64) - b).max()) for a, b in zip(run, ref)]


def _torch_state(kind, opt, p):
    keys = ('exp_avg', 'exp_avg_sq') if kind == 'adamw' else (('momentum_buffer',) if opt.param_groups[0]['momentum'] else ())
    return [p.detach().numpy()] + [opt.state[p][k].detach().numpy() for k in keys]


@pytest.mark.parametrize('clip', [False, True], ids=['unclipped', 'max_norm_10'])
@pytest.mark.parametrize('case', list(_CASES))
def test_restatement_is_as_close_to_f64_torch_as_torch_f32(case, clip):
    """30 steps on 4 099 elements, adam_ref.wide_gradients with seed 11: optim_ref (f32, every operation rounded separately)
    against torch.optim.{SGD,AdamW}(foreach=False) in f64 -- behind clip_grad_norm_(max_norm=10, foreach=False) in the
    clipped runs -- beside the same torch optimizer in f32.  The restatement's largest error over the run in p and in each
    state array may be at most 2 x torch's own f32 error against the same f64 run (DESIGN.md section 15's bound)."""
    kind, kw = _CASES[case]
    block = _block()
    rng = np.random.default_rng(11)
    n, steps = 4099, 30
    p0 = rng.standard_normal(n).astype(np.float32)
    grads = adam_ref.wide_gradients(rng, steps, n)
    p64 = torch.from_numpy(p0.astype(np.float64)).requires_grad_(True)
    p32 = torch.from_numpy(p0.copy()).requires_grad_(True)
    make = torch.optim.AdamW if kind == 'adamw' else torch.optim.SGD
    o64, o32 = make([p64], foreach=False, **kw), make([p32], foreach=False, **kw)
    p = p0.copy()
    m, v, buf = np.zeros(n, np.float32), np.zeros(n, np.float32), None
    worst_ref = worst_t32 = None
    for t, g in enumerate(grads, 1):
        p64.grad = torch.from_numpy(g.astype(np.float64))
        p32.grad = torch.from_numpy(g.copy())
        coef = None
        if clip:
            torch.nn.utils.clip_grad_norm_([p64], MAX_NORM, foreach=False)
            torch.nn.utils.clip_grad_norm_([p32], MAX_NORM, foreach=False)
            coef = optim_ref.clip_coef(optim_ref.grad_norm([g], block), MAX_NORM)
        o64.step()
        o32.step()
        if kind == 'adamw':
            p, m, v = optim_ref.adamw_step(p, g, m, v, t, coef=coef, **kw)
            mine = [p, m, v]
        else:
            p, buf = optim_ref.sgd_step(p, g, buf, coef=coef, **kw)
            mine = [p] if buf is None else [p, buf]
        want = _torch_state(kind, o64, p64)
        t32 = _torch_state(kind, o32, p32)
        assert len(mine) == len(want)
        e_ref, e_t32 = _errors(mine, want), _errors(t32, want)
        worst_ref = e_ref if worst_ref is None else [max(a, b) for a, b in zip(worst_ref, e_ref)]
        worst_t32 = e_t32 if worst_t32 is None else [max(a, b) for a, b in zip(worst_t32, e_t32)]
    for name, a, b in zip(['p', 'state0', 'state1'], worst_ref, worst_t32):
        print('%s clip %s  %s: restatement %.3e  torch f32 %.3e  ratio %.3f' % (case, clip, name, a, b, a / b))
        assert b > 0 and a <= 2 * b, (case, clip, name, a, b)


# ---- the norm ---------------------------------------------------------------------------------------------------------
def _ulp_distance(a, b):
    a, b = np.float32(a), np.float32(b)
    return abs(int(a.view(np.int32)) - int(b.view(np.int32)))


def test_the_norm_is_within_one_ulp_of_the_exactly_summed_one():
    """optim_ref.grad_norm (the kernel's block order) against f32(sqrt(math.fsum(g64 * g64))) on tensors of 1, block - 1,
    block, block + 1 and 2 block + 3 elements, one at a time and all together: the f64 sum of at most 2^25 exact squares
    carries a relative error below 2^25 x 2^-53, far under half an f32 ulp, so only a rounding tie can move the result."""
    block = _block()
    rng = np.random.default_rng(3)
    sizes = [1, block - 1, block, block + 1, 2 * block + 3]
    tensors = [g for n in sizes for g in adam_ref.wide_gradients(rng, 1, n)]

    def exact(ts):
        return np.float32(math.sqrt(math.fsum(x for t in ts for x in (t.astype(np.float64) ** 2).tolist())))
    for t in tensors:
        assert _ulp_distance(optim_ref.grad_norm([t], block), exact([t])) <= 1, t.size
    assert _ulp_distance(optim_ref.grad_norm(tensors, block), exact(tensors)) <= 1
    # a record without a gradient and an empty tensor count as zero
    with_gaps = [tensors[0], None, np.zeros(0, np.float32)] + tensors[1:]
    assert adam_ref.bits(optim_ref.grad_norm(with_gaps, block)) == adam_ref.bits(optim_ref.grad_norm(tensors, block))
    assert optim_ref.norm_slots(sizes + [0], block) == 1 + 1 + 1 + 2 + 3


def test_the_norm_of_zeros_and_of_a_nan():
    block = _block()
    zero = np.zeros(block + 5, np.float32)
    total = optim_ref.grad_norm([zero], block)
    assert total == 0 and adam_ref.bits(optim_ref.clip_coef(total, MAX_NORM)) == adam_ref.bits(np.float32(1.0))
    bad = np.ones(block + 5, np.float32)
    bad[block + 2] = np.nan
    total = optim_ref.grad_norm([bad], block)
    assert np.isnan(total) and np.isnan(optim_ref.clip_coef(total, MAX_NORM))
    inf = np.ones(7, np.float32)
    inf[3] = np.inf
    total = optim_ref.grad_norm([inf], block)
    assert np.isposinf(total) and optim_ref.clip_coef(total, MAX_NORM) == 0
    # |g| = 3e38: the f64 sum is finite, its f32 root is not
    big = np.full(3, 3e38, np.float32)
    assert np.isposinf(optim_ref.grad_norm([big], block))
    # the coefficient: ONE correctly rounded division, so it is the f32 nearest to the f64 quotient (torch's own f32 form,
    # `max_norm / tensor`, is reciprocal() * max_norm: two roundings, up to an ulp off this)
    for total in (np.float32(3.0), np.float32(10.0), np.float32(12345.678), np.float32(1e-30)):
        den = np.float32(total + np.float32(1e-6))
        want = np.float32(min(MAX_NORM / np.float64(den), 1.0))
        assert adam_ref.bits(optim_ref.clip_coef(total, MAX_NORM)) == adam_ref.bits(want)
        theirs = torch.clamp(MAX_NORM / (torch.tensor(total) + 1e-6), max=1.0)
        assert _ulp_distance(optim_ref.clip_coef(total, MAX_NORM), theirs.numpy()) <= 1


# ---- host behaviour ---------------------------------------------------------------------------------------------------
def _param(*shape, dtype=torch.float32):
    return torch.nn.Parameter(torch.zeros(*shape, dtype=dtype))


def test_refusals():
    from lidal_amd.optim import SGD, Adam, AdamW
    for cls, extra in ((AdamW, ('amsgrad', 'capturable')), (SGD, ())):
        for key in ('maximize', 'differentiable') + extra:
            with pytest.raises(ValueError, match=key):
                cls([_param(3)], **{key: True})
        with pytest.raises(ValueError, match='lr'):
            cls([_param(3)], lr=torch.tensor(1e-3))
        with pytest.raises(ValueError, match='float32'):
            cls([_param(3), _param(3, dtype=torch.float64)])
        with pytest.raises(ValueError, match='float32'):
            cls([_param(3, dtype=torch.bfloat16)])
        with pytest.raises(ValueError, match='contiguous'):
            cls([torch.nn.Parameter(torch.zeros(4, 6).t())])
        with pytest.raises(ValueError, match='more than one device'):
            cls([_param(3), torch.nn.Parameter(torch.zeros(3, device='meta'))])
        # gradients: sparse and non-f32 ones are refused by the step that sees them
        p = _param(4, 2)
        opt = cls([p])
        p.grad = torch.zeros(4, 2).to_sparse()
        with pytest.raises(ValueError, match='sparse'):
            opt.step()
        q = _param(4)
        opt = cls([q])
        q.grad = torch.zeros(4)
        q.grad.data = torch.zeros(4, dtype=torch.float16)
        with pytest.raises(ValueError, match='float32'):
            opt.step()
        assert opt.launches == 0
    # clip_grad_norm: a positive Python number or None, at construction and at the step that sees it
    for cls in (Adam, AdamW, SGD):
        for bad in (0, -1.0, torch.tensor(1.0), '10', True):
            with pytest.raises(ValueError, match='clip_grad_norm'):
                cls([_param(3)], clip_grad_norm=bad)
        p = _param(3)
        opt = cls([p], clip_grad_norm=5)
        assert opt.clip_grad_norm == 5 and opt.grad_norm is None
        opt.clip_grad_norm = 0.0
        p.grad = torch.zeros(3)
        with pytest.raises(ValueError, match='clip_grad_norm'):
            opt.step()
        assert opt.launches == 0
    # Nesterov: torch's own rule, also when a group is changed later
    with pytest.raises(ValueError, match='Nesterov'):
        SGD([_param(3)], nesterov=True)
    with pytest.raises(ValueError, match='Nesterov'):
        SGD([_param(3)], momentum=0.9, dampening=0.1, nesterov=True)
    p = _param(3)
    opt = SGD([p], momentum=0.9, nesterov=True)
    opt.param_groups[0]['momentum'] = 0
    p.grad = torch.zeros(3)
    with pytest.raises(ValueError, match='Nesterov'):
        opt.step()
    # Adam still refuses the decoupled form and says where it is; AdamW refuses the coupled one
    with pytest.raises(ValueError, match='decoupled_weight_decay.*AdamW'):
        Adam([_param(3)]).load_state_dict(torch.optim.AdamW([_param(3)]).state_dict())
    with pytest.raises(ValueError, match='decoupled_weight_decay'):
        AdamW([_param(3)]).load_state_dict(torch.optim.Adam([_param(3)]).state_dict())
    with pytest.raises(ValueError, match='amsgrad'):
        AdamW([_param(3)]).load_state_dict(torch.optim.AdamW([_param(3)], amsgrad=True).state_dict())


def test_cpu_parameters_raise_gpu_only():
    from lidal_amd.optim import SGD, AdamW
    for make in (lambda p: AdamW([p], clip_grad_norm=1.0), lambda p: SGD([p], momentum=0.9), lambda p: SGD([p])):
        p = _param(5)
        opt = make(p)
        p.grad = torch.ones(5)
        with pytest.raises(RuntimeError, match='GPU only'):
            opt.step()
        assert torch.equal(p.detach(), torch.zeros(5)) and opt.launches == 0


def test_a_step_without_gradients_is_a_no_op():
    from lidal_amd.optim import SGD, Adam, AdamW
    for make in (lambda p: AdamW(p, clip_grad_norm=1.0), lambda p: SGD(p, momentum=0.9, clip_grad_norm=1.0),
                 lambda p: Adam(p, clip_grad_norm=1.0)):
        opt = make([_param(5)])
        assert opt.step() is None and opt.launches == 0 and opt.table_uploads == 0 and len(opt.state) == 0
        assert opt.step(lambda: 3.0) == 3.0 and opt.grad_norm is None


def _named_spvcnn(golden_dir):
    from lidal_amd.network import SPVCNN
    model = SPVCNN(19)
    named = list(model.named_parameters())
    ref = json.load(open(os.path.join(golden_dir, 'state_dict_spvcnn.json')))
    want = [[k, s] for k, s, _ in ref if not k.endswith(('running_mean', 'running_var', 'num_batches_tracked'))]
    assert [[k, list(p.shape)] for k, p in named] == want
    g = torch.Generator().manual_seed(0)
    for _, p in named:
        p.grad = torch.randn(p.shape, generator=g)
    return named


def _same_dicts(a, b, named, keys):
    assert list(a) == list(b) == ['state', 'param_groups']
    assert list(a['state']) == list(b['state']) == list(range(len(named)))
    for i in a['state']:
        assert list(a['state'][i]) == list(b['state'][i]) == keys
        for k in keys:
            x, y = a['state'][i][k], b['state'][i][k]
            assert x.shape == y.shape and x.dtype == y.dtype and x.device == y.device and torch.equal(x, y), (i, k)
    ga, gb = a['param_groups'][0], b['param_groups'][0]
    assert ga['params'] == gb['params'] and ga['param_names'] == gb['param_names'] == [k for k, _ in named]
    assert set(ga) <= set(gb)
    for k in ga:
        assert ga[k] == gb[k], k


def test_adamw_state_dict_is_torchs_on_the_reference_parameter_names(golden_dir):
    """Keys, shapes and dtypes of AdamW.state_dict() equal torch.optim.AdamW's over SPVCNN's parameters; each optimizer
    loads the other's dict (decoupled_weight_decay=True travels with the group), and the loaded moments are copied into the
    flat buffers."""
    from lidal_amd.optim import AdamW
    named = _named_spvcnn(golden_dir)
    theirs = torch.optim.AdamW(named, lr=2e-3, weight_decay=0.02, foreach=False)
    theirs.step()
    mine = AdamW(named, lr=5e-4)
    mine.load_state_dict(copy.deepcopy(theirs.state_dict()))
    a, b = mine.state_dict(), theirs.state_dict()
    _same_dicts(a, b, named, ['step', 'exp_avg', 'exp_avg_sq'])
    assert a['param_groups'][0]['lr'] == 2e-3 and a['param_groups'][0]['weight_decay'] == 0.02
    assert a['param_groups'][0]['decoupled_weight_decay'] is True
    st = mine.state[named[0][1]]['exp_avg'].untyped_storage().data_ptr()
    assert all(mine.state[p]['exp_avg'].untyped_storage().data_ptr() == st for _, p in named)
    again = torch.optim.AdamW(named, foreach=False)
    again.load_state_dict(copy.deepcopy(a))
    assert again.param_groups[0]['decoupled_weight_decay'] is True
    again.step()
    assert all(float(again.state[p]['step']) == 2.0 for _, p in named)
    assert all(float(mine.state[p]['step']) == 1.0 for _, p in named)
    # a fresh AdamW's groups are torch's too
    fresh = AdamW(named).state_dict()['param_groups'][0]
    ref = torch.optim.AdamW(named).state_dict()['param_groups'][0]
    assert set(fresh) <= set(ref) and all(fresh[k] == ref[k] for k in fresh)


def test_sgd_state_dict_is_torchs_on_the_reference_parameter_names(golden_dir):
    """The same for SGD: state[p] is {'momentum_buffer': ...} after a step with momentum, views of ONE flat buffer here;
    with momentum 0 the state stays empty, as torch's does.  A loaded dict without a buffer for a parameter leaves that
    parameter at its first step."""
    from lidal_amd.optim import SGD
    named = _named_spvcnn(golden_dir)
    kw = dict(lr=0.02, momentum=0.9, nesterov=True, weight_decay=1e-4)
    theirs = torch.optim.SGD(named, foreach=False, **kw)
    theirs.step()
    mine = SGD(named, lr=5e-4)
    mine.load_state_dict(copy.deepcopy(theirs.state_dict()))
    a, b = mine.state_dict(), theirs.state_dict()
    _same_dicts(a, b, named, ['momentum_buffer'])
    assert all(a['param_groups'][0][k] == v for k, v in kw.items())
    st = mine.state[named[0][1]]['momentum_buffer'].untyped_storage().data_ptr()
    assert all(mine.state[p]['momentum_buffer'].untyped_storage().data_ptr() == st for _, p in named)
    assert mine._rt[0].uniform == 1                          # every parameter is past its first step
    again = torch.optim.SGD(named, foreach=False)
    again.load_state_dict(copy.deepcopy(a))
    again.step()
    assert again.param_groups[0]['nesterov'] is True and len(again.state) == len(named)
    # momentum 0: no state on either side, and the dicts load both ways
    plain_t = torch.optim.SGD(named, lr=0.1, foreach=False)
    plain_t.step()
    plain = SGD(named, lr=0.5)
    plain.load_state_dict(copy.deepcopy(plain_t.state_dict()))
    assert plain.state_dict()['state'] == plain_t.state_dict()['state'] == {}
    assert plain.param_groups[0]['lr'] == 0.1
    torch.optim.SGD(named, foreach=False).load_state_dict(copy.deepcopy(plain.state_dict()))
    # a dict that has a buffer for some parameters only (and None, as older torch wrote it, for another)
    part = copy.deepcopy(theirs.state_dict())
    del part['state'][0]
    part['state'][1] = {'momentum_buffer': None}
    half = SGD(named)
    half.load_state_dict(part)
    assert half._rt[0].steps[:3] == [0, 0, 1] and half._rt[0].uniform is None
    assert named[0][1] not in half.state and named[1][1] not in half.state and named[2][1] in half.state
