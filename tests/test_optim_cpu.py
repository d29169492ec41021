"""lidal_amd.optim.Adam without a GPU: the arithmetic it restates (tests/adam_ref.py) against torch.optim.Adam in f64, what
it refuses, and its state_dict against torch.optim.Adam's on the reference's parameter names."""
import copy
import json
import os

import numpy as np
import pytest
import torch

import adam_ref


def _errors(run, ref):
    """max |run - ref| over the elements, per quantity (p, m, v), in f64"""
    return [float(np.abs(np.asarray(a, np.float64) - b).max()) for a, b in zip(run, ref)]


@pytest.mark.parametrize('weight_decay', [0.0, 0.01])
def test_restatement_is_as_close_to_f64_adam_as_torch_f32(weight_decay):
    """30 steps on 4 099 elements, gradient magnitudes 1e-6 .. 1e3, every seventh step's gradient one-third zeros:
    adam_ref (f32, every operation rounded separately) against torch.optim.Adam(foreach=False) in f64, beside the same
    optimizer in f32.  Both f32 runs round one formula and differ only in contraction, so the restatement's largest
    error over the run in p, m and v may be at most 2 x torch's own f32 error against the same f64 run."""
    rng = np.random.default_rng(11)
    n, steps = 4099, 30
    p0 = rng.standard_normal(n).astype(np.float32)
    grads = adam_ref.wide_gradients(rng, steps, n)
    p64 = torch.from_numpy(p0.astype(np.float64)).requires_grad_(True)
    p32 = torch.from_numpy(p0.copy()).requires_grad_(True)
    o64 = torch.optim.Adam([p64], weight_decay=weight_decay, foreach=False)
    o32 = torch.optim.Adam([p32], weight_decay=weight_decay, foreach=False)
    p, m, v = p0.copy(), np.zeros(n, np.float32), np.zeros(n, np.float32)
    worst_ref, worst_t32 = [0.0] * 3, [0.0] * 3
    for t, g in enumerate(grads, 1):
        p64.grad = torch.from_numpy(g.astype(np.float64))
        p32.grad = torch.from_numpy(g.copy())
        o64.step()
        o32.step()
        p, m, v = adam_ref.adam_step(p, g, m, v, t, weight_decay=weight_decay)
        want = [x.detach().numpy() for x in (p64, o64.state[p64]['exp_avg'], o64.state[p64]['exp_avg_sq'])]
        t32 = [x.detach().numpy() for x in (p32, o32.state[p32]['exp_avg'], o32.state[p32]['exp_avg_sq'])]
        worst_ref = [max(a, b) for a, b in zip(worst_ref, _errors((p, m, v), want))]
        worst_t32 = [max(a, b) for a, b in zip(worst_t32, _errors(t32, want))]
    for name, mine, theirs in zip('pmv', worst_ref, worst_t32):
        print('weight_decay %g  %s: restatement %.3e  torch f32 %.3e  ratio %.3f' % (weight_decay, name, mine, theirs,
                                                                                     mine / theirs))
        assert theirs > 0 and mine <= 2 * theirs, (name, mine, theirs)


def test_restatement_keeps_subnormals():
    """(1 - beta2) g g is subnormal for |g| ~ 1e-20: the restatement keeps it (and so must the kernel)."""
    g = np.full(4, 1e-20, np.float32)
    z = np.zeros(4, np.float32)
    _, _, v = adam_ref.adam_step(z, g, z, z, 1)
    assert (v > 0).all() and (v < np.finfo(np.float32).tiny).all()


def _param(*shape, dtype=torch.float32):
    return torch.nn.Parameter(torch.zeros(*shape, dtype=dtype))


def test_refuses_what_it_does_not_implement():
    from lidal_amd.optim import Adam
    for kw in ({'amsgrad': True}, {'maximize': True}, {'capturable': True}, {'differentiable': True},
               {'lr': torch.tensor(1e-3)}):
        with pytest.raises(ValueError, match=next(iter(kw))):
            Adam([_param(3)], **kw)
    with pytest.raises(ValueError, match='float32'):
        Adam([_param(3), _param(3, dtype=torch.float64)])
    with pytest.raises(ValueError, match='float32'):
        Adam([_param(3, dtype=torch.bfloat16)])
    with pytest.raises(ValueError, match='contiguous'):
        Adam([torch.nn.Parameter(torch.zeros(4, 6).t())])
    with pytest.raises(ValueError, match='more than one device'):
        Adam([_param(3), torch.nn.Parameter(torch.zeros(3, device='meta'))])
    opt = Adam([_param(3)])
    opt.param_groups[0]['amsgrad'] = True                   # switched on later: refused by the step that sees it
    opt.param_groups[0]['params'][0].grad = torch.zeros(3)
    with pytest.raises(ValueError, match='amsgrad'):
        opt.step()
    # gradients: sparse and non-f32 ones are refused by the step that sees them
    p = _param(4, 2)
    opt = Adam([p])
    p.grad = torch.zeros(4, 2).to_sparse()
    with pytest.raises(ValueError, match='sparse'):
        opt.step()
    p.grad = None
    q = _param(4)
    opt = Adam([q])
    q.grad = torch.zeros(4)
    q.grad.data = torch.zeros(4, dtype=torch.float16)
    with pytest.raises(ValueError, match='float32'):
        opt.step()
    # a loaded dict that asks for AMSGrad
    theirs = torch.optim.Adam([_param(3)], amsgrad=True)
    with pytest.raises(ValueError, match='amsgrad'):
        Adam([_param(3)]).load_state_dict(theirs.state_dict())


def test_cpu_parameters_raise_gpu_only():
    from lidal_amd.optim import Adam
    p = _param(5)
    opt = Adam([p])
    p.grad = torch.ones(5)
    with pytest.raises(RuntimeError, match='GPU only'):
        opt.step()
    assert torch.equal(p.detach(), torch.zeros(5)) and opt.launches == 0


def test_a_step_without_gradients_is_a_no_op():
    from lidal_amd.optim import Adam
    opt = Adam([_param(5)])
    assert opt.step() is None and opt.launches == 0 and opt.table_uploads == 0 and len(opt.state) == 0
    assert opt.step(lambda: 3.0) == 3.0


def test_state_dict_is_torch_adams_on_the_reference_parameter_names(golden_dir):
    """Keys, shapes and dtypes of state_dict() equal torch.optim.Adam's over SPVCNN's parameters (names as in the
    reference's checkpoint surface, tests/golden/state_dict_spvcnn.json); each optimizer loads the other's dict, and the
    loaded moments are copied into the flat buffers (the views stay views)."""
    from lidal_amd.network import SPVCNN
    from lidal_amd.optim import Adam
    model = SPVCNN(19)
    named = list(model.named_parameters())
    ref = json.load(open(os.path.join(golden_dir, 'state_dict_spvcnn.json')))
    want = [[k, s] for k, s, _ in ref if not k.endswith(('running_mean', 'running_var', 'num_batches_tracked'))]
    assert [[k, list(p.shape)] for k, p in named] == want
    theirs = torch.optim.Adam(named, lr=2e-3, weight_decay=0.01, foreach=False)
    g = torch.Generator().manual_seed(0)
    for _, p in named:
        p.grad = torch.randn(p.shape, generator=g)
    theirs.step()
    mine = Adam(named, lr=5e-4)
    mine.load_state_dict(copy.deepcopy(theirs.state_dict()))
    a, b = mine.state_dict(), theirs.state_dict()
    assert list(a) == list(b) == ['state', 'param_groups']
    assert list(a['state']) == list(b['state']) == list(range(len(named)))
    for i in a['state']:
        assert list(a['state'][i]) == list(b['state'][i]) == ['step', 'exp_avg', 'exp_avg_sq']
        for k in a['state'][i]:
            x, y = a['state'][i][k], b['state'][i][k]
            assert x.shape == y.shape and x.dtype == y.dtype and x.device == y.device and torch.equal(x, y), (i, k)
    ga, gb = a['param_groups'][0], b['param_groups'][0]
    assert ga['params'] == gb['params'] and ga['param_names'] == gb['param_names'] == [k for k, _ in named]
    assert ga['lr'] == 2e-3 and ga['weight_decay'] == 0.01 and ga['betas'] == gb['betas'] and ga['eps'] == gb['eps']
    assert set(ga) <= set(gb)
    # the loaded moments live in ONE flat buffer per kind
    st = mine.state[named[0][1]]['exp_avg'].untyped_storage().data_ptr()
    assert all(mine.state[p]['exp_avg'].untyped_storage().data_ptr() == st for _, p in named)
    # ... and torch.optim.Adam takes the dict back and steps on it
    again = torch.optim.Adam(named, foreach=False)
    again.load_state_dict(copy.deepcopy(a))
    again.step()
    assert all(float(again.state[p]['step']) == 2.0 for _, p in named)
    assert all(float(mine.state[p]['step']) == 1.0 for _, p in named)
