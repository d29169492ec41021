"""lidal_amd.optim.AdamW / SGD and the gradient-norm clipping of all three optimizers on the GPU: the kernels (csrc/optim.hip)
bit for bit against the numpy restatement (tests/optim_ref.py, tests/adam_ref.py), the norm at its edges and in exact
scratch, against torch's optimizers on the device, their state across optimizers, and inside the training steps."""
import copy

import numpy as np
import pytest
import torch

import adam_ref
import optim_ref
from guarded_ws import Guarded

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _chunk():
    from lidal_amd import backend as B
    return int(B.lib_handle().lidal_adam_chunk_elems())


def _block():
    from lidal_amd import backend as B
    return int(B.lib_handle().lidal_grad_norm_block_elems())


def _np(t):
    return t.detach().cpu().numpy()


def _same_bits(a, b):
    return np.array_equal(adam_ref.bits(a).reshape(-1), adam_ref.bits(b).reshape(-1))


def _same_values(a, b):
    """Equal bits, except that any NaN equals any NaN (numpy's and the GPU's default NaN differ in the sign bit)."""
    a, b = np.asarray(a, np.float32).reshape(-1), np.asarray(b, np.float32).reshape(-1)
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(adam_ref.bits(a)[~na], adam_ref.bits(b)[~nb])


# ---- the restated optimizers, one parameter at a time -------------------------------------------------------------------
class _Ref:
    """One parameter of the restatement: p and whatever state its rule keeps."""

    def __init__(self, kind, p):
        self.kind, self.p, self.t = kind, p.reshape(-1).copy(), 0
        self.m = np.zeros(self.p.size, np.float32)
        self.v = np.zeros(self.p.size, np.float32)
        self.buf = None

    def step(self, g, hyper, coef):
        g = np.ascontiguousarray(g, np.float32).reshape(-1)
        if self.kind == 'sgd':
            self.p, self.buf = optim_ref.sgd_step(self.p, g, self.buf, coef=coef, **hyper)
            if hyper.get('momentum', 0) != 0:
                self.t += 1
            return
        self.t += 1
        kw = dict(hyper)
        beta1, beta2 = kw.pop('betas', (0.9, 0.999))
        fn = optim_ref.adamw_step if self.kind == 'adamw' else optim_ref.adam_step
        self.p, self.m, self.v = fn(self.p, g, self.m, self.v, self.t, beta1=beta1, beta2=beta2, coef=coef, **kw)

    def check(self, opt, p, where):
        assert _same_values(_np(p), self.p), ('p',) + where
        st = opt.state.get(p, {})
        if self.kind == 'sgd':
            if self.buf is None:
                assert st.get('momentum_buffer') is None, where
            else:
                assert list(st) == ['momentum_buffer'] and st['momentum_buffer'].shape == p.shape
                assert _same_values(_np(st['momentum_buffer']), self.buf), ('momentum_buffer',) + where
        elif self.t == 0:
            assert not st, where
        else:
            assert float(st['step']) == self.t, where
            assert _same_values(_np(st['exp_avg']), self.m), ('exp_avg',) + where
            assert _same_values(_np(st['exp_avg_sq']), self.v), ('exp_avg_sq',) + where


def _make(kind, groups, **kw):
    from lidal_amd.optim import SGD, Adam, AdamW
    return {'adamw': AdamW, 'adam': Adam, 'sgd': SGD}[kind](groups, **kw)


def _run_key(kind, hyper, done):
    """What the records of one update launch share: Adam's step count; for SGD whether the launch writes buf = g."""
    return (hyper.get('momentum', 0) != 0 and done == 0) if kind == 'sgd' else done


def _update_launches(kind, members, hyper, refs, has_grad, sizes):
    """Update launches of one step: per group the runs of consecutive parameters that have a gradient (and elements) and
    share their key -- one launch when every parameter of the group has a gradient and the same step count."""
    n = 0
    for mem, h in zip(members, hyper):
        if all(has_grad[i] for i in mem) and len({refs[i].t for i in mem}) == 1:
            n += 1
            continue
        prev = None
        for i in mem:
            if not has_grad[i] or sizes[i] == 0:
                prev = None
                continue
            if prev is None or _run_key(kind, h, refs[i].t) != _run_key(kind, h, refs[prev].t):
                n += 1
            prev = i
    return n


def _norm_launches(order, has_grad):
    """Launches of the norm: one per run of consecutive records that all have, or all lack, a gradient; and the finish."""
    flags = [has_grad[i] for i in order]
    return 1 + sum(1 for a, b in zip([None] + flags, flags) if a != b)


# ---- bit for bit against the restatement --------------------------------------------------------------------------------
_MAGNITUDES = (1e-20, 1e-6, 1.0, 1e3)


def _edge_gradient(rng, n):
    """magnitudes 1e-20, 1e-6, 1 and 1e3 (a different one per element), one element in eight an exact zero"""
    g = rng.choice(_MAGNITUDES, n) * rng.uniform(1.0, 2.0, n) * rng.choice([-1.0, 1.0], n)
    g[rng.random(n) < 0.125] = 0.0
    return g.astype(np.float32)


_RULES = {
    'adamw': ('adamw', [dict(lr=1e-3, weight_decay=0.0), dict(lr=3e-3, weight_decay=0.01)]),
    'sgd_momentum_nesterov_wd': ('sgd', [dict(lr=1e-3, momentum=0.9, nesterov=True, weight_decay=1e-4),
                                         dict(lr=3e-3, momentum=0.8, dampening=0.1)]),
    'sgd_momentum_0': ('sgd', [dict(lr=1e-3), dict(lr=3e-3, weight_decay=0.01)]),
    'adam_clipped': ('adam', [dict(lr=1e-3, weight_decay=0.0), dict(lr=3e-3, weight_decay=0.01)]),
}


@pytest.mark.parametrize('flat', [False, True], ids=['separate_gradients', 'flat_gradient_buffer'])
@pytest.mark.parametrize('rule', list(_RULES))
def test_kernels_equal_the_restatement_bit_for_bit(rule, flat):
    """One optimizer over 217 tensors -- 1, 3, 4, 5, 255, 256, 257, chunk - 1, chunk, chunk + 1, 2 chunk + 3 elements, the
    norm's block - 1, block, block + 1, 2 block + 3, 200 tensors of 1 to 7 elements, a view starting 4 bytes into its
    storage and one empty tensor -- in two groups with different hyperparameters, 12 steps: p and every state array equal
    the restatement bit for bit after every step, `.grad` is what it was, and optimizer.grad_norm has the restatement's
    bits in BOTH gradient forms (separately allocated: absolute addresses; views of one buffer in 16-byte slots that is a
    new allocation every step: the table is uploaded once), which is what makes the order independent of address and
    form.  Gradients of magnitude 1e-20, 1e-6, 1 and 1e3 with exact zeros, step 8 all zero, one parameter without a
    gradient on steps 3 to 5, lr and momentum (beta1) changed at step 6, clip_grad_norm None until step 3, 10 from step 4
    (it clips) and 1e9 from step 10 (coef is exactly 1)."""
    kind, hyper = _RULES[rule]
    hyper = [dict(h) for h in hyper]
    c, nb = _chunk(), _block()
    rng = np.random.default_rng(17)
    sizes = [1, 3, 4, 5, 255, 256, 257, c - 1, c, c + 1, 2 * c + 3]
    sizes += [n for n in (nb - 1, nb, nb + 1, 2 * nb + 3) if n not in sizes]
    sizes += [int(k) for k in np.random.default_rng(5).integers(1, 8, 200)]
    params = [torch.nn.Parameter(torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(DEV)) for n in sizes]
    odd = torch.from_numpy(rng.standard_normal(1030).astype(np.float32)).to(DEV)
    params.insert(9, torch.nn.Parameter(odd[1:]))            # 1 029 elements from byte 4 of their storage
    assert params[9].data_ptr() % 16 == 4 and params[9].is_contiguous()
    odd_first = float(odd[0])
    params.append(torch.nn.Parameter(torch.empty(0, device=DEV)))
    sizes = [p.numel() for p in params]
    n_par = len(params)
    members = [list(range(0, n_par, 2)), list(range(1, n_par, 2))]        # both groups get every kind of tensor
    order = members[0] + members[1]                                       # the records
    opt = _make(kind, [dict(params=[params[i] for i in mem], **h) for mem, h in zip(members, hyper)])
    assert opt.clip_grad_norm is None and opt.grad_norm is None
    group_of = {i: gi for gi, mem in enumerate(members) for i in mem}
    lagging = 6                                              # the 257-element tensor
    assert sizes[lagging] == 257 and lagging in members[0][1:-1]
    slots, total = [], 0
    for n in sizes:
        slots.append(total)
        total += (n + 3) & -4
    refs = [_Ref(kind, _np(p)) for p in params]
    kept, launches = [], 0
    for step in range(1, 13):
        if step == 4:
            opt.clip_grad_norm = 10
        if step == 10:
            opt.clip_grad_norm = 1e9
        if step == 6:
            opt.param_groups[0]['lr'] = hyper[0]['lr'] = 4e-4
            if kind == 'sgd' and hyper[0].get('momentum'):
                opt.param_groups[0]['momentum'] = hyper[0]['momentum'] = 0.85
            if kind != 'sgd':
                opt.param_groups[0]['betas'] = hyper[0]['betas'] = (0.85, 0.999)
        host = np.zeros(total + 16, np.float32)
        for i, n in enumerate(sizes):
            if step != 8:
                host[slots[i]:slots[i] + n] = _edge_gradient(rng, n)
        buf = torch.from_numpy(host).to(DEV)
        kept.append(buf)                                     # (alive: the next step's buffer is another allocation)
        has_grad = [not (i == lagging and 3 <= step <= 5) for i in range(n_par)]
        for i, p in enumerate(params):
            view = buf[slots[i]:slots[i] + sizes[i]]
            p.grad = None if not has_grad[i] else (view if flat else view.clone())
        grads = [host[slots[i]:slots[i] + sizes[i]] if has_grad[i] else None for i in range(n_par)]
        launches += _update_launches(kind, members, hyper, refs, has_grad, sizes)
        coef = None
        if opt.clip_grad_norm is not None:
            launches += _norm_launches(order, has_grad)
            norm = optim_ref.grad_norm([grads[i] for i in order], nb)
            coef = optim_ref.clip_coef(norm, opt.clip_grad_norm)
            assert (coef < 1) == (step in (4, 5, 6, 7, 9)), (step, norm, coef)
        opt.step()
        if coef is None:
            assert opt.grad_norm is None
        else:
            assert opt.grad_norm.shape == () and opt.grad_norm.dtype == torch.float32 and opt.grad_norm.is_cuda
            assert _same_bits(_np(opt.grad_norm), norm), (step, float(opt.grad_norm), float(norm))
            assert _same_bits(_np(opt._norm[1]), coef), (step, float(opt._norm[1]), float(coef))
        for i, p in enumerate(params):
            if has_grad[i]:
                refs[i].step(grads[i], hyper[group_of[i]], coef)
                assert _same_bits(_np(p.grad), grads[i]), ('grad', step, i)         # the clipped gradient is not written back
        for i, p in enumerate(params):
            refs[i].check(opt, p, (step, i, sizes[i]))
        assert opt.launches == launches, (step, opt.launches, launches)
    assert float(odd[0]) == odd_first                        # the float in front of the view
    if kind != 'sgd':
        assert refs[lagging].t == 9 and refs[0].t == 12
    if flat:
        assert opt.table_uploads == 1
    else:
        assert opt.table_uploads >= 1


_OFF_PHASE_RULES = {
    'adamw': ('adamw', dict(lr=3e-3, weight_decay=0.01), None),
    'adamw_clipped': ('adamw', dict(lr=3e-3, weight_decay=0.01), 10),
    'sgd_momentum_0': ('sgd', dict(lr=3e-3, weight_decay=0.01), None),
    'sgd_momentum': ('sgd', dict(lr=1e-3, momentum=0.9, nesterov=True, weight_decay=1e-4), None),
}
_PATTERN = 0xA5A5A5A5


@pytest.mark.parametrize('rule', list(_OFF_PHASE_RULES))
def test_every_rule_at_one_phase_off_the_16_byte_grid(rule):
    """The 16-byte path of every rule with a head and a tail: parameters of 1, 2, 3, 4, 5, 7, chunk - 1, chunk, chunk + 1
    and 2 chunk + 3 elements are views that start 1, 2 or 3 elements behind a 16-byte boundary of one arena, their
    gradients views at the same offsets of a second one, and the optimizer places the state at the parameter's phase: all
    arrays of a rule share a phase that is not 0 (asserted).  Two steps, so SGD with momentum writes buf = g and then
    reads it: p and every state array equal the restatement bit for bit, and no word of the arenas or of the state
    buffers outside the views changed."""
    kind, hyper, clip = _OFF_PHASE_RULES[rule]
    c, nb = _chunk(), _block()
    sizes = [1, 2, 3, 4, 5, 7, c - 1, c, c + 1, 2 * c + 3]
    rng = np.random.default_rng(41)
    starts, end = [], 0
    for i, n in enumerate(sizes):
        starts.append(((end + 4) & -4) + 1 + i % 3)          # (at least one arena word between two views)
        end = starts[-1] + n
    total = (end + 8) & -4
    inside = np.zeros(total, bool)
    for s, n in zip(starts, sizes):
        inside[s:s + n] = True
    host_p = np.full(total, _PATTERN, np.uint32).view(np.float32)
    for s, n in zip(starts, sizes):
        host_p[s:s + n] = rng.standard_normal(n).astype(np.float32)
    arena_p = torch.from_numpy(host_p).to(DEV)
    arena_g = torch.from_numpy(np.full(total, _PATTERN, np.uint32).view(np.float32)).to(DEV)
    assert arena_p.data_ptr() % 16 == 0 and arena_g.data_ptr() % 16 == 0
    params = [torch.nn.Parameter(arena_p[s:s + n]) for s, n in zip(starts, sizes)]
    opt = _make(kind, params, clip_grad_norm=clip, **hyper)
    refs = [_Ref(kind, _np(p)) for p in params]
    for step in (1, 2):
        host_g = np.full(total, _PATTERN, np.uint32).view(np.float32)
        for s, n in zip(starts, sizes):
            host_g[s:s + n] = _edge_gradient(rng, n)
        arena_g.copy_(torch.from_numpy(host_g))
        grads = [host_g[s:s + n] for s, n in zip(starts, sizes)]
        for p, s, n in zip(params, starts, sizes):
            p.grad = arena_g[s:s + n]
        coef = None
        if clip is not None:
            coef = optim_ref.clip_coef(optim_ref.grad_norm(grads, nb), clip)
            assert coef < 1
        opt.step()
        for i, p in enumerate(params):
            phase = p.data_ptr() % 16
            assert phase == 4 * (1 + i % 3) and p.grad.data_ptr() % 16 == phase
            for key, t in opt.state.get(p, {}).items():
                if key != 'step':
                    assert t.data_ptr() % 16 == phase, (key, i)
            refs[i].step(grads[i], hyper, coef)
            refs[i].check(opt, p, (step, i, sizes[i]))
        assert _same_bits(_np(arena_g), host_g)
        assert (adam_ref.bits(_np(arena_p))[~inside] == _PATTERN).all()
        g = opt._rt[0]
        used = np.zeros(max(g.size, 1), bool)
        for o, n in zip(g.offs, g.numels):
            used[o:o + n] = True
        for buf in g.bufs or []:
            assert not adam_ref.bits(_np(buf))[~used].any()
    n_state = {'adamw': 2, 'sgd': 1 if hyper.get('momentum') else 0}[kind]
    assert len(opt._rt[0].bufs or []) == n_state
    assert opt.launches == 2 * (1 if clip is None else 3)


# ---- edges of the norm ----------------------------------------------------------------------------------------------------
def _one_clipped_step(kind, kw, sizes, grads, monkeypatch=None):
    """A single clipped step of `kind` over tensors of `sizes` (grads[i] None: no gradient) beside the restatement."""
    from lidal_amd import backend as B
    rng = np.random.default_rng(29)
    nb = _block()
    params = [torch.nn.Parameter(torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(DEV)) for n in sizes]
    refs = [_Ref(kind, _np(p)) for p in params]
    opt = _make(kind, params, clip_grad_norm=10, **kw)
    for p, g in zip(params, grads):
        p.grad = None if g is None else torch.from_numpy(g).to(DEV)
    guard = None
    if monkeypatch is not None:
        guard = Guarded()
        monkeypatch.setattr(B, 'workspace', guard)
    opt.step()
    if guard is not None:
        guard.check()
    norm = optim_ref.grad_norm(grads, nb)
    coef = optim_ref.clip_coef(norm, 10)
    assert _same_values(_np(opt.grad_norm), norm) and _same_values(_np(opt._norm[1]), coef)
    for i, (p, g) in enumerate(zip(params, grads)):
        if g is not None:
            refs[i].step(g, kw, coef)
        refs[i].check(opt, p, (i, sizes[i]))
    return opt, norm, coef, guard


_EDGE_RULES = [('adamw', dict(lr=1e-2, weight_decay=0.01)), ('sgd', dict(lr=1e-2, momentum=0.9, nesterov=True, weight_decay=1e-4))]


@pytest.mark.parametrize('kind,kw', _EDGE_RULES, ids=['adamw', 'sgd'])
def test_an_infinite_gradient_element(kind, kw):
    """One +Inf element: the total is +Inf and coef 0, so every other element's clipped gradient is 0 and the Inf's is NaN;
    the parameters follow the restatement (nothing is skipped on a non-finite norm)."""
    nb = _block()
    sizes = [5, nb + 1]
    rng = np.random.default_rng(31)
    grads = [rng.standard_normal(n).astype(np.float32) for n in sizes]
    grads[1][nb - 3] = np.inf
    opt, norm, coef, _ = _one_clipped_step(kind, kw, sizes, grads)
    assert np.isposinf(norm) and coef == 0
    assert float(opt.grad_norm) == float('inf') and float(opt._norm[1]) == 0.0


@pytest.mark.parametrize('kind,kw', _EDGE_RULES, ids=['adamw', 'sgd'])
def test_a_norm_that_overflows_f32_only(kind, kw):
    """Elements of 3e38: the f64 sum of squares is finite (1.8e77), its root is not an f32 -- total +Inf, coef 0."""
    sizes = [7, 300]
    grads = [np.full(n, 3e38, np.float32) for n in sizes]
    grads[1][::2] *= -1
    opt, norm, coef, _ = _one_clipped_step(kind, kw, sizes, grads)
    assert np.isposinf(norm) and coef == 0 and float(opt.grad_norm) == float('inf')


def test_a_nan_gradient_element_gives_a_nan_coefficient():
    sizes = [9]
    g = np.ones(9, np.float32)
    g[4] = np.nan
    opt, norm, coef, _ = _one_clipped_step('sgd', dict(lr=1e-2), sizes, [g])
    assert np.isnan(norm) and np.isnan(coef) and bool(torch.isnan(opt._norm).all())
    assert bool(torch.isnan(opt.param_groups[0]['params'][0]).all())


def test_the_partials_workspace_is_exact(monkeypatch):
    """The norm's f64 partials in scratch of exactly 8 * sum(ceil(n_r / block)) bytes that arrives full of 0xA5, between
    untouched guards -- with a record that has no gradient (its slots are written as zeros) and an empty tensor."""
    nb = _block()
    sizes = [3, nb, 0, nb + 1, 2 * nb + 3, 17]
    rng = np.random.default_rng(37)
    grads = [adam_ref.wide_gradients(rng, 1, n)[0] for n in sizes]
    grads[3] = None
    opt, norm, coef, guard = _one_clipped_step('adamw', dict(lr=1e-3), sizes, grads, monkeypatch)
    assert [n for _, n in guard.bufs] == [8 * optim_ref.norm_slots(sizes, nb)] == [8 * 8]
    assert 0 < coef < 1
    assert opt.launches == 3 + 1 + 2                         # norm: present, absent, present; finish; two update runs


# ---- against torch on the device ----------------------------------------------------------------------------------------
_CASES = {
    'sgd_plain': ('sgd', dict(lr=1e-3)),
    'sgd_momentum': ('sgd', dict(lr=1e-3, momentum=0.9)),
    'sgd_nesterov_wd': ('sgd', dict(lr=1e-3, momentum=0.9, nesterov=True, weight_decay=1e-4)),
    'sgd_dampening_wd': ('sgd', dict(lr=1e-3, momentum=0.9, dampening=0.1, weight_decay=1e-4)),
    'adamw_lr1e-3_wd0.01': ('adamw', dict(lr=1e-3, weight_decay=0.01)),
    'adamw_lr8e-3_wd0.05': ('adamw', dict(lr=8e-3, weight_decay=0.05)),
}


def _state_keys(kind, kw):
    return ('exp_avg', 'exp_avg_sq') if kind == 'adamw' else (('momentum_buffer',) if kw.get('momentum') else ())


def _arrays(kind, kw, opt, p):
    return [p.detach()] + [opt.state[p][k] for k in _state_keys(kind, kw)]


def _errors(run, ref):
    return [float((a.double() - b).abs().max()) for a, b in zip(run, ref)]


def _torch_opt(kind, params, kw):
    make = torch.optim.AdamW if kind == 'adamw' else torch.optim.SGD
    return make(params, foreach=False, fused=False, **kw)


def _within_twice(mine, theirs, what):
    for i, (a, b) in enumerate(zip(mine, theirs)):
        print('%s  array %d: ours %.3e  torch f32 %.3e  ratio %.3f' % (what, i, a, b, a / b if b else float('nan')))
        assert b > 0 and a <= 2 * b, (what, i, a, b)


@pytest.mark.parametrize('clip', [None, 10.0], ids=['unclipped', 'max_norm_10'])
@pytest.mark.parametrize('case', list(_CASES))
def test_as_close_to_f64_torch_on_the_device_as_torch_f32(case, clip):
    """The CPU test's criterion on the device: 30 steps, 4 099 elements, adam_ref.wide_gradients with seed 11; the largest
    error of this optimizer in p and each state array against torch.optim.{SGD,AdamW}(foreach=False) in f64 -- behind
    clip_grad_norm_(foreach=False) in the clipped runs -- is at most 2 x that of the same torch optimizer in f32."""
    kind, kw = _CASES[case]
    rng = np.random.default_rng(11)
    n, steps = 4099, 30
    p0 = rng.standard_normal(n).astype(np.float32)
    grads = adam_ref.wide_gradients(rng, steps, n)
    p64 = torch.from_numpy(p0.astype(np.float64)).to(DEV).requires_grad_(True)
    p32 = torch.from_numpy(p0.copy()).to(DEV).requires_grad_(True)
    pm = torch.from_numpy(p0.copy()).to(DEV).requires_grad_(True)
    o64, o32 = _torch_opt(kind, [p64], kw), _torch_opt(kind, [p32], kw)
    om = _make(kind, [pm], clip_grad_norm=clip, **kw)
    worst_m = worst_t = None
    for g in grads:
        gd = torch.from_numpy(g).to(DEV)
        p64.grad, p32.grad, pm.grad = gd.double(), gd.clone(), gd.clone()
        if clip is not None:
            torch.nn.utils.clip_grad_norm_([p64], clip, foreach=False)
            torch.nn.utils.clip_grad_norm_([p32], clip, foreach=False)
        o64.step(); o32.step(); om.step()
        want = _arrays(kind, kw, o64, p64)
        em, et = _errors(_arrays(kind, kw, om, pm), want), _errors(_arrays(kind, kw, o32, p32), want)
        worst_m = em if worst_m is None else [max(a, b) for a, b in zip(worst_m, em)]
        worst_t = et if worst_t is None else [max(a, b) for a, b in zip(worst_t, et)]
    _within_twice(worst_m, worst_t, '%s clip %s' % (case, clip))
    assert om.launches == steps * (1 if clip is None else 3)


# ---- state round trips ----------------------------------------------------------------------------------------------------
def _fresh(p0s, dtype=torch.float32):
    return [torch.from_numpy(p.astype(np.float64)).to(dtype).to(DEV).requires_grad_(True) for p in p0s]


def _run(opt, params, grads, dtype=torch.float32):
    for gs in grads:
        for p, g in zip(params, gs):
            p.grad = torch.from_numpy(g).to(DEV).to(dtype)
        opt.step()


@pytest.mark.parametrize('kind,kw', [('adamw', dict(lr=2e-3, weight_decay=0.05)),
                                     ('sgd', dict(lr=2e-3, momentum=0.9, nesterov=True, weight_decay=1e-4))],
                         ids=['adamw', 'sgd'])
def test_state_round_trips_between_these_optimizers_and_torchs(kind, kw):
    """ours -> state_dict -> a new instance of ours continues bit for bit; ours -> torch's optimizer of the same name and
    torch's -> ours continue within the 2 x criterion (error against an f64 torch run of all ten steps, beside an f32
    torch run)."""
    rng = np.random.default_rng(23)
    sizes = [4099, 7, 300]
    p0s = [rng.standard_normal(n).astype(np.float32) for n in sizes]
    grads = [[g] + [adam_ref.wide_gradients(rng, 1, n)[0] for n in sizes[1:]] for g in adam_ref.wide_gradients(rng, 10, sizes[0])]
    keys = _state_keys(kind, kw)
    p64 = _fresh(p0s, torch.float64)
    o64 = _torch_opt(kind, p64, kw)
    _run(o64, p64, grads, torch.float64)
    p32 = _fresh(p0s)
    o32 = _torch_opt(kind, p32, kw)
    _run(o32, p32, grads)
    pa = _fresh(p0s)
    oa = _make(kind, pa, **kw)
    _run(oa, pa, grads[:5])
    half = copy.deepcopy(oa.state_dict())
    at_half = [p.detach().clone() for p in pa]
    _run(oa, pa, grads[5:])
    # ours -> ours
    pb = [p.clone().requires_grad_(True) for p in at_half]
    ob = _make(kind, pb, lr=1.0)                             # (the loaded dict brings the hyperparameters)
    ob.load_state_dict(copy.deepcopy(half))
    assert all(ob.param_groups[0][k] == v for k, v in kw.items())
    _run(ob, pb, grads[5:])
    for a, b in zip(pa, pb):
        assert torch.equal(a, b)
        for k in keys:
            assert _same_bits(_np(oa.state[a][k]), _np(ob.state[b][k]))
    st = ob.state[pb[0]][keys[0]].untyped_storage().data_ptr()
    assert all(ob.state[p][keys[0]].untyped_storage().data_ptr() == st for p in pb)         # still views of one buffer

    def errors(opt, params):
        out = None
        for p, q in zip(params, p64):
            e = _errors(_arrays(kind, kw, opt, p), _arrays(kind, kw, o64, q))
            out = e if out is None else [max(a, b) for a, b in zip(out, e)]
        return out
    yard = errors(o32, p32)
    # ours -> torch
    pc = [p.clone().requires_grad_(True) for p in at_half]
    oc = _torch_opt(kind, pc, {})
    oc.load_state_dict(copy.deepcopy(half))
    oc.param_groups[0]['foreach'] = oc.param_groups[0]['fused'] = False
    assert all(oc.param_groups[0][k] == v for k, v in kw.items())
    _run(oc, pc, grads[5:])
    _within_twice(errors(oc, pc), yard, 'ours -> torch')
    # torch -> ours
    pd = _fresh(p0s)
    od = _torch_opt(kind, pd, kw)
    _run(od, pd, grads[:5])
    pe = [p.detach().clone().requires_grad_(True) for p in pd]
    oe = _make(kind, pe)
    oe.load_state_dict(copy.deepcopy(od.state_dict()))
    _run(oe, pe, grads[5:])
    _within_twice(errors(oe, pe), yard, 'torch -> ours')
    if kind == 'adamw':
        assert all(float(o.state[p]['step']) == 10.0 for o, ps in ((oc, pc), (oe, pe)) for p in ps)


# ---- in the training steps ------------------------------------------------------------------------------------------------
def _batch(seed):
    from lidal_amd import synth
    b = synth.make_train_batch(n_frames=1, n_points=6000, seed=seed)
    return (torch.from_numpy(b['coords_v_b']).to(DEV), torch.from_numpy(b['feats_v_b']).to(DEV),
            torch.from_numpy(b['labels_v_b']).to(DEV))


_STEP_RULES = [('sgd', dict(lr=1e-2, momentum=0.9, nesterov=True, weight_decay=1e-4)), ('adamw', dict(lr=1e-2))]


@pytest.mark.parametrize('planned', [True, False], ids=['planned_step', 'per_operator_path'])
@pytest.mark.parametrize('kind,kw', _STEP_RULES, ids=['sgd', 'adamw'])
def test_in_the_training_step_every_parameter_equals_the_restatement(kind, kw, planned):
    """SPVCNN, dropout 0, bf16 autocast, two train_step calls with clip_grad_norm=10: after each step every parameter equals
    bit for bit what the restatement makes of the previous parameters, a copy of its (unclipped) gradient and the norm of
    all of them; three launches per step (partials, finish, update), and the weight epoch moved."""
    from lidal_amd import backend as B
    from lidal_amd.network import SPVCNN, plan
    from lidal_amd.train_step import train_step
    c, f, lab = _batch(9)
    nb = _block()
    saved = plan.ENABLED
    plan.ENABLED = planned
    try:
        torch.manual_seed(1)
        model = SPVCNN(19).to(DEV).train()
        model.dropout.p = 0.0
        params = list(model.parameters())
        opt = _make(kind, params, clip_grad_norm=10, **kw)
        refs = None
        losses = []
        for t in (1, 2):
            before = [_np(p).reshape(-1).copy() for p in params]
            if refs is None:
                refs = [_Ref(kind, b) for b in before]
            epoch = B.WEIGHT_EPOCH[0]
            loss, _ = train_step(model, opt, f, c, lab, autocast=True)
            losses.append(float(loss))
            assert B.WEIGHT_EPOCH[0] > epoch
            assert all(p.grad is not None for p in params)
            if t == 1:
                one_buffer = len({p.grad.untyped_storage().data_ptr() for p in params}) == 1
                assert one_buffer == planned
            grads = [_np(p.grad).reshape(-1).copy() for p in params]
            norm = optim_ref.grad_norm(grads, nb)
            coef = optim_ref.clip_coef(norm, 10)
            assert np.isfinite(norm) and norm > 0
            assert _same_bits(_np(opt.grad_norm), norm), (t, float(opt.grad_norm), float(norm))
            for i, p in enumerate(params):
                refs[i].step(grads[i], kw, coef)
                refs[i].check(opt, p, (t, i, tuple(p.shape)))
        assert opt.launches == 2 * 3
        assert len(set(losses)) == 2 and all(np.isfinite(losses))
        if planned:
            assert opt.table_uploads == 1
    finally:
        plan.ENABLED = saved


@pytest.mark.parametrize('kind,kw', _STEP_RULES, ids=['sgd', 'adamw'])
def test_the_mean_teacher_step_takes_these_optimizers(kind, kw):
    from lidal_amd import semi
    from lidal_amd.network import SPVCNN
    c, f, lab = _batch(11)
    torch.manual_seed(2)
    student = SPVCNN(19).to(DEV).train()
    opt = _make(kind, student.parameters(), clip_grad_norm=10, **kw)
    ema = semi.EmaTeacher(student, alpha=0.9, warmup=False)
    before = [p.detach().clone() for p in student.parameters()]
    loss, logits, cons = semi.semi_train_step(student, ema, opt, f, c, lab, cons_weight=0.5, autocast=True)
    assert np.isfinite(float(loss)) and np.isfinite(float(cons)) and np.isfinite(float(opt.grad_norm))
    assert opt.launches == 3
    moved = [not torch.equal(a, b) for a, b in zip(before, student.parameters())]
    assert sum(moved) > len(moved) // 2
