"""lidal_amd.optim.Adam on the GPU: the one-launch kernel (csrc/optim.hip) bit for bit against the numpy restatement
(tests/adam_ref.py), against torch.optim.Adam on the device, its state across optimizers, inside the planned and the
per-operator training step, and the inference caches behind it."""
import copy

import numpy as np
import pytest
import torch

import adam_ref

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _chunk():
    from lidal_amd import backend as B
    return int(B.lib_handle().lidal_adam_chunk_elems())


def _np(t):
    return t.detach().cpu().numpy()


def _same_bits(a, b):
    return np.array_equal(adam_ref.bits(a).reshape(-1), adam_ref.bits(b).reshape(-1))


# ---- bit for bit against adam_ref -------------------------------------------------------------------------------------
def _sizes():
    c = _chunk()
    rng = np.random.default_rng(5)
    return [1, 3, 4, 5, 255, 256, 257, c - 1, c, c + 1, 2 * c + 3] + [int(k) for k in rng.integers(1, 8, 200)]


_MAGNITUDES = (1e-20, 1e-6, 1.0, 1e3)


def _edge_gradient(rng, n, step):
    """magnitudes 1e-20, 1e-6, 1 and 1e3 (a different one per element), one element in eight an exact zero"""
    g = rng.choice(_MAGNITUDES, n) * rng.uniform(1.0, 2.0, n) * rng.choice([-1.0, 1.0], n)
    g[rng.random(n) < 0.125] = 0.0
    return g.astype(np.float32)


def _expected_launches(groups, steps_done, has_grad):
    """Launches of one step: per group the runs of consecutive parameters that have a gradient and share their step count."""
    n = 0
    for members in groups:
        prev = None
        for i in members:
            if not has_grad[i]:
                prev = None
                continue
            if prev is None or steps_done[i] != steps_done[prev]:
                n += 1
            prev = i
    return n


@pytest.mark.parametrize('flat', [False, True], ids=['separate_gradients', 'flat_gradient_buffer'])
def test_kernel_equals_the_restatement_bit_for_bit(flat):
    """One optimizer over 212 tensors -- 1, 3, 4, 5, 255, 256, 257, chunk - 1, chunk, chunk + 1, 2 chunk + 3 elements, 200
    tensors of 1 to 7 elements (many segments in one workgroup) and one parameter that is a view starting 4 bytes into
    its storage -- in two groups (lr 1e-3 without and lr 3e-3 with weight decay 0.01), 12 steps: p, exp_avg and
    exp_avg_sq equal adam_ref bit for bit after every step.  Gradients of magnitude 1e-20 (subnormal second moments),
    1e-6, 1 and 1e3 with exact zeros, step 8 all zero, one parameter without a gradient on steps 3 to 5 (it lags three
    steps from then on), lr changed at step 6.  Once with separately allocated gradients (absolute addresses), once as
    views of ONE buffer in 16-byte slots that is a different allocation every step (the planned step's layout: the table
    is uploaded once)."""
    from lidal_amd.optim import Adam
    rng = np.random.default_rng(17)
    sizes = _sizes()
    params = [torch.nn.Parameter(torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(DEV)) for n in sizes]
    odd = torch.from_numpy(rng.standard_normal(1030).astype(np.float32)).to(DEV)
    params.insert(9, torch.nn.Parameter(odd[1:]))            # 1 029 elements from byte 4 of their storage
    assert params[9].data_ptr() % 16 == 4 and params[9].is_contiguous()
    odd_first = float(odd[0])
    sizes = [p.numel() for p in params]
    n_par = len(params)
    members = [list(range(0, n_par, 2)), list(range(1, n_par, 2))]        # both groups get every kind of tensor
    hyper = [dict(lr=1e-3, weight_decay=0.0), dict(lr=3e-3, weight_decay=0.01)]
    opt = Adam([dict(params=[params[i] for i in mem], **h) for mem, h in zip(members, hyper)])
    group_of = {i: gi for gi, mem in enumerate(members) for i in mem}
    lagging = 6                                              # the 257-element tensor
    assert sizes[lagging] == 257
    slots, total = [], 0
    for n in sizes:
        slots.append(total)
        total += (n + 3) & -4
    ref = [[_np(p).copy(), np.zeros(n, np.float32), np.zeros(n, np.float32), 0] for p, n in zip(params, sizes)]
    kept, launches = [], 0
    for step in range(1, 13):
        if step == 6:
            opt.param_groups[0]['lr'] = 4e-4
            hyper[0]['lr'] = 4e-4
        host = np.zeros(total + 16, np.float32)
        for i, n in enumerate(sizes):
            if step != 8:
                host[slots[i]:slots[i] + n] = _edge_gradient(rng, n, step)
        buf = torch.from_numpy(host).to(DEV)
        kept.append(buf)                                     # (alive: the next step's buffer is another allocation)
        has_grad = [not (i == lagging and 3 <= step <= 5) for i in range(n_par)]
        for i, p in enumerate(params):
            view = buf[slots[i]:slots[i] + sizes[i]]
            p.grad = None if not has_grad[i] else (view if flat else view.clone())
        launches += _expected_launches(members, [r[3] for r in ref], has_grad)
        opt.step()
        for i, p in enumerate(params):
            if has_grad[i]:
                r = ref[i]
                r[3] += 1
                r[0], r[1], r[2] = adam_ref.adam_step(r[0], host[slots[i]:slots[i] + sizes[i]], r[1], r[2], r[3],
                                                      **hyper[group_of[i]])
        for i, p in enumerate(params):
            r = ref[i]
            assert _same_bits(_np(p), r[0]), ('p', step, i, sizes[i])
            if p in opt.state:
                st = opt.state[p]
                assert float(st['step']) == r[3]
                assert _same_bits(_np(st['exp_avg']), r[1]), ('exp_avg', step, i, sizes[i])
                assert _same_bits(_np(st['exp_avg_sq']), r[2]), ('exp_avg_sq', step, i, sizes[i])
            else:
                assert r[3] == 0
    assert float(odd[0]) == odd_first                        # the float in front of the view
    assert ref[lagging][3] == 9 and ref[0][3] == 12
    assert opt.launches == launches
    assert launches == 2 * 2 + 3 * 3 + 7 * 4                 # a launch per group; 2 runs around the missing gradient; 3 once it lags
    if flat:
        assert opt.table_uploads == 1
    else:
        assert opt.table_uploads >= 1


def test_subnormal_second_moments_and_neighbours_survive():
    """|g| = 1e-20 leaves a SUBNORMAL exp_avg_sq (not flushed).  Parameter AND gradient start 4 bytes into their storages
    (whole 16-byte vectors with three elements in front and two behind): the floats around the parameter are not touched."""
    from lidal_amd.optim import Adam
    base = torch.full((4 + 1031,), 7.0, device=DEV)
    p = torch.nn.Parameter(base[1:1 + 1029])
    opt = Adam([p])
    g = np.full(1029, 1e-20, np.float32)
    p.grad = torch.cat([torch.zeros(1), torch.from_numpy(g)]).to(DEV)[1:]
    assert p.data_ptr() % 16 == 4 and p.grad.data_ptr() % 16 == 4
    before = _np(p).copy()
    opt.step()
    want = adam_ref.adam_step(before, g, np.zeros(1029, np.float32), np.zeros(1029, np.float32), 1)
    v = _np(opt.state[p]['exp_avg_sq'])
    assert (v > 0).all() and (v < np.finfo(np.float32).tiny).all()
    assert _same_bits(v, want[2]) and _same_bits(_np(p), want[0]) and _same_bits(_np(opt.state[p]['exp_avg']), want[1])
    assert float(base[0]) == 7.0 and (base[1030:] == 7.0).all()


# ---- against torch on the device ----------------------------------------------------------------------------------------
def _errors(run, ref):
    return [float((a.double() - b).abs().max()) for a, b in zip(run, ref)]


def _triple(opt, p):
    return p.detach(), opt.state[p]['exp_avg'], opt.state[p]['exp_avg_sq']


def _within_twice(mine, theirs, what):
    for name, a, b in zip('pmv', mine, theirs):
        print('%s  %s: ours %.3e  torch f32 %.3e  ratio %.3f' % (what, name, a, b, a / b if b else float('nan')))
        assert b > 0 and a <= 2 * b, (what, name, a, b)


@pytest.mark.parametrize('weight_decay', [0.0, 0.01])
def test_as_close_to_f64_adam_on_the_device_as_torch_f32(weight_decay):
    """The CPU test's criterion on the device: 30 steps, 4 099 elements, gradient magnitudes 1e-6 .. 1e3; the largest error
    of this optimizer in p, m and v against torch.optim.Adam(foreach=False, fused=False) in f64 is at most 2 x that of the
    same torch optimizer in f32."""
    from lidal_amd.optim import Adam
    rng = np.random.default_rng(11)
    n, steps = 4099, 30
    p0 = rng.standard_normal(n).astype(np.float32)
    grads = adam_ref.wide_gradients(rng, steps, n)
    p64 = torch.from_numpy(p0.astype(np.float64)).to(DEV).requires_grad_(True)
    p32 = torch.from_numpy(p0.copy()).to(DEV).requires_grad_(True)
    pm = torch.from_numpy(p0.copy()).to(DEV).requires_grad_(True)
    o64 = torch.optim.Adam([p64], weight_decay=weight_decay, foreach=False, fused=False)
    o32 = torch.optim.Adam([p32], weight_decay=weight_decay, foreach=False, fused=False)
    om = Adam([pm], weight_decay=weight_decay)
    worst_m, worst_t = [0.0] * 3, [0.0] * 3
    for g in grads:
        gd = torch.from_numpy(g).to(DEV)
        p64.grad, p32.grad, pm.grad = gd.double(), gd.clone(), gd.clone()
        o64.step(); o32.step(); om.step()
        want = _triple(o64, p64)
        worst_m = [max(a, b) for a, b in zip(worst_m, _errors(_triple(om, pm), want))]
        worst_t = [max(a, b) for a, b in zip(worst_t, _errors(_triple(o32, p32), want))]
    _within_twice(worst_m, worst_t, 'weight_decay %g' % weight_decay)
    assert om.launches == steps


# ---- state round trips ----------------------------------------------------------------------------------------------------
def _fresh(p0s, dtype=torch.float32):
    return [torch.from_numpy(p.astype(np.float64)).to(dtype).to(DEV).requires_grad_(True) for p in p0s]


def _run(opt, params, grads, dtype=torch.float32):
    for gs in grads:
        for p, g in zip(params, gs):
            p.grad = torch.from_numpy(g).to(DEV).to(dtype)
        opt.step()


def test_state_round_trips_between_this_optimizer_and_torchs():
    """ours -> state_dict -> a new instance of ours continues bit for bit; ours -> torch.optim.Adam and torch -> ours
    continue within the 2 x criterion (error against an f64 torch run of all ten steps, beside an f32 torch run)."""
    from lidal_amd.optim import Adam
    rng = np.random.default_rng(23)
    sizes = [4099, 7, 300]
    p0s = [rng.standard_normal(n).astype(np.float32) for n in sizes]
    grads = [[g] + [adam_ref.wide_gradients(rng, 1, n)[0] for n in sizes[1:]] for g in adam_ref.wide_gradients(rng, 10, sizes[0])]
    kw = dict(lr=2e-3, weight_decay=0.01)
    tkw = dict(foreach=False, fused=False, **kw)
    # the yardsticks: torch in f64 and in f32, all ten steps
    p64 = _fresh(p0s, torch.float64)
    o64 = torch.optim.Adam(p64, **tkw)
    _run(o64, p64, grads, torch.float64)
    p32 = _fresh(p0s)
    o32 = torch.optim.Adam(p32, **tkw)
    _run(o32, p32, grads)
    # ours, all ten steps
    pa = _fresh(p0s)
    oa = Adam(pa, **kw)
    _run(oa, pa, grads[:5])
    half = copy.deepcopy(oa.state_dict())
    at_half = [p.detach().clone() for p in pa]
    _run(oa, pa, grads[5:])
    # ours -> ours
    pb = [p.clone().requires_grad_(True) for p in at_half]
    ob = Adam(pb, lr=1.0)                                   # (the loaded dict brings the hyperparameters)
    ob.load_state_dict(copy.deepcopy(half))
    assert ob.param_groups[0]['lr'] == 2e-3 and ob.param_groups[0]['weight_decay'] == 0.01
    _run(ob, pb, grads[5:])
    for a, b in zip(pa, pb):
        assert torch.equal(a, b)
        for k in ('exp_avg', 'exp_avg_sq'):
            assert _same_bits(_np(oa.state[a][k]), _np(ob.state[b][k]))
        assert float(oa.state[a]['step']) == float(ob.state[b]['step']) == 10.0
    st = ob.state[pb[0]]['exp_avg'].untyped_storage().data_ptr()
    assert all(ob.state[p]['exp_avg'].untyped_storage().data_ptr() == st for p in pb)       # still views of one buffer

    def errors(opt, params):
        out = [0.0] * 3
        for p, q in zip(params, p64):
            out = [max(a, b) for a, b in zip(out, _errors(_triple(opt, p), _triple(o64, q)))]
        return out
    yard = errors(o32, p32)
    # ours -> torch
    pc = [p.clone().requires_grad_(True) for p in at_half]
    oc = torch.optim.Adam(pc, foreach=False, fused=False)
    oc.load_state_dict(copy.deepcopy(half))
    oc.param_groups[0]['foreach'] = oc.param_groups[0]['fused'] = False
    _run(oc, pc, grads[5:])
    assert all(float(oc.state[p]['step']) == 10.0 for p in pc)
    _within_twice(errors(oc, pc), yard, 'ours -> torch')
    # torch -> ours
    pd = _fresh(p0s)
    od = torch.optim.Adam(pd, **tkw)
    _run(od, pd, grads[:5])
    pe = [p.detach().clone().requires_grad_(True) for p in pd]
    oe = Adam(pe)
    oe.load_state_dict(copy.deepcopy(od.state_dict()))
    _run(oe, pe, grads[5:])
    assert all(float(oe.state[p]['step']) == 10.0 for p in pe)
    _within_twice(errors(oe, pe), yard, 'torch -> ours')


# ---- in the training step -------------------------------------------------------------------------------------------------
def _batch(seed):
    from lidal_amd import synth
    b = synth.make_train_batch(n_frames=1, n_points=6000, seed=seed)
    return (torch.from_numpy(b['coords_v_b']).to(DEV), torch.from_numpy(b['feats_v_b']).to(DEV),
            torch.from_numpy(b['labels_v_b']).to(DEV))


@pytest.mark.parametrize('planned', [True, False], ids=['planned_step', 'per_operator_path'])
def test_in_the_training_step_every_parameter_equals_the_restatement(planned):
    """SPVCNN, dropout 0, bf16 autocast, three train_step calls with lidal_amd.optim.Adam: after each step every parameter
    equals bit for bit what adam_ref makes of the previous parameters and a copy of its gradient.  Planned step: the
    gradients are views of one flat buffer, the table is uploaded once and every step is one launch; LIDAL_PLAN=0 (the
    per-operator path): separately allocated gradients, the absolute form."""
    from lidal_amd.network import SPVCNN, plan
    from lidal_amd.optim import Adam
    from lidal_amd.train_step import train_step
    c, f, lab = _batch(9)
    saved = plan.ENABLED
    plan.ENABLED = planned
    try:
        torch.manual_seed(1)
        model = SPVCNN(19).to(DEV).train()
        model.dropout.p = 0.0
        params = list(model.parameters())
        opt = Adam(params, lr=1e-2)
        m = [np.zeros(p.numel(), np.float32) for p in params]
        v = [np.zeros(p.numel(), np.float32) for p in params]
        losses = []
        for t in (1, 2, 3):
            before = [_np(p).reshape(-1).copy() for p in params]
            loss, _ = train_step(model, opt, f, c, lab, autocast=True)
            losses.append(float(loss))
            assert all(p.grad is not None for p in params)
            if t == 1:
                one_buffer = len({p.grad.untyped_storage().data_ptr() for p in params}) == 1
                assert one_buffer == planned
            for i, p in enumerate(params):
                g = _np(p.grad).reshape(-1).copy()
                want, m[i], v[i] = adam_ref.adam_step(before[i], g, m[i], v[i], t, lr=1e-2)
                assert _same_bits(_np(p).reshape(-1), want), (t, i, tuple(p.shape))
                if t == 3:
                    assert _same_bits(_np(opt.state[p]['exp_avg']).reshape(-1), m[i])
                    assert _same_bits(_np(opt.state[p]['exp_avg_sq']).reshape(-1), v[i])
        assert opt.launches == 3
        assert len(set(losses)) == 3 and all(np.isfinite(losses))
        if planned:
            assert opt.table_uploads == 1
        else:
            assert 1 <= opt.table_uploads <= 3
    finally:
        plan.ENABLED = saved


def test_inference_caches_follow_training_with_this_optimizer():
    """tests/test_model_gpu.py::test_inference_caches_follow_training with lidal_amd.optim.Adam, which writes the parameters
    through raw pointers (no version counter moves) and tells the caches itself: evaluate -> train -> evaluate gives
    bitwise what a fresh model loaded with the same state_dict gives, and not what it gave before."""
    import lidal_amd
    from lidal_amd.network import SPVCNN
    from lidal_amd.optim import Adam
    from lidal_amd.train_step import train_step
    c, f, lab = _batch(9)
    torch.manual_seed(1)
    model = SPVCNN(19).to(DEV)
    opt = Adam(model.parameters(), lr=1e-2)

    def evaluate(m):
        m.eval()
        with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16):
            out = m(lidal_amd.SparseTensor(f, c))[0].float().clone()
        m.train()
        return out
    model.train()
    for _ in range(2):
        train_step(model, opt, f, c, lab, autocast=True)
    first = evaluate(model)                       # fills the inference caches
    for _ in range(2):
        train_step(model, opt, f, c, lab, autocast=True)
    second = evaluate(model)
    fresh = SPVCNN(19).to(DEV)
    fresh.load_state_dict(model.state_dict())
    want = evaluate(fresh)
    assert torch.equal(second, want)
    assert not torch.equal(first, second)


def test_a_step_moves_the_weight_epoch():
    from lidal_amd import backend as B
    from lidal_amd.optim import Adam
    p = torch.nn.Parameter(torch.ones(10, device=DEV))
    opt = Adam([p])
    p.grad = torch.ones(10, device=DEV)
    version, epoch, hits = p._version, B.WEIGHT_EPOCH[0], B.HITS.get('adam_step', 0)
    opt.step()
    assert B.WEIGHT_EPOCH[0] == epoch + 1 and B.HITS.get('adam_step', 0) == hits + 1
    assert p._version == version and not torch.equal(p.detach(), torch.ones(10, device=DEV))


# ---- what it refuses, with device tensors ---------------------------------------------------------------------------------
def test_refusals_on_the_device():
    from lidal_amd.optim import Adam
    with pytest.raises(ValueError, match='float32'):
        Adam([torch.nn.Parameter(torch.zeros(8, device=DEV, dtype=torch.bfloat16))])
    with pytest.raises(ValueError, match='contiguous'):
        Adam([torch.nn.Parameter(torch.zeros(4, 6, device=DEV).t())])
    p = torch.nn.Parameter(torch.ones(8, device=DEV))
    opt = Adam([p])
    p.grad = torch.ones(8, device=DEV)
    p.grad.data = torch.ones(8, device=DEV, dtype=torch.float16)
    with pytest.raises(ValueError, match='float32'):
        opt.step()
    assert opt.launches == 0 and torch.equal(p.detach(), torch.ones(8, device=DEV))
    # a dense gradient that is not contiguous is made contiguous
    q = torch.nn.Parameter(torch.ones(4, 6, device=DEV))
    opt = Adam([q])
    g = torch.arange(24, device=DEV, dtype=torch.float32).reshape(6, 4).t()
    assert not g.is_contiguous()
    q.grad = g
    opt.step()
    want = adam_ref.adam_step(np.ones(24, np.float32), _np(g.contiguous()).reshape(-1), np.zeros(24, np.float32),
                              np.zeros(24, np.float32), 1)
    assert _same_bits(_np(q).reshape(-1), want[0])
