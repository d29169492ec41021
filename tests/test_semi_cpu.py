"""lidal_amd.semi without a GPU: the numpy restatement tests/semi_ref.py against torch on the CPU -- the EMA bit for bit
against the op sequence, the f64 forms of the pseudo labels and of the consistency term with its gradient against
torch's own formulation in f64 -- the warm-up schedule, and every refusal the module makes before it touches a device."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import semi_ref as R
from lidal_amd import semi


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _edge_values(rng, n):
    v = (rng.normal(size=n) * 10.0 ** rng.integers(-3, 3, n)).astype(np.float32)
    tiny = np.finfo(np.float32).tiny
    special = np.array([0.0, -0.0, tiny / 4, -tiny / 8, tiny, np.inf, -np.inf, np.nan, 1e-45, 3.4e38], np.float32)
    idx = rng.choice(n, min(n, len(special)), replace=False)
    v[idx] = special[:len(idx)]
    return v


@pytest.mark.parametrize('alpha', [0.0, 0.5, 0.99, 0.999, 1.0])
def test_ema_restatement_equals_the_torch_op_sequence_bit_for_bit(alpha):
    rng = np.random.default_rng(1)
    t, s = _edge_values(rng, 4099), _edge_values(rng, 4099)
    tiny = np.finfo(np.float32).tiny
    t[:32] = tiny / 4 * np.arange(1, 33, dtype=np.float32) / 32        # both sides subnormal: so is the result
    s[:32] = tiny / 8 * np.arange(32, 0, -1, dtype=np.float32) / 32
    want = R.ema_update(t, s, alpha if alpha else 1e-300)              # (alpha = 0 is the copy: below)
    tt, ss = torch.from_numpy(t.copy()), torch.from_numpy(s.copy())
    oma = torch.tensor(1.0 - (alpha if alpha else 1e-300), dtype=torch.float64).to(torch.float32)
    got = (tt + (ss - tt) * oma).numpy()
    nan = np.isnan(want)
    assert np.array_equal(nan, np.isnan(got))
    assert np.array_equal(_bits(got)[~nan], _bits(want)[~nan])
    sub = (np.abs(want) > 0) & (np.abs(want) < np.finfo(np.float32).tiny)
    assert sub[:32].all()                                              # subnormals are kept, not flushed


def test_alpha_zero_is_a_copy_where_the_arithmetic_is_not():
    t = np.array([1e8, 1.0, np.inf, 3.0], np.float32)
    s = np.array([1.0, 1e-8, 1.0, np.nan], np.float32)
    got = R.ema_update(t, s, 0.0)
    assert np.array_equal(_bits(got), _bits(s))
    with np.errstate(all='ignore'):
        arith = t + (s - t) * np.float32(1.0)
    assert not np.array_equal(_bits(arith), _bits(s))                  # t + (s - t) is not s in floating point
    ints = np.array([0x7FC00000_7F800001, -1, 2 ** 62], np.int64)
    assert np.array_equal(R.ema_update(np.zeros(3, np.int64), ints, 0.5), ints)


def test_warm_up_schedule_matches_its_formula():
    for alpha in (0.0, 0.5, 0.999, 1.0):
        for k in (0, 1, 2, 9, 998, 999, 1000, 10 ** 6):
            want = min(alpha, 1.0 - 1.0 / (k + 1))
            assert semi.ema_alpha(alpha, k, True) == want == R.ema_alpha(alpha, k, True)
            assert semi.ema_alpha(alpha, k, False) == alpha
    assert semi.ema_alpha(0.999, 0) == 0.0                             # the first update copies
    assert semi.ema_alpha(0.999, 1) == 0.5
    m = torch.nn.Linear(3, 2)
    t = semi.EmaTeacher(m, alpha=0.9)
    assert [t.alpha_eff()] == [0.0] and not t.model.training
    assert all(not p.requires_grad for p in t.model.parameters())
    t.updates = 4
    assert t.alpha_eff() == 0.8
    t.updates = 100
    assert t.alpha_eff() == 0.9
    sd = t.state_dict()
    assert sd['updates'] == 100 and sd['alpha'] == 0.9 and set(sd['model']) == set(m.state_dict())
    u = semi.EmaTeacher(m, alpha=0.5)
    u.load_state_dict(sd)
    assert u.updates == 100 and u.alpha == 0.9


def _finite_logits(n, c, seed):
    rng = np.random.default_rng(seed)
    return np.clip(rng.normal(size=(n, c)) * rng.choice([1.0, 3.0, 30.0], size=(n, 1)), -80, 80)


@pytest.mark.parametrize('c', [1, 16, 19, 32])
def test_pseudo_labels_f64_against_torch(c):
    n, p = 300, 700
    rng = np.random.default_rng(c)
    x = _finite_logits(n, c, c)
    if c > 1:
        x[5, 1] = x[5, 0] = x[5].max() + 1.0                           # a tie: the first wins
    inverse = rng.integers(-1, n + 1, p)
    human = np.where(rng.random(p) < 0.2, rng.integers(0, c, p), 255)
    thr = rng.uniform(0.3, 0.99, c).astype(np.float32)
    out, stats, conf = R.pseudo_labels(x, thr, inverse, human, 255, np.float64)
    xt = torch.from_numpy(x)
    prob = torch.softmax(xt, 1)
    tconf, targ = prob.max(1)
    if c > 1:
        assert int(targ[5]) == 0
    inv = torch.from_numpy(inverse)
    inside = (inv >= 0) & (inv < n)
    safe = torch.where(inside, inv, torch.zeros_like(inv))
    ok = inside & (tconf[safe] >= torch.from_numpy(thr).double()[targ[safe]])
    want = torch.where(ok, targ[safe], torch.full_like(inv, 255))
    h = torch.from_numpy(human)
    want = torch.where(h != 255, h, want)
    near = (np.abs(conf - thr.astype(np.float64)[np.where(inside.numpy(), targ[safe].numpy(), 0)]) < 1e-12) & inside.numpy()
    assert not near.any()
    assert np.array_equal(out, want.numpy())
    assert np.abs(conf[inside.numpy()] - tconf[safe].numpy()[inside.numpy()]).max() < 1e-12
    free = (h == 255).numpy()
    assert stats[c + 1] == (~inside.numpy() & free).sum()
    assert stats[:c].sum() == (ok.numpy() & free).sum() and stats[c] == (inside.numpy() & ~ok.numpy() & free).sum()
    assert stats.sum() == free.sum()


def _torch_terms(zs, zt, kind):
    if kind == 'mse':
        return ((torch.softmax(zs, 1) - torch.softmax(zt, 1)) ** 2).sum(1)
    return F.kl_div(torch.log_softmax(zs, 1), torch.softmax(zt, 1), reduction='none').sum(1)


@pytest.mark.parametrize('kind', ['mse', 'kl'])
@pytest.mark.parametrize('c', [1, 16, 19, 32])
@pytest.mark.parametrize('masked', [False, True])
def test_consistency_f64_against_autograd(kind, c, masked):
    n = 257
    a, b = _finite_logits(n, c, 10 + c), _finite_logits(n, c, 20 + c)
    zs = torch.from_numpy(a).requires_grad_(True)
    zt = torch.from_numpy(b)
    conf = torch.softmax(zt, 1).max(1).values
    min_conf = 0.0
    if masked and c > 1:
        min_conf, gap = R.gap_threshold(conf.numpy())
        assert gap > 2e-5
    mask = conf >= float(np.float32(min_conf))
    denom = n * c if kind == 'mse' else n
    loss = (_torch_terms(zs, zt, kind) * mask).sum() / denom
    if not masked:
        whole = (F.mse_loss(torch.softmax(zs, 1), torch.softmax(zt, 1)) if kind == 'mse'
                 else F.kl_div(torch.log_softmax(zs, 1), torch.softmax(zt, 1), reduction='batchmean'))
        assert abs(float(whole.detach()) - float(loss.detach())) <= 1e-12 * max(abs(float(whole.detach())), 1e-300)
    (3.0 * loss).backward()
    got, r, m = R.consistency(a, b, kind, min_conf, False, np.float64)
    assert np.array_equal(m, mask.numpy())
    if masked and c > 1:
        assert 0 < m.sum() < n
    assert abs(got - float(loss.detach())) <= 1e-12 * abs(float(loss.detach()))
    dz = R.consistency_grad(a, b, 3.0, kind, min_conf, False, np.float64)
    ref = zs.grad.numpy()
    assert np.abs(dz - ref).max() <= 1e-12 * np.abs(ref).max()
    assert not dz[~m].any()


def test_probabilities_take_the_gradient_with_respect_to_them():
    n, c = 63, 19
    ps = torch.softmax(torch.from_numpy(_finite_logits(n, c, 1)), 1).requires_grad_(True)
    pt = torch.softmax(torch.from_numpy(_finite_logits(n, c, 2)), 1)
    loss = F.mse_loss(ps, pt)
    loss.backward()
    got, _, _ = R.consistency(ps.detach().numpy(), pt.numpy(), 'mse', 0.0, True, np.float64)
    assert abs(got - float(loss.detach())) <= 1e-12 * float(loss.detach())
    dz = R.consistency_grad(ps.detach().numpy(), pt.numpy(), 1.0, 'mse', 0.0, True, np.float64)
    assert np.abs(dz - ps.grad.numpy()).max() <= 1e-12 * np.abs(ps.grad.numpy()).max()


def test_np_sum_rows_is_numpys_order():
    rng = np.random.default_rng(0)
    for c in (1, 7, 8, 9, 16, 19, 31, 32):
        a = (rng.normal(size=(50, c)) * 10.0 ** rng.integers(-4, 4, (50, c))).astype(np.float32)
        want = np.array([np.add.reduce(np.ascontiguousarray(row)) for row in a], np.float32)
        assert np.array_equal(_bits(R.np_sum_rows(a)), _bits(want))


# ---- refusals: ValueError before anything touches a device ----------------------------------------------------------
class _Net(torch.nn.Module):
    def __init__(self, width=4, extra=False, dtype=torch.float32):
        super().__init__()
        self.lin = torch.nn.Linear(3, width).to(dtype)
        self.bn = torch.nn.BatchNorm1d(width)
        if extra:
            self.more = torch.nn.Linear(2, 2)


def test_ema_teacher_refusals_name_the_first_offender():
    E = semi.EmaTeacher
    with pytest.raises(ValueError, match='alpha'):
        E(_Net(), alpha=1.5)
    with pytest.raises(ValueError, match='buffers'):
        E(_Net(), buffers='mean')
    with pytest.raises(ValueError, match="'more.weight'.*missing in the teacher"):
        E(_Net(extra=True), model=_Net())
    with pytest.raises(ValueError, match="'more.weight'.*missing in the student"):
        E(_Net(), model=_Net(extra=True))
    with pytest.raises(ValueError, match="'lin.weight' has shape"):
        E(_Net(4), model=_Net(5))
    with pytest.raises(ValueError, match="'lin.weight' must be float32"):
        E(_Net(dtype=torch.float64), model=_Net(dtype=torch.float64))
    with pytest.raises(ValueError, match="'lin.weight' is torch.float32 in the teacher"):
        E(_Net(dtype=torch.float64), model=_Net())
    odd = _Net()
    odd.lin.weight = torch.nn.Parameter(torch.zeros(3, 4).t())
    with pytest.raises(ValueError, match="student's parameter 'lin.weight' is not contiguous"):
        E(odd, model=_Net())
    with pytest.raises(ValueError, match="teacher's parameter 'lin.weight' is not contiguous"):
        E(_Net(), model=odd)
    with pytest.raises(ValueError, match='more than one device'):
        E(_Net(), model=_Net().to('meta'))
    half = _Net()
    half.register_buffer('flags', torch.zeros(4, dtype=torch.uint8))
    other = _Net()
    other.register_buffer('flags', torch.zeros(4, dtype=torch.uint8))
    with pytest.raises(ValueError, match="'flags' has 1-byte elements"):
        E(half, model=other)
    wide = _Net()
    wide.bn.running_mean = wide.bn.running_mean.double()
    wide2 = _Net()
    wide2.bn.running_mean = wide2.bn.running_mean.double()
    E(wide, model=wide2)                                                # copied: any whole-word dtype
    with pytest.raises(ValueError, match="'bn.running_mean' must be float32 to be averaged"):
        E(wide, model=wide2, buffers='ema')
    same = _Net()
    with pytest.raises(ValueError, match='same memory'):
        E(same, model=same)
    with pytest.raises(RuntimeError, match='GPU only'):                # no CPU fallback
        E(_Net()).update()


def test_a_deep_copy_shares_no_cache_with_the_student():
    net = _Net()
    net.__dict__['_lidal_program'] = object()                          # (what cannot be deep-copied meaningfully)
    net.lin.__dict__['_lidal_trace'] = {'maps': [net.lin.weight], 'transposed': False}
    net.lin.weight._lidal_images = {'x': 1}
    t = semi.EmaTeacher(net)
    assert '_lidal_program' in net.__dict__ and '_lidal_trace' in net.lin.__dict__      # the student keeps its own
    for m in t.model.modules():
        assert not [k for k in m.__dict__ if k.startswith('_lidal_')]
    for x in list(t.model.parameters()) + list(t.model.buffers()):
        assert not [k for k in getattr(x, '__dict__', {}) if k.startswith('_lidal_')]
    mine = {x.data_ptr() for x in list(net.parameters()) + list(net.buffers())}
    assert not mine & {x.data_ptr() for x in list(t.model.parameters()) + list(t.model.buffers())}
    assert all(torch.equal(a, b) for a, b in zip(net.state_dict().values(), t.model.state_dict().values()))


def test_pseudo_label_refusals():
    f = semi.pseudo_labels
    x = torch.zeros(5, 4)
    i64 = torch.zeros(5, dtype=torch.int64)
    bad = [lambda: f(torch.zeros(5), 0.5), lambda: f(torch.zeros(5, 33), 0.5), lambda: f(torch.zeros(5, 0), 0.5),
           lambda: f(x.half(), 0.5), lambda: f(x.double(), 0.5), lambda: f(x, 0.5, inverse=i64.int()),
           lambda: f(x, 0.5, inverse=i64.reshape(5, 1)), lambda: f(x, 0.5, labels=i64[:4]),
           lambda: f(x, 0.5, inverse=torch.zeros(7, dtype=torch.int64), labels=i64),
           lambda: f(x, 0.5, labels=i64.float()), lambda: f(x, torch.zeros(5)), lambda: f(x, torch.zeros(4).double()),
           lambda: f(x, 'high'), lambda: f(x, 0.5, ignore_index=2 ** 63)]
    for call in bad:
        with pytest.raises(ValueError):
            call()
    with pytest.raises(RuntimeError, match='GPU only'):
        f(x, 0.5, inverse=i64, labels=i64)


def test_consistency_refusals():
    f = semi.consistency_loss
    x = torch.zeros(5, 4)
    bad = [lambda: f(x, x, kind='l1'), lambda: f(x, x, kind='kl', probs=True), lambda: f(x, torch.zeros(5, 3)),
           lambda: f(x, torch.zeros(4, 4)), lambda: f(torch.zeros(5, 33), torch.zeros(5, 33)),
           lambda: f(torch.zeros(5, 0), torch.zeros(5, 0)), lambda: f(x.half(), x), lambda: f(x, x.double()),
           lambda: f(x.bfloat16(), x, probs=True), lambda: f(x, x.bfloat16(), probs=True),
           lambda: f(torch.zeros(20), torch.zeros(20)), lambda: f(x, x, min_conf=float('nan')),
           lambda: f(x, x, min_conf='most'),
           lambda: f(torch.empty(2 ** 25, 32, device='meta'), torch.empty(2 ** 25, 32, device='meta'))]
    for call in bad:
        with pytest.raises(ValueError):
            call()
    with pytest.raises(RuntimeError, match='GPU only'):
        f(x, x)
    with pytest.raises(ValueError):
        semi.semi_train_step(torch.nn.Linear(2, 2), object(), None, None, None, None)
