"""lidal_amd/csrc/loss.hip on the GPU against the restatements of tests/loss_ref.py: Lovasz-softmax on probabilities
(bit for bit where the definition is integer or one f32 operation, 1e-9 on the f64 sums) and on logits (bars measured
in the test: 4 x what the f32 torch formulation on the CPU deviates from the all-f64 value on the same inputs), the
cross-entropy with class weights against torch's own in f64, determinism, exact workspace, and a training run."""
import numpy as np
import pytest
import torch

import loss_ref as R
from guarded_ws import Guarded

pytestmark = pytest.mark.gpu
DEV = 'cuda'

NS = [1, 2, 63, 64, 65, 255, 256, 257, 1025, 4099]
CS = [1, 2, 16, 19, 32]


def _F():
    from lidal_amd.nn import functional as F
    return F


def _case(n, c, seed, frac_ignored=0.1, ignore_index=255, scale=2.0):
    rng = np.random.RandomState(seed)
    z = (rng.randn(n, c) * scale).astype(np.float32)
    labels = rng.randint(0, c, n).astype(np.int64)
    labels[rng.rand(n) < frac_ignored] = ignore_index
    return z, R.softmax(z, np.float32), labels


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _check_flat(p, labels, ignore_index=255, classes='present'):
    """Everything lovasz_forward returns on probabilities against the f32 restatement."""
    ref = R.lovasz_flat(p, labels, ignore_index, classes)
    out = _F().lovasz_forward(_dev(p), _dev(labels), ignore_index, classes, probs=True, want_ranks=True)
    c = p.shape[1]
    stats = out.stats.cpu().numpy()
    assert np.array_equal(out.grad.cpu().numpy(), ref['grad'])
    assert np.array_equal(out.ranks.cpu().numpy(), ref['ranks'])
    assert int(stats[1]) == ref['present'] and int(stats[2]) == 0 and int(stats[3]) == ref['n_valid']
    assert np.array_equal(stats[4 + c:4 + 2 * c], ref['gts'].astype(np.float64))          # hence the class mask
    # f64 sums of <= 2^17 terms: n * 2^-53 = 1.5e-11; the rest of 1e-9 is margin for another association
    np.testing.assert_allclose(stats[4:4 + c], ref['per_class'], rtol=1e-9, atol=0)
    assert abs(stats[0] - ref['loss']) <= 1e-9 * abs(ref['loss'])
    return ref, out


@pytest.mark.parametrize('c', CS)
def test_flat_form_equals_the_restatement(c):
    for n in NS:
        _, p, labels = _case(n, c, 100 * c + n)
        _check_flat(p, labels, 255, 'present' if n % 2 else 'all')


def test_flat_form_edges():
    _, p, labels = _case(300, 5, 1)
    ref, _ = _check_flat(p, np.full(300, 255, np.int64))                # every row ignored
    assert ref['loss'] == 0.0 and ref['present'] == 0
    _check_flat(p, np.full(300, 255, np.int64), classes='all')
    one = np.full(300, 255, np.int64)
    one[257] = 2
    _check_flat(p, one)                                                  # one valid row
    _check_flat(p, one, classes='all')
    absent = labels.copy()
    absent[absent == 3] = 1                                              # a class absent: present against all
    a, _ = _check_flat(p, absent, classes='present')
    b, _ = _check_flat(p, absent, classes='all')
    assert a['present'] == b['present'] == 4 and a['loss'] != b['loss']
    _check_flat(p, np.full(300, 4, np.int64))                            # all rows of one class
    _check_flat(p, np.full(300, 4, np.int64), classes='all')
    for ign in (-100, 0, 77):                                            # ignore_index other than 255 (0: a class index)
        lab = labels.copy()
        lab[lab == 255] = ign
        _check_flat(p, lab, ignore_index=ign)


def test_flat_form_zero_errors_have_zero_gradient():
    """Probabilities of exactly 0 and 1: e == 0 where they agree with the label (gradient 0, torch's abs at 0),
    e == 1 where they contradict it."""
    rng = np.random.RandomState(5)
    n, c = 700, 4
    hard = rng.randint(0, c, n)
    p = np.zeros((n, c), np.float32)
    p[np.arange(n), hard] = 1.0
    p[::3] = R.softmax(rng.randn(len(p[::3]), c).astype(np.float32), np.float32)
    labels = np.where(rng.rand(n) < 0.5, hard, rng.randint(0, c, n)).astype(np.int64)
    ref, out = _check_flat(p, labels)
    agree = (p == (labels[:, None] == np.arange(c)[None, :]))
    assert agree.any() and not out.grad.cpu().numpy()[agree].any()


@pytest.mark.parametrize('c', [2, 19])
def test_flat_form_ties_across_workgroups_and_sort_tiles(c):
    """Blocks of 700 duplicated rows (labels differ inside a block): the ties span the 256-row workgroups, the
    2048-rank tiles and, with 4099 * c entries, the sort's 8192-entry tiles; the stable sort has to keep them in
    row order."""
    rng = np.random.RandomState(6)
    n = 4099
    base = R.softmax((rng.randn(6, c) * 2).astype(np.float32), np.float32)
    p = np.repeat(base, 700, axis=0)[:n]
    labels = rng.randint(0, c, n).astype(np.int64)
    labels[rng.rand(n) < 0.05] = 255
    _check_flat(p, labels)
    _check_flat(p, labels, classes='all')


def test_bad_labels_raise_and_limits_are_refused_before_any_launch():
    from lidal_amd import backend as B
    F = _F()
    z, p, labels = _case(300, 5, 2)
    for bad in (5, -1):
        lab = labels.copy()
        lab[123] = bad
        with pytest.raises(ValueError, match='outside'):
            F.lovasz_softmax(_dev(z), _dev(lab))
        with pytest.raises(ValueError, match='outside'):
            F.lovasz_softmax_flat(_dev(p), _dev(lab))
        out = F.lovasz_forward(_dev(p), _dev(lab), probs=True, check_labels=False)       # the status word, unchecked
        assert out.stats[2].item() == 1.0
    with pytest.raises(RuntimeError, match='classes must be in 1..32'):
        F.lovasz_softmax(torch.zeros(4, 33, device=DEV), torch.zeros(4, dtype=torch.int64, device=DEV))
    # n * c >= 2^30: refused on the arguments alone (no buffer of that size exists here, none is touched)
    L = B.lib()
    small = torch.zeros(64, device=DEV)
    lab = torch.zeros(8, dtype=torch.int64, device=DEV)
    n_big = (1 << 30) // 19 + 1
    assert L.lidal_lovasz_workspace_bytes(n_big, 19) == 0 and L.lidal_lovasz_workspace_bytes(n_big - 1, 19) > 0
    rc = L.lidal_lovasz_fwd(B.ptr(small), 0, 0, B.ptr(lab), n_big, 19, 255, 0, B.ptr(small), B.ptr(small), None,
                            B.ptr(small), 1 << 40, B.stream())
    assert rc == 2 and b'2^30' in B.lib_handle().lidal_last_error()
    rc = L.lidal_lovasz_bwd(B.ptr(small), 0, 0, B.ptr(lab), n_big, 19, 255, 0, B.ptr(small), B.ptr(small), B.ptr(small),
                            None, B.ptr(small), B.stream())
    assert rc == 2
    torch.cuda.synchronize()


def _relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('c', CS)
def test_logits_form_loss_against_the_f64_restatement(c, dtype):
    """The bar is measured, not fixed: 4 x the deviation of the f32 torch formulation on the CPU from the all-f64
    restatement on the same (already rounded) logits -- the GPU's expf and rounding points differ from the CPU's.

    Measured on an MI355X over the 100 inputs: the CPU formulation is off by 1.1e-8 / 1.8e-8 at the median for f32 /
    bf16 logits and by 1.1e-7 at most, the kernels by 9.6e-10 / 1.1e-9 and 2.6e-8 at most.  (While the key kernel took
    e from an f32 softmax, n = 63, c = 2, bf16 missed: CPU off by 8.2e-10, kernels by 4.8e-9.  It now rounds e once,
    from a softmax in f64, and is off by 2.7e-10 there.)"""
    F = _F()
    misses = []
    for n in NS:
        want, cpu, got, rounded = _loss_three_ways(F, n, c, dtype)
        print('lovasz loss n=%d c=%d %s: f64 %.9g, cpu f32 off by %.3g, gpu off by %.3g'
              % (n, c, dtype, want, abs(cpu - want), abs(got - want)))
        if not abs(got - want) <= 4 * abs(cpu - want):
            misses.append((n, got, want, cpu))
        assert rounded.dtype == torch.float32 and rounded.item() == np.float32(got)
    assert not misses, misses


def _loss_three_ways(F, n, c, dtype):
    z, _, labels = _case(n, c, 7 * c + n)
    zt = torch.from_numpy(z).to(dtype)
    z = zt.float().numpy()
    classes = 'all' if n % 2 else 'present'
    want = R.lovasz_logits(z, labels, 255, classes, np.float64)['loss']
    cpu = R.torch_lovasz_softmax(zt.float(), torch.from_numpy(labels), classes).item()
    got = F.lovasz_forward(zt.to(DEV), _dev(labels), 255, classes).stats[0].item()           # the loss as summed, f64
    return want, cpu, got, F.lovasz_softmax(zt.to(DEV), _dev(labels), 255, classes)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('c', CS)
def test_logits_form_loss_is_as_close_to_f64_as_f32_arithmetic_gets(c, dtype):
    """Beside the measured bar above, which compares two draws of rounding noise input by input, a bound from the
    formats alone.  L_k = sum_r e[r] g[r] with g >= 0, sum g = jac[last] <= 1 and e <= 1.  An error d in every e (the
    f32 softmax: expf, sum, division, then |fg - p|: <= 5 * 2^-24) moves L_k by <= d * sum g; an error d' in every
    jac (division and subtraction: <= 2 * 2^-24) moves it, summed by parts, by <= d' * e[0].  So |L_k - exact| <=
    7 * 2^-24, and so is their mean's; 8 * 2^-24 = 4.8e-7 absolute is asked."""
    F = _F()
    for n in NS:
        want, _, got, _ = _loss_three_ways(F, n, c, dtype)
        assert abs(got - want) <= 8 * 2.0 ** -24, (n, got, want)


SEPARATED = [(400, 2, False), (200, 3, False), (20, 19, False), (14, 32, False), (12, 3, True), (40, 2, True)]


@pytest.mark.parametrize('n,c,bf16', SEPARATED)
def test_logits_form_gradient_on_separated_inputs(n, c, bf16):
    """Errors at least 1e-3 apart inside every class (test_loss_cpu.py: f32 and f64 rank them alike), so every element
    of the gradient is compared.  Bar: 4 x the relative l2 deviation of the f32 torch formulation's autograd gradient on
    the CPU from the f64 restatement; a bf16 gradient is rounded to bf16 on top (8 significant bits: half an ulp is at
    most 2^-8 relative per element, hence of the l2 norm)."""
    F = _F()
    z, labels = R.separated_logits(n, c, seed=n + c, bf16=bf16)
    want = R.lovasz_logits(z, labels, ft=np.float64, upstream=1.7)
    zc = torch.from_numpy(z).requires_grad_(True)
    (R.torch_lovasz_softmax(zc, torch.from_numpy(labels)) * 1.7).backward()
    zg = _dev(z).to(torch.bfloat16 if bf16 else torch.float32).requires_grad_(True)
    loss, lk = F.lovasz_softmax(zg, _dev(labels), per_class=True)
    (loss * 1.7).backward()
    assert zg.grad.dtype == zg.dtype
    cpu_err, gpu_err = _relerr(zc.grad.numpy(), want['dz']), _relerr(zg.grad.float().cpu().numpy(), want['dz'])
    print('lovasz gradient n=%d c=%d bf16=%d: cpu f32 off by %.3g, gpu off by %.3g' % (n, c, bf16, cpu_err, gpu_err))
    assert gpu_err <= 4 * cpu_err + (2.0 ** -8 if bf16 else 0.0)
    assert not zg.grad[_dev(labels) == 255].any()
    np.testing.assert_allclose(lk.detach().cpu().numpy(), want['per_class'], rtol=1e-5)
    # the per-class losses are differentiable on their own: d L_k / dz, here of two classes at once
    v = np.zeros(c)
    v[0], v[c - 1] = 0.5, -2.0
    zg.grad = None
    (F.lovasz_softmax(zg, _dev(labels), per_class=True)[1] * _dev(v.astype(np.float32))).sum().backward()
    def dz_of(ref, ft):
        p, a = ref['p'], (ref['grad'] * v.astype(ft)[None, :]).astype(ft)
        dz = (p * (a - (a * p).sum(1, keepdims=True, dtype=ft))).astype(ft)
        dz[labels == 255] = 0
        return dz

    # measured the same way, the f32 restatement standing in for the torch formulation
    dz64 = dz_of(want, np.float64)
    cpu_err = _relerr(dz_of(R.lovasz_logits(z, labels, ft=np.float32), np.float32), dz64)
    gpu_err = _relerr(zg.grad.float().cpu().numpy(), dz64)
    print('lovasz per-class gradient n=%d c=%d bf16=%d: cpu f32 off by %.3g, gpu off by %.3g' % (n, c, bf16, cpu_err, gpu_err))
    assert gpu_err <= 4 * cpu_err + (2.0 ** -8 if bf16 else 0.0)


def test_flat_form_gradient_is_the_saved_one_scaled():
    F = _F()
    _, p, labels = _case(1025, 19, 3)
    labels[labels == 7] = 8
    for classes in ('present', 'all'):
        ref = R.lovasz_flat(p, labels, 255, classes)
        pg = _dev(p).requires_grad_(True)
        (F.lovasz_softmax_flat(pg, _dev(labels), classes=classes) * 3.0).backward()
        want = ref['grad'].astype(np.float64) * ref['scale'][None, :] * 3.0
        np.testing.assert_allclose(pg.grad.cpu().numpy(), want, rtol=3e-7, atol=0)       # two f32 roundings


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('zero', ['none', 'present', 'all'])
def test_weighted_cross_entropy_against_torch_in_f64(dtype, zero):
    """Loss and dlogits against torch.nn.functional.cross_entropy(weight=) in f64 on the CPU, at the bars the
    unweighted kernel is held to (tests/test_ops_gpu.py:570-571: loss 1e-5 relative, + 1e-6 for bf16 logits; gradient
    1e-5 / 1e-2 relative l2).  A zero weight on a present class is covered; zero weight on all of them is 0 / 0 =
    nan, as torch."""
    F = _F()
    for n, c in [(1, 1), (65, 2), (257, 16), (1025, 32), (4099, 19)]:
        z, _, labels = _case(n, c, 31 * c + n, scale=3.0)
        labels[0] = 0
        zt = torch.from_numpy(z).to(dtype)
        w = torch.rand(c, generator=torch.Generator().manual_seed(c)) + 0.1
        if zero == 'present':
            w[0] = 0.0
        if zero == 'all':
            w[:] = 0.0
        zr = zt.double().requires_grad_(True)
        ref = torch.nn.functional.cross_entropy(zr, torch.from_numpy(labels), weight=w.double(), ignore_index=255)
        (ref * 1.7).backward()
        zg = zt.to(DEV).requires_grad_(True)
        loss = F.cross_entropy(zg, _dev(labels), 255, weight=w.to(DEV))
        (loss * 1.7).backward()
        if zero == 'all' or (zero == 'present' and c == 1):
            assert torch.isnan(ref) and torch.isnan(loss)
            continue
        print('weighted ce n=%d c=%d %s: loss off by %.3g relative, gradient by %.3g'
              % (n, c, dtype, abs(loss.item() - ref.item()) / max(abs(ref.item()), 1e-300),
                 _relerr(zg.grad.float().cpu().numpy(), zr.grad.numpy())))
        if ref.item() == 0.0 and dtype == torch.float32:       # (one class: -log 1; the strict bar below cannot hold at 0)
            assert loss.item() == 0.0
        else:
            assert abs(loss.item() - ref.item()) < 1e-5 * abs(ref.item()) + (0 if dtype == torch.float32 else 1e-6)
        assert _relerr(zg.grad.float().cpu().numpy(), zr.grad.numpy()) < (1e-5 if dtype == torch.float32 else 1e-2)
        assert (zg.grad[_dev(labels) == 255] == 0).all()


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_cross_entropy_without_weights_is_the_fused_one(dtype):
    from lidal_amd.nn.functional import fused
    F = _F()
    z, _, labels = _case(4099, 19, 8)
    a = _dev(z).to(dtype).requires_grad_(True)
    b = _dev(z).to(dtype).requires_grad_(True)
    la = F.cross_entropy(a, _dev(labels), 255, weight=None)
    lb = fused.cross_entropy(b, _dev(labels), 255)
    la.backward()
    lb.backward()
    assert torch.equal(la, lb) and torch.equal(a.grad, b.grad)


def test_two_runs_give_the_same_bits():
    F = _F()
    z, _, labels = _case(4099, 19, 9)
    w = torch.rand(19, device=DEV) + 0.1

    def run():
        zg = _dev(z).requires_grad_(True)
        out = F.lovasz_forward(zg.detach(), _dev(labels), want_ranks=True)
        loss = F.combined_loss(zg, _dev(labels), class_weight=w)
        loss.backward()
        return out.stats, out.grad, out.ranks, loss.detach(), zg.grad

    first, second = run(), run()
    for a, b in zip(first, second):
        assert torch.equal(a, b)


@pytest.mark.parametrize('n,c', [(1, 1), (257, 19), (4099, 32)])
def test_workspace_is_carved_exactly(monkeypatch, n, c):
    from lidal_amd import backend as B
    F = _F()
    z, _, labels = _case(n, c, 10)
    want = F.lovasz_forward(_dev(z), _dev(labels), want_ranks=True)
    wce = F.cross_entropy(_dev(z), _dev(labels), weight=torch.ones(c, device=DEV))
    torch.cuda.synchronize()
    g = Guarded()
    monkeypatch.setattr(B, 'workspace', g)
    got = F.lovasz_forward(_dev(z), _dev(labels), want_ranks=True)
    gce = F.cross_entropy(_dev(z), _dev(labels), weight=torch.ones(c, device=DEV))
    g.check()
    assert len(g.bufs) == 2
    for a, b in zip(want, got):
        assert torch.equal(a, b)
    assert torch.equal(wce, gce)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_operands_off_the_16_byte_grid_take_the_scalar_path_to_the_same_bits(dtype):
    """`x[1:]` of a [n + 1, 19] matrix starts 76 (f32) or 38 (bf16) bytes into its allocation: the row-wise kernels
    cannot move it as 16-byte vectors and fall back to element accesses.  Same results as on an aligned copy, bit for
    bit, for both Lovasz forms, the backward passes and the weighted cross-entropy; the element past the view's end and
    the row in front of it are not touched."""
    F = _F()
    n, c = 1025, 19
    z, p, labels = _case(n, c, 21)
    lab = _dev(labels)
    w = torch.rand(c, device=DEV) + 0.1

    def run(x, probs):
        x = x.detach().requires_grad_(True)               # (a leaf on the same storage)
        out = F.lovasz_forward(x.detach(), lab, probs=probs, want_ranks=True)
        loss = F.lovasz_softmax_flat(x, lab) if probs else F.lovasz_softmax(x, lab) + F.cross_entropy(x, lab, weight=w)
        loss.backward()
        return out.stats, out.grad, out.ranks, loss.detach(), x.grad

    for src, probs in ((z, False), (p, True)):
        if probs and dtype != torch.float32:
            continue
        whole = torch.full((n + 1, c), 7.0, device=DEV).to(dtype)
        whole[1:] = _dev(src).to(dtype)
        view = whole[1:].detach()
        assert view.data_ptr() % 16 != 0 and view.is_contiguous()
        got = run(view, probs)
        want = run(view.clone(), probs)
        assert want[4].data_ptr() % 16 == 0
        for a, b in zip(got, want):
            assert torch.equal(a, b)
        assert bool((whole[0] == 7.0).all())


def test_class_weights_follow_their_formulas():
    from lidal_amd import data
    rng = np.random.RandomState(12)
    labels = rng.choice([0, 1, 2, 4, 255], 5000, p=[0.6, 0.25, 0.1, 0.01, 0.04]).astype(np.int64)
    counts = np.bincount(labels[labels != 255], minlength=6).astype(np.float64)
    f = counts / counts.sum()
    has = counts > 0
    for kind, raw in (('inverse', np.where(has, 1 / np.maximum(f, 1e-300), 0)),
                      ('inverse_sqrt', np.where(has, 1 / np.sqrt(np.maximum(f, 1e-300)), 0))):
        w = data.class_weights(_dev(labels).reshape(50, 100), 6, kind=kind).cpu().numpy()
        np.testing.assert_allclose(w, raw / raw[has].mean(), rtol=1e-6)
        assert w.dtype == np.float32 and w[3] == 0 and w[5] == 0
    w = data.class_weights(_dev(labels), 6, kind='log').cpu().numpy()
    np.testing.assert_allclose(w, 1 / np.log(1.02 + f), rtol=1e-6)


def test_training_with_the_combined_loss_drives_it_down():
    """train_step(criterion=combined_loss): 10 Adam steps on the scan of test_model_gpu.py's
    test_training_drives_the_loss_down lower the combined loss; criterion=None is the call that test makes."""
    from lidal_amd import data, synth
    from lidal_amd.network import SPVCNN
    from lidal_amd.train_step import train_step
    F = _F()
    b = synth.make_train_batch(n_frames=1, n_points=20000, seed=3)
    c = torch.from_numpy(b['coords_v_b']).to(DEV)
    f = torch.from_numpy(b['feats_v_b']).to(DEV)
    lab = (c[:, 2] // 40 % 19).long()
    lab[::10] = 255
    w = data.class_weights(lab, 19, kind='inverse_sqrt')
    torch.manual_seed(0)
    model = SPVCNN(19).to(DEV).train()
    opt = torch.optim.Adam(model.parameters())

    def criterion(logits, labels):
        return F.combined_loss(logits, labels, class_weight=w)

    losses = [train_step(model, opt, f, c, lab, criterion=criterion)[0].item() for _ in range(10)]
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    first = []
    for kwargs in ({}, {'criterion': None}):
        torch.manual_seed(0)                             # the weights and the dropout masks
        m = SPVCNN(19).to(DEV).train()
        first.append(train_step(m, torch.optim.Adam(m.parameters()), f, c, lab, **kwargs)[0])
    assert torch.equal(first[0], first[1])
