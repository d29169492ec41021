"""The restatements of tests/loss_ref.py against torch on the CPU (no GPU): they are what test_loss_gpu.py holds the
kernels of lidal_amd/csrc/loss.hip to."""
import numpy as np
import pytest
import torch

import loss_ref as R


def _random_case(n, c, seed, frac_ignored=0.1):
    rng = np.random.RandomState(seed)
    z = (rng.randn(n, c) * 2).astype(np.float32)
    labels = rng.randint(0, c, n).astype(np.int64)
    labels[rng.rand(n) < frac_ignored] = 255
    p = R.softmax(z, np.float32)
    return z, p, labels


@pytest.mark.parametrize('classes', ['present', 'all'])
@pytest.mark.parametrize('n,c', [(1, 3), (65, 2), (257, 19), (1025, 5)])
def test_restatement_equals_the_torch_formulation(n, c, classes):
    """Random probabilities (no ties: checked): loss within n * 2^-24 relative -- the torch formulation takes an f32
    dot product of n terms per class -- and the gradient with respect to the probabilities, which is +-g[rank] / classes
    in both, to f32 rounding of that one division."""
    z, p, labels = _random_case(n, c, 11 + n + c)
    if c == 5:
        labels[labels == 3] = 1                                         # a class absent
    for k in range(c):
        e = np.abs((labels == k) - p[:, k])[labels != 255]
        assert np.unique(e).size == e.size
    ref = R.lovasz_flat(p, labels, 255, classes)
    pt = torch.from_numpy(p).requires_grad_(True)
    loss = R.torch_lovasz_softmax_flat(pt, torch.from_numpy(labels), classes)
    loss.backward()
    assert abs(loss.item() - ref['loss']) <= n * 2.0 ** -24 * abs(ref['loss']) + 1e-30
    want = ref['grad'].astype(np.float64) * ref['scale'][None, :]
    np.testing.assert_allclose(pt.grad.numpy(), want, rtol=3e-7, atol=1e-12)
    assert ref['present'] == len(set(labels[labels != 255].tolist()))


def test_logits_form_matches_torch_autograd_in_f64():
    z, _, labels = _random_case(300, 7, 5)
    ref = R.lovasz_logits(z, labels, 255, 'present', np.float64, upstream=1.7)
    zt = torch.from_numpy(z).double().requires_grad_(True)
    loss = R.torch_lovasz_softmax(zt, torch.from_numpy(labels))
    (loss * 1.7).backward()
    assert abs(loss.item() - ref['loss']) <= 1e-12 * abs(ref['loss'])
    np.testing.assert_allclose(zt.grad.numpy(), ref['dz'], rtol=1e-9, atol=1e-15)


def test_loss_is_invariant_under_ties_and_the_gradient_follows_the_tie_rule():
    """Blocks of duplicated rows with different labels: permuting tied rows leaves the loss (the Lovasz extension does
    not depend on the order inside a tie; f32 jac: to n * 2^-24) and moves the gradient with the rows' positions --
    among equal errors of one class the ranks ascend with the row index."""
    rng = np.random.RandomState(2)
    base = R.softmax((rng.randn(8, 4) * 2).astype(np.float32), np.float32)
    p = np.repeat(base, 12, axis=0)                     # 8 blocks of 12 equal rows
    n = p.shape[0]
    labels = rng.randint(0, 4, n).astype(np.int64)
    a = R.lovasz_flat(p, labels)
    perm = np.arange(n)
    for b in range(8):                                  # shuffle inside every block: p stays, the labels move
        perm[b * 12:(b + 1) * 12] = b * 12 + rng.permutation(12)
    b_ = R.lovasz_flat(p, labels[perm])
    assert abs(a['loss'] - b_['loss']) <= n * 2.0 ** -24 * a['loss']
    assert not np.array_equal(a['grad'], b_['grad'])
    for out, lab in ((a, labels), (b_, labels[perm])):
        for k in range(4):
            e = np.abs((lab == k).astype(np.float32) - p[:, k])
            for v in np.unique(e):
                rows = np.nonzero(e == v)[0]
                assert np.all(np.diff(out['ranks'][rows, k]) > 0)


def test_zero_error_has_zero_gradient_and_empty_inputs_give_zero():
    p = np.array([[1, 0], [0, 1], [0.25, 0.75]], np.float32)
    labels = np.array([0, 1, 0], np.int64)
    out = R.lovasz_flat(p, labels)
    assert np.all(out['grad'][:2] == 0) and np.all(out['grad'][2] != 0)
    none = R.lovasz_flat(p, np.full(3, 255, np.int64))
    assert none['loss'] == 0.0 and none['present'] == 0 and not none['grad'].any() and np.all(none['ranks'] == -1)


@pytest.mark.parametrize('n,c,bf16', [(400, 2, False), (200, 3, False), (20, 19, False), (14, 32, False),
                                      (12, 3, True), (40, 2, True)])
def test_separated_inputs_rank_alike_in_f32_and_f64(n, c, bf16):
    """The inputs of the GPU gradient checks: errors at least 1e-3 apart inside every class (separated_logits
    verifies it), so the f32 and the f64 restatement order every class alike."""
    z, labels = R.separated_logits(n, c, seed=n + c, bf16=bf16)
    a = R.lovasz_logits(z, labels, ft=np.float32)
    b = R.lovasz_logits(z, labels, ft=np.float64)
    assert np.array_equal(a['ranks'], b['ranks'])
    assert a['present'] == b['present'] == min(n, c)


@pytest.mark.parametrize('zero', ['none', 'one', 'all'])
def test_weighted_cross_entropy_equals_torch(zero):
    z, _, labels = _random_case(500, 19, 9)
    rng = np.random.RandomState(4)
    w = rng.rand(19) + 0.1
    if zero == 'one':
        w[int(labels[0] if labels[0] != 255 else 3)] = 0.0
    if zero == 'all':
        w[:] = 0.0
    loss, dz = R.weighted_cross_entropy(z, labels, w, 255, upstream=1.7)
    zt = torch.from_numpy(z).double().requires_grad_(True)
    ref = torch.nn.functional.cross_entropy(zt, torch.from_numpy(labels), weight=torch.from_numpy(w),
                                            ignore_index=255)
    (ref * 1.7).backward()
    if zero == 'all':                                   # 0 / 0: nan, as torch
        assert np.isnan(loss) and torch.isnan(ref)
        return
    assert abs(loss - ref.item()) <= 1e-12 * abs(ref.item())
    np.testing.assert_allclose(dz, zt.grad.numpy(), rtol=1e-10, atol=1e-16)


def test_cpu_tensors_are_refused():
    from lidal_amd.nn import functional as F
    z = torch.zeros(4, 3)
    y = torch.zeros(4, dtype=torch.int64)
    for call in (lambda: F.lovasz_softmax(z, y), lambda: F.lovasz_softmax_flat(z, y),
                 lambda: F.cross_entropy(z, y, weight=torch.ones(3)), lambda: F.cross_entropy(z, y),
                 lambda: F.combined_loss(z, y)):
        with pytest.raises(RuntimeError, match='GPU only'):
            call()


def test_class_weights_refuses_cpu_and_unknown_kinds():
    from lidal_amd import data
    with pytest.raises(ValueError):
        data.class_weights(torch.zeros(4, dtype=torch.int64), 3, kind='cubic')
    with pytest.raises(RuntimeError, match='GPU only'):
        data.class_weights(torch.zeros(4, dtype=torch.int64), 3)
