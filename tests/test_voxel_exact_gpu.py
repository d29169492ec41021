"""Every form of the point-voxel sums (csrc/voxel.hip) against the f64 definition, bit for bit, at the edges of their
loops and splits (tests/voxel_ref.py: exact operands -- any association of the f32 sums holds the exact value, so the
result must equal the f64 sum rounded once to the output type); the gathers, the autograd wrappers and the list
builder beside them; and the per-element error bound with real counts and normal rows."""
import numpy as np
import pytest
import torch

import voxel_ref as R
from guarded_ws import GUARD, Guarded

pytestmark = pytest.mark.gpu
DEV = 'cuda'
IDS = [R.case_id(c) for c in R.CASES]


def _dev(ops):
    return {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in ops.items()}


def _same(got, ref64, what=''):
    """got == the f64 reference rounded once to got's type; nothing of the NaN fill is left."""
    assert not bool(torch.isnan(got).any()), what + ': rows were left unwritten'
    want = ref64.to(got.dtype)
    if not torch.equal(got, want):
        bad = torch.nonzero((got != want).any(dim=1)).view(-1)
        raise AssertionError('%s: %d rows differ from the f64 sums, first %s' % (what, bad.numel(), bad[:8].tolist()))


def _sorted_sum(op, ops, dtype, guarded):
    """lidal_voxelize_fwd_sorted / lidal_devoxelize_bwd_sorted through the C-ABI, as the wrappers call them: the lists
    from inverse_lists, n_entries = n or 8 n, a NaN-filled output, exactly the scratch the size query names."""
    from lidal_amd import backend as B
    from lidal_amd.nn.functional.invlist import inverse_lists
    L = B.lib()
    m, c, ne = ops['m'], ops['c'], ops['n_entries']
    assert ne == ops['idx'].numel()
    order, seg = inverse_lists(ops['idx'], m, ops.get('w'))
    nbytes = L.lidal_segment_workspace_bytes(ne, m, c)
    guarded(nbytes)
    ws = guarded.bufs[-1][0].data_ptr() + GUARD
    out = torch.full((m, c), float('nan'), dtype=R.TORCH[dtype], device=DEV)
    if op == 'vox':
        B.check(L.lidal_voxelize_fwd_sorted(B.ptr(ops['rows']), B.ptr(order), B.ptr(seg), B.ptr(ops['counts']), B.ptr(out),
                                            m, c, dtype, ne, ws, nbytes, B.stream()), 'voxelize_fwd_sorted')
    else:
        B.check(L.lidal_devoxelize_bwd_sorted(B.ptr(ops['rows']), B.ptr(order), B.ptr(seg), B.ptr(ops['w']), B.ptr(out),
                                              m, c, dtype, ne, ws, nbytes, B.stream()), 'devoxelize_bwd_sorted')
    return out, seg


def _reference(op, ops):
    if op == 'vox':
        return R.ref_voxelize(ops['rows'], ops['idx'], ops['counts'], ops['m'])
    return R.ref_devoxelize_bwd(ops['rows'], ops['idx'], ops['w'], ops['m'])


# ---- A. the ordered sums, form by form ------------------------------------------------------------------------------
@pytest.mark.parametrize('op', ['vox', 'devox'])
@pytest.mark.parametrize('case', R.CASES, ids=IDS)
def test_ordered_sums_equal_the_f64_sums(case, op):
    lay = R.layout(case, op)
    ops = _dev(R.build_case(case, op, lay))
    form = R.lib().lidal_segment_form(ops['n_entries'], case.m, case.c, case.dtype)
    print('%s %s: form %d, filler %d, %d entries' % (R.case_id(case), op, form, lay.filler, ops['n_entries']))
    assert form == case.form and ops['n_entries'] == lay.n_entries
    guarded = Guarded()
    out, seg = _sorted_sum(op, ops, case.dtype, guarded)
    # the lists are the ones the case asked for
    assert torch.equal(seg[1:] - seg[:-1], torch.from_numpy(lay.lengths).to(DEV))
    _same(out, _reference(op, ops), R.case_id(case) + ' ' + op)
    empty = torch.from_numpy(lay.lengths == 0).to(DEV)
    assert bool((out[empty] == 0).all())
    guarded.check()


# ---- B. devoxelize backward through the cells ------------------------------------------------------------------------
@pytest.mark.parametrize('dtype,c', R.CELLS)
def test_cell_form_equals_the_f64_sums_and_the_per_voxel_form(dtype, c):
    from lidal_amd import backend as B
    from lidal_amd.nn.functional import devoxelize as DV
    L = B.lib()
    ops = _dev(R.build_cells(dtype, c))
    m, idx8, w8, g = ops['m'], ops['idx'], ops['w'], ops['rows']
    vorder, vseg, corder, cseg = DV.devox_cells(idx8, m)
    points = torch.from_numpy(ops['points']).to(DEV)
    assert torch.equal(vseg[1:] - vseg[:-1], points) and int(points[m - 1]) == 0
    guarded = Guarded()
    nbytes = L.lidal_devoxelize_bwd_cells_workspace_bytes(m, c)
    assert nbytes == m * 8 * c * 4
    ws = guarded(nbytes)
    gin = torch.full((m, c), float('nan'), dtype=R.TORCH[dtype], device=DEV)
    B.check(L.lidal_devoxelize_bwd_cells(B.ptr(g), B.ptr(vorder), B.ptr(vseg), B.ptr(w8), B.ptr(corder), B.ptr(cseg),
                                         B.ptr(gin), m, c, dtype, B.ptr(ws), nbytes, B.stream()), 'devoxelize_bwd_cells')
    ref = R.ref_devoxelize_bwd(g, idx8, w8, m)
    _same(gin, ref, 'cells')
    guarded.check()
    # an empty cell adds nothing: its eight partial rows are zeros
    cs = ws.view(torch.float32).view(m, 8, c)
    assert bool((cs[points == 0] == 0).all())
    g2 = Guarded()
    gin2, _ = _sorted_sum('devox', ops, dtype, g2)
    g2.check()
    assert torch.equal(gin, gin2)


# ---- C. the gathers ------------------------------------------------------------------------------------------------------
GATHER_N = (1, 255, 256, 257, 1000)
GATHER_C = (3, 4, 12, 19, 32, 96, 256)          # scalar, 8-byte and 16-byte accesses under both element types


def _gather_operands(n, c, dtype, seed):
    m = 50
    rng = np.random.default_rng(seed)
    vox = R._rows(rng, m, c, dtype)
    pts = R._rows(rng, n, c, dtype)
    idx8 = rng.integers(0, m, size=(n, 8))
    dead = rng.random((n, 8))
    idx8[dead < 0.1] = -1
    big = (dead >= 0.1) & (dead < 0.2)
    idx8[big] = m + rng.integers(0, 2, size=int(big.sum())) * (2 ** 30)
    k = rng.integers(0, 65, size=(n, 8))
    k[rng.random((n, 8)) < 0.15] = 0
    counts = (1 << rng.integers(0, 7, size=m)).astype(np.int32)
    counts[rng.permutation(m)[:5]] = 0
    idx = idx8[:, 0].copy()
    idx[0] = int(np.nonzero(counts)[0][0])                     # (n = 1: a live point; dead ones in the larger cases)
    if n > 4:
        idx[1], idx[2], idx[3] = -1, m, int(np.nonzero(counts == 0)[0][0])
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).to(DEV)
    return dict(m=m, vox=vox.to(DEV), pts=pts.to(DEV), idx8=t(idx8, np.int32), w8=t(k / 64.0, np.float32),
                idx=t(idx, np.int32), counts=t(counts, np.int32))


@pytest.mark.parametrize('c', GATHER_C)
@pytest.mark.parametrize('dtype', [R.F32, R.BF16], ids=['f32', 'bf16'])
def test_gathers_equal_the_f64_definition(dtype, c):
    from lidal_amd import backend as B
    L = B.lib()
    for n in GATHER_N:
        o = _gather_operands(n, c, dtype, 100 * c + n + dtype)
        m = o['m']
        out = torch.full((n, c), float('nan'), dtype=R.TORCH[dtype], device=DEV)
        B.check(L.lidal_devoxelize_fwd(B.ptr(o['vox']), B.ptr(o['idx8']), B.ptr(o['w8']), B.ptr(out), n, m, c, dtype,
                                       B.stream()), 'devoxelize_fwd')
        _same(out, R.ref_devoxelize_fwd(o['vox'], o['idx8'], o['w8']), 'devoxelize_fwd n=%d' % n)
        idx, counts = o['idx'], o['counts']
        deadp = (idx < 0) | (idx >= m)
        deadp[~deadp] = counts[idx[~deadp].long()] == 0
        assert n <= 4 or int(deadp.sum()) >= 3
        for res in (None, o['pts']):
            gin = torch.full((n, c), float('nan'), dtype=R.TORCH[dtype], device=DEV)
            B.check(L.lidal_voxelize_bwd(B.ptr(o['vox']), B.ptr(idx), B.ptr(counts), B.ptr(res), B.ptr(gin), n, m, c,
                                         dtype, B.stream()), 'voxelize_bwd')
            _same(gin, R.ref_voxelize_bwd(o['vox'], idx, counts, res), 'voxelize_bwd n=%d' % n)
            # a dead point's gradient: nothing, or exactly what arrives through the other consumer
            assert torch.equal(gin[deadp], torch.zeros_like(gin[deadp]) if res is None else res[deadp])


# ---- D. through autograd ---------------------------------------------------------------------------------------------------
def _autograd_lists(m):
    lengths = np.full(m, 3, dtype=np.int64)
    lad = R.ladder(8, 0)
    lengths[np.random.default_rng(3).permutation(m)[:len(lad)]] = lad
    return lengths


@pytest.mark.parametrize('c', [3, 19, 32])            # 3 and 19: the f32 copy and the atomic kernels
@pytest.mark.parametrize('dtype', [R.F32, R.BF16], ids=['f32', 'bf16'])
def test_spvoxelize_and_spdevoxelize_through_autograd(dtype, c):
    from lidal_amd.nn import functional as F
    m, dt = 200, R.TORCH[dtype]
    lengths = _autograd_lists(m)
    rng = np.random.default_rng(c + dtype)
    # voxelize: forward, backward
    v = _dev(R.build_voxelize(m, c, dtype, lengths, 11 + c))
    feats = v['rows'].clone().requires_grad_(True)
    out = F.spvoxelize(feats, v['idx'], v['counts'])
    assert out.dtype == dt
    _same(out.detach(), R.ref_voxelize(v['rows'], v['idx'], v['counts'], m), 'spvoxelize')
    gout = R._rows(rng, m, c, dtype).to(DEV)
    out.backward(gout)
    _same(feats.grad, R.ref_voxelize_bwd(gout, v['idx'], v['counts']), 'spvoxelize backward')
    # devoxelize: forward, backward
    d = _dev(R.build_devoxelize(m, c, dtype, lengths, 12 + c))
    vfeats = R._rows(rng, m, c, dtype).to(DEV).requires_grad_(True)
    y = F.spdevoxelize(vfeats, d['idx'], d['w'])
    assert y.dtype == dt
    _same(y.detach(), R.ref_devoxelize_fwd(vfeats.detach(), d['idx'], d['w']), 'spdevoxelize')
    y.backward(d['rows'])
    _same(vfeats.grad, R.ref_devoxelize_bwd(d['rows'], d['idx'], d['w'], m), 'spdevoxelize backward')


@pytest.mark.parametrize('c', [19, 32])
@pytest.mark.parametrize('dtype', [R.F32, R.BF16], ids=['f32', 'bf16'])
def test_spvoxelize_fork_adds_the_alias_gradient_inside_the_kernel(dtype, c):
    """F.spvoxelize(..., fork=True): the input gradient is gout[idx] / counts plus what arrives through the alias."""
    from lidal_amd.nn import functional as F
    m = 200
    v = _dev(R.build_voxelize(m, c, dtype, _autograd_lists(m), 21 + c))
    rng = np.random.default_rng(40 + c + dtype)
    feats = v['rows'].clone().requires_grad_(True)
    out, alias = F.spvoxelize(feats, v['idx'], v['counts'], fork=True)
    _same(out.detach(), R.ref_voxelize(v['rows'], v['idx'], v['counts'], m), 'spvoxelize(fork)')
    assert torch.equal(alias.detach(), v['rows'])
    gout = R._rows(rng, m, c, dtype).to(DEV)
    gskip = R._rows(rng, v['rows'].shape[0], c, dtype).to(DEV)
    torch.autograd.backward([out, alias], [gout, gskip])
    _same(feats.grad, R.ref_voxelize_bwd(gout, v['idx'], v['counts'], gskip), 'spvoxelize(fork) backward')


# ---- E. the list builder ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('weights', [False, True], ids=['plain', 'weights'])
@pytest.mark.parametrize('m', [1, 255, 256, 257, 65535, 65536, 65537])       # the radix sort's key width, sentinel key m
def test_invlist_build_is_the_stable_sort_of_the_valid_entries(m, weights):
    from lidal_amd.nn.functional.invlist import inverse_lists
    for ne in (0, 1, 8191, 8192, 8193):
        rng = np.random.default_rng(m + 3 * ne + weights)
        idx = rng.integers(0, m, size=ne).astype(np.int64)
        kind = rng.random(ne)
        idx[kind < 0.1] = -1
        idx[(kind >= 0.1) & (kind < 0.2)] = m
        idx[(kind >= 0.2) & (kind < 0.25)] = m + 1
        idx[(kind >= 0.25) & (kind < 0.3)] = 2 ** 31 - 1
        if ne > 8:
            idx[4:8] = (0, m - 1, m - 1, 0)
        w = rng.integers(0, 65, size=ne).astype(np.float32) / 64.0
        w[rng.random(ne) < 0.2] = 0.0
        ok = (idx >= 0) & (idx < m) & ((w != 0) if weights else True)
        e = np.nonzero(ok)[0]
        want_order = e[np.argsort(idx[e], kind='stable')]
        want_seg = np.searchsorted(np.sort(idx[e]), np.arange(m + 1), side='left')
        tidx = torch.from_numpy(idx.astype(np.int32)).to(DEV)
        order, seg = inverse_lists(tidx, m, torch.from_numpy(w).to(DEV) if weights else None)
        assert seg.dtype == torch.int64 and seg.shape == (m + 1,)
        assert np.array_equal(seg.cpu().numpy(), want_seg), (m, ne)
        assert int(seg[m]) == len(e)
        assert np.array_equal(order[:len(e)].cpu().numpy(), want_order), (m, ne)


# ---- F. true counts and normal rows: a bound for every element -------------------------------------------------------------
@pytest.mark.parametrize('dtype', [R.F32, R.BF16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('form', sorted(R.SMALL), ids=[R.FORM_NAME[f] for f in sorted(R.SMALL)])
def test_mean_with_true_counts_is_within_the_rounding_bound_per_element(form, dtype):
    """counts = the real list lengths n_v = L_v, N(0, 1) rows: every quotient x_i / n_v carries one f32 rounding and the
    sum of L_v of them L_v - 1 more, in whatever association, so |got - ref| <= 1.01 * L_v * 2^-24 * sum_i |x_i| / n_v
    for every element (1.01: the second-order terms at L_v <= 5000), plus one rounding of the result, 2^-8 |ref|, for
    bf16 outputs."""
    case = R.SMALL[form][dtype]
    lay = R.layout(case, 'vox')
    ops = _dev(R.build_voxelize(case.m, case.c, case.dtype, lay.lengths, 900 + form, true_counts=True, normal=True))
    assert R.lib().lidal_segment_form(ops['n_entries'], case.m, case.c, case.dtype) == form
    guarded = Guarded()
    out, seg = _sorted_sum('vox', ops, case.dtype, guarded)
    guarded.check()
    lengths = torch.from_numpy(lay.lengths).to(DEV)
    assert torch.equal(seg[1:] - seg[:-1], lengths) and torch.equal(ops['counts'].long(), lengths)
    ref = R.ref_voxelize(ops['rows'], ops['idx'], ops['counts'], case.m)
    sumabs = R.ref_voxelize(ops['rows'].abs(), ops['idx'], torch.ones_like(ops['counts']), case.m)
    Lv = lengths.double().unsqueeze(1)
    bound = 1.01 * Lv * 2.0 ** -24 * sumabs / Lv.clamp_min(1.0)
    if dtype == R.BF16:
        bound = bound + 2.0 ** -8 * ref.abs()
    err = (out.double() - ref).abs()
    assert not bool(torch.isnan(out).any())
    worst = float((err / bound.clamp_min(1e-300)).max())
    print('%s: worst error / bound = %.3f' % (R.case_id(case), worst))
    assert bool((err <= bound).all()), worst
