"""tests/batchnorm_ref.py on its own, without a GPU: the f64 restatement is torch's batch_norm, the bounds and the
ambiguity cap hold for a numpy f32 evaluation of the kernel's expressions on every shape the GPU tests run, and the
restated launch geometry is the library's."""
import os

import numpy as np
import pytest
import torch

import batchnorm_ref as R

CASES = R.all_cases(with_one_row=True)
BIG = 3 << 20       # elements from which a case runs one forward and one backward variant instead of all


def _stats32(x64):
    mean, var, unb, inv = R.batch_stats(x64)
    return mean, var, unb, inv, mean.astype(np.float32), inv.astype(np.float32)


@pytest.mark.parametrize('relu,with_res', [(0, False), (1, False), (0, True), (1, True), (3, True), (2, True)])
@pytest.mark.parametrize('n,c', [(2, 4), (33, 24), (257, 8)])
def test_restatement_is_torch_batch_norm_in_f64(n, c, relu, with_res):
    case = R.Case('f32', n, c)
    x, dy, res = (case[k].astype(np.float64) for k in ('x', 'dy', 'res'))
    gamma, beta = case['gamma'].astype(np.float64), case['beta'].astype(np.float64)
    rm0, rv0 = case['rm0'].astype(np.float64), case['rv0'].astype(np.float64)
    tx, tg, tb = (torch.tensor(a, requires_grad=True) for a in (x, gamma, beta))
    rm, rv = torch.tensor(rm0), torch.tensor(rv0)
    ty = torch.nn.functional.batch_norm(tx, rm, rv, tg, tb, True, R.MOMENTUM, R.EPS)
    if relu & 1:
        ty = torch.relu(ty)
    if with_res:
        ty = ty + torch.tensor(res)
        if relu & 2:
            ty = torch.relu(ty)
    ty.backward(torch.tensor(dy))
    mean, var, unb, inv = R.batch_stats(x)
    _, v = R.forward_ratio(np.zeros_like(x), x, mean, inv, gamma, beta, relu, res if with_res else None, 'f32')
    assert np.abs(v - ty.detach().numpy()).max() < 1e-12
    assert np.abs((0.9 * rm0 + 0.1 * mean) - rm.numpy()).max() < 1e-12
    assert np.abs((0.9 * rv0 + 0.1 * unb) - rv.numpy()).max() < 1e-12
    d = np.where(v > 0, dy, 0.0) if (with_res and relu & 2) else dy
    bw = R.Backward(x, d, mean, inv, gamma, beta, relu & 1)
    scale = max(1.0, float(np.abs(tx.grad.numpy()).max()))
    assert np.abs(bw.dx_ref(bw.sum_b, bw.sum_g) - tx.grad.numpy()).max() < 1e-12 * scale * max(1.0, float(inv.max()) ** 2)
    assert np.abs(bw.sum_g - tg.grad.numpy()).max() < 1e-12 * max(1.0, float(bw.mag_g.max()))
    assert np.abs(bw.sum_b - tb.grad.numpy()).max() < 1e-12 * max(1.0, float(bw.mag_b.max()))


def test_helpers_round_and_measure_like_the_formats():
    rng = np.random.default_rng(5)
    a = np.concatenate([rng.standard_normal(4096).astype(np.float32) * np.float32(1e3),
                        np.array([1.00390625, 1.01171875, 0.0, -0.0, 3.0e38, 1e-40], dtype=np.float32)])
    assert np.array_equal(R.round_bf16(a), torch.from_numpy(a).bfloat16().float().numpy())
    v = np.abs(rng.standard_normal(4096)) * 10.0 ** rng.integers(-20, 20, 4096)
    v = v.astype(np.float32).astype(np.float64)
    assert np.array_equal(R.ulp32(v), np.spacing(v.astype(np.float32)).astype(np.float64))
    exact = np.array([1.0, 1.5, 2.0, 0.75, 1e-3], dtype=np.float32)
    assert np.array_equal(R.ulp32(exact.astype(np.float64)), np.spacing(exact).astype(np.float64))
    assert np.array_equal(R.ulp32(torch.tensor(v), R.TH).numpy(), R.ulp32(v))
    assert R.chain_length(32, 8) == 4 + 3 and R.chain_length(33, 1) == 33 and R.chain_length(1025, 256) == 5 + 8
    assert R.chain_length(40, 10) == 4 + 4


@pytest.mark.parametrize('dt,n,c', [('f32', 65, 24), ('bf16', 33, 48)])
def test_torch_namespace_gives_the_numpy_figures(dt, n, c):
    """The GPU tests evaluate the reference with torch tensors (xp = TH): the same figures as with numpy."""
    cs = R.Case(dt, n, c)
    x32, dy32, res32, gamma32, beta32 = (cs[k] for k in ('x', 'dy', 'res', 'gamma', 'beta'))
    t = {k: torch.from_numpy(cs[k]).double() for k in ('x', 'dy', 'res', 'gamma', 'beta')}
    a = {k: cs[k].astype(np.float64) for k in ('x', 'dy', 'res', 'gamma', 'beta')}
    sn, st = R.batch_stats(a['x']), R.batch_stats(t['x'], xp=R.TH)
    for u, v in zip(sn, st):
        assert np.allclose(u, v.numpy(), rtol=1e-13, atol=0)
    mu32, sig32 = sn[0].astype(np.float32), sn[3].astype(np.float32)
    assert R.stats_ulps(mu32, sig32, sn[0], sn[3]) == pytest.approx(
        R.stats_ulps(torch.from_numpy(mu32), torch.from_numpy(sig32), st[0], st[3], xp=R.TH), rel=1e-6)
    y = R.emulate_forward(x32, mu32, sig32, gamma32, beta32, 3, res32, dt)
    mu, sig = mu32.astype(np.float64), sig32.astype(np.float64)
    rn, _ = R.forward_ratio(y.astype(np.float64), a['x'], mu, sig, a['gamma'], a['beta'], 3, a['res'], dt)
    rt, _ = R.forward_ratio(torch.from_numpy(y).double(), t['x'], torch.from_numpy(mu), torch.from_numpy(sig), t['gamma'],
                            t['beta'], 3, t['res'], dt, xp=R.TH)
    assert 0 < rn <= 1 and rt == pytest.approx(rn, rel=1e-9)
    xhat, d = R.emulate_terms(x32, dy32, mu32, sig32, gamma32, beta32, 1)
    gb, gg = R.emulate_sums_f32(xhat, d, 32, R.rows_per_sweep(c, dt))
    dx = R.emulate_dx(xhat, d, sig32, gamma32, gb, gg, n, dt)
    bn = R.Backward(a['x'], a['dy'], mu, sig, a['gamma'], a['beta'], 1)
    bt = R.Backward(t['x'], t['dy'], torch.from_numpy(mu), torch.from_numpy(sig), t['gamma'], t['beta'], 1, xp=R.TH)
    f = lambda v: torch.from_numpy(v).double()          # noqa: E731
    k = R.chain_length(32, R.rows_per_sweep(c, dt))
    assert bt.sums_ratio_f32(f(gb), f(gg), k) == pytest.approx(bn.sums_ratio_f32(gb.astype(np.float64), gg.astype(np.float64), k))
    assert bt.sums_ratio_f64(f(gb), f(gg)) == pytest.approx(bn.sums_ratio_f64(gb.astype(np.float64), gg.astype(np.float64)))
    assert bt.dx_ratio(f(dx), f(gb), f(gg), dt) == pytest.approx(bn.dx_ratio(dx.astype(np.float64), gb.astype(np.float64),
                                                                             gg.astype(np.float64), dt))
    tiles = R.tile_sums_ref(bn.tb, bn.tg, 16)
    assert R.merged_ulps(f(gb).float(), torch.from_numpy(tiles), 0, xp=R.TH) == pytest.approx(R.merged_ulps(gb, tiles, 0))
    tr = R._tile_triples(torch.from_numpy(x32), 16)
    for u, v in zip(R.tile_merge(tr.numpy(), c), R.tile_merge(tr, c, xp=R.TH)):
        assert np.allclose(u, v.numpy(), rtol=1e-13, atol=0)
    for u, v in zip(R.tile_merge(tr.numpy(), c), sn):          # ... and the merge of the triples is the statistics
        assert np.allclose(u, v, rtol=1e-5)


def test_shape_list_reaches_every_edge_the_issue_names():
    f32, bf16 = R.shapes('f32'), R.shapes('bf16')
    for c in R.CHANNELS['f32']:
        assert all((n, c) in f32 for n in (2, 33, 8193)) and c % 4 == 0 and c // 4 <= 256
    for c in R.CHANNELS['bf16']:
        assert all((n, c) in bf16 for n in (2, 33, 8193)) and c % 8 == 0 and c // 8 <= 256
    assert max(R.CHANNELS['bf16']) == R.SLOT_CH
    assert all((n, c) in f32 and (n, c) in bf16 for n in R.ROWS for c in (96, 256))
    # 8193 rows: slabs of 33 rows, a short last slab, 249 workgroups; 33 rows: a second slab of one row
    assert R.rows_per_wg(8193) == 33 and R.nparts(8193) == 249 and 8193 - 248 * 33 == 9
    assert R.nparts(33) == 2 and R.nparts(32) == 1
    # the wide cases: 16 MiB of 1 KiB rows -- 512 element-wise workgroups, 256 for the statistics
    for dt, (n, c) in (('f32', R.WIDE['f32'][1]), ('bf16', R.WIDE['bf16'][1])):
        rb = c * R.ESIZE[dt]
        assert rb == 1024 and n * rb >= R.EW_WIDE_BYTES
        assert R.nslabs_ew(n, rb) == 497 and R.nparts(n) == 253
        assert R.nslabs_ew(n, rb) * c * 8 <= R.workspace_bytes(n, c)       # the bf16 slab sums fit the f64 workspace
    assert R.rows_per_sweep(4, 'f32') == 256 and R.rows_per_sweep(8, 'bf16') == 256
    assert R.rows_per_sweep(128, 'f32') == 8 and R.rows_per_sweep(516, 'f32') == 1 and R.rows_per_sweep(96, 'bf16') == 21


def test_grid_restatement_is_the_librarys():
    from lidal_amd import backend as B
    if not os.path.exists(B.LIB_PATH):
        pytest.skip('the library is not built here: tests/test_batchnorm_edges_gpu.py makes the same comparison')
    L = B.lib_handle()
    for dt, n, c in CASES + [('f32', 0, 96), ('bf16', 12289, 512), ('bf16', 12288, 512), ('f32', 396662, 96)]:
        code = 0 if dt == 'f32' else 1
        assert int(L.lidal_bn_workspace_bytes(n, c)) == R.workspace_bytes(n, c), (dt, n, c)
        assert int(L.lidal_bn_tail_parts(n, c, code)) == R.nslabs_ew(n, c * R.ESIZE[dt]), (dt, n, c)


@pytest.mark.parametrize('case', CASES, ids=R.case_id)
def test_bounds_and_cap_hold_for_an_f32_evaluation(case):
    """The kernel's expressions in numpy f32 (plain row order; f64 sums for the f64 forms; per-lane and tree order for
    the slab forms) stay inside every bound, and the reference's ambiguous share stays under the cap for the seed."""
    dt, n, c = case
    cs = R.Case(dt, n, c)
    big = n * c > BIG
    x32 = cs['x']
    x = x32.astype(np.float64)
    gamma32, beta32 = cs['gamma'], cs['beta']
    gamma, beta = gamma32.astype(np.float64), beta32.astype(np.float64)
    mean, var, unb, inv, mu32, sig32 = _stats32(x)
    em, ei = R.stats_ulps(mu32, sig32, mean, inv)
    assert em <= 1.0 and ei <= 2.0
    if n == 1:
        assert np.all(var == 0) and np.all(unb == 0)
    # running statistics: an evaluation with the products contracted (f64 then rounded) stays inside 2 ulp
    for r0, val in ((cs['rm0'], mean), (cs['rv0'], unb)):
        m = np.float32(R.MOMENTUM)
        fused = (np.float64(np.float32(1) - m) * r0.astype(np.float64)
                 + (m * val.astype(np.float32)).astype(np.float64)).astype(np.float32)
        assert R.running_ulps(fused, r0, val) <= 2.0
        assert R.running_ulps(R.running_ref(r0, val)[0], r0, val) == 0.0
    mu, sig = mu32.astype(np.float64), sig32.astype(np.float64)
    res32 = cs['res']
    for relu, r in (((3, res32),) if big else ((0, None), (1, None), (0, res32), (3, res32))):
        y = R.emulate_forward(x32, mu32, sig32, gamma32, beta32, relu, r, dt)
        ratio, _ = R.forward_ratio(y.astype(np.float64), x, mu, sig, gamma, beta, relu,
                                   None if r is None else r.astype(np.float64), dt)
        assert ratio <= 1.0, ('y', relu, ratio)
    if not big:
        var32 = var.astype(np.float32)
        y = R.emulate_forward(x32, mu32, var32, gamma32, beta32, 1, None, dt, var_in=True)
        sig_e = 1.0 / np.sqrt(var32.astype(np.float64) + np.float64(np.float32(R.EPS)))
        ratio, _ = R.forward_ratio(y.astype(np.float64), x, mu, sig_e, gamma, beta, 1, None, dt, var_in=True)
        assert ratio <= 1.0, ('eval', ratio)
    rb = c * R.ESIZE[dt]
    rpw, rpi = R.rows_per_wg_ew(n, rb), R.rows_per_sweep(c, dt)
    k = R.chain_length(rpw, rpi)
    dy32 = cs['dy']
    for relu in ((1,) if big else (0, 1)):
        bw = R.Backward(x, dy32.astype(np.float64), mu, sig, gamma, beta, relu)
        assert bw.ambiguous_share() <= R.AMBIGUOUS_CAP, 'choose another seed (batchnorm_ref.SEED_BUMP)'
        xhat, d = R.emulate_terms(x32, dy32, mu32, sig32, gamma32, beta32, relu)
        if relu:       # the f32 mask differs from the f64 one on ambiguous elements only
            assert not np.any(((d != 0) != (bw.dyp != 0)) & (dy32 != 0) & ~bw.amb)
        gb, gg = R.emulate_sums_f64(xhat, d)
        assert max(bw.sums_ratio_f64(gb.astype(np.float64), gg.astype(np.float64))) <= 1.0
        gb2, gg2 = R.emulate_sums_f32(xhat, d, rpw, rpi)
        assert max(bw.sums_ratio_f32(gb2.astype(np.float64), gg2.astype(np.float64), k)) <= 1.0
        for b_, g_ in ((gb, gg), (gb2, gg2)):
            dx = R.emulate_dx(xhat, d, sig32, gamma32, b_, g_, n, dt)
            assert bw.dx_ratio(dx.astype(np.float64), b_.astype(np.float64), g_.astype(np.float64), dt) <= 1.0
    # exact: integer gradients, every partial sum an integer below 2^24, in the f32 lane-and-tree order too
    if not big:
        dyi = cs['dyi']
        want = dyi.astype(np.int64).sum(0)
        xhat, d = R.emulate_terms(x32, dyi, mu32, sig32, gamma32, beta32, 0)
        assert np.array_equal(R.emulate_sums_f32(xhat, d, rpw, rpi)[0].astype(np.int64), want)
        assert np.array_equal(R.emulate_sums_f64(xhat, d)[0].astype(np.int64), want)
