"""Every BatchNorm kernel form of csrc/bn.hip, per element against the f64 restatement of tests/batchnorm_ref.py, at the
row and channel counts where the shared row loop changes path (batchnorm_ref.shapes), through the C entry points of
include/lidal_amd.h.  Every output and every workspace lies between guard bands (tests/guarded_ws.py); every call runs
twice and must give the same bits.  The bounds are derived in batchnorm_ref.py; the largest error of each form, as a
fraction of its bound, is printed by the last test of the file."""
import numpy as np
import pytest
import torch

import batchnorm_ref as R
from guarded_ws import FILL, Guarded

pytestmark = pytest.mark.gpu

DEV = 'cuda'
CASES = R.all_cases(with_one_row=True)
TDT = {'f32': torch.float32, 'bf16': torch.bfloat16}
WORST = {}


@pytest.fixture(autouse=True)
def _nothing_runs_on_a_device_that_reported_an_error():
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:           # a fault is sticky: the tests behind it would only repeat it
        pytest.exit('the device reported an error, no further test is started on it: %s' % e, returncode=3)


def _note(form, ratio):
    WORST[form] = max(WORST.get(form, 0.0), float(ratio))
    return ratio


def _lib():
    from lidal_amd import backend as B
    return B, B.lib()


def _ok(L, rc):
    assert rc == 0, L.lidal_last_error().decode()


class Bufs:
    """Typed tensors between guard bands, 0xA5-filled."""

    def __init__(self):
        self.g = Guarded()

    def new(self, shape, dtype=torch.float32):
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        count = int(np.prod(shape))
        t = self.g(count * torch.empty(0, dtype=dtype).element_size())
        return t.view(dtype).view(shape)

    def put(self, src):
        t = self.new(src.shape, src.dtype)
        t.copy_(src)
        return t

    def check(self):
        self.g.check()


def _untouched(t):
    return bool((t.contiguous().view(torch.uint8) == FILL).all())


def _up(a, dt=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t.to(TDT[dt]) if dt is not None else t


def _twice(fn):
    a, b = fn(), fn()
    torch.cuda.synchronize()
    for u, v in zip(a, b):
        if u is not None:
            assert torch.equal(u.view(torch.uint8) if u.dtype == torch.bfloat16 else u,
                               v.view(torch.uint8) if v.dtype == torch.bfloat16 else v), 'a second run gave other bits'
    return a


class Ops:
    """One (dtype, n, c): its operands on the device (in the dtype, and in f64 for the reference)."""

    def __init__(self, case):
        self.dt, self.n, self.c = case
        self.cs = R.Case(*case)
        self.B, self.L = _lib()
        self.code = self.B.dtype_code(TDT[self.dt])
        self.vec = R.VEC[self.dt]
        self.nb = int(self.L.lidal_bn_workspace_bytes(self.n, self.c))
        self.bufs = Bufs()
        self._t, self._d = {}, {}

    def t(self, name):          # the operand in its dtype (per-channel arrays: f32)
        if name not in self._t:
            a = self.cs[name]
            self._t[name] = _up(a, self.dt if a.ndim == 2 else None)
        return self._t[name]

    def d(self, name):          # ... in f64
        if name not in self._d:
            self._d[name] = self.t(name).double()
        return self._d[name]

    def stats(self, name='x'):
        """The f64 statistics of an operand and their f32 roundings (what a forward pass saves)."""
        key = 'stats:' + name
        if key not in self._d:
            mean, var, unb, inv = R.batch_stats(self.d(name), xp=R.TH)
            self._d[key] = (mean, var, unb, inv, mean.float().contiguous(), inv.float().contiguous())
        return self._d[key]

    def ptr(self, t):
        return None if t is None else t.data_ptr()

    def stream(self):
        return self.B.stream()

    def finish(self, fused_used=True):
        self.bufs.check()
        if fused_used:
            assert self.L.lidal_bn_check_device() == 0, self.L.lidal_last_error().decode()


def _check_forward(o, got, relu, res, mean_ref, unb_ref, inv_ref, form, mean_bar=True):
    y, mean, inv, rm, rv, nbt = got
    em, ei = R.stats_ulps(mean, inv, mean_ref, inv_ref, xp=R.TH)
    print('%s %s-%dx%d relu=%d res=%d: mean %.3f ulp, invstd %.3f ulp' % (form, o.dt, o.n, o.c, relu, res is not None, em, ei))
    if mean_bar:
        assert _note(form + ': save_mean, ulp / 1', em) <= 1.0
    assert _note(form + ': save_invstd, ulp / 2', ei / 2.0) <= 1.0
    cs = o.cs
    e1 = R.running_ulps(rm.cpu().numpy(), cs['rm0'], mean_ref.cpu().numpy())
    e2 = R.running_ulps(rv.cpu().numpy(), cs['rv0'], unb_ref.cpu().numpy())
    assert _note(form + ': running statistics, ulp / 2', max(e1, e2) / 2.0) <= 1.0
    assert int(nbt.item()) == 6
    ratio, _ = R.forward_ratio(y.double(), o.d('x'), mean.double(), inv.double(), o.d('gamma'), o.d('beta'), relu,
                               None if res is None else o.d('res'), o.dt, xp=R.TH)
    print('   y: %.3f of its bound' % ratio)
    assert _note(form + ': y', ratio) <= 1.0


VARIANTS = ((0, False), (1, False), (0, True), (3, True))


@pytest.mark.parametrize('case', CASES, ids=R.case_id)
def test_train_forward_own_statistics(case):
    o = Ops(case)
    L, n, c = o.L, o.n, o.c
    mean_ref, var_ref, unb_ref, inv_ref = o.stats()[:4]
    if n == 1:
        assert bool((var_ref == 0).all())
    for relu, with_res in VARIANTS:
        res = o.t('res') if with_res else None

        def run():
            b = o.bufs
            y, mean, inv = b.new((n, c), TDT[o.dt]), b.new(c), b.new(c)
            rm, rv, nbt = b.put(o.t('rm0')), b.put(o.t('rv0')), b.new(1, torch.int64)
            nbt.fill_(5)
            ws = b.new(o.nb, torch.uint8)
            _ok(L, L.lidal_bn_train_fwd(o.ptr(o.t('x')), o.code, n, c, o.ptr(o.t('gamma')), o.ptr(o.t('beta')), R.EPS, R.MOMENTUM,
                                        o.ptr(rm), o.ptr(rv), o.ptr(nbt), relu, o.ptr(res), o.ptr(y), o.ptr(mean), o.ptr(inv),
                                        o.ptr(ws), o.nb, o.stream()))
            return y, mean, inv, rm, rv, nbt
        # (save_mean has a test of its own below: test_own_statistics_save_mean_within_one_ulp)
        _check_forward(o, _twice(run), relu, res, mean_ref, unb_ref, inv_ref, 'train_fwd', mean_bar=False)
    o.finish(False)


@pytest.mark.parametrize('case', CASES, ids=R.case_id)
def test_own_statistics_save_mean_within_one_ulp(case):
    """save_mean of lidal_bn_train_fwd within 1 ulp of the f64 mean.

    The statistics pass shifts every value by the slab's first row K.  Between two f32 values x - K rounds in f32
    (2^-24 |x - K| per term); while the mean was taken from the sum of those rounded differences, a column whose mean is
    small beside its spread showed it: 4 - 512 ulp on two rows (2 x 1024: 512), 5 - 318 ulp on 31 - 65 rows (33 x 516:
    318, 33 x 256: 186, 63 x 256: 103), 0.6 ulp at most from 8191 rows on, where the error averages out; bf16 rows were
    inside 0.5 ulp, their differences being exact in f32.  bn_stats_partial_kernel now takes the mean of f32 rows from
    a sum of the differences in f64: 0.50 ulp on every shape.  M2 is still summed over the f32 differences about their
    own mean (the exact M2 of values 2^-24 away from the data): invstd stays inside its 2 ulp (1.46 at most)."""
    o = Ops(case)
    L, n, c = o.L, o.n, o.c
    mean_ref, _, _, inv_ref = o.stats()[:4]
    b = o.bufs
    y, mean, inv, ws = b.new((n, c), TDT[o.dt]), b.new(c), b.new(c), b.new(o.nb, torch.uint8)
    _ok(L, L.lidal_bn_train_fwd(o.ptr(o.t('x')), o.code, n, c, o.ptr(o.t('gamma')), o.ptr(o.t('beta')), R.EPS, R.MOMENTUM,
                                None, None, None, 0, None, o.ptr(y), o.ptr(mean), o.ptr(inv), o.ptr(ws), o.nb, o.stream()))
    em, _ = R.stats_ulps(mean, inv, mean_ref, inv_ref, xp=R.TH)
    print('save_mean %s: %.3f ulp' % (R.case_id(case), em))
    o.finish(False)
    assert _note('train_fwd: save_mean, ulp / 1', em) <= 1.0


@pytest.mark.parametrize('case', CASES, ids=R.case_id)
def test_train_forward_tile_statistics_fused_and_apart(case):
    o = Ops(case)
    L, n, c = o.L, o.n, o.c
    tiles = R._tile_triples(o.t('x'))
    n_tiles = tiles.shape[0]
    assert n_tiles == -(-n // R.TILE)
    mean_ref, _, unb_ref, inv_ref = R.tile_merge(tiles, c, xp=R.TH)
    outs = {}
    try:
        for fused in (1, 0):
            L.lidal_bn_set_fused(fused)
            for relu, with_res in VARIANTS:
                res = o.t('res') if with_res else None

                def run():
                    b = o.bufs
                    y, mean, inv = b.new((n, c), TDT[o.dt]), b.new(c), b.new(c)
                    rm, rv, nbt = b.put(o.t('rm0')), b.put(o.t('rv0')), b.new(1, torch.int64)
                    nbt.fill_(5)
                    _ok(L, L.lidal_bn_train_fwd_tiles(o.ptr(o.t('x')), o.code, n, c, o.ptr(o.t('gamma')), o.ptr(o.t('beta')), R.EPS,
                                                      R.MOMENTUM, o.ptr(rm), o.ptr(rv), o.ptr(nbt), relu, o.ptr(res), o.ptr(y),
                                                      o.ptr(mean), o.ptr(inv), o.ptr(tiles), n_tiles, o.stream()))
                    return y, mean, inv, rm, rv, nbt
                got = _twice(run)
                _check_forward(o, got, relu, res, mean_ref, unb_ref, inv_ref, 'train_fwd_tiles(fused=%d)' % fused)
                outs[(fused, relu, with_res)] = got
            torch.cuda.synchronize()
            assert L.lidal_bn_check_device() == 0, L.lidal_last_error().decode()
    finally:
        L.lidal_bn_set_fused(1)
    o.finish()


@pytest.mark.parametrize('case', CASES, ids=R.case_id)
def test_eval_forward(case):
    """y = (x - running_mean) / sqrt(running_var + eps) * gamma + beta: sigma in f32 costs three more roundings."""
    o = Ops(case)
    L, n, c = o.L, o.n, o.c
    rmean, rvar = o.t('rm0'), o.t('rv0')
    sig = 1.0 / torch.sqrt(rvar.double() + float(np.float32(R.EPS)))
    for relu in (0, 1):
        def run():
            y = o.bufs.new((n, c), TDT[o.dt])
            _ok(L, L.lidal_bn_eval_fwd(o.ptr(o.t('x')), o.code, n, c, o.ptr(o.t('gamma')), o.ptr(o.t('beta')), o.ptr(rmean),
                                       o.ptr(rvar), R.EPS, relu, o.ptr(y), o.stream()))
            return (y,)
        y, = _twice(run)
        ratio, _ = R.forward_ratio(y.double(), o.d('x'), rmean.double(), sig, o.d('gamma'), o.d('beta'), relu, None, o.dt,
                                   xp=R.TH, var_in=True)
        print('eval_fwd %s relu=%d: %.3f of its bound' % (R.case_id(case), relu, ratio))
        assert _note('eval_fwd: y', ratio) <= 1.0
    o.finish(False)


@pytest.mark.parametrize('c', [1, 255, 256, 257, 2048])
def test_fold(c):
    """scale = gamma / sqrt(var + eps), shift = beta - mean * scale against f64.  scale: the sum, the root (which halves
    the error it is handed), the division and the product: 3.5 roundings, held to 3 ulp.  shift: 3 ulp at the largest of
    |beta|, |mean scale| and the result (its product and difference round there), plus the 3.5u |mean scale| that scale's
    own error hands on."""
    B, L = _lib()
    rng = np.random.default_rng(c)
    gamma, beta, mean = (rng.standard_normal(c).astype(np.float32) for _ in range(3))
    var = (rng.random(c, dtype=np.float32) + np.float32(0.01))
    var[0] = 0.0
    for with_affine in (True, False):
        bufs = Bufs()
        g, b = (_up(gamma), _up(beta)) if with_affine else (None, None)
        m, v = _up(mean), _up(var)
        scale, shift = bufs.new(c), bufs.new(c)
        _ok(L, L.lidal_bn_fold(B.ptr(g), B.ptr(b), B.ptr(m), B.ptr(v), R.EPS, c, B.ptr(scale), B.ptr(shift), B.stream()))
        bufs.check()
        g64 = gamma.astype(np.float64) if with_affine else np.ones(c)
        b64 = beta.astype(np.float64) if with_affine else np.zeros(c)
        sc = g64 / np.sqrt(var.astype(np.float64) + np.float64(np.float32(R.EPS)))
        sh = b64 - mean.astype(np.float64) * sc
        e_sc = np.abs(scale.cpu().numpy().astype(np.float64) - sc) / R.ulp32(sc)
        mag = np.maximum(np.maximum(np.abs(b64), np.abs(mean * sc)), np.abs(sh))
        tol = 3.0 * R.ulp32(mag) + 3.5 * R.U * np.abs(mean * sc)
        e_sh = np.abs(shift.cpu().numpy().astype(np.float64) - sh) / tol
        print('fold c=%d affine=%d: scale %.3f ulp, shift %.3f of its bound' % (c, with_affine, e_sc.max(), e_sh.max()))
        assert _note('fold: scale, ulp / 3', e_sc.max() / 3.0) <= 1.0
        assert _note('fold: shift', e_sh.max()) <= 1.0


def _embed(dy, stride):
    """dy as the last c columns of a [n, stride] matrix whose other columns hold NaN."""
    n, c = dy.shape
    if stride == c:
        return dy.contiguous()
    wide = torch.full((n, stride), float('nan'), dtype=dy.dtype, device=dy.device)
    wide[:, stride - c:] = dy
    return wide[:, stride - c:]


def _check_backward(o, bw, got, sums, form, k=None, exact=None):
    dx, gg, gb = got
    gb64, gg64 = gb.double(), gg.double()
    assert bw.ambiguous_share() <= R.AMBIGUOUS_CAP
    if exact is not None:
        assert torch.equal(gb64, exact), form + ': grad_beta of integer gradients is not the integer column sum'
    if isinstance(sums, str) and sums == 'f64':
        rb, rg = bw.sums_ratio_f64(gb64, gg64)
    elif isinstance(sums, str):
        rb, rg = bw.sums_ratio_f32(gb64, gg64, k)
    else:
        rb = R.merged_ulps(gb, sums, 0, xp=R.TH)
        rg = R.merged_ulps(gg, sums, 1, xp=R.TH)
    assert _note(form + ': grad_beta', rb) <= 1.0, (form, rb)
    assert _note(form + ': grad_gamma', rg) <= 1.0, (form, rg)
    if dx is not None:
        rd = bw.dx_ratio(dx.double(), gb64, gg64, o.dt)
        assert _note(form + ': dx', rd) <= 1.0, (form, rd)
    else:
        rd = float('nan')
    print('%s %s-%dx%d: grad_beta %.3f grad_gamma %.3f dx %.3f of their bounds' % (form, o.dt, o.n, o.c, rb, rg, rd))


@pytest.mark.parametrize('case', CASES, ids=R.case_id)
def test_backward(case):
    """lidal_bn_bwd: f64 partial sums (f32; bf16 with slab sums off) and f32 slab sums (bf16), merged inside the dx launch
    and apart, with and without the ReLU mask, dy contiguous and as the last columns of a wider matrix, dx = NULL, and
    integer gradients whose column sums must come out exactly."""
    o = Ops(case)
    L, n, c = o.L, o.n, o.c
    mu32, sig32 = o.stats()[4:]
    mu, sig = mu32.double(), sig32.double()
    rb = c * R.ESIZE[o.dt]
    k = R.chain_length(R.rows_per_wg_ew(n, rb), R.rows_per_sweep(c, o.dt))
    strides = (c, c + o.vec, 2 * c)
    dys = {s: _embed(o.t('dy'), s) for s in strides}
    dyi = o.t('dyi')
    want_i = o.d('dyi').sum(0)
    bws = {relu: R.Backward(o.d('x'), o.d('dy'), mu, sig, o.d('gamma'), o.d('beta'), relu, xp=R.TH) for relu in (0, 1)}
    bwi = R.Backward(o.d('x'), o.d('dyi'), mu, sig, o.d('gamma'), o.d('beta'), 0, xp=R.TH)

    def launch(dy, stride, relu, want_dx=True):
        def run():
            b = o.bufs
            dx = b.new((n, c), TDT[o.dt]) if want_dx else None
            gg, gb, ws = b.new(c), b.new(c), b.new(o.nb, torch.uint8)
            _ok(L, L.lidal_bn_bwd(o.ptr(o.t('x')), o.ptr(dy), stride, o.code, n, c, o.ptr(o.t('gamma')), o.ptr(o.t('beta')), relu,
                                  o.ptr(mu32), o.ptr(sig32), o.ptr(dx), o.ptr(gg), o.ptr(gb), o.ptr(ws), o.nb, o.stream()))
            return dx, gg, gb
        return _twice(run)
    was = L.lidal_bn_set_slab_sums(1)
    try:
        for slab in ((1, 0) if o.dt == 'bf16' else (1,)):
            L.lidal_bn_set_slab_sums(slab)
            sums = 'f32' if (o.dt == 'bf16' and slab) else 'f64'
            for fused in (1, 0):
                L.lidal_bn_set_fused(fused)
                form = 'bn_bwd(%s sums, fused=%d)' % (sums, fused)
                for relu in (0, 1):
                    first = None
                    for s in strides:
                        got = launch(dys[s], s, relu)
                        if first is None:
                            first = got
                            _check_backward(o, bws[relu], got, sums, form, k)
                        else:           # the same values behind another row stride: the same bits
                            assert all(torch.equal(a.float(), b_.float()) for a, b_ in zip(first, got)), (form, s)
                    _check_backward(o, bws[relu], launch(dys[c], c, relu, want_dx=False), sums, form + ', dx = NULL', k)
                _check_backward(o, bwi, launch(dyi, c, 0), sums, form + ', integers', k, exact=want_i)
            torch.cuda.synchronize()
            assert L.lidal_bn_check_device() == 0, L.lidal_last_error().decode()
    finally:
        L.lidal_bn_set_fused(1)
        L.lidal_bn_set_slab_sums(was)
    o.finish()


def _tile_sums(bw, rows):
    """f32 (sum dy', sum dy' xhat) per `rows` rows, [c][tiles][2], from the f64 terms."""
    n, c = bw.tb.shape
    tiles = -(-n // rows)

    def per_tile(t):
        if tiles * rows != n:
            t = torch.cat([t, torch.zeros(tiles * rows - n, c, dtype=t.dtype, device=t.device)])
        return t.view(tiles, rows, c).sum(1).t()
    return torch.stack([per_tile(bw.tb), per_tile(bw.tg)], 2).float().contiguous()


@pytest.mark.parametrize('case', CASES, ids=R.case_id)
def test_backward_from_tile_sums(case):
    """lidal_bn_bwd_tiles: the sums per 128 rows are handed in (f32, [c][tiles][2]); their merge in f64 is held to one
    ulp of the f64 sum of the same pairs, dx to its bound."""
    o = Ops(case)
    L, n, c = o.L, o.n, o.c
    mu32, sig32 = o.stats()[4:]
    mu, sig = mu32.double(), sig32.double()
    try:
        for fused in (1, 0):
            L.lidal_bn_set_fused(fused)
            for relu, name in ((0, 'dy'), (1, 'dy'), (0, 'dyi')):
                bw = R.Backward(o.d('x'), o.d(name), mu, sig, o.d('gamma'), o.d('beta'), relu, xp=R.TH)
                ts = o.bufs.put(_tile_sums(bw, R.TILE))
                for want_dx in (True, False):
                    def run():
                        b = o.bufs
                        dx = b.new((n, c), TDT[o.dt]) if want_dx else None
                        gg, gb = b.new(c), b.new(c)
                        _ok(L, L.lidal_bn_bwd_tiles(o.ptr(o.t('x')), o.ptr(o.t(name)), c, o.code, n, c, o.ptr(o.t('gamma')),
                                                    o.ptr(o.t('beta')), relu, o.ptr(mu32), o.ptr(sig32), o.ptr(dx), o.ptr(gg),
                                                    o.ptr(gb), o.ptr(ts), ts.shape[1], o.stream()))
                        return dx, gg, gb
                    _check_backward(o, bw, _twice(run), ts, 'bn_bwd_tiles(fused=%d)' % fused,
                                    exact=o.d('dyi').sum(0) if name == 'dyi' else None)
            torch.cuda.synchronize()
            assert L.lidal_bn_check_device() == 0, L.lidal_last_error().decode()
    finally:
        L.lidal_bn_set_fused(1)
    o.finish()


def _tail_operands(o, integers):
    """(g, gm reference, per BatchNorm: x name, gamma, beta, saved statistics, Backward over the masked gradient)"""
    gname = 'dyi' if integers else 'dy'
    out = o.t('out')
    gm_ref = torch.where(out > 0, o.t(gname), torch.zeros_like(out))
    norms = []
    for xname, gname_, bname in (('x', 'gamma', 'beta'), ('xb', 'beta', 'gamma')):
        mu32, sig32 = o.stats(xname)[4:]
        bw = R.Backward(o.d(xname), gm_ref.double(), mu32.double(), sig32.double(), o.d(gname_), o.d(bname), 0, xp=R.TH)
        norms.append((xname, o.t(gname_), o.t(bname), mu32, sig32, bw))
    return o.t(gname), gm_ref, norms


@pytest.mark.parametrize('case', CASES, ids=R.case_id)
def test_block_tail_with_f64_partial_sums(case):
    """lidal_add_relu_bwd_bn_sums + lidal_bn_bwd_from_sums, one BatchNorm and two: gm = g * (out > 0) exactly, the sums
    and dx against the reference (no ReLU inside the BatchNorm: nothing is ambiguous)."""
    o = Ops(case)
    L, n, c = o.L, o.n, o.c
    try:
        for integers in (False, True):
            g, gm_ref, norms = _tail_operands(o, integers)
            for fused in (1, 0):
                L.lidal_bn_set_fused(fused)
                for dual in (True, False):
                    (xa, _, _, mua, siga, _), (xb, _, _, mub, sigb, _) = norms

                    def run():
                        b = o.bufs
                        gm, pa = b.new((n, c), TDT[o.dt]), b.new(o.nb, torch.uint8)
                        pb = b.new(o.nb, torch.uint8) if dual else None
                        _ok(L, L.lidal_add_relu_bwd_bn_sums(o.ptr(o.t('out')), o.ptr(g), o.ptr(gm), o.code, n, c, o.ptr(o.t(xa)),
                                                            o.ptr(mua), o.ptr(siga), o.ptr(pa), o.ptr(o.t(xb)) if dual else None,
                                                            o.ptr(mub) if dual else None, o.ptr(sigb) if dual else None,
                                                            o.ptr(pb), o.nb, o.stream()))
                        outs = [gm]
                        for (xn, ga, be, mu32, sig32, _), part in zip(norms[:2 if dual else 1], (pa, pb)):
                            dx, gg, gb = b.new((n, c), TDT[o.dt]), b.new(c), b.new(c)
                            _ok(L, L.lidal_bn_bwd_from_sums(o.ptr(o.t(xn)), o.ptr(gm), c, o.code, n, c, o.ptr(ga), o.ptr(be), 0,
                                                            o.ptr(mu32), o.ptr(sig32), o.ptr(dx), o.ptr(gg), o.ptr(gb), o.ptr(part),
                                                            o.nb, o.stream()))
                            outs += [dx, gg, gb]
                        return outs
                    got = _twice(run)
                    assert torch.equal(got[0].float(), gm_ref.float())
                    for i, nm in enumerate(norms[:2 if dual else 1]):
                        _check_backward(o, nm[5], got[1 + 3 * i:4 + 3 * i], 'f64',
                                        'add_relu_bwd_bn_sums(%s, fused=%d)' % ('dual' if dual else 'single', fused),
                                        exact=gm_ref.double().sum(0) if integers else None)
            torch.cuda.synchronize()
            assert L.lidal_bn_check_device() == 0, L.lidal_last_error().decode()
    finally:
        L.lidal_bn_set_fused(1)
    o.finish()


@pytest.mark.parametrize('case', CASES, ids=R.case_id)
def test_block_tail_with_f32_slab_sums(case):
    """lidal_add_relu_bwd_bn_tile_sums + lidal_bn_bwd_tiles with n_parts = lidal_bn_tail_parts: gm exactly, every slab's
    pair and the merged gradients inside the f32 chain bound, dx inside its bound."""
    o = Ops(case)
    L, n, c = o.L, o.n, o.c
    rb = c * R.ESIZE[o.dt]
    rpw, rpi = R.rows_per_wg_ew(n, rb), R.rows_per_sweep(c, o.dt)
    parts = int(L.lidal_bn_tail_parts(n, c, o.code))
    assert parts == R.nslabs_ew(n, rb) == -(-n // rpw)
    k = R.chain_length(rpw, rpi)
    try:
        for integers in (False, True):
            g, gm_ref, norms = _tail_operands(o, integers)
            for fused in (1, 0):
                L.lidal_bn_set_fused(fused)
                for dual in (True, False):
                    (xa, _, _, mua, siga, _), (xb, _, _, mub, sigb, _) = norms

                    def run():
                        b = o.bufs
                        gm, sa = b.new((n, c), TDT[o.dt]), b.new((c, parts, 2))
                        sb = b.new((c, parts, 2)) if dual else None
                        _ok(L, L.lidal_add_relu_bwd_bn_tile_sums(o.ptr(o.t('out')), o.ptr(g), o.ptr(gm), o.code, n, c,
                                                                 o.ptr(o.t(xa)), o.ptr(mua), o.ptr(siga), o.ptr(sa),
                                                                 o.ptr(o.t(xb)) if dual else None, o.ptr(mub) if dual else None,
                                                                 o.ptr(sigb) if dual else None, o.ptr(sb), parts, o.stream()))
                        outs = [gm]
                        for (xn, ga, be, mu32, sig32, _), sums in zip(norms[:2 if dual else 1], (sa, sb)):
                            dx, gg, gb = b.new((n, c), TDT[o.dt]), b.new(c), b.new(c)
                            _ok(L, L.lidal_bn_bwd_tiles(o.ptr(o.t(xn)), o.ptr(gm), c, o.code, n, c, o.ptr(ga), o.ptr(be), 0,
                                                        o.ptr(mu32), o.ptr(sig32), o.ptr(dx), o.ptr(gg), o.ptr(gb), o.ptr(sums),
                                                        parts, o.stream()))
                            outs += [dx, gg, gb, sums]
                        return outs
                    got = _twice(run)
                    assert torch.equal(got[0].float(), gm_ref.float())
                    form = 'add_relu_bwd_bn_tile_sums(%s, fused=%d)' % ('dual' if dual else 'single', fused)
                    for i, nm in enumerate(norms[:2 if dual else 1]):
                        dx, gg, gb, sums = got[1 + 4 * i:5 + 4 * i]
                        bw = nm[5]
                        # every slab's pair: the same chain bound on the slab's own sum of magnitudes
                        ref = _tile_sums(bw, rpw)                       # (f32-rounded f64 slab sums: only their layout is used)
                        pad = parts * rpw - n

                        def slabs(t):
                            t = torch.cat([t, torch.zeros(pad, c, dtype=t.dtype, device=t.device)]) if pad else t
                            return t.view(parts, rpw, c).sum(1).t()
                        assert ref.shape == sums.shape
                        for j, term in enumerate((bw.tb, bw.tg)):
                            err = (sums[:, :, j].double() - slabs(term)).abs()
                            bound = (k + 3) * R.U * slabs(term.abs())
                            assert _note(form + ': slab sums', R._ratio(err, bound, R.TH)) <= 1.0
                        _check_backward(o, bw, (dx, gg, gb), 'f32', form, k,
                                        exact=gm_ref.double().sum(0) if integers else None)
            torch.cuda.synchronize()
            assert L.lidal_bn_check_device() == 0, L.lidal_last_error().decode()
    finally:
        L.lidal_bn_set_fused(1)
    o.finish()


@pytest.mark.parametrize('case', CASES, ids=R.case_id)
def test_colsum(case):
    """lidal_colsum: exact on integers; on random data f64 sums rounded once, u sum|x|."""
    o = Ops(case)
    L, n, c = o.L, o.n, o.c
    nb = o.nb + 12 * c
    for name in ('dyi', 'x'):
        def run():
            out, ws = o.bufs.new(c), o.bufs.new(nb, torch.uint8)
            _ok(L, L.lidal_colsum(o.ptr(o.t(name)), o.code, n, c, o.ptr(out), o.ptr(ws), nb, o.stream()))
            return (out,)
        out, = _twice(run)
        want = o.d(name).sum(0)
        if name == 'dyi':
            assert torch.equal(out.double(), want)
        else:
            ratio = R._ratio((out.double() - want).abs(), R.U * o.d(name).abs().sum(0), R.TH)
            print('colsum %s: %.3f of its bound' % (R.case_id(case), ratio))
            assert _note('colsum', ratio) <= 1.0
    o.finish(False)


def _off_grid(bufs, src):
    """src behind one float of an allocation: 4-byte aligned only, a sentinel float on either side."""
    c = src.numel()
    buf = bufs.new(c + 2)
    assert buf.data_ptr() % 16 == 0
    view = buf[1:c + 1]
    view.copy_(src)
    return buf, view


@pytest.mark.parametrize('case', [(dt, n, c) for dt in ('f32', 'bf16') for n, c in R.shapes(dt) if n in (33, 8193)],
                         ids=R.case_id)
def test_per_channel_arrays_off_the_16_byte_grid(case):
    """gamma, beta, save_mean and save_invstd as views one float into their allocations (load_channels' scalar branch):
    the forward-tiles, backward and eval forms give the bits they give on aligned arrays, and the floats on either side
    of each view are not written."""
    o = Ops(case)
    L, n, c = o.L, o.n, o.c
    mu32, sig32 = o.stats()[4:]
    tiles = R._tile_triples(o.t('x'))
    results = []
    sentinels = []
    try:
        for off in (False, True):
            L.lidal_bn_set_fused(1)
            arrs = {}
            for name, src in (('gamma', o.t('gamma')), ('beta', o.t('beta')), ('mu', mu32), ('sig', sig32),
                              ('rm', o.t('rm0')), ('rv', o.t('rv0')), ('mean_out', mu32), ('inv_out', sig32)):
                if off:
                    buf, view = _off_grid(o.bufs, src)
                    sentinels.append(buf)
                    arrs[name] = view
                else:
                    arrs[name] = o.bufs.put(src)
                    assert arrs[name].data_ptr() % 16 == 0
            got = []
            for fused in (1, 0):
                L.lidal_bn_set_fused(fused)
                y = o.bufs.new((n, c), TDT[o.dt])
                rm, rv = o.bufs.put(o.t('rm0')), o.bufs.put(o.t('rv0'))
                _ok(L, L.lidal_bn_train_fwd_tiles(o.ptr(o.t('x')), o.code, n, c, o.ptr(arrs['gamma']), o.ptr(arrs['beta']), R.EPS,
                                                  R.MOMENTUM, o.ptr(rm), o.ptr(rv), None, 1, None, o.ptr(y), o.ptr(arrs['mean_out']),
                                                  o.ptr(arrs['inv_out']), o.ptr(tiles), tiles.shape[0], o.stream()))
                got += [y, arrs['mean_out'].clone(), arrs['inv_out'].clone()]
                for slab in ((1, 0) if o.dt == 'bf16' else (1,)):
                    was = L.lidal_bn_set_slab_sums(slab)
                    dx, gg, gb, ws = o.bufs.new((n, c), TDT[o.dt]), o.bufs.new(c), o.bufs.new(c), o.bufs.new(o.nb, torch.uint8)
                    _ok(L, L.lidal_bn_bwd(o.ptr(o.t('x')), o.ptr(o.t('dy')), c, o.code, n, c, o.ptr(arrs['gamma']),
                                          o.ptr(arrs['beta']), 1, o.ptr(arrs['mu']), o.ptr(arrs['sig']), o.ptr(dx), o.ptr(gg),
                                          o.ptr(gb), o.ptr(ws), o.nb, o.stream()))
                    L.lidal_bn_set_slab_sums(was)
                    got += [dx, gg, gb]
            y = o.bufs.new((n, c), TDT[o.dt])
            _ok(L, L.lidal_bn_eval_fwd(o.ptr(o.t('x')), o.code, n, c, o.ptr(arrs['gamma']), o.ptr(arrs['beta']), o.ptr(arrs['rm']),
                                       o.ptr(arrs['rv']), R.EPS, 1, o.ptr(y), o.stream()))
            got.append(y)
            torch.cuda.synchronize()
            results.append(got)
    finally:
        L.lidal_bn_set_fused(1)
    for a, b in zip(*results):
        assert torch.equal(a.float(), b.float())
    for buf in sentinels:
        assert _untouched(buf[:1]) and _untouched(buf[-1:]), 'a float beside an off-grid array was written'
    o.finish()


def test_grid_restatement_is_the_librarys():
    B, L = _lib()
    for dt, n, c in CASES + [('bf16', 12289, 512), ('bf16', 12288, 512), ('f32', 396662, 96)]:
        assert int(L.lidal_bn_workspace_bytes(n, c)) == R.workspace_bytes(n, c)
        assert int(L.lidal_bn_tail_parts(n, c, B.dtype_code(TDT[dt]))) == R.nslabs_ew(n, c * R.ESIZE[dt])


@pytest.mark.parametrize('dt', ['f32', 'bf16'])
def test_refusals_leave_every_output_untouched(dt):
    """Each refused call returns non-zero, names its reason in lidal_last_error() and writes nothing."""
    B, L = _lib()
    vec = R.VEC[dt]
    n, c = 65, 12 * vec
    code = B.dtype_code(TDT[dt])
    bufs = Bufs()
    td = TDT[dt]
    x = torch.ones(n, 2 * c, dtype=td, device=DEV)
    chan = torch.ones(4 * c, device=DEV)
    tiles = torch.ones(4 * c * 4 * 3, device=DEV)
    outs = {k: bufs.new((n, 2 * c), td) for k in ('y', 'dx', 'gm')}
    outs.update({k: bufs.new(4 * c) for k in ('mean', 'inv', 'gg', 'gb', 'rm', 'rv')})
    outs['nbt'] = bufs.new(1, torch.int64)
    nb = int(L.lidal_bn_workspace_bytes(n, 2 * c)) + 24 * c
    outs['ws'], outs['ws2'] = bufs.new(nb, torch.uint8), bufs.new(nb, torch.uint8)
    outs['sums'], outs['sums2'] = bufs.new((4 * c, 8, 2)), bufs.new((4 * c, 8, 2))
    p = {k: v.data_ptr() for k, v in outs.items()}
    X, CH, TL, S = x.data_ptr(), chan.data_ptr(), tiles.data_ptr(), B.stream()

    def fwd(n_=n, c_=c, code_=code, ws=None):
        ws = int(L.lidal_bn_workspace_bytes(n_, c_)) if ws is None else ws
        return L.lidal_bn_train_fwd(X, code_, n_, c_, CH, CH, R.EPS, R.MOMENTUM, p['rm'], p['rv'], p['nbt'], 0, None, p['y'],
                                    p['mean'], p['inv'], p['ws'], ws, S)

    def fwd_tiles(n_=n, c_=c, code_=code, n_tiles=1):
        return L.lidal_bn_train_fwd_tiles(X, code_, n_, c_, CH, CH, R.EPS, R.MOMENTUM, p['rm'], p['rv'], p['nbt'], 0, None,
                                          p['y'], p['mean'], p['inv'], TL, n_tiles, S)

    def ev(n_=n, c_=c, code_=code):
        return L.lidal_bn_eval_fwd(X, code_, n_, c_, CH, CH, CH, CH, R.EPS, 0, p['y'], S)

    def bwd(n_=n, c_=c, code_=code, ws=None, stride=None):
        ws = int(L.lidal_bn_workspace_bytes(n_, c_)) if ws is None else ws
        return L.lidal_bn_bwd(X, X, c_ if stride is None else stride, code_, n_, c_, CH, CH, 0, CH, CH, p['dx'], p['gg'], p['gb'],
                              p['ws'], ws, S)

    def bwd_tiles(n_=n, c_=c, code_=code, stride=None, n_tiles=1):
        return L.lidal_bn_bwd_tiles(X, X, c_ if stride is None else stride, code_, n_, c_, CH, CH, 0, CH, CH, p['dx'], p['gg'],
                                    p['gb'], TL, n_tiles, S)

    def tail(n_=n, c_=c, code_=code, ws=None):
        ws = int(L.lidal_bn_workspace_bytes(n_, c_)) if ws is None else ws
        return L.lidal_add_relu_bwd_bn_sums(X, X, p['gm'], code_, n_, c_, X, CH, CH, p['ws'], X, CH, CH, p['ws2'], ws, S)

    def from_sums(n_=n, c_=c, code_=code, ws=None, stride=None):
        ws = int(L.lidal_bn_workspace_bytes(n_, c_)) if ws is None else ws
        return L.lidal_bn_bwd_from_sums(X, X, c_ if stride is None else stride, code_, n_, c_, CH, CH, 0, CH, CH, p['dx'], p['gg'],
                                        p['gb'], p['ws'], ws, S)

    def tail_tiles(n_=n, c_=c, code_=code, parts=None):
        parts = int(L.lidal_bn_tail_parts(n_, c_, code_ if code_ in (0, 1) else code)) if parts is None else parts
        return L.lidal_add_relu_bwd_bn_tile_sums(X, X, p['gm'], code_, n_, c_, X, CH, CH, p['sums'], X, CH, CH, p['sums2'],
                                                 parts, S)

    def colsum(n_=n, c_=c, code_=code, ws=None):
        ws = int(L.lidal_bn_workspace_bytes(n_, c_)) + 12 * c_ if ws is None else ws
        return L.lidal_colsum(X, code_, n_, c_, p['gg'], p['ws'], ws, S)
    every = (fwd, fwd_tiles, ev, bwd, bwd_tiles, tail, from_sums, tail_tiles, colsum)
    training = (fwd, fwd_tiles, bwd, bwd_tiles, tail, from_sums, tail_tiles, colsum)
    refused = []
    for f in every:
        refused += [(f, dict(c_=c + vec // 2), 'multiple'), (f, dict(c_=256 * vec + vec), 'multiple'), (f, dict(c_=0), 'multiple'),
                    (f, dict(code_=7), 'dtype')]
    refused += [(f, dict(n_=0), 'row') for f in training]
    for f in (bwd, bwd_tiles, from_sums):
        refused += [(f, dict(stride=c - vec), 'stride'), (f, dict(stride=c + vec // 2), 'stride')]
    refused += [(f, dict(ws=int(L.lidal_bn_workspace_bytes(n, c)) - 1), 'small') for f in (fwd, bwd, tail, from_sums)]
    refused += [(colsum, dict(ws=int(L.lidal_bn_workspace_bytes(n, c)) + 12 * c - 1), 'small')]
    parts = int(L.lidal_bn_tail_parts(n, c, code))
    refused += [(tail_tiles, dict(parts=parts + 1), 'parts'), (tail_tiles, dict(parts=parts - 1), 'parts')]
    refused += [(fwd_tiles, dict(n_tiles=0), 'tile'), (bwd_tiles, dict(n_tiles=0), 'tile')]
    for f, kw, word in refused:
        rc = f(**kw)
        msg = L.lidal_last_error().decode()
        assert rc != 0, (f.__name__, kw)
        assert word in msg, (f.__name__, kw, msg)
    assert ev(n_=0) == 0                # nothing to do is not an error for the eval form
    torch.cuda.synchronize()
    for k, v in outs.items():
        assert _untouched(v), 'a refused call wrote ' + k
    bufs.check()
    # ... and the same calls with valid arguments are accepted (the refusals above were not the operands')
    for f in every:
        assert f() == 0, (f.__name__, L.lidal_last_error().decode())
    torch.cuda.synchronize()
    bufs.check()
    assert L.lidal_bn_check_device() == 0


@pytest.mark.parametrize('what', ['n=1', 'f32 c=22', 'bf16 c=4', '3-d'])
def test_python_layer_falls_back_to_torch_where_the_kernels_do_not_apply(what):
    import lidal_amd.nn as spnn
    from lidal_amd import backend as B
    from lidal_amd.nn.functional import norm
    g = torch.Generator().manual_seed(len(what))
    shape, dtype, train = {'n=1': ((1, 32), torch.float32, False), 'f32 c=22': ((50, 22), torch.float32, True),
                           'bf16 c=4': ((50, 4), torch.bfloat16, True), '3-d': ((6, 32, 5), torch.float32, True)}[what]
    c = shape[1]
    x = torch.randn(*shape, generator=g).to(dtype)
    go = torch.randn(*shape, generator=g).to(dtype).to(DEV)
    mine, ref = spnn.BatchNorm1d(c).to(DEV), torch.nn.BatchNorm1d(c).to(DEV)
    with torch.no_grad():
        for m in (mine, ref):
            m.weight.copy_(torch.linspace(0.5, 1.5, c))
            m.bias.copy_(torch.linspace(-0.3, 0.3, c))
    mine.train(train), ref.train(train)
    assert not norm.supported(x.to(DEV), mine.weight, mine.bias)
    before = dict(B.HITS)
    if what == 'n=1':                   # torch refuses one value per channel in training: so does the fallback
        mine.train(), ref.train()
        with pytest.raises(ValueError):
            mine(x.to(DEV))
        mine.eval(), ref.eval()
    xs = [x.to(DEV).requires_grad_(True) for _ in range(2)]
    ys = [m(xi) for m, xi in zip((mine, ref), xs)]
    for y in ys:
        y.backward(go)
    torch.cuda.synchronize()
    assert torch.equal(ys[0], ys[1]) and torch.equal(xs[0].grad, xs[1].grad)
    assert torch.equal(mine.weight.grad, ref.weight.grad) and torch.equal(mine.bias.grad, ref.bias.grad)
    assert torch.equal(mine.running_mean, ref.running_mean) and torch.equal(mine.running_var, ref.running_var)
    launched = {k: v - before.get(k, 0) for k, v in B.HITS.items() if v != before.get(k, 0)}
    assert launched.get('torch_fallback:BatchNorm1d', 0) >= 1
    assert not [k for k in launched if k.startswith('bn_') or k == 'colsum'], launched


@pytest.mark.parametrize('n,c', [(2, 96), (50, 20)])
def test_smallest_supported_shapes_run_on_the_hip_path_of_the_python_layer(n, c):
    """Two rows, and f32 c = 20 (five channel groups: a multiple of 4, so norm.supported says yes)."""
    import lidal_amd.nn as spnn
    from lidal_amd import backend as B
    mine, ref = spnn.BatchNorm1d(c).to(DEV), torch.nn.BatchNorm1d(c).to(DEV)
    before = B.HITS.get('bn_train_fwd', 0)
    x = torch.randn(n, c, generator=torch.Generator().manual_seed(n)).to(DEV)
    y = mine(x)
    torch.cuda.synchronize()
    assert B.HITS.get('bn_train_fwd', 0) == before + 1
    want = ref(x)
    assert float((y - want).abs().max()) <= 1e-5 * float(want.abs().max())


def test_zz_report_of_the_largest_errors():
    """Not a check: prints the largest error seen per form as a fraction of its bound (run with -s to read it)."""
    for form in sorted(WORST):
        print('bn-edges worst %-60s %.4f' % (form, WORST[form]))
