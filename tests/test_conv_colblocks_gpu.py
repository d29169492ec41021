"""Column blocks of one row tile, paired on one XCD (csrc/conv_img.hip, tile_of_block).

A convolution wider than a workgroup's columns runs several column blocks per 128-row tile.  Since round 7 such
launches use a 1-D grid that a kernel decodes into (row tile, column block) itself; every reader of the hardware's
block indices -- weight slab addresses, tile masks, output columns, BatchNorm tile statistics, BatchNorm backward sums,
the f32 partial tiles of a split launch -- takes the decoded values.  The decode changes WHERE and WHEN a workgroup
runs, never what it computes, and these tests prove that without the previous build:

  * a launch of co columns equals, bit for bit, the launches on its 128-column and on its 64-column pieces of the same
    weights.  The accumulation order of an output element (offsets ascending, reduction slices ascending) does not
    depend on the column tiling; a 64-column launch has ONE column block per tile and therefore always takes the 2-D
    grid, whose kernels are instruction for instruction the previous ones;
  * integer-valued operands whose sums stay below 2^24 are exact in the f32 accumulators: the result must EQUAL the
    dense index_select -> mm -> index_add in f64 (rounded to bf16 once) -- so the pieces cannot all be wrong alike.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda'
BF = torch.bfloat16
TILE = 128


def _B():
    from lidal_amd import backend as B
    return B


def _table(n_in, n_out, k, seed, density):
    """A neighbour table [k, n_out] (-1 = no rule).  Rows come in runs of 96 that share a random subset of the offsets
    (each kept with probability `density`), thinned per row: after lidal_kmap_order's sort by occupancy pattern the
    128-row tiles have DIFFERENT offset masks, most of them sparse."""
    g = torch.Generator().manual_seed(seed)
    idx = torch.randint(0, n_in, (k, n_out), generator=g, dtype=torch.int32)
    runs = -(-n_out // 96)
    keep_run = (torch.rand(k, runs, generator=g) < density).repeat_interleave(96, 1)[:, :n_out]
    keep_run[seed % k] = True                                      # no row without any rule
    keep = keep_run & (torch.rand(k, n_out, generator=g) < 0.8)
    keep[seed % k, 0] = True
    return torch.where(keep, idx, torch.full_like(idx, -1)).to(DEV)


def _order(nbr):
    from lidal_amd.nn.functional.conv import RowOrder
    return RowOrder(nbr)


def _image(w, role, n_out):
    """w: [k][ci][co] (role 0, forward) or [k][co][ci] (role 1, data gradient), bf16 image for n_out output rows"""
    B = _B()
    L = B.lib()
    k = w.shape[0]
    n_red, n_col = (w.shape[1], w.shape[2]) if role == 0 else (w.shape[2], w.shape[1])
    nb = L.lidal_conv_weight_image_bytes(k, n_red, n_col, B.BF16, n_out)
    img = torch.empty(nb, dtype=torch.uint8, device=DEV)
    B.check(L.lidal_conv_weight_image(B.ptr(w), B.dtype_code(w.dtype), role, B.ptr(img), B.BF16, k, n_red, n_col, n_out,
                                      B.stream()), 'image')
    return img


def _forward(x, w, order, kflip, use_perm, scale=None, shift=None, relu=0, res=None, stats=False, ws=None):
    """lidal_conv_apply_image (with a workspace: _ws) of w [k][ci][co]; returns (out, tile statistics [co][tiles][3])"""
    B = _B()
    L = B.lib()
    n_out, (k, ci, co) = order.n_rows, w.shape
    out = torch.full((n_out, co), float('nan'), dtype=BF, device=DEV)
    tiles = -(-n_out // TILE)
    st = torch.full((co, tiles, 3), float('nan'), dtype=torch.float32, device=DEV) if stats else None
    args = (B.ptr(x), B.ptr(_image(w, 0, n_out)), B.ptr(order.table), B.ptr(order.perm) if use_perm else None,
            B.ptr(order.tile_masks), B.ptr(out), x.shape[0], n_out, ci, co, k, kflip, B.BF16, B.ptr(scale), B.ptr(shift),
            relu, B.ptr(res), B.ptr(st))
    if ws is None:
        B.check(L.lidal_conv_apply_image(*args, B.stream()), 'conv')
    else:
        B.check(L.lidal_conv_apply_image_ws(*args, B.ptr(ws), ws.numel(), B.stream()), 'conv')
    return out, st


def _dgrad(gout, w, order, kflip, use_perm, bn, relu, ws=None):
    """lidal_conv_dgrad_bn_sums of w [k][c_gin][c_gout]; bn = (x, mean, invstd, gamma, beta) of the BatchNorm whose
    output gradient the launch produces; returns (gin, sums [c_gin][tiles][2])"""
    B = _B()
    L = B.lib()
    n_gin, (k, c_gin, c_gout) = order.n_rows, w.shape
    gin = torch.full((n_gin, c_gin), float('nan'), dtype=BF, device=DEV)
    tiles = -(-n_gin // TILE)
    sums = torch.full((c_gin, tiles, 2), float('nan'), dtype=torch.float32, device=DEV)
    args = (B.ptr(gout), B.ptr(_image(w, 1, n_gin)), B.ptr(order.table), B.ptr(order.perm) if use_perm else None,
            B.ptr(order.tile_masks), B.ptr(gin), gout.shape[0], n_gin, c_gout, c_gin, k, kflip, B.BF16,
            B.ptr(bn[0]), B.ptr(bn[1]), B.ptr(bn[2]), B.ptr(bn[3]), B.ptr(bn[4]), relu, B.ptr(sums))
    if ws is None:
        B.check(L.lidal_conv_dgrad_bn_sums(*args, B.stream()), 'dgrad')
    else:
        B.check(L.lidal_conv_dgrad_bn_sums_ws(*args, B.ptr(ws), ws.numel(), B.stream()), 'dgrad')
    return gin, sums


def _same(a, b, what):
    assert not torch.isnan(a.float()).any(), what
    assert torch.equal(a, b), (what, int((a != b).sum()))


def _check_pieces(n_out, n_in, ci, co, k, seed, density, split=False):
    """Every epilogue the model uses, wide launch against its 128- and 64-column pieces."""
    B = _B()
    g = torch.Generator().manual_seed(seed)
    order = _order(_table(n_in, n_out, k, seed, density))
    x = torch.randn(n_in, ci, generator=g).to(BF).to(DEV)
    w = (torch.randn(k, ci, co, generator=g) * 0.1).to(BF).to(DEV)                  # forward: [k][ci][co]
    wd = (torch.randn(k, co, ci, generator=g) * 0.1).to(BF).to(DEV)                 # data gradient: [k][c_gin][c_gout]
    scale, shift = (torch.rand(co, generator=g) + 0.5).to(DEV), (torch.randn(co, generator=g) * 0.2).to(DEV)
    res = torch.randn(n_out, co, generator=g).to(BF).to(DEV)
    bn = ((torch.randn(n_out, co, generator=g) * 1.5 + 0.3).to(BF).to(DEV), (torch.randn(co, generator=g) * 0.1).to(DEV),
          (torch.rand(co, generator=g) + 0.5).to(DEV), (torch.rand(co, generator=g) + 0.5).to(DEV),
          (torch.randn(co, generator=g) * 0.2).to(DEV))
    ws = None
    if split:
        wsb = B.lib().lidal_conv_apply_workspace_bytes(n_out, co)
        assert wsb > 0
        ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    tag = (n_out, ci, co, k)
    # (kflip, row permutation): plain output with tile statistics | affine map + ReLU + residual + ReLU | BatchNorm sums
    wide = [_forward(x, w, order, 0, True, stats=True, ws=ws),
            _forward(x, w, order, 1, False, scale, shift, 3, res, ws=ws),
            _dgrad(x, wd, order, 1, True, bn, 1, ws=ws),
            _dgrad(x, wd, order, 0, False, bn, 0, ws=ws)]
    for width in (128, 64):
        for c0 in range(0, co, width):
            c1 = c0 + width
            wp, wdp = w[:, :, c0:c1].contiguous(), wd[:, c0:c1].contiguous()
            bnp = (bn[0][:, c0:c1].contiguous(), bn[1][c0:c1].contiguous(), bn[2][c0:c1].contiguous(),
                   bn[3][c0:c1].contiguous(), bn[4][c0:c1].contiguous())
            o, st = _forward(x, wp, order, 0, True, stats=True, ws=ws)
            _same(wide[0][0][:, c0:c1], o, tag + ('plain', width, c0))
            _same(wide[0][1][c0:c1], st, tag + ('tile statistics', width, c0))
            o, _ = _forward(x, wp, order, 1, False, scale[c0:c1].contiguous(), shift[c0:c1].contiguous(), 3,
                            res[:, c0:c1].contiguous(), ws=ws)
            _same(wide[1][0][:, c0:c1], o, tag + ('epilogue', width, c0))
            for j, (kf, up, relu) in ((2, (1, True, 1)), (3, (0, False, 0))):
                o, sm = _dgrad(x, wdp, order, kf, up, bnp, relu, ws=ws)
                _same(wide[j][0][:, c0:c1], o, tag + ('data gradient', kf, width, c0))
                _same(wide[j][1][c0:c1], sm, tag + ('BatchNorm sums', kf, width, c0))


# tile counts 1, 1, 1, 2, 7, 8 (the last tile partial), 8, 9: around the decode's groups of 8
ROWS = (1, 127, 128, 129, 6 * 128 + 5, 7 * 128 + 5, 8 * 128, 8 * 128 + 1)


@pytest.mark.parametrize('k,density', [(27, 0.3), (8, 0.7)])
@pytest.mark.parametrize('n_out', ROWS)
def test_wide_launch_equals_its_column_pieces(n_out, k, density):
    """co = 256 (2-4 column blocks) and co = 384 (3-6: the data gradient of the model's 384 -> 256 layers) against their
    128- and 64-column pieces, ci in {64, 128, 256, 384}, sparse 27-offset and 8-offset tables, kflip on and off, with
    and without the row permutation, with affine map / ReLU / residual, with tile statistics, with BatchNorm sums."""
    n_in = max(n_out // 2, 8) if k == 8 else n_out
    for ci, co in ((64, 256), (128, 256), (256, 256), (384, 256), (128, 384)):
        _check_pieces(n_out, n_in, ci, co, k, seed=n_out + ci + k, density=density)


@pytest.mark.parametrize('ci', [256, 384])
def test_deep_kernel_equals_its_column_pieces(ci):
    """30 080 rows (235 tiles: the last group of 8 has 5 empty places) with ci >= 256 take conv_lean_deep_kernel."""
    _check_pieces(30080, 30080, ci, 256, 27, seed=ci, density=0.25)


@pytest.mark.parametrize('n_out', [129, 7 * 128 + 5])
def test_split_launch_equals_its_column_pieces(n_out):
    """With a workspace and few enough workgroups the tile's offsets are split over blockIdx.z and the f32 partial
    tiles are combined by a second kernel: 2 and 8 tiles x (4, 2 or 1 column blocks) all split four ways, so the
    partial sums associate alike and the pieces must still agree bit for bit."""
    _check_pieces(n_out, n_out, 256, 256, 27, seed=n_out, density=0.6, split=True)


def _exact_case(n_out, ci, co, k, kflip, use_perm, seed, on_host):
    g = torch.Generator().manual_seed(seed)
    nbr = _table(n_out, n_out, k, seed, 0.4)
    order = _order(nbr)
    x = torch.randint(-2, 3, (n_out, ci), generator=g).to(BF).to(DEV)
    w = torch.randint(-2, 3, (k, ci, co), generator=g).to(BF).to(DEV)       # |sum| <= 27 * 384 * 4 < 2^24
    out, _ = _forward(x, w, order, kflip, use_perm)
    dev = 'cpu' if on_host else DEV
    xd, wd, tab = x.to(dev).double(), w.to(dev).double(), nbr.to(dev).long()
    want = torch.zeros(n_out, co, dtype=torch.float64, device=dev)
    for j in range(k):
        rows = tab[k - 1 - j] if kflip else tab[j]                 # kflip: weight slab j meets table row k - 1 - j
        has = (rows >= 0).nonzero().squeeze(1)
        want.index_add_(0, has, xd.index_select(0, rows[has]) @ wd[j])
    if not use_perm:                                               # without the permutation the rows stay in sorted order
        want = want.index_select(0, order.perm.to(dev).long())
    assert want.abs().max() < 2 ** 24
    assert torch.equal(out.to(dev), want.to(BF)), (n_out, ci, co, kflip, use_perm)


@pytest.mark.parametrize('n_out,ci,co,kflip,use_perm', [(7 * 128 + 5, 128, 256, 0, True), (8 * 128 + 1, 64, 384, 1, False),
                                                        (129, 256, 256, 1, True)])
def test_integer_operands_equal_the_dense_f64_sum(n_out, ci, co, kflip, use_perm):
    """Exact operands: the launch must EQUAL index_select -> mm -> index_add in f64 on the host, rounded to bf16."""
    _exact_case(n_out, ci, co, 27, kflip, use_perm, seed=n_out + ci, on_host=True)


def test_integer_operands_equal_the_dense_f64_sum_deep_kernel():
    """The same on the 30 080-row shape of the deep kernel (the f64 reference by torch on the device: 100 GFLOP)."""
    _exact_case(30080, 256, 256, 27, 0, True, seed=5, on_host=False)
