"""GPU experiment: achieved bandwidth of the BatchNorm launches per (rows, channels) of the bench
batch's levels, called straight through the C-ABI (no autograd): forward with the statistics pass
(3 N C b algorithmic bytes), forward on the convolution's tile statistics (2 N C b), backward
(5 N C b); the two tails of a residual block (lidal_add_relu_bwd_bn_sums, lidal_add_relu_bwd_bn_tile_sums, with the
shortcut's BatchNorm: 5 N C b) and lidal_colsum (N C b).  bf16, then f32 (BN_DTYPES=bf16 for one of them).  The last
line is JSON: the median of fifteen rounds of twenty calls, us, per dtype, shape and call -- what two libraries
(LIDAL_AMD_LIB) are compared by."""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
from lidal_amd import backend as B  # noqa: E402

SHAPES = [(396662, 32), (396662, 96), (226000, 32), (226000, 64), (105000, 64), (105000, 128), (43000, 128),
          (43000, 256), (16000, 256)]
if os.environ.get('BN_SHAPES'):         # e.g. BN_SHAPES=396662x96 for a counter pass over one shape
    SHAPES = [tuple(int(v) for v in t.split('x')) for t in os.environ['BN_SHAPES'].split(',')]
DTYPES = os.environ.get('BN_DTYPES', 'bf16,f32').split(',')
TDT = {'bf16': torch.bfloat16, 'f32': torch.float32}


def timeit(fn, reps=20, rounds=15):
    """median over the rounds of the mean time of `reps` calls, us"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / reps)
    return statistics.median(ts)


def main():
    dev = torch.device('cuda')
    print('lib', B.LIB_PATH)
    L = B.lib()
    res = {dt: sweep(dev, L, dt) for dt in DTYPES}
    print(json.dumps({'lib': B.LIB_PATH, 'median_us': res}))


def sweep(dev, L, dt='bf16'):
    tot = [0.0, 0.0, 0.0]
    code, esz, res = B.dtype_code(TDT[dt]), torch.empty(0, dtype=TDT[dt]).element_size(), {}
    print('dtype', dt)
    for n, c in SHAPES:
        x = torch.randn(n, c, device=dev).to(TDT[dt])
        go = torch.randn(n, c, device=dev).to(TDT[dt])
        xb = torch.randn(n, c, device=dev).to(TDT[dt])
        y, dx = torch.empty_like(x), torch.empty_like(x)
        w, b = torch.ones(c, device=dev), torch.zeros(c, device=dev)
        rm, rv = torch.zeros(c, device=dev), torch.ones(c, device=dev)
        mean, invstd = torch.empty(c, device=dev), torch.empty(c, device=dev)
        gg, gb = torch.empty(c, device=dev), torch.empty(c, device=dev)
        nbytes = L.lidal_bn_workspace_bytes(n, c)
        ws = torch.empty(nbytes + 3 * c * 4, dtype=torch.uint8, device=dev)
        ws2 = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        parts = int(L.lidal_bn_tail_parts(n, c, code))
        sums, sums2 = torch.empty(c, parts, 2, device=dev), torch.empty(c, parts, 2, device=dev)
        n_tiles = -(-n // 128)
        ts = torch.zeros(n_tiles, c, 3, device=dev)
        ts[:, :, 0] = 128.0
        ts[:, :, 2] = 128.0

        def fwd():
            B.check(L.lidal_bn_train_fwd(B.ptr(x), code, n, c, B.ptr(w), B.ptr(b), 1e-5, 0.1, B.ptr(rm), B.ptr(rv),
                                         None, 1, None, B.ptr(y), B.ptr(mean), B.ptr(invstd), B.ptr(ws), nbytes,
                                         B.stream()), 'fwd')

        def fwd_tiles():
            B.check(L.lidal_bn_train_fwd_tiles(B.ptr(x), code, n, c, B.ptr(w), B.ptr(b), 1e-5, 0.1, B.ptr(rm),
                                               B.ptr(rv), None, 1, None, B.ptr(y), B.ptr(mean), B.ptr(invstd),
                                               B.ptr(ts), n_tiles, B.stream()), 'fwd_tiles')

        def bwd():
            B.check(L.lidal_bn_bwd(B.ptr(x), B.ptr(go), c, code, n, c, B.ptr(w), B.ptr(b), 1, B.ptr(mean),
                                   B.ptr(invstd), B.ptr(dx), B.ptr(gg), B.ptr(gb), B.ptr(ws), nbytes,
                                   B.stream()), 'bwd')

        def bwd_params():       # statistics of the backward only (dx = NULL): the reducing pass + its final
            B.check(L.lidal_bn_bwd(B.ptr(x), B.ptr(go), c, code, n, c, B.ptr(w), B.ptr(b), 1, B.ptr(mean),
                                   B.ptr(invstd), None, B.ptr(gg), B.ptr(gb), B.ptr(ws), nbytes,
                                   B.stream()), 'bwd')

        def tail_sums():        # mask + f64 partial sums of two BatchNorms (y as the block's output, dx as gm)
            B.check(L.lidal_add_relu_bwd_bn_sums(B.ptr(y), B.ptr(go), B.ptr(dx), code, n, c, B.ptr(x), B.ptr(mean),
                                                 B.ptr(invstd), B.ptr(ws), B.ptr(xb), B.ptr(mean), B.ptr(invstd),
                                                 B.ptr(ws2), nbytes, B.stream()), 'tail_sums')

        def tail_tile_sums():   # mask + f32 slab sums of two BatchNorms
            B.check(L.lidal_add_relu_bwd_bn_tile_sums(B.ptr(y), B.ptr(go), B.ptr(dx), code, n, c, B.ptr(x), B.ptr(mean),
                                                      B.ptr(invstd), B.ptr(sums), B.ptr(xb), B.ptr(mean), B.ptr(invstd),
                                                      B.ptr(sums2), parts, B.stream()), 'tail_tile_sums')

        def colsum():
            B.check(L.lidal_colsum(B.ptr(go), code, n, c, B.ptr(gg), B.ptr(ws), nbytes + 3 * c * 4, B.stream()), 'colsum')
        fwd()
        t = [timeit(fwd), timeit(fwd_tiles), timeit(bwd)]
        tp = timeit(bwd_params)
        tt = [timeit(tail_sums), timeit(tail_tile_sums), timeit(colsum)]
        by = n * c * esz
        tot = [a + b_ for a, b_ in zip(tot, t)]
        res['%dx%d' % (n, c)] = dict(fwd=t[0], fwd_tiles=t[1], bwd=t[2], bwd_params=tp, tail_sums=tt[0],
                                     tail_tile_sums=tt[1], colsum=tt[2])
        print('%7d x %3d   fwd %6.1f us (%5.2f TB/s)   fwd on tile stats %6.1f us (%5.2f TB/s)   bwd %6.1f us (%5.2f TB/s)'
              % (n, c, t[0], 3 * by / t[0] / 1e6, t[1], 2 * by / t[1] / 1e6, t[2], 5 * by / t[2] / 1e6)
              + '   [reduce %5.1f us (%4.2f TB/s), dx %5.1f us (%4.2f TB/s)]'
              % (tp, 2 * by / tp / 1e6, t[2] - tp, 3 * by / (t[2] - tp) / 1e6)
              + '   tail f64 sums %6.1f us (%4.2f TB/s)   tail slab sums %6.1f us (%4.2f TB/s)   colsum %5.1f us (%4.2f TB/s)'
              % (tt[0], 5 * by / tt[0] / 1e6, tt[1], 5 * by / tt[1] / 1e6, tt[2], by / tt[2] / 1e6), flush=True)
    print('sum fwd %.1f  fwd_tiles %.1f  bwd %.1f us' % tuple(tot))
    return res


if __name__ == '__main__':
    main()
