"""A digest of every output of the BatchNorm entry points of include/lidal_amd.h (csrc/bn.hip), on seeded inputs, for
comparing two builds bit for bit.

  LIDAL_AMD_LIB=/elsewhere/liblidal_amd.so python scripts/exp/bn_digest.py --out parent.json
  python scripts/exp/bn_digest.py --out new.json
  python scripts/exp/bn_digest.py --compare parent.json new.json        # exit status 1 unless all are equal

One process per library.  lidal_bn_train_fwd, _train_fwd_tiles, _eval_fwd, _bwd (with and without dx, dy rows of c and
of c + one 16-byte piece), lidal_add_relu_bwd_bn_sums and _bn_tile_sums (one BatchNorm and two), lidal_bn_bwd_from_sums,
lidal_bn_bwd_tiles, lidal_bn_fold and lidal_colsum at tests/batchnorm_ref.all_cases(with_one_row=True): the six ReLU /
residual combinations, lidal_bn_set_fused 0 and 1, lidal_bn_set_slab_sums 0 and 1.  Every output tensor and the
statistics / sums workspace (cleared before the call) is digested.
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import batchnorm_ref as R  # noqa: E402

DEV = 'cuda'
TDT = {'f32': torch.float32, 'bf16': torch.bfloat16}
FLAGS = [(0, False), (1, False), (0, True), (1, True), (2, True), (3, True)]      # (relu bits, residual)


def digest(t):
    return hashlib.sha256(t.detach().contiguous().reshape(-1).view(torch.uint8).cpu().numpy().tobytes()).hexdigest()[:16]


def run(only=None):
    from lidal_amd import backend as B
    L = B.lib()
    out = {}
    p, s = B.ptr, B.stream

    def ok(rc):
        assert rc == 0, L.lidal_last_error().decode()

    def put(key, **tensors):
        for name, t in tensors.items():
            if t is not None:
                out['%s/%s' % (key, name)] = digest(t)

    def up(a, dt=None):
        t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
        return t.to(TDT[dt]) if dt is not None else t

    for dt, n, c in R.all_cases(with_one_row=True):
        if only and R.case_id((dt, n, c)) not in only:
            continue
        cs, code, vec, T = R.Case(dt, n, c), B.dtype_code(TDT[dt]), R.VEC[dt], TDT[dt]
        base = R.case_id((dt, n, c))
        x, dy, res, o_, xb = (up(cs[k], dt) for k in ('x', 'dy', 'res', 'out', 'xb'))
        gamma, beta, rm0, rv0 = (up(cs[k]) for k in ('gamma', 'beta', 'rm0', 'rv0'))
        stats = {}
        for name in ('x', 'xb'):
            mean, var, _, inv = R.batch_stats(cs[name].astype(np.float64))
            stats[name] = (up(mean.astype(np.float32)), up(inv.astype(np.float32)), up(var.astype(np.float32)))
        mean, inv, var = stats['x']
        nb = int(L.lidal_bn_workspace_bytes(n, c))
        new = lambda *shape, dtype=T: torch.zeros(*shape, dtype=dtype, device=DEV)        # noqa: E731
        tiles = R._tile_triples(torch.from_numpy(cs['x'])).to(DEV).contiguous()
        n_tiles = tiles.shape[0]
        wide = new(n, c + vec)
        wide[:, :c] = dy

        # ---- forward
        for relu, has_res in FLAGS:
            r = res if has_res else None
            key = '%s/relu%d_res%d' % (base, relu, has_res)
            y, sm, si, rm, rv, nbt, ws = new(n, c), new(c, dtype=torch.float32), new(c, dtype=torch.float32), rm0.clone(), \
                rv0.clone(), new(1, dtype=torch.int64), new(nb, dtype=torch.uint8)
            ok(L.lidal_bn_train_fwd(p(x), code, n, c, p(gamma), p(beta), R.EPS, R.MOMENTUM, p(rm), p(rv), p(nbt), relu, p(r),
                                    p(y), p(sm), p(si), p(ws), nb, s()))
            put(key + '/train_fwd', y=y, mean=sm, invstd=si, rm=rm, rv=rv, nbt=nbt, ws=ws)
            for fused in (0, 1):
                L.lidal_bn_set_fused(fused)
                y, sm, si, rm, rv, nbt = new(n, c), new(c, dtype=torch.float32), new(c, dtype=torch.float32), rm0.clone(), \
                    rv0.clone(), new(1, dtype=torch.int64)
                ok(L.lidal_bn_train_fwd_tiles(p(x), code, n, c, p(gamma), p(beta), R.EPS, R.MOMENTUM, p(rm), p(rv), p(nbt),
                                              relu, p(r), p(y), p(sm), p(si), p(tiles), n_tiles, s()))
                put('%s/train_fwd_tiles_fused%d' % (key, fused), y=y, mean=sm, invstd=si, rm=rm, rv=rv, nbt=nbt)
            L.lidal_bn_set_fused(1)
        for relu in (0, 1):
            y = new(n, c)
            ok(L.lidal_bn_eval_fwd(p(x), code, n, c, p(gamma), p(beta), p(mean), p(var), R.EPS, relu, p(y), s()))
            put('%s/eval_fwd_relu%d' % (base, relu), y=y)
        scale, shift = new(c, dtype=torch.float32), new(c, dtype=torch.float32)
        ok(L.lidal_bn_fold(p(gamma), p(beta), p(mean), p(var), R.EPS, c, p(scale), p(shift), s()))
        put(base + '/fold', scale=scale, shift=shift)

        # ---- backward
        parts = int(L.lidal_bn_tail_parts(n, c, code))
        for fused in (0, 1):
            L.lidal_bn_set_fused(fused)
            for relu in (0, 1):
                for slab in (0, 1):
                    was = L.lidal_bn_set_slab_sums(slab)
                    for want_dx in (0, 1):
                        for g, stride in ((dy, c), (wide, c + vec)):
                            dx, gg, gb, ws = new(n, c), new(c, dtype=torch.float32), new(c, dtype=torch.float32), \
                                new(nb, dtype=torch.uint8)
                            ok(L.lidal_bn_bwd(p(x), p(g), stride, code, n, c, p(gamma), p(beta), relu, p(mean), p(inv),
                                              p(dx) if want_dx else None, p(gg), p(gb), p(ws), nb, s()))
                            put('%s/bwd_fused%d_relu%d_slab%d_dx%d_ld%d' % (base, fused, relu, slab, want_dx, stride),
                                dx=dx if want_dx else None, gg=gg, gb=gb, ws=ws)
                    L.lidal_bn_set_slab_sums(was)
            for dual in (0, 1):
                key = '%s/tail_fused%d_dual%d' % (base, fused, dual)
                b_x, b_mean, b_inv = (xb, stats['xb'][0], stats['xb'][1]) if dual else (None, None, None)
                gm, pa, pb = new(n, c), new(nb, dtype=torch.uint8), new(nb, dtype=torch.uint8)
                ok(L.lidal_add_relu_bwd_bn_sums(p(o_), p(dy), p(gm), code, n, c, p(x), p(mean), p(inv), p(pa), p(b_x), p(b_mean),
                                                p(b_inv), p(pb) if dual else None, nb, s()))
                put(key + '/sums', gm=gm, part_a=pa, part_b=pb if dual else None)
                gm2, sa, sb = new(n, c), new(c, parts, 2, dtype=torch.float32), new(c, parts, 2, dtype=torch.float32)
                ok(L.lidal_add_relu_bwd_bn_tile_sums(p(o_), p(dy), p(gm2), code, n, c, p(x), p(mean), p(inv), p(sa), p(b_x),
                                                     p(b_mean), p(b_inv), p(sb) if dual else None, parts, s()))
                put(key + '/tile_sums', gm=gm2, sums_a=sa, sums_b=sb if dual else None)
                for which, (xn, st, part, sums) in enumerate([(x, stats['x'], pa, sa), (xb, stats['xb'], pb, sb)][:1 + dual]):
                    for relu in (0, 1):
                        for want_dx in (0, 1):
                            k2 = '%s/bn%d_relu%d_dx%d' % (key, which, relu, want_dx)
                            dx, gg, gb = new(n, c), new(c, dtype=torch.float32), new(c, dtype=torch.float32)
                            ok(L.lidal_bn_bwd_from_sums(p(xn), p(gm), c, code, n, c, p(gamma), p(beta), relu, p(st[0]), p(st[1]),
                                                        p(dx) if want_dx else None, p(gg), p(gb), p(part), nb, s()))
                            put(k2 + '/from_sums', dx=dx if want_dx else None, gg=gg, gb=gb)
                            dx, gg, gb = new(n, c), new(c, dtype=torch.float32), new(c, dtype=torch.float32)
                            ok(L.lidal_bn_bwd_tiles(p(xn), p(gm2), c, code, n, c, p(gamma), p(beta), relu, p(st[0]), p(st[1]),
                                                    p(dx) if want_dx else None, p(gg), p(gb), p(sums), parts, s()))
                            put(k2 + '/bwd_tiles', dx=dx if want_dx else None, gg=gg, gb=gb)
        L.lidal_bn_set_fused(1)
        # dy rows wider than c into lidal_bn_bwd_tiles as well, on the sums of the last tail
        dx, gg, gb = new(n, c), new(c, dtype=torch.float32), new(c, dtype=torch.float32)
        ok(L.lidal_bn_bwd_tiles(p(x), p(wide), c + vec, code, n, c, p(gamma), p(beta), 1, p(mean), p(inv), p(dx), p(gg), p(gb),
                                p(sa), parts, s()))
        put(base + '/bwd_tiles_wide', dx=dx, gg=gg, gb=gb)

        cb = nb + 3 * c * 4
        csum, ws = new(c, dtype=torch.float32), new(cb, dtype=torch.uint8)
        ok(L.lidal_colsum(p(dy), code, n, c, p(csum), p(ws), cb, s()))
        put(base + '/colsum', out=csum, ws=ws[:nb - 256])
        assert L.lidal_bn_check_device() == 0, L.lidal_last_error().decode()
    torch.cuda.synchronize()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out')
    ap.add_argument('--only', nargs='*', help='case ids such as bf16-33x96')
    ap.add_argument('--compare', nargs=2)
    a = ap.parse_args()
    if a.compare:
        x, y = (json.load(open(f)) for f in a.compare)
        bad = sorted(k for k in set(x) | set(y) if x.get(k) != y.get(k))
        print('%d tensors compared, %d differ' % (len(set(x) | set(y)), len(bad)))
        for k in bad[:40]:
            print('  differs:', k)
        sys.exit(1 if bad or not x else 0)
    from lidal_amd import backend as B
    res = run(a.only)
    json.dump(res, open(a.out, 'w'), indent=0, sort_keys=True)
    print('%d tensors digested with %s' % (len(res), B.LIB_PATH))


if __name__ == '__main__':
    main()
