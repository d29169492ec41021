"""A digest of every output of the convolution entry points of csrc/conv_img.hip, on seeded inputs, for comparing two
builds bit for bit.

  LIDAL_AMD_LIB=/elsewhere/liblidal_amd.so python scripts/exp/conv_digest.py --out parent.json
  python scripts/exp/conv_digest.py --out new.json
  python scripts/exp/conv_digest.py --compare parent.json new.json      # exit status 1 unless all are equal

One process per library.  Every output buffer is NaN-filled before its call and digested whole (SHA-256), with the tile
statistics / BatchNorm sums and every weight image; workspace sizes are kept as numbers.  Covered, at the smallest shapes
that reach each form (130, 300 and 1100 rows = 1, 3 and 9 row tiles, the last one ragged):
  lean     bf16 and f32, co 32 / 64 / 96 / 128 (NB 2 / 4 / 6 / 4) with ci giving 64-, 128- and 192-byte slices, each with
           tables of 27 and of 8 offsets (kflip 0 / 1 x with / without the row permutation) and dense (no table); NB 8 on
           49 200 rows (co 128, and co 256 on the paired grid) with the three slices, 27 offsets ((0, perm), (1, none))
           and dense; paired column blocks at NB 4 / 6 (co 192 / 256 / 384 on 3 and 9 tiles); the epilogues (plain + tile
           statistics, affine + ReLU + residual + ReLU, lidal_conv_dgrad_bn_sums).  Not the full cross product: one row
           count per (co, slice), and the 8-offset tables and all four (kflip, perm) pairs only at NB 2 / 4 / 6.
  split    bf16 _ws launches that split 4, 3 and 2 ways + conv_combine_kernel
  deep     30 080 rows, ci 256, co 256 / 384
  generic  f32 ci = 4, bf16 ci = 48 (96-byte rows), one and three column blocks
  f32split conv_split_kernel NB 2 / 4 / 6 / 8, dense and with a table, without a workspace and with one (4 and 3 shares)
  images   lidal_conv_weight_image, _pair, _job + _batch for the four dtype pairs and LIDAL_F32_SPLIT, roles 0 and 1 (of a
           job also its host bytes behind the three pointers)
"""
import argparse
import ctypes
import hashlib
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

DEV = 'cuda'
TDT = {'f32': torch.float32, 'bf16': torch.bfloat16}
TILE = 128


def digest(t):
    return hashlib.sha256(t.detach().contiguous().reshape(-1).view(torch.uint8).cpu().numpy().tobytes()).hexdigest()[:16]


def table(n_in, n_out, k, seed, density):
    """[k, n_out] neighbour table (-1 = no rule): runs of 96 rows share a random subset of the offsets, thinned per row,
    so that the sorted 128-row tiles have different, mostly sparse offset masks"""
    g = torch.Generator().manual_seed(seed)
    idx = torch.randint(0, n_in, (k, n_out), generator=g, dtype=torch.int32)
    runs = -(-n_out // 96)
    keep_run = (torch.rand(k, runs, generator=g) < density).repeat_interleave(96, 1)[:, :n_out]
    keep_run[seed % k] = True
    keep = keep_run & (torch.rand(k, n_out, generator=g) < 0.8)
    keep[seed % k, 0] = True
    return torch.where(keep, idx, torch.full_like(idx, -1)).to(DEV)


def run():
    from lidal_amd import backend as B
    from lidal_amd.nn.functional.conv import RowOrder
    L = B.lib()
    p, s = B.ptr, B.stream
    out = {}
    orders = {}
    CODE = {'f32': B.F32, 'bf16': B.BF16, 'split': B.F32_SPLIT}

    def ok(rc):
        assert rc == 0, L.lidal_last_error().decode()

    def put(key, **tensors):
        for name, t in tensors.items():
            if t is not None:
                assert '%s/%s' % (key, name) not in out, key
                out['%s/%s' % (key, name)] = digest(t)

    def nan(*shape, dtype):
        return torch.full(shape, float('nan'), dtype=dtype, device=DEV)

    def order(n_in, n_out, k, density):
        key = (n_in, n_out, k, density)
        if key not in orders:
            orders[key] = RowOrder(table(n_in, n_out, k, n_out + k, density))
        return orders[key]

    def image(key, w, role, code, n_out):
        k = w.shape[0]
        n_red, n_col = (w.shape[1], w.shape[2]) if role == 0 else (w.shape[2], w.shape[1])
        nb = L.lidal_conv_weight_image_bytes(k, n_red, n_col, code, n_out)
        assert nb > 0
        img = torch.full((nb,), 0xA5, dtype=torch.uint8, device=DEV)
        ok(L.lidal_conv_weight_image(p(w), B.dtype_code(w.dtype), role, p(img), code, k, n_red, n_col, n_out, s()))
        out['%s/image%d_tiling' % (key, role)] = int(L.lidal_conv_weight_image_tiling(n_red, n_col, code, n_out))
        put(key, **{'image%d' % role: img})
        return img

    def conv(key, dt, code, n_out, ci, co, k, density=0.4, dense=False, ws=False, epilogues=(0, 1, 2), flips=((0, True), (1, False))):
        """the launches of one shape: epilogue 0 = plain + tile statistics, 1 = affine + ReLU + residual + ReLU,
        2 = lidal_conv_dgrad_bn_sums; flips = (kflip, with the row permutation)"""
        T = TDT[dt]
        g = torch.Generator().manual_seed(n_out * 7 + ci * 3 + co + k)
        n_in = n_out if (dense or k != 8) else max(n_out // 2, 8)
        od = None if dense else order(n_in, n_out, k, density)
        x = torch.randn(n_in, ci, generator=g).to(T).to(DEV)
        w = (torch.randn(k, ci, co, generator=g) * 0.1).to(T).to(DEV)
        wd = (torch.randn(k, co, ci, generator=g) * 0.1).to(T).to(DEV)
        scale, shift = (torch.rand(co, generator=g) + 0.5).to(DEV), (torch.randn(co, generator=g) * 0.2).to(DEV)
        res = torch.randn(n_out, co, generator=g).to(T).to(DEV)
        bn = ((torch.randn(n_out, co, generator=g) * 1.5 + 0.3).to(T).to(DEV), (torch.randn(co, generator=g) * 0.1).to(DEV),
              (torch.rand(co, generator=g) + 0.5).to(DEV), (torch.rand(co, generator=g) + 0.5).to(DEV),
              (torch.randn(co, generator=g) * 0.2).to(DEV))
        wsb = int(L.lidal_conv_apply_workspace_bytes(n_out, co)) if ws else 0
        wst = torch.full((max(wsb, 1),), 0xFF, dtype=torch.uint8, device=DEV) if ws else None      # (0xFF...: NaN as f32)
        assert not ws or wsb > 0, key
        img_f = image(key, w, 0, code, n_out)
        img_d = image(key, wd, 1, code, n_out) if (2 in epilogues and code != B.F32_SPLIT) else None
        tiles = -(-n_out // TILE)
        tab, masks = (None, None) if dense else (p(od.table), p(od.tile_masks))
        for kflip, use_perm in (((0, False),) if dense else flips):
            perm = p(od.perm) if (use_perm and not dense) else None
            tag = '%s/flip%d_perm%d' % (key, kflip, use_perm)
            for e in epilogues:
                o = nan(n_out, co, dtype=T)
                if e == 2:
                    if img_d is None:
                        continue
                    sums = nan(co, tiles, 2, dtype=torch.float32)
                    args = (p(x), p(img_d), tab, perm, masks, p(o), n_in, n_out, ci, co, k, kflip, code, p(bn[0]), p(bn[1]),
                            p(bn[2]), p(bn[3]), p(bn[4]), kflip, p(sums))
                    ok(L.lidal_conv_dgrad_bn_sums_ws(*args, p(wst), wsb, s()) if ws else L.lidal_conv_dgrad_bn_sums(*args, s()))
                    put(tag + '/dgrad', gin=o, sums=sums)
                    continue
                st = nan(co, tiles, 3, dtype=torch.float32) if (e == 0 and code != B.F32_SPLIT) else None
                args = (p(x), p(img_f), tab, perm, masks, p(o), n_in, n_out, ci, co, k, kflip, code,
                        p(scale) if e else None, p(shift) if e else None, 3 if e else 0, p(res) if e else None, p(st))
                ok(L.lidal_conv_apply_image_ws(*args, p(wst), wsb, s()) if ws else L.lidal_conv_apply_image(*args, s()))
                put('%s/epi%d' % (tag, e), out=o, stats=st)

    t0 = time.time()
    rows = (130, 300, 1100)
    ALL4 = ((0, True), (1, False), (0, False), (1, True))
    # ---- lean kernel, generic kernel
    for dt in ('bf16', 'f32'):
        esz = 2 if dt == 'bf16' else 4
        code = CODE[dt]
        for i, co in enumerate((32, 64, 96, 128)):
            for j, slice_bytes in enumerate((64, 128, 192)):
                ci = slice_bytes // esz
                n = rows[(i + j) % 3]
                conv('lean/%s/%dx%d->%d/k27' % (dt, n, ci, co), dt, code, n, ci, co, 27, flips=ALL4)
                conv('lean/%s/%dx%d->%d/k8' % (dt, n, ci, co), dt, code, n, ci, co, 8, density=0.7, flips=ALL4)
                conv('lean/%s/%dx%d->%d/dense' % (dt, n, ci, co), dt, code, n, ci, co, 1, dense=True, epilogues=(0, 1))
        for ci, co in ((128 // esz, 128), (256 // esz, 128)):         # two slices per offset; ci == co: with the data gradient
            conv('lean/%s/1100x%d->%d/k27' % (dt, ci, co), dt, code, 1100, ci, co, 27)
        for slice_bytes in (64, 128, 192):            # NB = 8: more than 384 row tiles; co = 256 on the paired grid
            ci = slice_bytes // esz
            conv('lean/%s/49200x%d->128/k27' % (dt, ci), dt, code, 49200, ci, 128, 27, density=0.2)
            conv('lean/%s/49200x%d->128/dense' % (dt, ci), dt, code, 49200, ci, 128, 1, dense=True, epilogues=(0, 1))
            conv('paired/%s/49200x%d->256/k27' % (dt, ci), dt, code, 49200, ci, 256, 27, density=0.2)
        conv('paired/%s/49200x%d->256/dense' % (dt, 128 // esz), dt, code, 49200, 128 // esz, 256, 1, dense=True, epilogues=(0, 1))
        for n, co in ((300, 192), (1100, 256), (300, 384), (1100, 192)):      # paired column blocks, 3 and 9 row tiles
            ci = co if co != 384 else 128 // esz
            conv('paired/%s/%dx%d->%d/k27' % (dt, n, ci, co), dt, code, n, ci, co, 27)
            conv('paired/%s/%dx%d->%d/dense' % (dt, n, ci, co), dt, code, n, ci, co, 1, dense=True, epilogues=(0, 1))
        gci = 48 if dt == 'bf16' else 4
        for n, co in ((300, 64), (1100, 192)):
            conv('generic/%s/%dx%d->%d/k27' % (dt, n, gci, co), dt, code, n, gci, co, 27)
            conv('generic/%s/%dx%d->%d/dense' % (dt, n, gci, co), dt, code, n, gci, co, 1, dense=True, epilogues=(0, 1))
    # ---- bf16 launches that split 4, 3 and 2 ways (36, 164 and 220 workgroups), and the combining kernel
    for n in (1100, 5127, 7000):
        conv('splitws/bf16/%dx256->256/k27' % n, 'bf16', B.BF16, n, 256, 256, 27, density=0.5, ws=True)
    # ---- deep kernel
    for co in (256, 384):
        conv('deep/bf16/30080x256->%d/k27' % co, 'bf16', B.BF16, 30080, 256, co, 27, density=0.25)
    # ---- the split form of the f32 product
    for co in (32, 64, 96, 128):
        conv('f32split/1100x64->%d/k27' % co, 'f32', B.F32_SPLIT, 1100, 64, co, 27, epilogues=(0, 1))
        conv('f32split/1100x64->%d/k27ws' % co, 'f32', B.F32_SPLIT, 1100, 64, co, 27, epilogues=(0, 1), ws=True)         # 4 shares
        conv('f32split/300x64->%d/dense' % co, 'f32', B.F32_SPLIT, 300, 64, co, 1, dense=True, epilogues=(0, 1))
    conv('f32split/38405x64->128/k27ws', 'f32', B.F32_SPLIT, 38405, 64, 128, 27, density=0.2, epilogues=(1,), ws=True,
         flips=((0, True),))                                                                                                  # 3 shares
    # ---- weight images: pairs and batched jobs
    jb = int(L.lidal_conv_weight_image_job_bytes())
    g = torch.Generator().manual_seed(11)
    for wdt in ('f32', 'bf16'):
        for idt in ('f32', 'bf16', 'split'):
            code, wcode = CODE[idt], CODE[wdt]
            shapes = [(27, 64, 96, 1100, 300), (8, 32, 64, 130, 60000), (1, 96, 32, 300, 300), (27, 128, 256, 50000, 1100)]
            if idt != 'split':
                shapes.append((27, 4 if idt == 'f32' else 8, 20, 300, 130))
            jobs, total, keep = ctypes.create_string_buffer(jb * 4 * len(shapes)), 0, []
            for k, ci, co, n_f, n_b in shapes:
                w = (torch.randn(k, ci, co, generator=g) * 0.3).to(TDT[wdt]).to(DEV)
                key = 'images/%s->%s/%dx%dx%d' % (wdt, idt, k, ci, co)
                fb, bb = (int(L.lidal_conv_weight_image_bytes(k, ci, co, code, n_f)),
                          int(L.lidal_conv_weight_image_bytes(k, co, ci, code, n_b)))
                out[key + '/bytes'] = [fb, bb]
                fill = lambda nb: torch.full((nb,), 0xA5, dtype=torch.uint8, device=DEV)        # noqa: E731
                if idt != 'split':
                    a, b = fill(fb), fill(bb)
                    ok(L.lidal_conv_weight_image_pair(p(w), wcode, p(a), n_f, p(b), n_b, code, k, ci, co, s()))
                    put(key + '/pair', fwd=a, bwd=b)
                for role in (0, 1):                      # role 1: the same bytes read as [k][co][ci]
                    a = fill(fb)
                    ok(L.lidal_conv_weight_image(p(w), wcode, role, p(a), code, k, ci, co, n_f, s()))
                    put('%s/single_role%d' % (key, role), img=a)
                    for both in (0, 1):
                        a, b = fill(fb), fill(bb)
                        at = ctypes.addressof(jobs) + jb * len(keep)
                        n = int(L.lidal_conv_weight_image_job(ctypes.c_void_p(at), p(w), role, p(a), n_f, p(b) if both else None,
                                                              n_b, code, k, ci, co, total))
                        assert n > 0, L.lidal_last_error().decode()
                        host = jobs.raw[jb * len(keep) + 24:jb * (len(keep) + 1)]           # behind the three pointers
                        out['%s/job_role%d_both%d' % (key, role, both)] = [n, hashlib.sha256(host).hexdigest()[:16]]
                        total += n
                        keep.append((key, role, both, w, a, b))
            tab = torch.frombuffer(bytearray(jobs.raw[:jb * len(keep)]), dtype=torch.uint8).to(DEV)
            ok(L.lidal_conv_weight_image_batch(p(tab), len(keep), total, wcode, code, s()))
            for key, role, both, w, a, b in keep:
                put('%s/batch_role%d_both%d' % (key, role, both), fwd=a, bwd=b if both else None)
    # ---- workspace sizes
    for n in (0, 1, 127, 128, 129, 1100, 4096, 8192, 16384, 30080, 32768, 32769, 65536, 65537, 100000):
        for co in (4, 32, 64, 96, 128, 132, 192, 256, 384):
            out['workspace/%dx%d' % (n, co)] = int(L.lidal_conv_apply_workspace_bytes(n, co))
    torch.cuda.synchronize()
    return out, time.time() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out')
    ap.add_argument('--compare', nargs=2)
    a = ap.parse_args()
    if a.compare:
        x, y = (json.load(open(f)) for f in a.compare)
        bad = sorted(k for k in set(x) | set(y) if x.get(k) != y.get(k))
        print('%d entries compared, %d differ' % (len(set(x) | set(y)), len(bad)))
        for k in bad[:40]:
            print('  differs:', k)
        sys.exit(1 if bad or not x else 0)
    from lidal_amd import backend as B
    res, secs = run()
    json.dump(res, open(a.out, 'w'), indent=0, sort_keys=True)
    print('%d entries digested in %.1f s with %s' % (len(res), secs, B.LIB_PATH))


if __name__ == '__main__':
    main()
