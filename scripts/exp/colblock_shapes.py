"""GPU: every layer shape of the U-Net that runs more than one column block per row tile, alone, on the bench batch:
time per launch (forward through lidal_conv_apply_image, data gradient through lidal_conv_dgrad_bn_sums) and a digest
of the results.  Run it in two checkouts to compare them (profiles/README.md, round 7: column blocks of a tile paired
on one XCD); with COUNTERS=1 every shape is launched exactly twice, untimed, for a counter collection
(rocprofv3 --pmc ... -- python scripts/exp/colblock_shapes.py: the second dispatch of a kernel run is the warm one)."""
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
from exp_img import make_image, timeit  # noqa: E402
from lidal_amd import backend as B, synth  # noqa: E402
from lidal_amd.nn import functional as F  # noqa: E402

# (stride, reduction channels, output columns): forward shapes of the encoder / decoder at strides 8 and 16 and the
# data gradients wider than 128 columns (384 = the gradient of 384 -> 256, 192 = of 192 -> 128 at stride 4)
SHAPES = [(8, 256, 256), (8, 384, 256), (8, 256, 384), (8, 128, 256), (16, 256, 256), (16, 128, 256), (4, 128, 192)]


def main():
    dev = torch.device('cuda')
    lib = B.lib()
    counters = os.environ.get('COUNTERS') == '1'
    batch = synth.make_train_batch(n_frames=5, n_points=120000, seed=7122)
    levels = {1: torch.from_numpy(batch['coords_v_b']).to(dev)}
    s = 1
    while s < 16:
        levels[s * 2] = F.spdownsample(levels[s], 2, 2, s)
        s *= 2
    print('%-30s %10s %10s  %s' % ('shape', 'fwd us', 'dgrad us', 'digest'))
    for stride, ci, co in SHAPES:
        c = levels[stride]
        kmap, _ = F.build_kernel_map(c, (stride,) * 3, (3, 3, 3), (1, 1, 1))
        n = c.shape[0]
        g = torch.Generator(device='cpu').manual_seed(ci * 1000 + co)
        x = torch.randn(n, ci, generator=g).to(dev).bfloat16()
        w = (torch.randn(27, ci, co, generator=g) * 0.05).to(dev)
        bx = torch.randn(n, co, generator=g).to(dev).bfloat16()
        mean, invstd = torch.zeros(co, device=dev), torch.ones(co, device=dev)
        o = kmap.order_out
        img = make_image(w, torch.bfloat16, n)
        out = torch.empty((n, co), dtype=torch.bfloat16, device=dev)
        sums = torch.empty((co, -(-n // 128), 2), dtype=torch.float32, device=dev)

        def fwd():
            B.check(lib.lidal_conv_apply_image(B.ptr(x), B.ptr(img), B.ptr(o.table), B.ptr(o.perm), B.ptr(o.tile_masks),
                                               B.ptr(out), n, n, ci, co, 27, 0, B.BF16, None, None, 0, None, None,
                                               B.stream()), 'conv')

        def dgrad():
            B.check(lib.lidal_conv_dgrad_bn_sums(B.ptr(x), B.ptr(img), B.ptr(o.table), B.ptr(o.perm), B.ptr(o.tile_masks),
                                                 B.ptr(out), n, n, ci, co, 27, 1, B.BF16, B.ptr(bx), B.ptr(mean),
                                                 B.ptr(invstd), None, None, 1, B.ptr(sums), B.stream()), 'dgrad')
        h = hashlib.sha1()
        ts = []
        for fn in (fwd, dgrad):
            fn()
            torch.cuda.synchronize()
            h.update(out.view(torch.int16).cpu().numpy().tobytes())
            if counters:
                fn()
                torch.cuda.synchronize()
                ts.append(float('nan'))
            else:
                ts.append(timeit(fn, reps=20, rounds=5))
        h.update(sums.cpu().numpy().tobytes())
        print('s%-2d %3d->%-3d (%6d rows)      %10.1f %10.1f  %s' % (stride, ci, co, n, ts[0], ts[1], h.hexdigest()[:12]),
              flush=True)


if __name__ == '__main__':
    main()
