"""lidal_amd.optim.AdamW with gradient-norm clipping and lidal_amd.optim.SGD (csrc/optim.hip) against
torch's own on SPVCNN(19)'s 161 parameters, on the same GPU in ONE process, arms alternated, one JSON file (default
profiles/optim_family_timing.json):

  * AdamW(clip_grad_norm=10).step() against torch.nn.utils.clip_grad_norm_(params, 10) followed by
    torch.optim.AdamW(fused=True).step();
  * SGD(momentum=0.9, nesterov=True, weight_decay=1e-4).step() against torch.optim.SGD(foreach=True).step().

Each arm has its own copy of the parameters.  This optimizer's gradients are views of one flat buffer in 16-byte slots, as
the planned training step leaves them; torch's are separate tensors.  Per arm: host time of the call and wall time until
the GPU is done on an idle GPU; device time between two events behind a spin (the launches are all queued before the
first event passes); kernels and copies counted by torch's profiler in a call of its own.  Medians of REPS with
min .. max after WARMUP calls.  A record, not a gate.

    python scripts/exp/optim_family_timing.py [--quick] [--out FILE]"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from lidal_amd import backend as B                                 # noqa: E402
from lidal_amd import optim                                        # noqa: E402
from lidal_amd.network import SPVCNN                               # noqa: E402

QUICK = '--quick' in sys.argv
WARMUP, REPS = (2, 5) if QUICK else (5, 30)
SPIN = 4000000 if QUICK else 40000000
MAX_NORM = 10.0


def _stats(xs):
    return {'median': round(float(np.median(xs)), 4), 'min': round(float(np.min(xs)), 4), 'max': round(float(np.max(xs)), 4)}


def _launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        ev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
        copies = sum(1 for e in ev if 'memcpy' in e.name.lower() or 'memset' in e.name.lower())
        return {'kernels': len(ev) - copies, 'copies_and_memsets': copies} if ev else 'not measured'
    except Exception as e:                                         # a profiler that does not start is not a timing problem
        return 'not measured (%s)' % type(e).__name__


def measure(arms):
    """arms: [(name, fn)] -> {name: {host_ms, wall_ms, device_ms, launches}}."""
    for _, fn in arms:
        for _ in range(WARMUP):
            fn()
    torch.cuda.synchronize()
    host, wall, device = ({n: [] for n, _ in arms} for _ in range(3))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for r in range(REPS):
        for name, fn in (arms if r % 2 == 0 else arms[::-1]):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            host[name].append((t1 - t0) * 1e3)
            wall[name].append((t2 - t0) * 1e3)
    for r in range(REPS):
        for name, fn in (arms if r % 2 == 0 else arms[::-1]):
            torch.cuda._sleep(SPIN)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            device[name].append(e0.elapsed_time(e1))
    return {name: {'host_ms': _stats(host[name]), 'wall_ms': _stats(wall[name]), 'device_ms': _stats(device[name]),
                   'launches': _launches(fn)} for name, fn in arms}


def _parameters(dev):
    """Two copies of SPVCNN(19)'s parameters with the same gradients: ours as views of one flat buffer, torch's apart."""
    torch.manual_seed(7122)
    model = SPVCNN(19).to(dev)
    ours = [torch.nn.Parameter(p.detach().clone()) for p in model.parameters()]
    theirs = [torch.nn.Parameter(p.detach().clone()) for p in model.parameters()]
    total = sum((p.numel() + 3) & -4 for p in ours)
    g = torch.Generator(device=dev).manual_seed(7122)
    flat = torch.randn(total, generator=g, device=dev) * 1e-2
    off = 0
    for p, q in zip(ours, theirs):
        n = p.numel()
        p.grad = flat[off:off + n].view(p.shape)
        q.grad = p.grad.clone()
        off += (n + 3) & -4
    return ours, theirs, flat


def adamw_clip(dev):
    ours, theirs, flat = _parameters(dev)
    mine = optim.AdamW(ours, lr=1e-3, weight_decay=0.01, clip_grad_norm=MAX_NORM)
    torchs = torch.optim.AdamW(theirs, lr=1e-3, weight_decay=0.01, fused=True)

    def torch_arm():
        torch.nn.utils.clip_grad_norm_(theirs, MAX_NORM)
        torchs.step()

    res = measure([('fused', mine.step), ('torch', torch_arm)])
    n = sum(p.numel() for p in ours)
    res.update({'tensors': len(ours), 'elements': n, 'table_uploads': mine.table_uploads,
                'grad_norm': float(mine.grad_norm), 'norm_slots': mine._n_slots,
                'bytes_moved_fused': 4 * n * (1 + 7)})              # the norm reads g; the update reads p g m v, writes p m v
    res['fused']['GB_per_s_device'] = round(res['bytes_moved_fused'] / (res['fused']['device_ms']['median'] * 1e-3) / 1e9, 1)
    return res


def sgd(dev):
    ours, theirs, flat = _parameters(dev)
    kw = dict(lr=1e-3, momentum=0.9, nesterov=True, weight_decay=1e-4)
    mine = optim.SGD(ours, **kw)
    torchs = torch.optim.SGD(theirs, foreach=True, **kw)
    res = measure([('fused', mine.step), ('torch', torchs.step)])
    n = sum(p.numel() for p in ours)
    res.update({'tensors': len(ours), 'elements': n, 'table_uploads': mine.table_uploads,
                'bytes_moved_fused': 4 * n * 5})                    # reads p g buf, writes p buf
    res['fused']['GB_per_s_device'] = round(res['bytes_moved_fused'] / (res['fused']['device_ms']['median'] * 1e-3) / 1e9, 1)
    return res


def main():
    out_path = os.path.join(ROOT, 'profiles', 'optim_family_timing.json')
    if '--out' in sys.argv:
        out_path = sys.argv[sys.argv.index('--out') + 1]
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    B.lib()
    B.bind_cpus_near(dev.index)
    out = {'metric': 'optim_family_ms', 'reps': REPS, 'warmup': WARMUP, 'max_norm': MAX_NORM,
           'norm_block_elems': int(B.lib_handle().lidal_grad_norm_block_elems())}
    out['adamw_clip_spvcnn19'] = adamw_clip(dev)
    out['sgd_nesterov_spvcnn19'] = sgd(dev)
    with open(out_path, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
