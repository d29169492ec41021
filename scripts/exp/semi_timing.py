"""The three pieces of the mean-teacher step (lidal_amd.semi, csrc/semi.hip) against the
straightforward torch formulation -- which lives in this script only -- on the same GPU in ONE process, arms
alternated, one JSON file (default profiles/semi_timing.json):

  * EmaTeacher.update on SPVCNN(19) against torch._foreach_lerp_ over the parameters plus torch._foreach_copy_ over the
    buffers;
  * pseudo_labels on 396 662 x 19 logits and 600 000 points against softmax / max / compare / where / index;
  * consistency_loss forward + backward on 396 662 x 19 logits, 'mse' and 'kl', against F.mse_loss of two softmaxes and
    F.kl_div(log_softmax, softmax, 'batchmean').

Per arm: host time of the call and wall time until the GPU is done on an idle GPU; device time between two events
behind a spin (the fused calls' launches are all queued before the first event passes); kernels and copies counted by
torch's profiler in a call of its own.  Medians of REPS with min .. max after WARMUP calls.  A record, not a gate.

    python scripts/exp/semi_timing.py [--quick] [--out FILE]"""
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as TF

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from lidal_amd import backend as B                                 # noqa: E402
from lidal_amd import semi                                         # noqa: E402
from lidal_amd.network import SPVCNN                               # noqa: E402

QUICK = '--quick' in sys.argv
WARMUP, REPS = (2, 5) if QUICK else (5, 30)
N, C, P = 396662, 19, 600000
SPIN = 4000000 if QUICK else 40000000


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


def ema(dev):
    torch.manual_seed(7122)
    student = SPVCNN(19).to(dev)
    fused = semi.EmaTeacher(student, alpha=0.999, warmup=False)
    other = semi.EmaTeacher(student, alpha=0.999, warmup=False).model           # the torch arm's teacher
    tp, sp = list(other.parameters()), [p.detach() for p in student.parameters()]
    tb, sb = list(other.buffers()), list(student.buffers())
    oma = 1.0 - 0.999

    @torch.no_grad()
    def torch_arm():
        torch._foreach_lerp_(tp, sp, oma)
        torch._foreach_copy_(tb, sb)

    words = sum(p.numel() for p in tp) + sum(b.numel() * (b.element_size() // 4) for b in tb)
    moved = 12 * sum(p.numel() for p in tp) + 8 * sum(b.numel() * (b.element_size() // 4) for b in tb)
    res = measure([('fused', lambda: fused.update()), ('torch', torch_arm)])
    res.update({'tensors': len(tp) + len(tb), 'parameters': len(tp), 'buffers': len(tb), 'words': words,
                'bytes_moved': moved, 'table_uploads': fused.table_uploads, 'fused_launches_counted': fused.launches})
    res['fused']['GB_per_s_device'] = round(moved / (res['fused']['device_ms']['median'] * 1e-3) / 1e9, 1)
    return res


def pseudo(dev):
    g = torch.Generator().manual_seed(7122)
    logits = (torch.randn(N, C, generator=g) * 3).to(dev)
    inverse = torch.randint(0, N, (P,), generator=g).to(dev)
    labels = torch.full((P,), 255, dtype=torch.int64)
    labels[torch.rand(P, generator=g) < 0.02] = 3
    labels = labels.to(dev)
    thr = torch.full((C,), 0.9, device=dev)

    def torch_arm():
        prob = torch.softmax(logits.float(), 1)
        conf, arg = prob.max(1)
        ok = conf >= thr[arg]
        out_v = torch.where(ok, arg, torch.full_like(arg, 255))
        out = torch.where(labels != 255, labels, out_v[inverse])
        taken = (labels == 255) & ok[inverse]
        stats = torch.bincount(arg[inverse][taken], minlength=C)
        return out, stats

    a, _ = semi.pseudo_labels(logits, thr, inverse=inverse, labels=labels)
    b, _ = torch_arm()
    res = measure([('fused', lambda: semi.pseudo_labels(logits, thr, inverse=inverse, labels=labels)), ('torch', torch_arm)])
    res['labels_that_differ'] = int((a != b).sum())                 # (a confidence an ulp from the threshold may)
    return res


def consistency(dev, kind):
    g = torch.Generator().manual_seed(7122)
    zs = (torch.randn(N, C, generator=g) * 3).to(dev).requires_grad_(True)
    zt = (torch.randn(N, C, generator=g) * 3).to(dev)

    def fused():
        zs.grad = None
        semi.consistency_loss(zs, zt, kind=kind).backward()

    def torch_arm():
        zs.grad = None
        if kind == 'mse':
            loss = TF.mse_loss(torch.softmax(zs, 1), torch.softmax(zt, 1))
        else:
            loss = TF.kl_div(torch.log_softmax(zs, 1), torch.softmax(zt, 1), reduction='batchmean')
        loss.backward()

    fused()
    gf = zs.grad.clone()
    torch_arm()
    gt = zs.grad.clone()
    res = measure([('fused', fused), ('torch', torch_arm)])
    res['grad_rel_l2_fused_vs_torch'] = float((gf.double() - gt.double()).norm() / gt.double().norm())
    return res


def main():
    out_path = os.path.join(ROOT, 'profiles', 'semi_timing.json')
    if '--out' in sys.argv:
        out_path = sys.argv[sys.argv.index('--out') + 1]
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    B.lib()
    B.bind_cpus_near(dev.index)
    out = {'metric': 'semi_ms', 'rows': N, 'classes': C, 'points': P, 'reps': REPS, 'warmup': WARMUP}
    out['ema_update_spvcnn19'] = ema(dev)
    out['pseudo_labels'] = pseudo(dev)
    out['consistency_mse_fwd_bwd'] = consistency(dev, 'mse')
    out['consistency_kl_fwd_bwd'] = consistency(dev, 'kl')
    with open(out_path, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
