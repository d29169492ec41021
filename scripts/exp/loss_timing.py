"""The Lovasz-softmax loss of lidal_amd (csrc/loss.hip, ONE sort for all classes) against the well-known pure-torch
formulation (per class: mask, abs, sort, gather, two cumsums, dot) on the same GPU in ONE process, arms alternated, one
JSON line (profiles/README.md "Lovasz-softmax in one sort"):

  * the loss alone, forward + backward, at the bench batch's size (396 662 rows, 19 classes), fully labelled and with
    2 % of the rows labelled.  On an idle GPU: host time of the call and wall time until the GPU is done (the torch
    formulation synchronises inside the call, so the two coincide for it; the fused call only enqueues).  Behind a spin
    on the GPU: device time between two events (the fused call's launches are all queued before the first event
    passes; the torch arm's figure includes the host's gaps).  Kernel launches counted by torch's profiler in a call of
    its own.  Medians of REPS with min .. max;
  * the training step (bench.py's: SPVCNN, bf16 autocast, single-scan and 5-scan batches, coordinate tables
    prefetched, lidal_amd.optim.Adam) with the default objective, with combined_loss (its default: nothing read back)
    and with combined_loss(check_labels=True) (one read-back per step): ROUNDS rounds of STEPS steps each, arms
    alternated, wall time around a synchronise.

    python scripts/exp/loss_timing.py [--quick]"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import bench                                                       # noqa: E402
import loss_ref as R                                               # noqa: E402
from lidal_amd import backend as B                                 # noqa: E402
from lidal_amd.network import SPVCNN, GeometryPrefetcher           # noqa: E402
from lidal_amd.nn import functional as F                           # noqa: E402
from lidal_amd.optim import Adam                                   # noqa: E402
from lidal_amd.train_step import train_step                        # noqa: E402

QUICK = '--quick' in sys.argv
ROUNDS, STEPS, WARMUP, REPS = (3, 5, 2, 5) if QUICK else (7, 20, 5, 30)
N, C = 396662, 19


def _stats(xs):
    return {'median': round(float(np.median(xs)), 4), 'min': round(float(np.min(xs)), 4), 'max': round(float(np.max(xs)), 4)}


def _fused(z, labels):
    z.grad = None
    F.lovasz_softmax(z, labels, check_labels=False).backward()


def _torch(z, labels):
    z.grad = None
    R.torch_lovasz_softmax(z, labels).backward()


def _launches(fn, z, labels):
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn(z, labels)
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
        return n if n > 0 else 'not measured'
    except Exception as e:                                         # a profiler that does not start is not a timing problem
        return 'not measured (%s)' % type(e).__name__


def loss_alone(dev):
    g = torch.Generator().manual_seed(7122)
    logits = (torch.randn(N, C, generator=g) * 3).to(dev)
    full = torch.randint(0, C, (N,), generator=g)
    res = {}
    for name, frac in (('labelled_100', 1.0), ('labelled_2', 0.02)):
        lab = full.clone()
        lab[torch.rand(N, generator=g) >= frac] = 255
        lab = lab.to(dev)
        z = logits.clone().requires_grad_(True)
        arms = [('fused', _fused), ('torch', _torch)]
        for _, fn in arms:
            for _ in range(WARMUP):
                fn(z, lab)
        torch.cuda.synchronize()
        _fused(z, lab)
        gf = z.grad.clone()
        lf = F.lovasz_softmax(z, lab).item()
        _torch(z, lab)
        gt = z.grad.clone()
        lt = R.torch_lovasz_softmax(z, lab).item()
        host, wall, device = ({'fused': [], 'torch': []} for _ in range(3))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        # 1. on an idle GPU: host time of the call alone, and wall time until the GPU is done.  The torch formulation
        #    synchronises inside the call (boolean-mask indexing, `fg.sum() == 0` per class), so its host time IS its
        #    wall time; the fused call only enqueues.
        for r in range(REPS):
            for arm, fn in (arms if r % 2 == 0 else arms[::-1]):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(z, lab)
                t1 = time.perf_counter()
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                host[arm].append((t1 - t0) * 1e3)
                wall[arm].append((t2 - t0) * 1e3)
        # 2. device time between two events behind ~17 ms of spinning: the fused call's launches are all queued before the
        #    GPU reaches e0, so this is its kernels back to back.  The torch arm waits for the spin at its first
        #    synchronisation and then runs in lock-step with the GPU: its figure includes the host's gaps.
        for r in range(REPS):
            for arm, fn in (arms if r % 2 == 0 else arms[::-1]):
                torch.cuda._sleep(40000000)
                e0.record()
                fn(z, lab)
                e1.record()
                torch.cuda.synchronize()
                device[arm].append(e0.elapsed_time(e1))
        one = {'valid_rows': int((lab != 255).sum()), 'loss_fused': lf, 'loss_torch': lt,
               'grad_rel_l2_fused_vs_torch': float((gf.double() - gt.double()).norm() / gt.double().norm())}
        for arm, fn in arms:
            one['host_ms_' + arm] = _stats(host[arm])
            one['wall_ms_' + arm] = _stats(wall[arm])
            one['device_ms_' + arm] = _stats(device[arm])
            one['launches_' + arm] = _launches(fn, z, lab)
        res[name] = one
    return res


class Arm:
    def __init__(self, name, batch, dev):
        torch.manual_seed(7122)
        self.name = name
        self.model = SPVCNN(19).to(dev).train()
        self.opt = Adam(list(self.model.parameters()))
        self.batch = batch
        self.pf = GeometryPrefetcher(self.model, device=dev)
        self.ahead = self.pf.submit(batch[0])
        self.criterion = {'default': None, 'combined': F.combined_loss,
                          'combined_checked': lambda z, y: F.combined_loss(z, y, check_labels=True)}[name]

    def step(self):
        coords, feats, labels = self.batch
        out = train_step(self.model, self.opt, feats, coords, labels, autocast=True, geometry=self.ahead,
                         criterion=self.criterion)
        self.ahead = self.pf.submit(coords)
        return out

    def steps_ms(self, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            self.step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n


def steps(dev):
    res = {}
    for label, frames in (('1scan', 1), ('5scan', 5)):
        batch = bench.make_batch(frames, 120000, 7122, dev)
        arms = [Arm(n, batch, dev) for n in ('default', 'combined', 'combined_checked')]
        for arm in arms:
            for _ in range(WARMUP):
                arm.step()
        torch.cuda.synchronize()
        times = {arm.name: [] for arm in arms}
        for r in range(ROUNDS):
            k = r % len(arms)
            for arm in arms[k:] + arms[:k]:                        # rotate who goes first
                times[arm.name].append(arm.steps_ms(STEPS))
        one = {'voxels': int(batch[0].shape[0]), 'logit_dtype': str(arms[0].step()[1].dtype)}
        for arm in arms:
            one['step_ms_' + arm.name] = _stats(times[arm.name])
        for n in ('combined', 'combined_checked'):
            one['added_ms_' + n] = round(one['step_ms_' + n]['median'] - one['step_ms_default']['median'], 4)
        res[label] = one
        del arms
        torch.cuda.empty_cache()
    return res


def main():
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    B.lib()
    B.bind_cpus_near(dev.index)
    out = {'metric': 'lovasz_loss_ms', 'rows': N, 'classes': C, 'reps': REPS, 'rounds': ROUNDS, 'steps_per_round': STEPS}
    out['loss_alone'] = loss_alone(dev)
    print(json.dumps(out), flush=True)
    out['step'] = steps(dev)
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
