"""torch.optim.Adam(fused=True) against lidal_amd.optim.Adam (one launch, csrc/optim.hip) in ONE process, interleaved, one
JSON line (profiles/README.md "Adam in one launch"):

  * the training step (bench.py's: SPVCNN, bf16 autocast, the bench's single-scan and 5-scan batches, coordinate tables
    prefetched) with each optimizer: ROUNDS rounds, each STEPS steps of one optimizer and then STEPS steps of the other
    on its own copy of the model, wall time around a synchronise; median over the rounds and their spread (min .. max);
  * the optimizer call alone on the gradients the last step left: host time of the call (the launch is not waited for)
    and device time between two events, median of REPS calls after a warm-up;
  * the bytes the update must move -- 7 x 4 B per element: p, grad, m, v read, p, m, v written -- over the device time.

    python scripts/exp/adam_step.py"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import bench                                                       # noqa: E402
from lidal_amd import backend as B                                 # noqa: E402
from lidal_amd.network import SPVCNN, GeometryPrefetcher           # noqa: E402
from lidal_amd.optim import Adam                                   # noqa: E402
from lidal_amd.train_step import train_step                        # noqa: E402

ROUNDS, STEPS, WARMUP, REPS = 9, 20, 5, 50


class Arm:
    def __init__(self, name, batch, dev):
        torch.manual_seed(7122)
        self.name = name
        self.model = SPVCNN(19).to(dev).train()
        params = list(self.model.parameters())
        self.opt = Adam(params) if name == 'lidal' else torch.optim.Adam(params, fused=True)
        self.batch = batch
        self.pf = GeometryPrefetcher(self.model, device=dev)
        self.ahead = self.pf.submit(batch[0])

    def step(self):
        coords, feats, labels = self.batch
        out = train_step(self.model, self.opt, feats, coords, labels, autocast=True, geometry=self.ahead)
        self.ahead = self.pf.submit(coords)
        return out

    def steps_ms(self, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            self.step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n

    def optimizer_alone(self):
        """(host ms of the call, device ms between events): the gradients of the last step are still there."""
        for _ in range(WARMUP):
            self.opt.step()
        torch.cuda.synchronize()
        host, device = [], []
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(REPS):
            torch.cuda._sleep(4000000)          # (~2 ms of spinning: every launch of the call is queued before the GPU gets to e0)
            e0.record()
            t0 = time.perf_counter()
            self.opt.step()
            host.append((time.perf_counter() - t0) * 1e3)
            e1.record()
            torch.cuda.synchronize()
            device.append(e0.elapsed_time(e1))
        return host, device


def _stats(xs):
    return {'median': round(float(np.median(xs)), 4), 'min': round(float(np.min(xs)), 4), 'max': round(float(np.max(xs)), 4)}


def main():
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    B.lib()
    B.bind_cpus_near(dev.index)
    out = {'metric': 'adam_step_ms', 'rounds': ROUNDS, 'steps_per_round': STEPS, 'reps': REPS}
    for label, frames in (('1scan', 1), ('5scan', 5)):
        batch = bench.make_batch(frames, 120000, 7122, dev)
        arms = [Arm('torch_fused', batch, dev), Arm('lidal', batch, dev)]
        for arm in arms:
            for _ in range(WARMUP):
                arm.step()
        torch.cuda.synchronize()
        times = {arm.name: [] for arm in arms}
        for r in range(ROUNDS):
            for arm in (arms if r % 2 == 0 else arms[::-1]):        # alternate who goes first
                times[arm.name].append(arm.steps_ms(STEPS))
        res = {'voxels': int(batch[0].shape[0])}
        for arm in arms:
            res['step_ms_' + arm.name] = _stats(times[arm.name])
        res['step_ms_gain'] = round(res['step_ms_torch_fused']['median'] - res['step_ms_lidal']['median'], 4)
        if frames == 1:
            n = sum(p.numel() for p in arms[0].model.parameters())
            for arm in arms:
                host, device = arm.optimizer_alone()
                res['optimizer_host_ms_' + arm.name] = _stats(host)
                res['optimizer_device_ms_' + arm.name] = _stats(device)
            mine = arms[1].opt
            res['elements'] = n
            res['bytes_moved_MB'] = round(7 * 4 * n / 1e6, 1)
            res['lidal_TB_per_s'] = round(7 * 4 * n / (res['optimizer_device_ms_lidal']['median'] * 1e-3) / 1e12, 3)
            res['lidal_launches_per_step'] = mine.launches / max(1, WARMUP + ROUNDS * STEPS + WARMUP + REPS)
            res['lidal_table_uploads'] = mine.table_uploads
        out[label] = res
        del arms
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
