"""Time of a scan-to-scan registration (lidal_amd/score/registration.py) on one GPU, one JSON line.
A measurement, not a gate.
  workload   two synthetic scans of --points points (64 beams x 2048 azimuths, thinned), 1.04 m and 2 degrees apart
  normals    IcpTarget of the first scan: the k-NN search, the normals kernel, the f64 copy (the grid is built at the first
             icp() and is timed there, in the warm-up)
  icp        icp(check=False) from the identity with the default schedule, stride 1 and 4: stream ms between two events
             around the call, host ms the host clock around the enqueue alone; the iterations that ran, from the trace
  split      torch.profiler over one run per stride: device time of the accumulate and of the finish kernels
  cells      stride 1 again on grids of --cells metres (the default grid's cell is the largest max_dist, 1 m); the pose
             must come out the same bits
One warm-up, then --passes runs; the median with min .. max.
    python scripts/exp/icp_timing.py [--points 120000] [--passes 7] [--cells 0.5 0.25] [--out FILE]"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from lidal_amd import synth                                           # noqa: E402
from lidal_amd.score import IcpTarget, icp                            # noqa: E402
from lidal_amd.score.registration import TRACE                        # noqa: E402


def timed(fn, passes):
    """(median, min, max) stream ms and median host ms of fn() over `passes` runs after one warm-up."""
    fn()
    torch.cuda.synchronize()
    stream, host = [], []
    for _ in range(passes):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        host.append((time.perf_counter() - t0) * 1e3)
        torch.cuda.synchronize()
        stream.append(e0.elapsed_time(e1))
    return {'stream_ms': float(np.median(stream)), 'stream_min': min(stream), 'stream_max': max(stream),
            'host_ms': float(np.median(host))}


def kernel_split(fn):
    """Device ms of one fn() by kernel: {'accumulate': ..., 'finish': ..., 'other': ...}, launches alongside."""
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        out = {'accumulate_ms': 0.0, 'finish_ms': 0.0, 'other_ms': 0.0, 'launches': 0}
        for e in prof.key_averages():
            if e.device_type != torch.autograd.DeviceType.CUDA:
                continue
            us = getattr(e, 'device_time_total', None)
            if us is None:
                us = e.cuda_time_total
            key = 'accumulate_ms' if 'icp_accumulate' in e.key else 'finish_ms' if 'icp_finish' in e.key else 'other_ms'
            out[key] += us / 1e3
            out['launches'] += e.count
        return out
    except Exception as e:                                   # the split is a by-product: report why it is missing
        return 'not measured (%s)' % type(e).__name__


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--points', type=int, default=120000)
    ap.add_argument('--passes', type=int, default=7)
    ap.add_argument('--cells', type=float, nargs='*', default=[0.5, 0.25])
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    world = synth.make_world(7122)
    yaw = math.radians(2.0)
    rz = np.array([[math.cos(yaw), -math.sin(yaw), 0.0], [math.sin(yaw), math.cos(yaw), 0.0], [0.0, 0.0, 1.0]])
    host = [synth.raycast_scan(world, o, np.random.default_rng([7122, f]), n_points=args.points)[0]
            for f, o in enumerate(((10.0, 0.0), (11.0, 0.3)))]
    host[1] = (host[1].astype(np.float64) @ rz).astype(np.float32)
    dev = [torch.from_numpy(np.ascontiguousarray(h)).cuda() for h in host]
    truth = np.eye(4)
    truth[:3, :3], truth[:3, 3] = rz, (1.0, 0.3, 0.0)
    out = {'points': [int(d.shape[0]) for d in dev], 'passes': args.passes, 'device': torch.cuda.get_device_name(0)}
    out['normals'] = timed(lambda: IcpTarget(dev[0]), args.passes)
    target = IcpTarget(dev[0])
    out['normals']['zeroed'] = float((target.normals == 0).all(1).double().mean())
    for stride in (1, 4):
        run = lambda: icp(dev[1], target, stride=stride, check=False)           # noqa: E731
        rec = timed(run, args.passes)
        pose, trace = run()
        trace = trace.cpu()
        status = trace[:, TRACE['status']].to(torch.int64).tolist()
        err = np.abs(pose.cpu().numpy() - truth)
        rec.update(iterations=sum(s in (0, 1) for s in status), status=status,
                   pairs_last=int(max(trace[i, TRACE['pairs']] for i, s in enumerate(status) if s in (0, 1))),
                   translation_error=float(err[:3, 3].max()), rotation_error=float(err[:3, :3].max()),
                   kernels=kernel_split(run))
        out['icp_stride_%d' % stride] = rec
    # the same run on grids of smaller cells (the default is the largest max_dist, 1 m): more cells probed, shorter walks
    for cell in args.cells:
        small = IcpTarget(dev[0], cell=cell)
        run = lambda: icp(dev[1], small, check=False)                           # noqa: E731
        rec = timed(run, args.passes)
        rec['same_pose'] = bool(torch.equal(run()[0], icp(dev[1], target, check=False)[0]))
        out['icp_stride_1_cell_%g' % cell] = rec
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
