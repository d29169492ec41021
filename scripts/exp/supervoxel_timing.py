"""Times of the size-constrained k-means supervoxels on one GPU, one JSON line:
  one raycast scan of about 130 k points, K = 20, slack 0.05; `data.kmeans_supervoxels` for a batch of 1 and a batch of
  64 (the same scan with 5 mm of seeded jitter per copy, so that every frame is its own problem), host wall time until
  the results are read back, median of 3 calls after a warm-up; the balanced assignment alone (`data.balanced_assign`
  on the costs to the seed rows) for the same batches, so that what the host-driven seeding, update and sorts cost is
  the difference; the augmentation counts; and the CPU time of scipy's HiGHS on the transportation LP of a 12 k-point
  scan, the only exact solver at hand (the reference's own solver is not available: no comparison with it).
    python scripts/exp/supervoxel_timing.py [--batch 64]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
import supervoxel_inputs as SI                                     # noqa: E402
import supervoxel_ref as R                                         # noqa: E402
from lidal_amd import data                                         # noqa: E402

REPS = 3


def _wall(fn):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(ms)), 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--no-lp', action='store_true')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    xyz = SI.full_scan()
    rng = np.random.RandomState(0)
    scans = [torch.from_numpy(xyz).to(dev)]
    for _ in range(args.batch - 1):
        scans.append(torch.from_numpy((xyz + rng.randn(*xyz.shape).astype(np.float32) * 0.005)).to(dev))
    p, k = len(xyz), 20
    lo, hi = data.supervoxel_bounds(p, k)
    out = {'metric': 'supervoxel_ms', 'points': p, 'clusters': k, 'size_min': lo, 'size_max': hi, 'batch': args.batch,
           'reps': REPS}
    res = data.kmeans_supervoxels(scans, details=True)
    out['augmentations_first'] = [r[3]['augmentations'][0] for r in res][:4]
    out['augmentations_second'] = [r[3]['augmentations'][1] for r in res][:4]
    out['augmentations_batch_mean'] = round(float(np.mean([sum(r[3]['augmentations']) for r in res])), 1)
    out['supervoxels_batch1_ms'] = _wall(lambda: data.kmeans_supervoxels(scans[0]))
    t = _wall(lambda: data.kmeans_supervoxels(scans))
    out['supervoxels_batch%d_ms' % args.batch], out['supervoxels_batch%d_ms_per_frame' % args.batch] = t, round(
        t / args.batch, 2)
    costs = [data.supervoxel_costs(s, s.double()[r[3]['seeds'].long()]) for s, r in zip(scans, res)]
    out['assign_first_batch1_ms'] = _wall(lambda: data.balanced_assign(costs[0], lo, hi))
    t = _wall(lambda: data.balanced_assign(costs, lo, hi))
    out['assign_first_batch%d_ms' % args.batch], out['assign_first_batch%d_ms_per_frame' % args.batch] = t, round(
        t / args.batch, 2)
    out['assign_first_us_per_augmentation_batch1'] = round(
        1e3 * out['assign_first_batch1_ms'] / max(1, res[0][3]['augmentations'][0]), 2)
    if not args.no_lp:
        small = SI.scan(*SI.FRAMES[1][1:])
        r = R.supervoxel_kmeans(small)
        t0 = time.perf_counter()
        lp = R.lp_optimum(r['cost1'], r['lo'], r['hi'])
        out['highs_lp_points'] = len(small)
        out['highs_lp_first_assignment_s'] = round(time.perf_counter() - t0, 2)
        out['highs_lp_equals_kernel_objective'] = bool(
            lp == data.kmeans_supervoxels(torch.from_numpy(small).to(dev), details=True)[3]['objective'][0])
    print(json.dumps(out))


if __name__ == '__main__':
    main()
