"""Times of the VCCS supervoxels on one GPU, one JSON line:
  one raycast scan of about 130 k points at the default resolutions; `data.vccs_supervoxels` for a batch of 1 and a
  batch of 64 (the same scan with 5 mm of seeded jitter per copy, so that every frame is its own problem), host wall
  time until the results are read back, median of 5 calls after a warm-up; the device time of the library call alone
  (events on the launch stream); and the numpy restatement's CPU time for the same scan.  No comparison with the PCL
  library exists: it is not available here.
    python scripts/exp/vccs_timing.py [--batch 64] [--no-ref]
  The split between the stages comes from a kernel trace, in a run of its own:
    rocprofv3 --kernel-trace --output-format csv -d OUT -- python scripts/exp/vccs_timing.py --once [--batch 64]
    python scripts/exp/vccs_timing.py --trace OUT/.../*_kernel_trace.csv
  --once makes three batched calls and leaves; --trace adds up the kernels of the last call by stage.  The stages are
  told apart by the kernel that opens them (point_key: voxels; adjacency: normals; seed_key: seeds; state_init: rounds;
  label: CSR), so the sorts and scans count where they run; torch's own kernels (the concatenation, the finiteness
  check, the slicing of the results) are listed apart."""
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
import vccs_ref as R                                               # noqa: E402
from lidal_amd import backend as B                                 # noqa: E402
from lidal_amd import data                                         # noqa: E402

REPS = 5


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


def _library_ms(scans):
    """Device time of the lidal_vccs call alone (events on the launch stream), median of REPS."""
    times = []

    def sink(name, args, e0, e1):
        if name == 'lidal_vccs':
            times.append((e0, e1))

    try:
        B.set_call_timer(sink)
        for _ in range(REPS + 1):
            data.vccs_supervoxels(scans)
        torch.cuda.synchronize()
    finally:
        B.set_call_timer(None)
    return round(float(np.median([a.elapsed_time(b) for a, b in times[1:]])), 2)


OPENERS = (('point_key_kernel', 'voxels'), ('adjacency_kernel', 'normals'), ('seed_key_kernel', 'seeds'),
           ('state_init_kernel', 'rounds'), ('label_kernel', 'csr'))
OURS = ('_kernel', 'rocclr')          # the library's kernels (anonymous namespace of vccs.hip / sort.hip) and its memsets


def trace_split(path):
    """Kernel time per stage of the LAST lidal_vccs call in a rocprofv3 kernel trace, ms."""
    import csv
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r['Start_Timestamp']))
    starts = [i for i, r in enumerate(rows) if 'point_key_kernel' in r['Kernel_Name']]
    stage, out = None, {}
    for r in rows[starts[-1]:]:
        name = r['Kernel_Name']
        for opener, st in OPENERS:
            if opener in name:
                stage = st
        mine = 'at::native' not in name and any(t in name for t in OURS)
        key = stage if mine else 'torch'
        out[key] = out.get(key, 0.0) + (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e6
    return {k: round(v, 3) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--no-ref', action='store_true')
    ap.add_argument('--once', action='store_true')
    ap.add_argument('--trace')
    args = ap.parse_args()
    if args.trace:
        print(json.dumps({'metric': 'vccs_stage_ms', **trace_split(args.trace)}))
        return
    dev = torch.device('cuda:0')
    xyz = SI.full_scan()
    rng = np.random.RandomState(0)
    scans = [torch.from_numpy(xyz).to(dev)]
    for _ in range(args.batch - 1):
        scans.append(torch.from_numpy((xyz + rng.randn(*xyz.shape).astype(np.float32) * 0.005)).to(dev))
    p = len(xyz)
    if args.once:
        for _ in range(3):
            data.vccs_supervoxels(scans)
        torch.cuda.synchronize()
        return
    min_seed, rounds = data.vccs_parameters()
    res = data.vccs_supervoxels(scans[0], details=True)
    out = {'metric': 'vccs_ms', 'points': p, 'voxels': int(res[3]['owners'].numel()),
           'seeds': int(res[3]['seed_voxels'].numel()), 'rounds': rounds, 'min_seed': round(min_seed, 3),
           'supervoxels_kept': int(res[1].numel() - 1), 'points_unlabelled': int((res[0] == 0).sum()),
           'batch': args.batch, 'reps': REPS}
    out['vccs_batch1_ms'] = _wall(lambda: data.vccs_supervoxels(scans[0]))
    t = _wall(lambda: data.vccs_supervoxels(scans))
    out['vccs_batch%d_ms' % args.batch], out['vccs_batch%d_ms_per_frame' % args.batch] = t, round(t / args.batch, 2)
    out['library_batch1_ms'] = _library_ms(scans[:1])
    out['library_batch%d_ms' % args.batch] = _library_ms(scans)
    if not args.no_ref:
        t0 = time.perf_counter()
        r = R.vccs(xyz)
        out['restatement_cpu_s'] = round(time.perf_counter() - t0, 2)
        out['restatement_equals_kernel_labels'] = bool(np.array_equal(r['labels'], res[0].cpu().numpy()))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
