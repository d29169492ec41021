"""Device and host times of the panoptic sums on one GPU, one JSON line; a record, not a gate:
  one batch of 5 synthetic scans of about 130 k rows each over the 19 SemanticKITTI classes (8 things), some 70 annotated
  objects per scan; the prediction repeats the annotation except for class flips, objects split in two, pairs of objects
  merged and rows left unassigned.  Three arms over the same device tensors:
    evaluate.panoptic_accumulate   as HIP-event time and as host wall time around a synchronise, median / min / max of
                                   30 calls after 3 warm-ups, and the kernels of one call from torch's profiler by group;
    (a) tests/panoptic_ref.py      numpy on the host, the copy of the four columns to the host counted (--host-reps);
    (b) torch.unique               the formulation a user has without the library: three torch.unique calls, bincounts and
                                   an index_add_ on the same GPU, timed the same way.  Its f64 sums come from atomics, so
                                   their order is not fixed; its integer sums are compared with the library's.
  Run it under a time limit of its own:
    timeout -k 10 300 python scripts/exp/panoptic_timing.py [--host-reps 3] [--out profiles/panoptic_timing.json]"""
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
import panoptic_ref as R                                           # noqa: E402
from lidal_amd import data                                         # noqa: E402
from lidal_amd.evaluate import PanopticStats, panoptic_accumulate  # noqa: E402

REPS, WARM = 30, 3
C, THINGS, MIN_POINTS = 19, data.SK_THINGS, 50
ID_MAX = 2 ** 30 - 2


def _stats(ms):
    return {'median': round(float(np.median(ms)), 4), 'min': round(float(np.min(ms)), 4), 'max': round(float(np.max(ms)), 4)}


def make_scans(seed=0, n_scans=5, rows=130000, n_objects=70):
    """-> per scan (pred_sem i64, pred_inst i32, gt_sem i64, gt_inst i32), the objects annotated in all scans"""
    rng = np.random.RandomState(seed)
    scans, total = [], 0
    for s in range(n_scans):
        p = rows + int(rng.randint(-300, 300))
        gs = rng.choice(np.arange(8, C), p)                        # stuff everywhere ...
        gs[rng.rand(p) < 0.03] = 255                               # ... 3 % unlabelled ...
        gi = np.zeros(p, np.int64)
        at = 0
        for k in range(n_objects + s):                             # ... and the objects, a few hundred rows each
            n = int(rng.randint(30, 900))
            gs[at:at + n], gi[at:at + n] = k % 8, k + 1
            at += n
        total += n_objects + s
        ps, pi = gs.copy(), gi.copy()
        flip = rng.rand(p) < 0.08
        ps[flip] = rng.randint(0, C, int(flip.sum()))
        ps[rng.rand(p) < 0.01] = 255
        split = (gi % 5 == 0) & (gi > 0) & (rng.rand(p) < 0.4)     # every fifth object loses 40 % to a second id
        pi[split] += 1000
        merged = (gi % 7 == 0) & (gi > 0)                          # every seventh object is merged into the next of its class
        pi[merged] += 8
        pi[(rng.rand(p) < 0.05) & (gi > 0)] = -1
        order = rng.permutation(p)
        scans.append((ps[order].astype(np.int64), pi[order].astype(np.int32), gs[order].astype(np.int64),
                      gi[order].astype(np.int32)))
    return scans, total


def torch_arm(ps, pi, gs, gi, scan, is_thing):
    """(tp, fp, fn i64 [C], iou f64 [C]) of one batch by torch.unique; scan: i64 [P], the scan of every row."""
    pi, gi = pi.long(), gi.long()
    live = (gs >= 0) & (gs < C)
    gsc, psc = gs.clamp(0, C - 1), ps.clamp(0, C - 1)
    g_thing = live & is_thing[gsc]
    live = live & ~(g_thing & ((gi < -1) | (gi > ID_MAX)))
    has = live & (ps >= 0) & (ps < C)
    p_thing = has & is_thing[psc]
    has = has & ~(p_thing & ((pi < -1) | (pi > ID_MAX)))
    gkey = (gsc << 36) | (scan << 31) | torch.where(g_thing, gi + 1, torch.zeros_like(gi))
    pkey = (psc << 36) | (scan << 31) | torch.where(p_thing, pi + 1, torch.zeros_like(pi))
    ug, ginv, gcnt = torch.unique(gkey[live], return_inverse=True, return_counts=True)
    up, pinv, pcnt = torch.unique(pkey[has], return_inverse=True, return_counts=True)
    gseg, pseg = torch.full_like(gs, -1), torch.full_like(gs, -1)
    gseg[live], pseg[has] = ginv, pinv
    both = has & (ps == gs)
    pair, inter = torch.unique(gseg[both] * max(len(up), 1) + pseg[both], return_counts=True)
    g, p = pair // max(len(up), 1), pair % max(len(up), 1)
    union = gcnt[g] + pcnt[p] - inter
    m = 2 * inter > union
    gcls, pcls = ug >> 36, up >> 36
    g_hit, p_hit = torch.zeros_like(ug, dtype=torch.bool), torch.zeros_like(up, dtype=torch.bool)
    g_hit[g[m]], p_hit[p[m]] = True, True
    tp = torch.bincount(gcls[g[m]], minlength=C)
    fn = torch.bincount(gcls[~g_hit & (gcnt >= MIN_POINTS)], minlength=C)
    fp = torch.bincount(pcls[~p_hit & (pcnt >= MIN_POINTS)], minlength=C)
    iou = torch.zeros(C, dtype=torch.float64, device=gs.device).index_add_(0, gcls[g[m]], inter[m].double() / union[m].double())
    return tp, fp, fn, iou


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    dev_ms, host_ms, out = [], [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        host_ms.append((time.perf_counter() - t0) * 1e3)
        dev_ms.append(e0.elapsed_time(e1))
    return {'device_ms': _stats(dev_ms), 'host_ms': _stats(host_ms)}, out


def profiled(fn):
    """The kernels of one call by group, from torch's profiler; None where it reports no device activity."""
    try:
        from torch.profiler import profile, ProfilerActivity
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        events = [e for e in prof.events() if str(getattr(e, 'device_type', '')).endswith('CUDA')]
        if not events:
            return None

        def us(e):
            return float(getattr(e, 'device_time_total', 0.0) or getattr(e, 'cuda_time_total', 0.0) or 0.0)
        groups = {'sorts': [0, 0.0], 'scans': [0, 0.0], 'keys_segments_match_finalise': [0, 0.0], 'copies_memsets': [0, 0.0],
                  'torch': [0, 0.0]}
        for e in events:
            name = e.name.lower()
            if 'memcpy' in name or 'memset' in name:
                g = 'copies_memsets'
            elif 'pq_' in name:
                g = 'keys_segments_match_finalise'
            elif 'scan_counts' in name or 'scan_tile' in name:
                g = 'scans'
            elif 'sort_' in name:
                g = 'sorts'
            else:
                g = 'torch'
            groups[g][0] += 1
            groups[g][1] += us(e)
        return {k: {'launches': v[0], 'us': round(v[1], 1)} for k, v in groups.items()}
    except Exception as exc:                                        # a profiler that does not work here is not a result
        return {'error': repr(exc)[:200]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--host-reps', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    scans, n_objects = make_scans()
    cols = [[torch.from_numpy(sc[j]).to(dev) for sc in scans] for j in range(4)]
    flat = [torch.cat(c) for c in cols]
    sizes = [len(sc[0]) for sc in scans]
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    scan = torch.repeat_interleave(torch.arange(len(sizes), device=dev), torch.tensor(sizes, device=dev))
    is_thing = torch.zeros(C, dtype=torch.bool, device=dev)
    is_thing[list(THINGS)] = True
    stats = PanopticStats(C, dev)

    def library():
        return panoptic_accumulate(stats, *cols, things=THINGS, min_points=MIN_POINTS)
    for _ in range(WARM):
        library()
        torch_arm(*flat, scan, is_thing)
    lib_times, _ = timed(library, REPS)
    where = profiled(library) or 'not measured'
    uni_times, uni = timed(lambda: torch_arm(*flat, scan, is_thing), REPS)
    fresh = panoptic_accumulate(PanopticStats(C, dev), *cols, things=THINGS, min_points=MIN_POINTS).cpu()
    mine = {k: getattr(fresh, k).numpy() for k in R.KEYS}
    out = {'metric': 'panoptic_accumulate_ms', 'reps': REPS, 'warm_ups': WARM, 'scans': len(sizes), 'rows': sizes,
           'classes': C, 'things': list(THINGS), 'min_points': MIN_POINTS, 'annotated_objects': int(n_objects),
           'tp': int(mine['tp'].sum()), 'fp': int(mine['fp'].sum()), 'fn': int(mine['fn'].sum()),
           'panoptic_accumulate': dict(lib_times, read_backs=0, device_time_of_one_call=where),
           'torch_unique_same_gpu': dict(uni_times, integer_sums_equal=bool(all(
               np.array_equal(uni[j].cpu().numpy(), mine[k]) for j, k in enumerate(('tp', 'fp', 'fn')))),
               iou_max_abs_difference=float(np.abs(uni[3].cpu().numpy() - mine['iou']).max()))}
    ref_ms, want = [], None
    for _ in range(max(args.host_reps, 0)):
        t0 = time.perf_counter()
        want = R.panoptic_ref(*[t.cpu().numpy() for t in flat], ptr, C, THINGS, MIN_POINTS)
        ref_ms.append((time.perf_counter() - t0) * 1e3)
    if ref_ms:
        out['numpy_host'] = {'host_ms': _stats(ref_ms), 'reps': len(ref_ms), 'same_bits': bool(R.same(mine, want))}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
