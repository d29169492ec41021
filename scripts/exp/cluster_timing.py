"""Device and host times of Euclidean clustering on one GPU, one JSON line; a record, not a gate:
  5 raycast scans of about 130 k points each, labelled by geometry (ground and building fronts are not clustered; what
  stands between the fronts is class 1 below 0.3 m and class 2 above), tolerance 0.5 m for both thing classes, one call
  for the batch.  Two arms: data.euclidean_clusters, as HIP-event time and as host wall time around a synchronise, median /
  min / max of 30 calls after 3 warm-ups, and where its device time goes (the kernels of one call from torch's profiler,
  grouped into sorts, union and the rest: keys, records and tables); and the formulation a user has without it --
  scipy.spatial.cKDTree.query_pairs per scan and class plus scipy.sparse.csgraph.connected_components on the host, the
  copy of points and labels to the host counted -- as host wall time (fewer calls: --host-reps, it takes seconds).  The
  host arm lives in this script only; its partition is compared with the library's.
    python scripts/exp/cluster_timing.py [--host-reps 3] [--out profiles/cluster_timing.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from lidal_amd import data, synth                                  # noqa: E402

REPS, WARM = 30, 3
TOL = {1: 0.5, 2: 0.5}
MIN_POINTS = 10


def _stats(ms):
    return {'median': round(float(np.median(ms)), 4), 'min': round(float(np.min(ms)), 4), 'max': round(float(np.max(ms)), 4)}


def make_scans():
    world = synth.make_world(3)
    scans, labels = [], []
    for i in range(5):
        pts, _ = synth.raycast_scan(world, (30.0 + 2.0 * i, 0.0), np.random.default_rng([0, i]))
        lab = np.where(pts[:, 2] < -synth.SENSOR_H + 0.2, 0, np.where(np.abs(pts[:, 1]) >= 9.0, 3,
                       np.where(pts[:, 2] < 0.3, 1, 2))).astype(np.int64)
        scans.append(pts)
        labels.append(lab)
    return scans, labels


def host_arm(scans_dev, labels_dev):
    """root per point (-1: not clustered), by scipy on the host; the copies from the device are part of it."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    from scipy.spatial import cKDTree
    out, pairs_total, off = [], 0, 0
    for x, l in zip(scans_dev, labels_dev):
        xyz, lab = x.cpu().numpy().astype(np.float64), l.cpu().numpy()
        root = np.full(len(xyz), -1, dtype=np.int64)
        for c, t in TOL.items():
            rows = np.nonzero(lab == c)[0]
            if not len(rows):
                continue
            pairs = cKDTree(xyz[rows]).query_pairs(t, output_type='ndarray')
            pairs_total += len(pairs)
            graph = coo_matrix((np.ones(len(pairs), dtype=np.int8), (pairs[:, 0], pairs[:, 1])), shape=(len(rows),) * 2)
            _, comp = connected_components(graph, directed=False)
            first = np.full(comp.max() + 1, len(xyz), dtype=np.int64)
            np.minimum.at(first, comp, rows)
            root[rows] = first[comp] + off
        out.append(root)
        off += len(xyz)
    return np.concatenate(out), pairs_total


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
        groups = {'sorts': [0, 0.0], 'union': [0, 0.0], 'keys_records_tables': [0, 0.0], 'copies_memsets': [0, 0.0],
                  'torch': [0, 0.0]}
        for e in events:
            name = e.name.lower()
            if 'memcpy' in name or 'memset' in name:
                g = 'copies_memsets'
            elif 'ec_union' in name:
                g = 'union'
            elif any(t in name for t in ('ec_', 'scan_counts', 'scan_tile', 'records_kernel')):
                g = 'keys_records_tables'
            elif 'at::' in name or 'elementwise' in name or 'cat' in name:
                g = 'torch'
            else:
                g = 'sorts'
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
    scans, labels = make_scans()
    sd, ld = [torch.from_numpy(x).to(dev) for x in scans], [torch.from_numpy(l).to(dev) for l in labels]

    def library():
        return data.euclidean_clusters(sd, ld, tolerance=TOL, min_points=MIN_POINTS)
    for _ in range(WARM):
        ins = library()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    dev_ms, host_ms = [], []
    for _ in range(REPS):
        t0 = time.perf_counter()
        e0.record()
        ins = library()
        e1.record()
        torch.cuda.synchronize()
        host_ms.append((time.perf_counter() - t0) * 1e3)
        dev_ms.append(e0.elapsed_time(e1))
    where = profiled(library) or 'not measured'
    scipy_ms, pairs = [], 0
    for _ in range(max(args.host_reps, 0)):
        t0 = time.perf_counter()
        root, pairs = host_arm(sd, ld)
        scipy_ms.append((time.perf_counter() - t0) * 1e3)
    out = {'metric': 'euclidean_clusters_ms', 'reps': REPS, 'warm_ups': WARM, 'scans': 5,
           'points': [int(len(x)) for x in scans],
           'clustered_points': int(sum(int(np.isin(l, list(TOL)).sum()) for l in labels)), 'tolerance': TOL,
           'min_points': MIN_POINTS, 'instances': len(ins), 'points_in_instances': int(ins.members.numel()),
           'euclidean_clusters': {'device_ms': _stats(dev_ms), 'host_ms': _stats(host_ms), 'read_backs': 1,
                                  'device_time_of_one_call': where}}
    if scipy_ms:
        # the same partition?  scipy decides in f64: a pair within rounding of 0.5 m may fall on the other side
        inst = ins.inst.cpu().numpy()
        sizes = np.bincount(root[root >= 0], minlength=len(root))
        kept = (root >= 0) & (sizes[np.maximum(root, 0)] >= MIN_POINTS)
        first = ins.members[ins.member_ptr[:-1]].cpu().numpy().astype(np.int64)
        mine = np.where(inst >= 0, first[np.maximum(inst, 0)], -1)
        out['scipy_host'] = {'host_ms': _stats(scipy_ms), 'reps': len(scipy_ms), 'pairs': int(pairs),
                             'points_on_another_side': int((np.where(kept, root, -1) != mine).sum())}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
