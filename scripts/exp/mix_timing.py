"""Device and host times of building mixed samples on one GPU, one JSON line:
  5 raycast scans of about 130 k points each; per batch one LaserMix pair and one PolarMix pair with 3 rotations (4 mixed
  samples); two arms in the same process, alternating call by call -- the straightforward torch formulation (atan2,
  boolean masks, nonzero, cat; it lives in this script only) and data.mix_scans; each as HIP-event time and as host wall
  time around a synchronise, median / min / max of 30 calls after a warm-up, with fresh draws every round (the same for
  both arms); the kernels, copies and read-backs of one call of each arm (kernels, their device time and copies from torch's
  profiler, 'not measured' where it gives nothing; read-backs counted by the arms themselves); and how many rows of the two arms
  differ: the torch arm decides by atan2 and may put a point next to a boundary on the other side.
    python scripts/exp/mix_timing.py"""
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from lidal_amd import data, synth                                  # noqa: E402

REPS = 30
PASTE = (1, 5, 6, 7)
READ_BACKS = {'torch': 0, 'mix_scans': 0}


def _stats(ms):
    return {'median': round(float(np.median(ms)), 4), 'min': round(float(np.min(ms)), 4), 'max': round(float(np.max(ms)), 4)}


def _rows(keep):
    READ_BACKS['torch'] += 1                                        # nonzero sizes its result on the host
    return keep.nonzero().squeeze(1)


def torch_arm(scans, labels, row0, mixes):
    """The same samples with torch ops: per mix and scan the angles, a mask per part, nonzero, gathers, one cat per
    output.  Returns the dict of mix_scans (point_ptr and parts from the shapes: no further read-back)."""
    dev = scans[0][0].device
    pts, inten, lab, src, ptr, parts = [], [], [], [], [0], []
    for m in mixes:
        bounds = torch.from_numpy(np.arctan(m.tans.astype(np.float64))).to(dev)
        cells = (len(m.tans) + 1) * (1 if m.wedge is None else 2)
        count = [0] * 6
        for part, (j, take) in enumerate(((m.a, m.take_a), (m.b, m.take_b))):
            xyz = scans[j][0]
            x, y, z = xyz[:, 0].double(), xyz[:, 1].double(), xyz[:, 2].double()
            cell = (torch.atan2(z, torch.hypot(x, y))[:, None] >= bounds[None, :]).sum(1)
            if m.wedge is not None:
                alpha = math.atan2(float(m.wedge[1]), float(m.wedge[0]))
                rel = torch.remainder(torch.atan2(y, x) - alpha, 2 * math.pi)
                cell = cell + (len(m.tans) + 1) * (rel < math.pi)
            table = torch.tensor([(take >> c) & 1 for c in range(cells)], dtype=torch.bool, device=dev)
            idx = _rows(table[cell])
            pts.append(xyz[idx]), inten.append(scans[j][1][idx]), lab.append(labels[j][idx]), src.append(idx + row0[j])
            count[part] = idx.shape[0]
        if len(m.paste_rot):
            classes = torch.tensor([c for c in range(64) if (m.paste_classes >> c) & 1], device=dev)
            idx = _rows(torch.isin(labels[m.b], classes))
            xyz = scans[m.b][0][idx]
            for k, (c, s) in enumerate(m.paste_rot):
                rot = torch.stack([float(c) * xyz[:, 0] - float(s) * xyz[:, 1], float(s) * xyz[:, 0] + float(c) * xyz[:, 1],
                                   xyz[:, 2]], 1)
                pts.append(rot), inten.append(scans[m.b][1][idx]), lab.append(labels[m.b][idx]), src.append(idx + row0[m.b])
                count[2 + k] = idx.shape[0]
        parts.append(count)
        ptr.append(ptr[-1] + sum(count))
    return {'points': torch.cat(pts), 'intensity': torch.cat(inten), 'labels': torch.cat(lab), 'src': torch.cat(src),
            'point_ptr': np.array(ptr, dtype=np.int64), 'parts': np.array(parts, dtype=np.int64)}


def library_arm(scans, labels, mixes):
    READ_BACKS['mix_scans'] += 1
    return data.mix_scans([s[0] for s in scans], [s[1] for s in scans], labels, mixes)


def draw(rs):
    return list(data.draw_lasermix(0, 1, rs)) + list(data.draw_polarmix(2, 3, rs, PASTE, n_rot=3))


def rows_differing(a, b):
    """Rows (as (mix, part, source row) triples) that one arm holds and the other does not."""
    def triples(o):
        ids = np.repeat(np.arange(o['parts'].size), o['parts'].reshape(-1))
        return set(zip(ids.tolist(), o['src'].cpu().numpy().tolist()))
    return len(triples(a) ^ triples(b))


def profiled(fn):
    """Kernels and copies of one call, from torch's profiler; None where it reports no device activity."""
    try:
        from torch.profiler import profile, ProfilerActivity
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        dev_events = [e for e in prof.events() if str(getattr(e, 'device_type', '')).endswith('CUDA')]
        if not dev_events:
            return None
        def us(e):
            return float(getattr(e, 'device_time_total', 0.0) or getattr(e, 'cuda_time_total', 0.0) or 0.0)
        copies = [e for e in dev_events if 'memcpy' in e.name.lower()]
        kernels = [e for e in dev_events if 'memcpy' not in e.name.lower() and 'memset' not in e.name.lower()]
        res = {'kernels': len(kernels), 'copies': len(copies), 'memsets': len(dev_events) - len(kernels) - len(copies),
               'kernel_us_total': round(sum(us(e) for e in kernels), 1)}
        if len(kernels) <= 8:
            res['kernel_us'] = [[e.name.replace('(anonymous namespace)::', '').split('(')[0][-40:], round(us(e), 1)] for e in kernels]
        return res
    except Exception as exc:                                        # a profiler that does not work here is not a result
        return {'error': repr(exc)[:200]}


def main():
    dev = torch.device('cuda:0')
    world = synth.make_world(3)
    scans, labels = [], []
    for i in range(5):
        pts, inten = synth.raycast_scan(world, (30.0 + 2.0 * i, 0.0), np.random.default_rng([0, i]))
        scans.append((torch.from_numpy(pts).to(dev), torch.from_numpy(inten).to(dev)))
        lab = np.random.default_rng([1, i]).choice(20, len(pts), p=[0.05] * 19 + [0.05]).astype(np.int64)
        lab[lab == 19] = 255
        lab[np.isin(lab, PASTE) & (np.random.default_rng([2, i]).uniform(size=len(pts)) > 0.05)] = 9      # rare classes: 1 % of the points
        labels.append(torch.from_numpy(lab).to(dev))
    row0 = np.concatenate([[0], np.cumsum([s[0].shape[0] for s in scans])])[:-1].tolist()
    rs = np.random.RandomState(7)
    arms = {'torch': lambda mx: torch_arm(scans, labels, row0, mx), 'mix_scans': lambda mx: library_arm(scans, labels, mx)}
    for _ in range(3):
        mixes = draw(rs)
        for fn in arms.values():
            fn(mixes)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    dev_ms, host_ms = {k: [] for k in arms}, {k: [] for k in arms}
    differing, rows = [], []
    for _ in range(REPS):
        mixes = draw(rs)
        outs = {}
        for name, fn in arms.items():
            t0 = time.perf_counter()
            e0.record()
            outs[name] = fn(mixes)
            e1.record()
            torch.cuda.synchronize()
            host_ms[name].append((time.perf_counter() - t0) * 1e3)
            dev_ms[name].append(e0.elapsed_time(e1))
        differing.append(rows_differing(outs['torch'], outs['mix_scans']))
        rows.append(int(outs['mix_scans']['point_ptr'][-1]))
    mixes = draw(rs)
    for k in READ_BACKS:
        READ_BACKS[k] = 0
    counted = {}
    for name, fn in arms.items():
        counted[name] = {'profiler': profiled(lambda: fn(mixes)) or 'not measured', 'read_backs': READ_BACKS[name]}
    slots = data._mix_arguments([s[0].shape[0] for s in scans], mixes, True)[1]
    out = {'metric': 'mix_scans_ms', 'reps': REPS, 'scans': 5, 'points': [int(s[0].shape[0]) for s in scans], 'mixes': 4,
           'slots': int(slots), 'rows_out': {'median': int(np.median(rows)), 'min': min(rows), 'max': max(rows)},
           'rows_differing': {'median': int(np.median(differing)), 'min': min(differing), 'max': max(differing)},
           'counted': counted}
    for name in arms:
        out[name] = {'device_ms': _stats(dev_ms[name]), 'host_ms': _stats(host_ms[name])}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
