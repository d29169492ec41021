"""Device and host times of building a whole batch of network input on one GPU, one JSON line:
  two shapes -- one raycast scan (~120 k points) as 8 augmented views (the score batch), and 5 such scans (the training
  batch); two arms in the same process, alternating call by call -- the per-view path (voxelize_scan per sample, then
  collate) and voxelize_batch; each as HIP-event time and as host wall time around a synchronise, median / min / max of
  30 calls after a warm-up; the launches and read-backs of each arm as the code makes them (counted from the sources,
  not traced); and two frames back to back: input build + infer_frame (MinkUNet, bf16) twice in a row, host time until
  everything is queued and until the stream is drained.
    python scripts/exp/voxelize_batch_timing.py"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from lidal_amd import data, synth                                  # noqa: E402
from lidal_amd.network import MinkUNet                             # noqa: E402
from lidal_amd.score.prob_inference import infer_frame             # noqa: E402

REPS = 30


def _stats(ms):
    return {'median': round(float(np.median(ms)), 4), 'min': round(float(np.min(ms)), 4), 'max': round(float(np.max(ms)), 4)}


def _time_alternating(arms):
    """arms: name -> callable.  REPS rounds; in a round every arm runs once, in turn.  name -> device / host stats."""
    for _ in range(3):
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    dev_ms, host_ms = {k: [] for k in arms}, {k: [] for k in arms}
    for _ in range(REPS):
        for name, fn in arms.items():
            t0 = time.perf_counter()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            host_ms[name].append((time.perf_counter() - t0) * 1e3)
            dev_ms[name].append(e0.elapsed_time(e1))
    return {name: {'device_ms': _stats(dev_ms[name]), 'host_ms': _stats(host_ms[name])} for name in arms}


def per_view(samples, draws):
    parts = []
    for (pts, inten), (m, r) in zip(samples, draws):
        cv, fv, _, inv = data.voxelize_scan(pts, inten, m, r)
        parts.append({'coords_v': cv, 'feats_v': fv, 'inverse_idxs': inv})
    return data.collate(parts)


def batched(samples, draws, shared):
    ms, rs = [d[0] for d in draws], [d[1] for d in draws]
    if shared:
        return data.voxelize_batch(samples[0][0], samples[0][1], ms, rs)
    return data.voxelize_batch([s[0] for s in samples], [s[1] for s in samples], ms, rs)


def _sort_launches(n, bits):
    """csrc/sort.hip run_sort: the histogram (and its reduction above 32 tiles of 8192 items), then one pass per 8 key bits."""
    return 1 + (1 if n > 32 * 8192 else 0) + (bits + 7) // 8


def counted(p_each, s, shared):
    """Launches (kernels, memsets, copies) and read-backs as the sources make them: data.py and csrc/kmap.hip."""
    sbits = (s - 1).bit_length()
    per_view_arm = {
        'library_calls': s, 'read_backs': s, 'uploads': 2 * s,
        # memset + affine, offset, keys + sort + head_count, scan, compact; feats_p[uniq]; collate: full, cat, add per
        # sample and the three final cats
        'launches': s * (1 + 3 + _sort_launches(p_each, 39) + 3 + 1 + 3) + 3,
    }
    batch_arm = {
        'library_calls': 1, 'read_backs': 1, 'uploads': 1,
        # affine, offset, keys + sort + head_count, scan, compact; the two cats of a list of scans
        'launches': 3 + _sort_launches(p_each * s, 39 + sbits) + 3 + (0 if shared else 2),
    }
    return {'per_view': per_view_arm, 'batch': batch_arm}


def two_frames(model, build):
    """Host ms until two frames' input build + inference are queued, and until they are done."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(2):
        b = build()
        infer_frame(model, b['coords_v_b'], b['feats_v_b'], b['inverse_indices_b'], inf_reps=8, autocast=True)
    queued = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    return queued, (time.perf_counter() - t0) * 1e3


def main():
    dev = torch.device('cuda:0')
    world = synth.make_world(3)
    scans = []
    for i in range(5):
        pts, inten = synth.raycast_scan(world, (30.0 + 2.0 * i, 0.0), np.random.default_rng([0, i]))
        scans.append((torch.from_numpy(pts).to(dev), torch.from_numpy(inten).to(dev)))
    rs = np.random.RandomState(7)
    out = {'metric': 'voxelize_batch_ms', 'reps': REPS}
    shapes = {'views8': ([scans[0]] * 8, True), 'train5': (scans, False)}
    for name, (samples, shared) in shapes.items():
        draws = [data.draw_augmentation(rs) for _ in samples]
        a, b = per_view(samples, draws), batched(samples, draws, shared)
        equal = all(torch.equal(a[k], b[k]) for k in ('coords_v_b', 'feats_v_b', 'inverse_indices_b'))
        res = _time_alternating({'per_view': lambda: per_view(samples, draws), 'batch': lambda: batched(samples, draws, shared)})
        p_each = int(samples[0][0].shape[0])
        out[name] = {'samples': len(samples), 'points': int(sum(s[0].shape[0] for s in samples)),
                     'voxels': int(b['coords_v_b'].shape[0]), 'bit_equal': bool(equal), 'counted': counted(p_each, len(samples), shared)}
        out[name].update(res)
    # two frames back to back (the score mode: 8 views of one scan, then the network)
    torch.manual_seed(3)
    model = MinkUNet(19).to(dev).eval()
    samples = [scans[0]] * 8
    builds = {'per_view': lambda: per_view(samples, [data.draw_augmentation(rs) for _ in samples]),
              'batch': lambda: data.score_sample(scans[0][0], scans[0][1], 8, rs)}
    for _ in range(3):
        for build in builds.values():
            two_frames(model, build)
    queued, done = {k: [] for k in builds}, {k: [] for k in builds}
    for _ in range(REPS):
        for name, build in builds.items():
            q, d = two_frames(model, build)
            queued[name].append(q)
            done[name].append(d)
    out['two_frames'] = {name: {'host_queued_ms': _stats(queued[name]), 'host_done_ms': _stats(done[name])} for name in builds}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
