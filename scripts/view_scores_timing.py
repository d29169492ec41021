"""Device time of lidal_view_scores beside lidal_view_mean_softmax, and frames/s of view_sequence beside score_sequence,
on one GPU, one JSON line:
  kernels    the logits MinkUNet(19) gives for the 8 collated views of a 120 k-point synthetic scan and the batch's
             inverse indices (p = 120 000, reps 8, c 19); HIP events around each call, the two calls alternating, the
             median of --launches launches each after a warm-up; the view-mean kernel of the same run is the yardstick
  sequences  --frames such scans: view_sequence (no window, no exchange) and score_sequence (nei 10) over the same
             frames, one warm-up pass each, then --passes timed passes each, alternating; the median
    python scripts/view_scores_timing.py [--launches 30] [--frames 16] [--passes 5] [--points 120000]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lidal_amd                                                # noqa: E402
from lidal_amd import synth                                     # noqa: E402
from lidal_amd.network import MinkUNet                          # noqa: E402
from lidal_amd.score import interframe, score_sequence, view_sequence           # noqa: E402
from lidal_amd.score.prob_inference import view_mean_softmax, view_scores      # noqa: E402


def _event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def _wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=30)
    ap.add_argument('--frames', type=int, default=16)
    ap.add_argument('--passes', type=int, default=5)
    ap.add_argument('--points', type=int, default=120000)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    reps, nei = 8, 10
    torch.manual_seed(7122)
    model = MinkUNet(19).eval().to(dev)
    frames = synth.make_sequence(args.frames, n_points=args.points, seed=7122)
    rng = np.random.default_rng(7122)
    dev_frames = []
    for f in frames:
        sb = synth.make_score_batch(f['points'], f['intensity'], rng, inf_reps=reps)
        ptr, idx, _ = interframe.sv_csr(f['sv2point'], dev)
        dev_frames.append({'coords': torch.from_numpy(sb['coords_v_b']).to(dev),
                           'feats': torch.from_numpy(sb['feats_v_b']).to(dev),
                           'inverse': torch.from_numpy(sb['inverse_indices_b']).to(dev),
                           'world': torch.from_numpy(f['world']).to(dev), 'sv_ptr': ptr, 'sv_idx': idx})
    d = dev_frames[0]
    with torch.no_grad():
        logits, _ = model(lidal_amd.SparseTensor(d['feats'], d['coords']))
    logits = logits.float().contiguous()
    out = {'metric': 'view_scores_device_ms', 'points': int(d['world'].shape[0]), 'reps': reps,
           'classes': int(logits.shape[1]), 'voxel_rows': int(logits.shape[0]), 'launches': args.launches}
    calls = {'view_scores': lambda: view_scores(logits, d['inverse'], reps),
             'view_mean_softmax': lambda: view_mean_softmax(logits, d['inverse'], reps)}
    a, b = calls['view_scores'](), calls['view_mean_softmax']()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for _ in range(5):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(args.launches):
        for k, fn in calls.items():
            ms[k].append(_event_ms(fn))
    for k, v in ms.items():
        out[k + '_ms'] = round(float(np.median(v)), 4)
        out[k + '_ms_min_max'] = [round(min(v), 4), round(max(v), 4)]
    out['ratio'] = round(out['view_scores_ms'] / out['view_mean_softmax_ms'], 3)
    if args.frames >= nei + 3:
        runs = {'view_sequence': lambda: view_sequence(model, dev_frames, inf_reps=reps),
                'score_sequence': lambda: score_sequence(model, dev_frames, 0, args.frames, nei_num=nei, inf_reps=reps)}
        for fn in runs.values():
            fn()
        out['sequence_frames'] = args.frames
        out['score_sequence_nei'] = nei
        secs = {k: [] for k in runs}
        for _ in range(args.passes):
            for k, fn in runs.items():
                secs[k].append(_wall(fn))
        for k, v in secs.items():
            out[k + '_frames_per_s'] = round(args.frames / float(np.median(v)), 2)
            out[k + '_frames_per_s_min_max'] = [round(args.frames / max(v), 2), round(args.frames / min(v), 2)]
    print(json.dumps(out))


if __name__ == '__main__':
    main()
