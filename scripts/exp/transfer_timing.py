"""Time of carrying labels and predictions across frames (lidal_amd/score/transfer.py) on one GPU,
one JSON line.  A measurement, not a gate.
  workload   --frames synthetic frames of --points points (scripts/view_scores_timing.py's), window 10, 19 classes, 6 of
             the 20 supervoxels of a frame annotated
  match      match_points per frame, and score_points of the same frames beside it (its stage 1 is the same kernel)
  stage 2    on the SAME match table: transfer_labels + fuse_predictions (one launch each) against a torch formulation
             (gather, one_hot sum, argmax, where); the two are held to the same outputs before anything is timed
Per arm: one warm-up pass over the frames, then --passes timed passes, the arms alternating inside a pass; the median
pass, per frame.  stream_ms: HIP events around the pass; host_ms: the host clock around the enqueue alone (no
synchronise inside).  Kernel counts: torch.profiler over one frame, in a pass of its own.
    python scripts/exp/transfer_timing.py [--frames 16] [--points 120000] [--passes 7]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from lidal_amd import synth                                                                     # noqa: E402
from lidal_amd.score import FrameBank, fuse_predictions, match_points, neighbour_ids, transfer_labels      # noqa: E402
from lidal_amd.score.interframe import score_points                                             # noqa: E402

C, IGN, NEI = 19, 255, 10


def torch_stage2(match, nei_labels, own, q_prob, nei_prob):
    """transfer_labels(min_votes=1, min_agree=1.0, no gate) and fuse_predictions in torch operators."""
    p = match.shape[1]
    hist = torch.zeros((p, C), dtype=torch.int32, device=match.device)
    total = q_prob.clone()
    cnt = torch.zeros(p, dtype=torch.int32, device=match.device)
    for n in range(match.shape[0]):
        ok = match[n] >= 0
        j = match[n].clamp(min=0).long()
        lab = nei_labels[n][j]
        vote = ok & (lab != IGN) & (lab >= 0) & (lab < C)
        hist += torch.nn.functional.one_hot(torch.where(vote, lab, 0), C).to(torch.int32) * vote[:, None]
        total = total + torch.where(ok[:, None], nei_prob[n][j], 0.0)
        cnt += ok
    agree, winner = hist.max(1)
    nv = hist.sum(1)
    passes = (nv > 0) & (agree == nv)
    out = torch.where(own != IGN, own, torch.where(passes, winner, IGN))
    fused = (total.double() / (cnt + 1).double()[:, None]).float()
    conf, pred = fused.max(1)
    return out, fused, pred, conf, cnt


def hip_stage2(bank, i, labels, frames, match):
    out, _ = transfer_labels(bank, i, labels, C, frames=frames, match=match)
    prob, pred, conf, cnt = fuse_predictions(bank, i, frames=frames, match=match)
    return out, prob, pred, conf, cnt


def timed_pass(arms, n_items):
    """{arm: (stream ms, host ms)} per item for one pass; arms: {name: fn(item)}, alternating per item."""
    ev = {k: [] for k in arms}
    host = {k: 0.0 for k in arms}
    torch.cuda.synchronize()
    for it in range(n_items):
        for k, fn in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            fn(it)
            e1.record()
            host[k] += time.perf_counter() - t0
            ev[k].append((e0, e1))
    torch.cuda.synchronize()
    return {k: (sum(a.elapsed_time(b) for a, b in ev[k]) / n_items, host[k] * 1e3 / n_items) for k in arms}


def kernel_count(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(e.count for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA)
    except Exception as e:                                   # the count is a by-product: report why it is missing
        return 'not measured (%s)' % type(e).__name__


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=16)
    ap.add_argument('--points', type=int, default=120000)
    ap.add_argument('--passes', type=int, default=7)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    frames = synth.make_sequence(args.frames, n_points=args.points, seed=7122)
    rng = np.random.default_rng(7122)
    bank = FrameBank(0.1)
    labels = {}
    for f, fr in enumerate(frames):
        w = fr['world']
        lg = rng.standard_normal((w.shape[0], C)).astype(np.float32) + (np.sin(w[:, :1] * 0.7) * 2).astype(np.float32)
        bank.add(torch.from_numpy(w).to(dev), torch.softmax(torch.from_numpy(lg).to(dev), 1))
        cell = np.floor(w / 2.0).astype(np.int64)
        cls = (7 * cell[:, 0] + 13 * cell[:, 1] + 5 * cell[:, 2]) % C
        lab = np.full(w.shape[0], IGN, np.int64)
        for s in rng.choice(len(fr['sv2point']), 6, replace=False):
            lab[fr['sv2point'][s]] = cls[fr['sv2point'][s]]
        labels[f] = torch.from_numpy(lab).to(dev)
    ids = list(range(args.frames))
    nei = {i: neighbour_ids(i, args.frames, NEI) for i in ids}
    match = {i: match_points(bank, i, frames=nei[i]) for i in ids}         # (builds every grid: not part of any window)

    def torch_arm(i):
        return torch_stage2(match[i], [labels[f] for f in nei[i]], labels[i], bank.prob[i], [bank.prob[f] for f in nei[i]])

    # the two arms compute the same thing
    carried = matched = 0
    for i in ids:
        a, b = hip_stage2(bank, i, labels, nei[i], match[i]), torch_arm(i)
        for x, y in zip(a, b):
            assert torch.equal(x, y.to(x.dtype)), i
        carried += int(((a[0] != IGN) & (labels[i] == IGN)).sum())
        matched += int((match[i] >= 0).sum())
    out = {'metric': 'transfer_ms_per_frame', 'frames': args.frames, 'points': args.points, 'window': NEI, 'classes': C,
           'passes': args.passes, 'matches_per_point': round(matched / (args.frames * args.points), 3),
           'labels_carried_per_frame': carried // args.frames}
    stage1 = {'match_points': lambda i: match_points(bank, i, frames=nei[i]),
              'score_points': lambda i: score_points(bank, i, NEI)}
    stage2 = {'hip_transfer_and_fuse': lambda i: hip_stage2(bank, i, labels, nei[i], match[i]), 'torch_formulation': torch_arm}
    for arms in (stage1, stage2):
        timed_pass(arms, args.frames)                        # warm-up: every shape of the window
        runs = [timed_pass(arms, args.frames) for _ in range(args.passes)]
        for k in arms:
            s = [r[k][0] for r in runs]
            h = [r[k][1] for r in runs]
            out[k] = {'stream_ms': round(float(np.median(s)), 4), 'stream_ms_min_max': [round(min(s), 4), round(max(s), 4)],
                      'host_ms': round(float(np.median(h)), 4), 'kernels': kernel_count(lambda: arms[k](args.frames // 2))}
    out['match_share_of_score_points'] = round(out['match_points']['stream_ms'] / out['score_points']['stream_ms'], 3)
    out['torch_over_hip_stream'] = round(out['torch_formulation']['stream_ms'] / out['hip_transfer_and_fuse']['stream_ms'], 2)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
