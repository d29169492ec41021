"""What the counter-based dropout (csrc/dropout.hip) costs and buys, on one GPU, one JSON line per part:
  op         lidal_dropout_apply against torch's in-place formulation (noise = empty_like(x).bernoulli_(1 - p).div_(1 - p);
             x.mul_(noise): three kernels forward, one backward, a tensor-sized buffer held between them) on the two
             tensors SPVCNN drops in the --frames-scan step (n[4] x 256, n[2] x 128), bf16 and f32: HIP events around each
             call, the candidates alternating, the median of --launches after a warm-up; host = the enqueue time of the call
  step       the SPVCNN training step (bf16, tables prefetched, fused Adam: bench.py's loop) with dropout_seed=0 against
             nn.Dropout, --frames scans and one scan: --runs runs of --steps steps each, the two models alternating; wall
             time per step behind a synchronise, lidal_plan_run calls per step
  sequence   frames/s of mc_sequence (8 passes of one view) beside view_sequence (8 views) on --seq-frames synthetic
             120 000-point frames, the same SPVCNN: one warm-up pass each, then --passes timed passes each, alternating
    python scripts/exp/dropout_timing.py [--frames 5] [--points 120000] [--launches 30] [--runs 3] [--steps 20]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from lidal_amd import backend as B                              # noqa: E402
from lidal_amd import data, synth                               # noqa: E402
from lidal_amd.network import SPVCNN, GeometryPrefetcher, plan  # noqa: E402
from lidal_amd.network.geometry import Geometry                 # noqa: E402
from lidal_amd.nn.dropout import dropout_apply_                 # noqa: E402
from lidal_amd.score import interframe, mc_sequence, view_sequence              # noqa: E402
from lidal_amd.train_step import train_step                     # noqa: E402

P_DROP = 0.3


def _timed(fn):
    """(device ms between two events around fn, host seconds fn took to return)"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    t0 = time.perf_counter()
    fn()
    host = time.perf_counter() - t0
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), host


def _train_batch(frames, points, dev, seed=7122):
    b = synth.make_train_batch(n_frames=frames, n_points=points, seed=seed)
    return tuple(torch.from_numpy(b[k]).to(dev) for k in ('coords_v_b', 'feats_v_b', 'labels_v_b'))


def time_op(model, batch, launches):
    g = Geometry.build(model, batch[0], True)
    n = plan._tables(g, True, True, model.cs).n
    out = {'metric': 'dropout_op_ms', 'p': P_DROP, 'launches': launches, 'kernels': {'counter_fwd': 1, 'counter_bwd': 1,
           'torch_fwd': 3, 'torch_bwd': 1}, 'shapes': []}
    for rows, c in ((n[4], model.cs[4]), (n[2], model.cs[6])):
        for dtype in (torch.bfloat16, torch.float32):
            x = torch.randn(rows, c, device=batch[0].device).to(dtype)
            held = {}

            def torch_fwd():
                held['noise'] = torch.empty_like(x).bernoulli_(1 - P_DROP).div_(1 - P_DROP)
                x.mul_(held['noise'])
            calls = {'counter_fwd': lambda: dropout_apply_(x, P_DROP, 1, 2), 'torch_fwd': torch_fwd,
                     'counter_bwd': lambda: dropout_apply_(x, P_DROP, 1, 2),
                     'torch_bwd': lambda: torch.mul(x, held['noise'], out=x)}
            for _ in range(5):
                for fn in calls.values():
                    fn()
                x.normal_()
            ms = {k: [] for k in calls}
            host = {k: [] for k in calls}
            for _ in range(launches):
                for k, fn in calls.items():
                    d, h = _timed(fn)
                    ms[k].append(d)
                    host[k].append(h)
                x.normal_()                     # (the values shrink towards 0 under repeated masks otherwise)
            row = {'rows': int(rows), 'channels': int(c), 'dtype': str(dtype).split('.')[1],
                   'tensor_MB': round(x.numel() * x.element_size() / 1e6, 3)}
            for k in calls:
                row[k + '_device_us'] = round(1e3 * float(np.median(ms[k])), 2)
                row[k + '_device_us_min'] = round(1e3 * min(ms[k]), 2)
                row[k + '_host_us'] = round(1e6 * float(np.median(host[k])), 2)
            out['shapes'].append(row)
    print(json.dumps(out), flush=True)


def _stepper(seed, batch, dev):
    torch.manual_seed(7122)
    model = SPVCNN(19, dropout_seed=seed).to(dev).train()
    opt = torch.optim.Adam(model.parameters(), fused=True)
    pf = GeometryPrefetcher(model, device=dev)
    ahead = [pf.submit(batch[0])]

    def step():
        coords, feats, labels = batch
        out = train_step(model, opt, feats, coords, labels, autocast=True, geometry=ahead[0])
        ahead[0] = pf.submit(coords)
        return out
    return step, pf


def time_step(batch, dev, runs, steps, what):
    arms = {'counter_dropout': _stepper(0, batch, dev), 'nn_dropout': _stepper(None, batch, dev)}
    out = {'metric': 'spvcnn_step_ms', 'batch': what, 'voxels': int(batch[0].shape[0]), 'dtype': 'bf16', 'runs': runs,
           'steps_per_run': steps}
    for name, (step, _) in arms.items():
        for _ in range(3):
            step()
        torch.cuda.synchronize()
        B.HITS.clear()
        step()
        out[name + '_plan_run_calls_per_step'] = int(B.HITS.get('plan_run', 0))
    ms = {k: [] for k in arms}
    for _ in range(runs):
        for name, (step, _) in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                loss, _ = step()
            torch.cuda.synchronize()
            ms[name].append(1e3 * (time.perf_counter() - t0) / steps)
            assert np.isfinite(loss.item())
    for name, (_, pf) in arms.items():
        pf.drain()
        out[name + '_ms_per_step'] = [round(v, 3) for v in ms[name]]
    out['median_ratio_counter_over_nn'] = round(float(np.median(ms['counter_dropout']) / np.median(ms['nn_dropout'])), 4)
    print(json.dumps(out), flush=True)


def time_sequence(dev, n_frames, points, passes):
    torch.manual_seed(7122)
    model = SPVCNN(19, dropout_seed=0).eval().to(dev)
    rs = np.random.RandomState(7122)
    views, mcs = [], []
    for f in synth.make_sequence(n_frames, n_points=points, seed=7122):
        pts, inten = torch.from_numpy(f['points'][:, :3]).to(dev), torch.from_numpy(f['intensity']).to(dev)
        ptr, idx, _ = interframe.sv_csr(f['sv2point'], dev)
        common = {'world': torch.from_numpy(f['world']).to(dev), 'sv_ptr': ptr, 'sv_idx': idx}
        for frames, sb in ((views, data.score_sample(pts, inten, 8, rs)), (mcs, data.mc_sample(pts, inten, 8, rs))):
            frames.append(dict(common, coords=sb['coords_v_b'], feats=sb['feats_v_b'], inverse=sb['inverse_indices_b']))
    runs = {'mc_sequence': lambda: mc_sequence(model, mcs, passes=8), 'view_sequence': lambda: view_sequence(model, views, inf_reps=8)}
    out = {'metric': 'mc_sequence_frames_per_s', 'frames': n_frames, 'points': points, 'passes_or_views': 8,
           'timed_passes': passes, 'model': 'SPVCNN f32'}
    for k, fn in runs.items():
        B.HITS.clear()
        fn()
        out[k + '_plan_run_calls_per_frame'] = B.HITS.get('plan_run', 0) / n_frames
    secs = {k: [] for k in runs}
    for _ in range(passes):
        for k, fn in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            secs[k].append(time.perf_counter() - t0)
    for k, v in secs.items():
        out[k + '_frames_per_s'] = round(n_frames / float(np.median(v)), 2)
        out[k + '_frames_per_s_min_max'] = [round(n_frames / max(v), 2), round(n_frames / min(v), 2)]
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=5)
    ap.add_argument('--points', type=int, default=120000)
    ap.add_argument('--launches', type=int, default=30)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--seq-frames', type=int, default=16)
    ap.add_argument('--passes', type=int, default=3)
    ap.add_argument('--parts', default='op,step,sequence')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('dropout_timing.py measures on the GPU; none is visible')
    dev = torch.device('cuda:0')
    parts = args.parts.split(',')
    batch = _train_batch(args.frames, args.points, dev)
    if 'op' in parts:
        torch.manual_seed(7122)
        time_op(SPVCNN(19).to(dev).train(), batch, args.launches)
    if 'step' in parts:
        time_step(batch, dev, args.runs, args.steps, '%d scans' % args.frames)
        time_step(_train_batch(1, args.points, dev), dev, args.runs, args.steps, '1 scan')
    if 'sequence' in parts:
        time_sequence(dev, args.seq_frames, args.points, args.passes)


if __name__ == '__main__':
    main()
