"""Times of the greedy selection on one synthetic board, one JSON line:
  `select` (the reference's loop, host), `centre_pairs` (the neighbour table, GPU: first call and the median of 5 more),
  `select_indexed` with that table given (host); the flags of the two loops must be equal.
The board: `--sequences` trajectories of `--frames` frames about 1 m apart on a gently turning path, 20 supervoxels per
frame scattered +-25 m across it, sequence k shifted by 1000 k m (LiDAL.py:218), uniform divergences and entropies,
50..2000 points per supervoxel, nothing labelled, train_point_num = all points (so each pass spends 1 % of them).
Also the device time of each of the two library calls between events, operands resident.
Seeded.  The default size, 600 000 supervoxels (SemanticKITTI has about 4.6e5), is the one at which `select` takes about
a minute on the host of the GPU machine it was measured on (profiles/README.md); its time grows with the square of the
size (41.7 s at 500 000 there; 0.57 s at 40 000 and 2.35 s at 80 000 on a slower host).
    python scripts/exp/select_indexed_timing.py [--sequences 24 --frames 1250] [--host-only]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from lidal_amd.score.selection import centre_pairs, select, select_indexed      # noqa: E402

SV_PER_FRAME = 20


def make_board(sequences, frames, seed=0):
    rs = np.random.RandomState(seed)
    centers = []
    for k in range(sequences):
        heading = np.cumsum(rs.normal(0.0, 0.01, frames))                       # a gently turning path
        step = rs.uniform(0.8, 1.2, frames)                                     # about 1 m between frames
        pose = np.stack([np.cumsum(step * np.cos(heading)), np.cumsum(step * np.sin(heading)), np.zeros(frames)], 1)
        across = np.stack([-np.sin(heading), np.cos(heading), np.zeros(frames)], 1)
        for f in range(frames):
            c = pose[f] + across[f] * rs.uniform(-25, 25, (SV_PER_FRAME, 1)) + rs.normal(0, [2.0, 2.0, 0.7], (SV_PER_FRAME, 3))
            centers.append(c.astype(np.float32) + np.float32(k * 1000.0))
    centers = np.concatenate(centers)
    n = centers.shape[0]
    return dict(sv_flags=np.zeros(n, dtype=np.int64), sv_interds=rs.uniform(0, 1, n).astype(np.float32),
                sv_interes=rs.uniform(0, 3, n).astype(np.float32), sv_pnums=rs.randint(50, 2001, n), sv_centers=centers)


def _device_ms(centers, pairs, reps=5):
    """Median time between events around each of the two library calls, operands resident on the device."""
    import torch

    from lidal_amd import backend as B
    c = torch.from_numpy(centers).cuda()
    n = c.shape[0]
    row_ptr = torch.empty(n + 1, dtype=torch.int64, device=c.device)
    status = torch.empty(1, dtype=torch.int32, device=c.device)
    col = torch.empty(int(pairs[0][-1]), dtype=torch.int32, device=c.device)
    nbytes = B.lib().lidal_radius_pairs_workspace_bytes(n)
    ws = B.workspace(nbytes, c.device)
    calls = (lambda: B.lib().lidal_radius_pairs_count(B.ptr(c), n, 5.0, B.ptr(row_ptr), B.ptr(status), B.ptr(ws), nbytes,
                                                      B.stream()),
             lambda: B.lib().lidal_radius_pairs_fill(B.ptr(c), n, 5.0, B.ptr(row_ptr), B.ptr(col), B.ptr(ws), nbytes,
                                                     B.stream()))
    ms = []
    for call in calls:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t = []
        for _ in range(reps):
            e0.record()
            B.check(call(), 'radius_pairs')
            e1.record()
            torch.cuda.synchronize()
            t.append(e0.elapsed_time(e1))
        ms.append(round(float(np.median(t)), 3))
    assert np.array_equal(row_ptr.cpu().numpy(), pairs[0]) and np.array_equal(col.cpu().numpy(), pairs[1])
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sequences', type=int, default=24)
    ap.add_argument('--frames', type=int, default=1250)
    ap.add_argument('--host-only', action='store_true', help='time `select` alone (to size the board without a GPU)')
    args = ap.parse_args()
    b = make_board(args.sequences, args.frames)
    tpn = int(b['sv_pnums'].sum())
    board = (b['sv_flags'], b['sv_interds'], b['sv_interes'], b['sv_pnums'], b['sv_centers'], tpn)
    out = {'metric': 'select_indexed_s', 'supervoxels': int(b['sv_flags'].size), 'sequences': args.sequences,
           'frames': args.frames, 'train_point_num': tpn}
    if not args.host_only:
        import torch
        t0 = time.perf_counter()
        pairs = centre_pairs(b['sv_centers'], 5.0)
        out['centre_pairs_first_s'] = round(time.perf_counter() - t0, 4)        # with the library load and the first launches
        reps = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            again = centre_pairs(b['sv_centers'], 5.0)                          # upload, two calls, read-back of the table
            reps.append(time.perf_counter() - t0)
        assert np.array_equal(again[0], pairs[0]) and np.array_equal(again[1], pairs[1])
        out['centre_pairs_s'] = round(float(np.median(reps)), 4)
        out['count_device_ms'], out['fill_device_ms'] = _device_ms(b['sv_centers'], pairs)
        out['pairs'] = int(pairs[0][-1])
        out['longest_row'] = int(np.diff(pairs[0]).max())
        t0 = time.perf_counter()
        got, counts = select_indexed(*board, pairs=pairs, details=True)
        out['select_indexed_s'] = round(time.perf_counter() - t0, 4)
        out.update(counts)
        print('so far:', json.dumps(out), file=sys.stderr, flush=True)          # `select` takes its minute now
    t0 = time.perf_counter()
    want = select(*board)
    out['select_s'] = round(time.perf_counter() - t0, 3)
    out['selected'] = [int((want == 1).sum()), int((want == 2).sum())]
    if not args.host_only:
        assert np.array_equal(got, want), 'select_indexed and select disagree'
        out['flags_equal'] = True
    print(json.dumps(out))


if __name__ == '__main__':
    main()
