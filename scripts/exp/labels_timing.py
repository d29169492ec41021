"""Device and host times of the training-label path on one GPU, one JSON line:
  one raycast scan (~120 k points), 20 angular supervoxels, SemanticKITTI u32 annotation words, pseudo labels;
  voxelize_scan alone, train_labels alone (with and without its read-back), train_sample (voxelize_scan + train_labels),
  each as HIP-event time and as host wall time around a synchronise, median of 30 calls after a warm-up; and the host
  time of the numpy restatement of the label semantics (tests/labels_ref.py) with the per-batch upload the reference's
  loader pays left out.
    python scripts/exp/labels_timing.py"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import labels_ref                                                  # noqa: E402
from lidal_amd import data, synth                                  # noqa: E402
from lidal_amd.score.interframe import sv_csr                      # noqa: E402

REPS = 30


def _time(fn):
    """(median device ms between two events, median host ms until the stream is drained)."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    dev_ms, host_ms = [], []
    for _ in range(REPS):
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        host_ms.append((time.perf_counter() - t0) * 1e3)
        dev_ms.append(e0.elapsed_time(e1))
    return round(float(np.median(dev_ms)), 4), round(float(np.median(host_ms)), 4)


def main():
    dev = torch.device('cuda:0')
    rng = np.random.default_rng(0)
    pts, inten = synth.raycast_scan(synth.make_world(3), (30.0, 0.0), rng)
    p = pts.shape[0]
    lists = synth.angular_supervoxels(pts, 20)
    flags = np.array([1, 2, 0, 0] * 5)
    table = data.sk_label_map()
    ids = np.nonzero(table != 255)[0]
    raw = (rng.choice(ids, p) | (rng.integers(1, 65536, p) << 16)).astype(np.uint32)
    pseudo = rng.integers(0, 19, p)
    trans_m, rnd = data.draw_augmentation(np.random.RandomState(7))
    pts_d, inten_d = torch.from_numpy(pts).to(dev), torch.from_numpy(inten).to(dev)
    raw_d, pseudo_d, table_d = torch.from_numpy(raw.view(np.int32)).to(dev), torch.from_numpy(pseudo).to(dev), torch.from_numpy(table).to(dev)
    csr = sv_csr(lists, dev)[:2]
    flags_d = torch.from_numpy(flags).to(dev)
    uniq = data.voxelize_scan(pts_d, inten_d, trans_m, rnd)[2]
    out = {'metric': 'labels_ms', 'points': int(p), 'voxels': int(uniq.shape[0]), 'supervoxels': 20, 'reps': REPS}
    rs = np.random.RandomState(7)
    cases = {
        'voxelize_scan': lambda: data.voxelize_scan(pts_d, inten_d, trans_m, rnd),
        'train_labels': lambda: data.train_labels(raw_d, table_d, csr, flags_d, pseudo_d, uniq),
        'train_labels_nocheck': lambda: data.train_labels(raw_d, table_d, csr, flags_d, pseudo_d, uniq, check=False),
        'train_sample': lambda: data.train_sample(pts_d, inten_d, raw_d, table_d, csr, flags_d, pseudo_d, rng=rs),
        'train_sample_nocheck': lambda: data.train_sample(pts_d, inten_d, raw_d, table_d, csr, flags_d, pseudo_d, rng=rs,
                                                          check=False),
    }
    for name, fn in cases.items():
        out[name + '_device_ms'], out[name + '_host_ms'] = _time(fn)
    uniq_h = uniq.cpu().numpy()
    host = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        labels_ref.train_labels(raw, table, lists, flags, pseudo, uniq_h)
        host.append((time.perf_counter() - t0) * 1e3)
    out['numpy_restatement_host_ms'] = round(float(np.median(host)), 4)
    lp, lv = data.train_labels(raw_d, table_d, csr, flags_d, pseudo_d, uniq)
    ref = labels_ref.train_labels(raw, table, lists, flags, pseudo, uniq_h)
    out['equal_to_restatement'] = bool(np.array_equal(lp.cpu().numpy(), ref[0]) and np.array_equal(lv.cpu().numpy(), ref[1]))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
