"""Device times of the ReDAL kernels on one GPU, one JSON line:
  surface variation of a 120 k-point synthetic scan; region scores of that frame (20 supervoxels, 19 classes, 96
  features); kmeans on [200k, 96] with k 150 and n_init 10; scikit-learn's KMeans on the same data where installed.
    python scripts/redal_timing.py [--no-sklearn]"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lidal_amd import synth                                     # noqa: E402
from lidal_amd.score import interframe, kmeans, region_scores, surface_variation   # noqa: E402


def _time(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(reps):
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms))


def main():
    dev = torch.device('cuda:0')
    out = {'metric': 'redal_device_ms'}
    frame = synth.make_sequence(1, n_points=120000, seed=7122)[0]
    xyz = torch.from_numpy(frame['points']).to(dev)
    out['points'] = int(xyz.shape[0])
    out['surface_variation_ms'] = _time(lambda: surface_variation(xyz), 5)
    rs = np.random.RandomState(0)
    p = xyz.shape[0]
    logit = torch.from_numpy(rs.normal(0, 2, size=(p, 19)).astype(np.float32)).to(dev)
    prob = torch.softmax(logit, 1).contiguous()
    feat = torch.relu(torch.from_numpy(rs.normal(size=(p, 96)).astype(np.float32)).to(dev)).contiguous()
    curv = surface_variation(xyz)
    ptr, idx, _ = interframe.sv_csr(frame['sv2point'], dev)
    out['region_scores_ms'] = _time(lambda: region_scores(prob, feat, curv, ptr, idx), 20)
    centres = rs.uniform(-2, 2, size=(300, 96))
    x = (centres[rs.randint(300, size=200000)] + rs.normal(size=(200000, 96))).astype(np.float32)
    xd = torch.from_numpy(x).to(dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _, _, inertia, n_iter = kmeans(xd, n_clusters=150, random_state=0, n_init=10)
    torch.cuda.synchronize()
    out['kmeans_200k_96_k150_ninit10_s'] = time.perf_counter() - t0
    out['kmeans_inertia'] = inertia
    out['kmeans_n_iter_best'] = n_iter
    if '--no-sklearn' not in sys.argv:
        try:
            from sklearn.cluster import KMeans
        except ImportError:
            out['sklearn'] = 'not installed'
        else:
            t0 = time.perf_counter()
            m = KMeans(n_clusters=150, random_state=0, n_init=10).fit(x)
            out['sklearn_s'] = time.perf_counter() - t0
            out['sklearn_inertia'] = float(m.inertia_)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
