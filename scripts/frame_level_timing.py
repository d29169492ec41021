"""Device times of the frame-level kernels on one GPU, one JSON line:
  frame_uncertainty, segment_entropy and frame_feature on a 120 k-point frame (19 classes, 20 and 300 supervoxels,
  96 features); coreset at N = 19 130 and 28 130 frames, D = 96, 1 % and 10 % labeled; where installed, the CPU time
  of the reference's expressions (scipy's entropy, numpy's sort and mean, outfeat.mean(0), the segment_entropy loop)
  and of core_set.py's loop with sklearn's pairwise_distances.
    python scripts/frame_level_timing.py [--no-cpu | --cpu-only]
(--cpu-only: the reference timings alone, on a host without a GPU.)"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
import frame_inputs as FI                                                              # noqa: E402
from lidal_amd.score import coreset, frame_feature, frame_uncertainty, interframe, segment_entropy   # noqa: E402


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


def _wall(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def _sv(p, n_sv, rs):
    cuts = np.sort(rs.choice(np.arange(1, p), size=n_sv - 1, replace=False))
    return [np.sort(c).astype(np.int64) for c in np.split(rs.permutation(p), cuts)]


def _device(out, prob, feat, pred, svs):
    dev = torch.device('cuda:0')
    prob_d, feat_d, pred_d = (torch.from_numpy(a).to(dev) for a in (prob, feat, pred))
    out['frame_uncertainty_ms'] = _time(lambda: frame_uncertainty(prob_d), 20)
    for n_sv, sv in svs.items():
        ptr, idx, _ = interframe.sv_csr(sv, dev)
        out['segment_entropy_sv%d_ms' % n_sv] = _time(lambda: segment_entropy(pred_d, ptr, idx, 19), 20)
    out['frame_feature_d96_ms'] = _time(lambda: frame_feature(feat_d), 20)
    for n in (19130, 28130):
        x = torch.from_numpy(FI.large_feats(n)).to(dev)
        for share in (0.01, 0.10):
            lab = np.zeros(n, bool)
            lab[np.random.RandomState(1).choice(n, int(share * n), replace=False)] = True
            out['coreset_n%d_lab%d_ms' % (n, round(100 * share))] = _time(lambda: coreset(x, lab), 3)


def main():
    out = {'metric': 'frame_level_device_ms'}
    p = 120000
    rs = np.random.RandomState(0)
    prob = FI._prob(rs, p, 19)
    feat = np.maximum(rs.normal(size=(p, FI.FT_DIM)), 0).astype(np.float32)
    pred = prob.argmax(1).astype(np.int64)
    out['points'] = p
    svs = {n_sv: _sv(p, n_sv, rs) for n_sv in (20, 300)}
    if '--cpu-only' not in sys.argv:
        _device(out, prob, feat, pred, svs)

    if '--no-cpu' not in sys.argv:
        try:
            from scipy.stats import entropy
            from sklearn.metrics import pairwise_distances
        except ImportError:
            out['cpu_reference'] = 'scipy / scikit-learn not installed'
        else:
            def srt():
                s = np.sort(prob, axis=-1)
                return np.mean(s[:, -1] - s[:, -2]), np.mean(s[:, -1])
            out['cpu_entropy_ms'] = _wall(lambda: np.mean(entropy(prob, axis=1)))
            out['cpu_margin_conf_ms'] = _wall(srt)
            out['cpu_outfeat_mean_ms'] = _wall(lambda: feat.mean(0))

            def segent():
                f = 0.0
                for ids in svs[300]:
                    sp = pred[ids]
                    sv = 0.0
                    for c in range(19):
                        q = (sp == c).sum() / sp.shape[0]
                        sv += -q * np.log2(q + 1e-12)
                    f += sv * sp.shape[0] / pred.shape[0]
                return f
            out['cpu_segment_entropy_sv300_ms'] = _wall(segent)

            def sk_coreset(x, lab):
                labeled_ids = np.where(lab)[0]
                dist = pairwise_distances(x, x[labeled_ids], metric='euclidean')
                min_dist = np.min(dist, axis=1).reshape(-1, 1)
                for _ in range(round(0.01 * x.shape[0])):
                    ind = np.argmax(min_dist)
                    dist = pairwise_distances(x, x[ind].reshape(1, -1), metric='euclidean')
                    min_dist = np.minimum(min_dist, dist)
            x = FI.large_feats(19130)
            lab = np.zeros(19130, bool)
            lab[np.random.RandomState(1).choice(19130, 1913, replace=False)] = True
            out['cpu_sklearn_coreset_n19130_lab10_ms'] = _wall(lambda: sk_coreset(x, lab))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
