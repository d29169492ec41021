"""A digest of every output tensor of the entry points built on csrc/rows.h, on seeded inputs, for comparing two builds.

  LIDAL_AMD_LIB=/elsewhere/liblidal_amd.so python scripts/exp/rows_digest.py --out parent.json
  python scripts/exp/rows_digest.py --out new.json
  python scripts/exp/rows_digest.py --compare parent.json new.json        # exit status 1 unless all are equal

One process per library.  lidal_ce_*, lidal_ce_weighted_*, lidal_lovasz_* on logits and on probabilities,
lidal_pseudo_labels, lidal_consistency_* ('mse' and 'kl', logits and probabilities, the four student / teacher dtype
pairs, min_conf 0 and 0.9), lidal_view_mean_softmax and lidal_view_scores (reps 1 and 3); n in {1, 255, 256, 257, 1025},
c in {1, 2, 19, 32}, f32 and bf16, operands on the 16-byte grid and one element behind it, a tenth of the labels
ignored and, at n = 1025, the whole second workgroup's.
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
DEV = 'cuda'
NS, CS = (1, 255, 256, 257, 1025), (1, 2, 19, 32)
DTYPES = {'f32': torch.float32, 'bf16': torch.bfloat16}


def digest(t):
    return hashlib.sha256(t.detach().contiguous().reshape(-1).view(torch.uint8).cpu().numpy().tobytes()).hexdigest()[:16]


def place(a, dtype, off):
    """`a` [n, c] on the device as `dtype`: on the 16-byte grid, or (off) one element behind it"""
    n, c = a.shape
    flat = torch.zeros(n * c + 1, dtype=dtype, device=DEV)
    view = flat[1:] if off else flat[:-1]
    view.copy_(torch.from_numpy(a).to(DEV).reshape(-1))
    assert (view.data_ptr() % 16 != 0) == bool(off)
    return view.view(n, c)


def run():
    from lidal_amd import semi
    from lidal_amd.nn import functional as F
    from lidal_amd.score.prob_inference import view_mean_softmax, view_scores
    out = {}

    def put(key, names, tensors):
        for name, t in zip(names, tensors):
            if t is not None:
                out['%s/%s' % (key, name)] = digest(t)

    def grad_of(fn, x):
        x = x.detach().requires_grad_(True)
        loss = fn(x)
        (loss * 1.5).backward()
        return loss, x.grad

    for n in NS:
        for c in CS:
            rng = np.random.default_rng(1000 * n + c)
            z = (rng.normal(size=(n, c)) * rng.choice([1.0, 3.0, 10.0], size=(n, 1))).astype(np.float32)
            zt = (rng.normal(size=(n, c)) * rng.choice([1.0, 3.0, 10.0], size=(n, 1))).astype(np.float32)
            e = np.exp(z - z.max(1, keepdims=True))
            pr = (e / e.sum(1, keepdims=True)).astype(np.float32)
            et = np.exp(zt - zt.max(1, keepdims=True))
            prt = (et / et.sum(1, keepdims=True)).astype(np.float32)
            labels = rng.integers(0, c, n)
            labels[rng.random(n) < 0.1] = 255
            labels[256:512] = 255
            lab = torch.from_numpy(labels.astype(np.int64)).to(DEV)
            w = torch.from_numpy(rng.random(c).astype(np.float32) + 0.1).to(DEV)
            inv = torch.from_numpy(rng.integers(0, n, 3 * (n + 3)).astype(np.int64)).to(DEV)
            for off in (0, 1):
                for dname, dtype in DTYPES.items():
                    key = 'n%d/c%d/%s/off%d' % (n, c, dname, off)
                    x = place(z, dtype, off)
                    put(key + '/ce', ('loss', 'dx'), grad_of(lambda t: F.cross_entropy(t, lab), x))
                    put(key + '/ce_weighted', ('loss', 'dx'), grad_of(lambda t: F.cross_entropy(t, lab, weight=w), x))
                    for classes in ('present', 'all'):
                        put(key + '/lovasz_' + classes, ('stats', 'grad', 'ranks'),
                            F.lovasz_forward(x, lab, classes=classes, want_ranks=True))
                        put(key + '/lovasz_' + classes, ('loss', 'dx'),
                            grad_of(lambda t: F.lovasz_softmax(t, lab, classes=classes), x))
                    put(key + '/pseudo', ('out', 'stats', 'conf'), semi.pseudo_labels(x, 0.6, return_conf=True))
                    put(key + '/pseudo_inv', ('out', 'stats', 'conf'),
                        semi.pseudo_labels(x, w, inverse=inv[:n + 3], labels=lab[inv[:n + 3]], return_conf=True))
                    for tname, tdtype in DTYPES.items():
                        t = place(zt, tdtype, off)
                        for kind in ('mse', 'kl'):
                            for mc in (0.0, 0.9):
                                k2 = '%s/cons_%s_%s_%g' % (key, tname, kind, mc)
                                put(k2, ('out2', 'per_row'), semi.consistency_forward(x, t, kind, mc, per_row=True))
                                put(k2, ('loss', 'dz'),
                                    grad_of(lambda s: semi.consistency_loss(s, t, kind=kind, min_conf=mc), x))
                key = 'n%d/c%d/probs/off%d' % (n, c, off)
                p, pt = place(pr, torch.float32, off), place(prt, torch.float32, off)
                put(key + '/lovasz', ('stats', 'grad', 'ranks'), F.lovasz_forward(p, lab, probs=True, want_ranks=True))
                put(key + '/lovasz', ('loss', 'dx'), grad_of(lambda t: F.lovasz_softmax_flat(t, lab), p))
                for mc in (0.0, 0.9):
                    k2 = '%s/cons_mse_%g' % (key, mc)
                    put(k2, ('out2', 'per_row'), semi.consistency_forward(p, pt, 'mse', mc, probs=True, per_row=True))
                    put(k2, ('loss', 'dz'),
                        grad_of(lambda s: semi.consistency_loss(s, pt, min_conf=mc, probs=True), p))
                x = place(z, torch.float32, off)
                for reps in (1, 3):
                    put('%s/view_mean_%d' % (key, reps), ('prob', 'pred'), view_mean_softmax(x, inv[:reps * (n + 3)], reps))
                    put('%s/view_scores_%d' % (key, reps), ('prob', 'pred', 'viewd', 'viewe', 'agree'),
                        view_scores(x, inv[:reps * (n + 3)], reps))
    torch.cuda.synchronize()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out')
    ap.add_argument('--compare', nargs=2)
    a = ap.parse_args()
    if a.compare:
        x, y = (json.load(open(f)) for f in a.compare)
        bad = sorted(k for k in set(x) | set(y) if x.get(k) != y.get(k))
        print('%d tensors compared, %d differ' % (len(set(x) | set(y)), len(bad)))
        for k in bad[:40]:
            print('  differs:', k)
        sys.exit(1 if bad or not x else 0)
    from lidal_amd import backend as B
    res = run()
    json.dump(res, open(a.out, 'w'), indent=0, sort_keys=True)
    print('%d tensors digested with %s' % (len(res), B.LIB_PATH))


if __name__ == '__main__':
    main()
