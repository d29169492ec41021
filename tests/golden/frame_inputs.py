"""Seeded inputs of the frame-level fixtures (tests/golden/make_golden_frame.py) that are too large to commit: the
generator and the tests both make them here, and the fixture keeps their sha256 so that a drift is caught."""
import hashlib

import numpy as np

FT_DIM = 96
# worker_func sizes: around the leaf (128) and numpy's 8192-value reduce buffer, and one full-size frame
WORKER_SIZES = [1, 7, 8, 9, 128, 129, 8192, 8193, 16385, 20000, 120000]
SEQS = ['00', '01', '02', '03', '04', '05', '06', '07', '09', '10']      # the reference's SK train_split


def sha256(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def _prob(rs, p, c, spread=3.0):
    logit = rs.normal(0.0, spread, size=(p, c))
    e = np.exp(logit - logit.max(1, keepdims=True))
    prob = (e / e.sum(1, keepdims=True)).astype(np.float32)
    prob[rs.random_sample((p, c)) < 0.03] = 0.0          # exact zeros: entr(0) = 0
    top = prob.argmax(1)
    tie = rs.random_sample(p) < 0.02                       # equal top two: margin 0
    prob[tie, (top[tie] + 1) % c] = prob[tie, top[tie]]
    return prob


def _sv2point(rs, p, n_sv):
    if p == 1:
        return [np.array([0], np.int64)]
    n_sv = max(1, min(n_sv, p))
    cuts = np.sort(rs.choice(np.arange(1, p), size=n_sv - 1, replace=False)) if n_sv > 1 else []
    perm = rs.permutation(p)
    sv = [np.sort(c).astype(np.int64) for c in np.split(perm, cuts)]
    if p > 2:                                              # a one-point supervoxel
        sv[-1], extra = sv[-1][:1], sv[-1][1:]
        sv[0] = np.sort(np.concatenate([sv[0], extra]))
    return sv


def worker_frame(k):
    """Frame k of the worker_func fixture: P = WORKER_SIZES[k], C = 19 (16 for odd k), prob, pred (frame 3 has
    predictions outside [0, C)), and its supervoxels (one of them a single point)."""
    p = WORKER_SIZES[k]
    c = 16 if k % 2 else 19
    rs = np.random.RandomState(1000 + k)
    prob = _prob(rs, p, c)
    pred = prob.argmax(1).astype(np.int64)
    if k == 3:
        pred[[1, 4]] = [-1, c]
    sv2point = _sv2point(rs, p, max(1, min(300, p // 40)))
    return {'prob': prob, 'pred': pred, 'sv2point': sv2point, 'class_num': c}


def empty_sv_frame():
    """A frame whose second supervoxel is empty: segment_entropy.py returns NaN (0 / 0)."""
    f = worker_frame(4)
    f['sv2point'] = [f['sv2point'][0], np.zeros(0, np.int64)] + list(f['sv2point'][1:])
    return f


# the __main__ trees: ENT / MAR / CONF / SEGENT / RAND on 10 sequences of 30 frames (num_add = 3)
MAIN_FRAMES, MAIN_P, MAIN_C = 30, 60, 19


def main_flags_in(seed=3):
    rs = np.random.RandomState(seed)
    return [rs.random_sample(MAIN_FRAMES) < 0.1 for _ in SEQS]


def main_frame(s_i, i):
    rs = np.random.RandomState(20000 + 100 * s_i + i)
    prob = _prob(rs, MAIN_P, MAIN_C, spread=1.0 + 3.0 * rs.random_sample())
    return {'prob': prob, 'pred': prob.argmax(1).astype(np.int64), 'sv2point': _sv2point(rs, MAIN_P, 4)}


# CSET: 10 sequences of 200 tiny frames (num_add = 20), 10 % labeled
CSET_FRAMES, CSET_P = 200, 12


def cset_flags_in(seed):
    rs = np.random.RandomState(seed)
    return [rs.random_sample(CSET_FRAMES) < 0.1 for _ in SEQS]


def cset_outfeat(seed, s_i, i):
    rs = np.random.RandomState(seed * 1000003 % (2 ** 31) + 1000 * s_i + i)
    return np.maximum(rs.normal(0.2 * rs.random_sample(), 1.0, size=(CSET_P, FT_DIM)), 0.0).astype(np.float32)


def cset_feats(seed):
    """all frames' outfeat.mean(0), in train_split order: f32 [2000, 96]"""
    return np.stack([cset_outfeat(seed, s, i).mean(0) for s in range(len(SEQS)) for i in range(CSET_FRAMES)])


def large_feats(n, d=FT_DIM, seed=0):
    """core-set input of dataset size: n frame features (rows of a few hundred clusters, ReLU-like)"""
    rs = np.random.RandomState(seed)
    centres = rs.uniform(0.0, 1.0, size=(300, d))
    return np.maximum(centres[rs.randint(300, size=n)] + rs.normal(0.0, 0.3, size=(n, d)), 0.0).astype(np.float32)
