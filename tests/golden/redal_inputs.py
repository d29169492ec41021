"""Seeded inputs of the ReDAL fixtures (tests/golden/make_golden_redal.py) that are too large to commit: the generator
and the tests both make them here, and the fixture keeps their sha256 so that a drift in the generator is caught."""
import hashlib

import numpy as np

N_CLASSES, FT_DIM = 19, 96


def sha256(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def blobs():
    """150 well-separated blobs of 20 rows in 96 dimensions (spread 0.3, centres ~U(-50, 50)), rows shuffled."""
    rs = np.random.RandomState(1234)
    centres = rs.uniform(-50.0, 50.0, size=(150, FT_DIM))
    x = np.repeat(centres, 20, axis=0) + rs.normal(0.0, 0.3, size=(3000, FT_DIM))
    return x[rs.permutation(3000)].astype(np.float32)


def overlapping():
    """8000 rows around 40 centres with unit spread: clusters that overlap, k = 150 has no clean answer."""
    rs = np.random.RandomState(4321)
    centres = rs.uniform(-2.0, 2.0, size=(40, FT_DIM))
    return (centres[rs.randint(40, size=8000)] + rs.normal(0.0, 1.0, size=(8000, FT_DIM))).astype(np.float32)


def _frame(rs, p, n_sv):
    logit = rs.normal(0.0, 2.0, size=(p, N_CLASSES))
    e = np.exp(logit - logit.max(1, keepdims=True))
    prob = (e / e.sum(1, keepdims=True)).astype(np.float32)
    outfeat = np.maximum(rs.normal(0.0, 1.0, size=(p, FT_DIM)), 0.0).astype(np.float32)
    curvature = np.minimum(rs.uniform(0.0, 0.15, size=p), 0.1).astype(np.float32)
    cuts = np.sort(rs.choice(np.arange(1, p), size=n_sv - 1, replace=False))
    perm = rs.permutation(p)
    sv2point = [np.sort(c).astype(np.int64) for c in np.split(perm, cuts)]
    return {'prob': prob, 'outfeat': outfeat, 'curvature': curvature, 'sv2point': sv2point}


def worker_frames():
    """worker_func inputs: three frames of 600 points in 20 regions of random size, and one of 2400 points in 4 regions
    (> 128 points each: numpy's pairwise sum splits them)."""
    rs = np.random.RandomState(77)
    frames = [_frame(rs, 600, 20) for _ in range(3)] + [_frame(rs, 2400, 4)]
    gid = 0
    for f in frames:
        n = len(f['sv2point'])
        f['sv_id'] = np.arange(gid, gid + n, dtype=np.int64)
        gid += n
    return frames


MAIN_SEQS = ['00', '01', '02', '03', '04', '05', '06', '07', '09', '10']     # ReDAL.py:100
MAIN_FRAMES, MAIN_P, MAIN_SV = 8, 160, 20


def main_frames(seq_index):
    """The frames of one sequence of the ReDAL.py __main__ tree: 8 frames of 160 points in 20 regions each."""
    rs = np.random.RandomState(500 + seq_index)
    return [_frame(rs, MAIN_P, MAIN_SV) for _ in range(MAIN_FRAMES)]
