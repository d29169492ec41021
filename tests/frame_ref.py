"""numpy restatement of the frame-level kernels' defined orders (csrc/frame_level.hip): the
per-frame entropy / margin / confidence means, the segment entropy, the frame feature and the project's core-set
distance and greedy loop.  Test infrastructure: the CPU side of the bit-for-bit checks."""
import numpy as np

from redal_ref import d2, np_mean_f32


def rows_pairwise_f32(a):
    """numpy's pairwise sum of each row of a f32 [P, C] (C <= 128: one leaf), vectorised over the rows."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    c = a.shape[1]
    if c < 8:
        r = np.zeros(a.shape[0], np.float32)
        for j in range(c):
            r = r + a[:, j]
        return r
    c8 = c - c % 8
    r = a[:, :8].copy()
    for i in range(8, c8, 8):
        r = r + a[:, i:i + 8]
    res = ((r[:, 0] + r[:, 1]) + (r[:, 2] + r[:, 3])) + ((r[:, 4] + r[:, 5]) + (r[:, 6] + r[:, 7]))
    for j in range(c8, c):
        res = res + a[:, j]
    return res


def entr_f32(pk):
    """scipy.special.entr on f32: -x log x in f64, rounded once; 0 at 0, -inf below."""
    x = pk.astype(np.float64)
    with np.errstate(all='ignore'):
        v = np.where(x > 0, -x * np.log(np.where(x > 0, x, 1.0)), np.where(x == 0, 0.0, -np.inf))
    return v.astype(np.float32)


def point_uncertainty(prob):
    """per point: (entropy, top1 - top2, top1), f32 [P] each"""
    prob = np.ascontiguousarray(prob, dtype=np.float32)
    s = rows_pairwise_f32(prob)
    ent = rows_pairwise_f32(entr_f32(prob / s[:, None]))
    srt = np.sort(prob, axis=1)
    return ent, srt[:, -1] - srt[:, -2], srt[:, -1].copy()


def uncertainty(prob):
    """(ENT, MAR, CONF) of one frame: np_mean_f32 of the per-point values"""
    return tuple(np_mean_f32(v) for v in point_uncertainty(prob))


def segment_entropy(pred, sv2point, class_num):
    """segment_entropy.py:41-50 written out: f64, classes in order, supervoxels in order, sv * n / P left to right."""
    pred = np.asarray(pred)
    p = pred.shape[0]
    frame = 0.0
    with np.errstate(all='ignore'):
        for ids in sv2point:
            v = pred[np.asarray(ids, dtype=np.int64)]
            n = v.shape[0]
            cnt = np.bincount(v[(v >= 0) & (v < class_num)], minlength=class_num)
            sv = 0.0
            for c in range(class_num):
                q = np.float64(cnt[c]) / np.float64(n)
                sv = sv + -q * np.log2(q + 1e-12)
            frame = frame + np.float64(sv) * np.float64(n) / np.float64(p)
    return np.float64(frame)


def frame_feature(feat):
    """outfeat.mean(0): per column the sequential f32 sum of the rows (d = 1: np_mean_f32), over f32(P)"""
    feat = np.ascontiguousarray(feat, dtype=np.float32)
    p, d = feat.shape
    if d == 1:
        return np.array([np_mean_f32(feat[:, 0])], np.float32)
    if p == 0:
        with np.errstate(invalid='ignore'):
            return np.zeros(d, np.float32) / np.float32(0)          # numpy's 0 / 0
    return (np.cumsum(feat, axis=0, dtype=np.float32)[-1] / np.float32(p)).astype(np.float32)


def dist(x, c):
    """The project's core-set distance of every row of x f32 [N, D] to the row c f32 [D]: f32(numpy's pairwise f64 sum
    of the squared differences), then the f32 square root."""
    return np.sqrt(d2(x.astype(np.float64), c.astype(np.float64)).astype(np.float32))


def initial_min_dist(x, labeled_ids, block=512):
    """min over the labeled rows of dist, exactly: an f64 Gram-matrix estimate of every squared distance picks, per row,
    the labeled rows within a safe margin of its smallest estimate; only those are evaluated in the defined order."""
    x = np.asarray(x, np.float32)
    x64 = x.astype(np.float64)
    lab = np.asarray(labeled_ids, np.int64)
    c64 = x64[lab]
    nx = (x64 ** 2).sum(1)
    nc = (c64 ** 2).sum(1)
    out = np.empty(len(x), np.float32)
    for b in range(0, len(x), block):
        est = nx[b:b + block, None] - 2.0 * (x64[b:b + block] @ c64.T) + nc[None]
        margin = 1e-9 * (nx[b:b + block, None] + nc[None]).max(1) + 1e-30
        lo = est.min(1)
        for r in range(est.shape[0]):
            cand = lab[est[r] <= lo[r] + 4 * margin[r]]
            v = np.sqrt(d2(x64[cand], x64[b + r]).astype(np.float32))
            out[b + r] = v.min()
    return out


def coreset(x, labeled, num_add):
    """core_set.py:74-92 with the project's distance: (picks [num_add] in order, final min_dist f32 [N]); ValueError
    where the reference asserts (a pick already selected)."""
    x = np.asarray(x, np.float32)
    labeled = np.asarray(labeled, bool)
    min_dist = initial_min_dist(x, np.where(labeled)[0])
    selected = labeled.copy()
    picks = []
    for _ in range(num_add):
        ind = int(np.argmax(min_dist))
        if selected[ind]:
            raise ValueError('pick %d already selected' % (len(picks) + 1))
        min_dist = np.minimum(min_dist, dist(x, x[ind]))
        selected[ind] = True
        picks.append(ind)
    return np.array(picks, np.int64), min_dist


def argpartition_probe(u, num_add):
    """What the host's numpy returns on u equal keys: the reference's zero-half selection, largest and smallest."""
    z = np.zeros(u, np.float32)
    return np.argpartition(z, -num_add)[-num_add:], np.argpartition(z, num_add)[:num_add]
