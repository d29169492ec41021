"""The specification of lidal_panoptic_accumulate (include/lidal_amd.h) in numpy, twice:
panoptic_ref, vectorised with one np.unique per scan, class and side, and panoptic_brute, row by row with dictionaries
and no sort, which decides a match by the f64 quotient instead of the integers.  test_panoptic_cpu.py holds the two
against each other bit for bit; the GPU tests hold the library against panoptic_ref.

A row is void iff gt_sem is outside [0, C); a thing row (class in `things`) has id = inst + 1, a stuff row id = 0; an
instance value of a thing row outside [-1, 2^30 - 2] voids the row (gt) or takes its prediction away (pred) and sets
status.  Segments are per scan.  A gt and a predicted segment of one class match iff 2 * inter > union; an unmatched
segment counts (fn / fp) iff its area >= min_points; iou[c] = iou_in[c] + part[c], part[c] = 0.0 + the matches'
inter / union one by one in ascending (scan, gt id)."""
import numpy as np

ID_MAX = 2 ** 30 - 2
KEYS = ('tp', 'fp', 'fn', 'iou', 'status')


def zeros(C):
    return dict(tp=np.zeros(C, np.int64), fp=np.zeros(C, np.int64), fn=np.zeros(C, np.int64), iou=np.zeros(C, np.float64),
                status=np.zeros(1, np.int64))


def _start(C, acc):
    out = zeros(C)
    if acc is not None:
        for k in KEYS:
            out[k] = np.array(acc[k], dtype=out[k].dtype).reshape(out[k].shape).copy()
    return out


# ---------------------------------------------------------------- vectorised
def panoptic_ref(pred_sem, pred_inst, gt_sem, gt_inst, ptr, C, things, min_points=50, acc=None):
    """-> dict(tp, fp, fn i64 [C], iou f64 [C], status i64 [1]); acc: the same dict of an earlier call, carried on."""
    ps, gs = np.asarray(pred_sem, np.int64), np.asarray(gt_sem, np.int64)
    pi, gi = np.asarray(pred_inst, np.int64), np.asarray(gt_inst, np.int64)
    out = _start(C, acc)
    is_thing = np.zeros(C, bool)
    is_thing[list(things)] = True
    live = (gs >= 0) & (gs < C)
    g_thing = live & is_thing[np.clip(gs, 0, C - 1)]
    g_bad = g_thing & ((gi < -1) | (gi > ID_MAX))
    live &= ~g_bad
    has = live & (ps >= 0) & (ps < C)
    p_thing = has & is_thing[np.clip(ps, 0, C - 1)]
    p_bad = p_thing & ((pi < -1) | (pi > ID_MAX))
    has &= ~p_bad
    if g_bad.any() or p_bad.any():
        out['status'][0] = max(int(out['status'][0]), 1)
    gid, pid = np.where(g_thing, gi + 1, 0), np.where(p_thing, pi + 1, 0)
    part = [0.0] * C
    for s in range(len(ptr) - 1):
        lo, hi = int(ptr[s]), int(ptr[s + 1])
        for c in range(C):
            g = live[lo:hi] & (gs[lo:hi] == c)
            p = has[lo:hi] & (ps[lo:hi] == c)
            gids, garea = np.unique(gid[lo:hi][g], return_counts=True)
            pids, parea = np.unique(pid[lo:hi][p], return_counts=True)
            both = g & p
            pair, inter = np.unique((gid[lo:hi][both] << 31) | pid[lo:hi][both], return_counts=True)
            ug, up = pair >> 31, pair & (2 ** 31 - 1)
            union = garea[np.searchsorted(gids, ug)] + parea[np.searchsorted(pids, up)] - inter
            match = 2 * inter > union
            for v in inter[match].astype(np.float64) / union[match].astype(np.float64):   # ascending gt id
                part[c] = part[c] + float(v)
            out['tp'][c] += int(match.sum())
            out['fn'][c] += int(((garea >= min_points) & ~np.isin(gids, ug[match])).sum())
            out['fp'][c] += int(((parea >= min_points) & ~np.isin(pids, up[match])).sum())
    for c in range(C):
        out['iou'][c] = out['iou'][c] + np.float64(part[c])
    return out


# ---------------------------------------------------------------- row by row
def panoptic_brute(pred_sem, pred_inst, gt_sem, gt_inst, ptr, C, things, min_points=50, acc=None):
    out = _start(C, acc)
    things = set(int(t) for t in things)
    g_area, p_area, inter = {}, {}, {}
    bad = False
    scan = 0
    for i in range(len(gt_sem)):
        while i >= ptr[scan + 1]:
            scan += 1
        c = int(gt_sem[i])
        if not 0 <= c < C:
            continue
        ident = 0
        if c in things:
            if not -1 <= int(gt_inst[i]) <= ID_MAX:
                bad = True
                continue
            ident = int(gt_inst[i]) + 1
        g = (c, scan, ident)
        g_area[g] = g_area.get(g, 0) + 1
        d = int(pred_sem[i])
        if not 0 <= d < C:
            continue
        ident = 0
        if d in things:
            if not -1 <= int(pred_inst[i]) <= ID_MAX:
                bad = True
                continue
            ident = int(pred_inst[i]) + 1
        p = (d, scan, ident)
        p_area[p] = p_area.get(p, 0) + 1
        if c == d:
            inter[(g, p)] = inter.get((g, p), 0) + 1
    g_match, p_match = {}, set()
    for (g, p), n in inter.items():
        q = float(n) / float(g_area[g] + p_area[p] - n)
        if q > 0.5:
            assert g not in g_match and p not in p_match, 'a segment with two matches'
            g_match[g] = q
            p_match.add(p)
    part = [0.0] * C
    for g in sorted(g_match):                              # (class, scan, id): ascending (scan, gt id) inside a class
        part[g[0]] = part[g[0]] + g_match[g]
        out['tp'][g[0]] += 1
    for g, n in g_area.items():
        if g not in g_match and n >= min_points:
            out['fn'][g[0]] += 1
    for p, n in p_area.items():
        if p not in p_match and n >= min_points:
            out['fp'][p[0]] += 1
    for c in range(C):
        out['iou'][c] = out['iou'][c] + np.float64(part[c])
    if bad:
        out['status'][0] = max(int(out['status'][0]), 1)
    return out


def same(a, b):
    """every integer equal, iou equal as 64-bit patterns"""
    return all(np.array_equal(np.asarray(a[k]).view(np.int64), np.asarray(b[k]).view(np.int64)) and
               np.asarray(a[k]).dtype == np.asarray(b[k]).dtype for k in KEYS)


def segments(pred_sem, pred_inst, gt_sem, gt_inst, ptr, C, things):
    """What the tests ask of a scene: ({gt segment: area}, {predicted segment: area}, {(gt, pred): inter}, matched gt
    set, matched pred set), segments as (class, scan, id); no bad ids."""
    things = set(things)
    ga, pa, it = {}, {}, {}
    for s in range(len(ptr) - 1):
        for i in range(int(ptr[s]), int(ptr[s + 1])):
            c, d = int(gt_sem[i]), int(pred_sem[i])
            if not 0 <= c < C:
                continue
            g = (c, s, int(gt_inst[i]) + 1 if c in things else 0)
            ga[g] = ga.get(g, 0) + 1
            if not 0 <= d < C:
                continue
            p = (d, s, int(pred_inst[i]) + 1 if d in things else 0)
            pa[p] = pa.get(p, 0) + 1
            if c == d:
                it[(g, p)] = it.get((g, p), 0) + 1
    gm = {g for (g, p), n in it.items() if 2 * n > ga[g] + pa[p] - n}
    pm = {p for (g, p), n in it.items() if 2 * n > ga[g] + pa[p] - n}
    return ga, pa, it, gm, pm


# ---------------------------------------------------------------- inputs
SCENE_C = 8
SCENE_THINGS = (0, 1, 2, 3)


def permuted(cols, ptr, seed):
    """the columns with the rows of every scan permuted (the same permutation for every column)"""
    rng = np.random.RandomState(seed)
    order = np.concatenate([int(ptr[s]) + rng.permutation(int(ptr[s + 1] - ptr[s])) for s in range(len(ptr) - 1)])
    return [np.asarray(c)[order] for c in cols]


def scene(seed=7):
    """3 scans of about 3 000 rows, C = 8 (things 0..3, stuff 4..7), the failure cases built on purpose in every scan:
    an object split 120 / 80 (a match and a false positive), an object split 50 / 50 (IoU exactly 1/2 twice: no match,
    two unmatched predictions of area 50), two objects merged (a match and a miss), objects of 70, 50 and 49 rows
    predicted as road (misses, the last below min_points = 50), objects of 55 and 49 rows predicted on stuff, a stuff
    class half mislabelled in scan 0 (IoU exactly 1/2), void rows, rows without a prediction, unassigned rows (-1) on
    both sides, garbage in the instance columns of stuff rows; the rows of a scan shuffled.
    -> (pred_sem i64, pred_inst i32, gt_sem i64, gt_inst i32, ptr i64 [4])"""
    rng = np.random.RandomState(seed)
    scans = []
    for s in range(3):
        rows = []                                          # (n, gt_sem, gt_inst, pred_sem, pred_inst); None: garbage

        def add(n, gs, gi, ps, pi):
            rows.append((n, gs, gi, ps, pi))

        for k in range(6):                                 # found objects, a tenth of each left unassigned
            c, n = int(rng.randint(0, 4)), int(rng.randint(60, 200))
            add(n - n // 10, c, k + 1, c, 100 + k)
            add(n // 10, c, k + 1, c, -1)
        add(120, 0, 50, 0, 150); add(80, 0, 50, 0, 151)    # split: 0.6 matches, 80 is a false positive
        add(50, 1, 51, 1, 152); add(50, 1, 51, 1, 153)     # split in halves: 1/2 and 1/2
        add(100, 2, 52, 2, 154); add(60, 2, 53, 2, 154)    # merged: 100 / 160 matches, 60 is a miss
        add(70, 3, 54, 4, None)                            # missed: predicted as class 4
        add(49, 3, 55, 4, None)
        add(50, 0, 56, 4, None)
        add(55, 5, None, 1, 160)                           # hallucinated on class 5
        add(49, 5, None, 2, 161)
        add(40, 3, -1, 3, -1)                              # unassigned on both sides: segment 0 of class 3
        add(500, 4, None, 4, None)
        add(400, 5, None, 5, None)
        if s == 0:
            add(200, 6, None, 6, None); add(200, 6, None, 7, None)        # half mislabelled: 200 / 400
        else:
            add(400, 6, None, 6, None)
        add(300, 7, None, 7, None)
        add(30, 7, None, 255, None)                        # no prediction
        add(100, 255, None, None, None)                    # void, whatever is predicted
        cols = [[], [], [], []]
        for n, gs, gi, ps, pi in rows:
            garbage = lambda: rng.randint(-2 ** 31, 2 ** 31 - 1, n)
            cols[0].append(rng.randint(0, SCENE_C, n) if ps is None else np.full(n, ps))
            cols[1].append(garbage() if pi is None and ps not in (None,) + SCENE_THINGS else
                           rng.randint(0, 5, n) if pi is None else np.full(n, pi))
            cols[2].append(np.full(n, gs))
            cols[3].append(garbage() if gi is None and gs not in SCENE_THINGS else
                           rng.randint(0, 5, n) if gi is None else np.full(n, gi))
        cols = [np.concatenate(c) for c in cols]
        order = rng.permutation(len(cols[0]))
        scans.append([c[order] for c in cols])
    ptr = np.concatenate([[0], np.cumsum([len(sc[0]) for sc in scans])]).astype(np.int64)
    ps, pi, gs, gi = (np.concatenate([sc[j] for sc in scans]) for j in range(4))
    return ps.astype(np.int64), pi.astype(np.int32), gs.astype(np.int64), gi.astype(np.int32), ptr


def random_case(seed, n_scans=3, rows=1000, C=SCENE_C, n_ids=6, agree=0.75):
    """Random rows: gt classes 0..C-1 and 255, ids -1..n_ids-2; the prediction repeats the annotation with probability
    `agree` per column and is random otherwise (classes 0..C-1 and 255)."""
    rng = np.random.RandomState(seed)
    sizes = rng.randint(rows // 2, rows + rows // 2, n_scans)
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    p = int(ptr[-1])
    classes = np.concatenate([np.arange(C), [255]])
    gs = classes[rng.randint(0, C + 1, p)]
    gi = rng.randint(-1, n_ids - 1, p)
    ps = np.where(rng.rand(p) < agree, gs, classes[rng.randint(0, C + 1, p)])
    pi = np.where(rng.rand(p) < agree, gi, rng.randint(-1, n_ids - 1, p))
    return ps.astype(np.int64), pi.astype(np.int32), gs.astype(np.int64), gi.astype(np.int32), ptr
