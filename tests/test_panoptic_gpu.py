"""evaluate.panoptic_accumulate (lidal_panoptic_accumulate) against the numpy restatement
tests/panoptic_ref.py: the integer sums equal, the IoU sums equal as 64-bit patterns, no tolerance anywhere -- on the
scene of the CPU test, across two calls, at the match threshold and the size threshold, at the borders of the scan's
tiles, at the ends of the key's fields, with bad ids, with garbage in the columns that are not looked at, under a row
permutation, in exactly-sized scratch between guards -- and end to end through euclidean_clusters and a model."""
import numpy as np
import pytest
import torch

import panoptic_ref as R
from guarded_ws import Guarded

pytestmark = pytest.mark.gpu
DEV = 'cuda'
C, THINGS = R.SCENE_C, R.SCENE_THINGS


def _g(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _host(stats):
    torch.cuda.synchronize()
    return {k: getattr(stats, k).cpu().numpy() for k in R.KEYS}


def _accumulate(cols, ptr, n_classes=C, things=THINGS, min_points=50, stats=None, lists=True):
    """cols = (pred_sem, pred_inst, gt_sem, gt_inst) on the host -> the stats after one call"""
    from lidal_amd.evaluate import PanopticStats, panoptic_accumulate
    stats = PanopticStats(n_classes, DEV) if stats is None else stats
    dev = [_g(np.asarray(c)) for c in cols]
    if lists:
        dev = [[t[int(ptr[s]):int(ptr[s + 1])] for s in range(len(ptr) - 1)] for t in dev]
    else:
        assert len(ptr) == 2
    assert panoptic_accumulate(stats, *dev, things=things, min_points=min_points) is stats
    return stats


def _check(cols, ptr, n_classes=C, things=THINGS, min_points=50):
    """One call on fresh stats against the reference -> the reference's dict."""
    want = R.panoptic_ref(*cols, ptr, n_classes, things, min_points)
    got = _host(_accumulate(cols, ptr, n_classes, things, min_points))
    assert R.same(got, want), (got, want)
    return want


def _one(ps, pi, gs, gi):
    cols = (np.asarray(ps, np.int64), np.asarray(pi, np.int32), np.asarray(gs, np.int64), np.asarray(gi, np.int32))
    return cols, np.array([0, len(cols[0])], np.int64)


@pytest.fixture(scope='module')
def scene():
    ps, pi, gs, gi, ptr = R.scene()
    return dict(cols=(ps, pi, gs, gi), ptr=ptr, want=R.panoptic_ref(ps, pi, gs, gi, ptr, C, THINGS, 50))


# ---- 1. the scene ----------------------------------------------------------------------------------------------------------
def test_the_scene(scene):
    from lidal_amd import backend as B
    before = B.HITS.get('panoptic_accumulate', 0)
    got = _host(_accumulate(scene['cols'], scene['ptr']))
    assert B.HITS['panoptic_accumulate'] == before + 1                    # one library call
    assert R.same(got, scene['want']), (got, scene['want'])
    assert got['tp'].sum() > 0 and got['fp'].sum() > 0 and got['fn'].sum() > 0
    again = _host(_accumulate(scene['cols'], scene['ptr']))               # fresh stats: the same bits
    assert R.same(again, got)


def test_one_tensor_is_one_scan(scene):
    """Without the list the rows are one scan: equal ids of different scans merge, as the reference says for one scan."""
    ptr1 = np.array([0, len(scene['cols'][0])], np.int64)
    want = R.panoptic_ref(*scene['cols'], ptr1, C, THINGS, 50)
    assert not R.same(want, scene['want'])
    assert R.same(_host(_accumulate(scene['cols'], ptr1, lists=False)), want)


def test_two_calls_accumulate(scene):
    other = R.random_case(4)
    stats = _accumulate(scene['cols'], scene['ptr'])
    stats = _accumulate(other[:4], other[4], stats=stats)
    want = R.panoptic_ref(*other, C, THINGS, 50, acc=scene['want'])
    assert R.same(_host(stats), want)
    stats = _accumulate(scene['cols'], scene['ptr'], min_points=1, stats=stats)       # a third, with another threshold
    assert R.same(_host(stats), R.panoptic_ref(*scene['cols'], scene['ptr'], C, THINGS, 1, acc=want))


@pytest.mark.parametrize('seed', [1, 2])
def test_random_rows(seed):
    case = R.random_case(seed)
    for min_points in (1, 20):
        _check(case[:4], case[4], min_points=min_points)


# ---- 2. the thresholds ---------------------------------------------------------------------------------------------------
def test_exactly_one_half_is_no_match():
    cols, ptr = _one([0, 0, 0, 0], [7, 7, 8, 8], [0, 0, 0, 0], [3, 3, 3, 3])        # gt 4 rows, pred 2 + 2 of them
    want = _check(cols, ptr, 1, (0,), 1)
    assert (want['tp'][0], want['fp'][0], want['fn'][0], want['iou'][0]) == (0, 2, 1, 0.0)
    cols, ptr = _one([0, 0, 0], [7, 7, 8], [0, 0, 0], [3, 3, 3])                    # gt 3 rows, pred 2 of them: 2/3
    want = _check(cols, ptr, 1, (0,), 1)
    assert (want['tp'][0], want['fp'][0], want['fn'][0], want['iou'][0]) == (1, 1, 0, 2.0 / 3.0)
    cols, ptr = _one([1, 1, 0, 0], [0, 0, 0, 0], [1, 1, 1, 1], [0, 0, 0, 0])        # the same on a stuff class
    want = _check(cols, ptr, 2, (), 1)
    assert want['tp'].tolist() == [0, 0] and want['fp'].tolist() == [1, 1] and want['fn'].tolist() == [0, 1]


def test_min_points_counts_from_its_value_on():
    """Unmatched segments of 49 and 50 rows on either side: at min_points = 50 only the larger ones count."""
    gs = np.zeros(49 + 50 + 49 + 50 + 10, np.int64)
    gi = np.concatenate([np.full(49, 1), np.full(50, 2), np.full(99, 3), np.full(10, 4)])
    ps = np.concatenate([np.full(99, 255), np.zeros(109, np.int64)])                 # the first two are missed
    pi = np.concatenate([np.zeros(99), np.full(49, 5), np.full(50, 6), np.full(10, 7)])  # 3 is split 49 / 50: 50/99 matches
    cols, ptr = _one(ps, pi, gs, gi)
    want = _check(cols, ptr, 1, (0,), 50)
    assert (want['tp'][0], want['fp'][0], want['fn'][0]) == (2, 0, 1) and want['iou'][0] == 50.0 / 99.0 + 1.0
    want = _check(cols, ptr, 1, (0,), 49)
    assert (want['tp'][0], want['fp'][0], want['fn'][0]) == (2, 1, 2)
    want = _check(cols, ptr, 1, (0,), 1)
    assert (want['tp'][0], want['fp'][0], want['fn'][0]) == (2, 1, 2)
    want = _check(cols, ptr, 1, (0,), 51)
    assert (want['tp'][0], want['fp'][0], want['fn'][0]) == (2, 0, 0)


# ---- 3. tile borders of the flag scan (2048 rows) ------------------------------------------------------------------------
@pytest.mark.parametrize('p', [1, 63, 64, 65, 2047, 2048, 2049, 4097])
def test_tile_borders(p):
    """One thing class, every row live, so a row's sorted position is its rank by id: segments of random sizes, one of
    which (when there are that many rows) covers the sorted positions 2040 .. 2059 on the gt side; the predictions move
    a quarter of the rows to a neighbouring id, so runs of all three sorts cross the border."""
    rng = np.random.RandomState(p)
    sizes = []
    while sum(sizes) < p:
        sizes.append(20 if sum(sizes) == 2040 else min(int(rng.randint(1, 40)), 2040 - sum(sizes))
                     if sum(sizes) < 2040 else int(rng.randint(1, 40)))
    gi = np.repeat(np.arange(len(sizes)), sizes)[:p]
    if p >= 2049:
        assert gi[2039] != gi[2040] and gi[2040] == gi[2047] == gi[2048] == gi[min(2049, p - 1)]
    pi = np.where(rng.rand(p) < 0.25, gi + 1, gi)
    order = rng.permutation(p)
    zeros = np.zeros(p, np.int64)
    cols, ptr = _one(zeros, pi[order], zeros, gi[order])
    want = _check(cols, ptr, 1, (0,), 1)
    assert want['tp'][0] + want['fn'][0] == len(np.unique(gi))
    _check(cols, ptr, 1, (0,), 25)


# ---- 4. the ends of the fields -----------------------------------------------------------------------------------------------
def test_field_extremes():
    """Class 63 of 64, gt id 65535 (the largest a label word holds), pred ids 2^30 - 2 and -1, 32 scans of which only
    the first and the last have rows -- with the same ids, which must stay apart."""
    n = 40
    gs, ps = np.full(2 * n, 63, np.int64), np.full(2 * n, 63, np.int64)
    gi = np.tile(np.concatenate([np.full(25, 65535), np.full(15, 0)]), 2)
    pi = np.tile(np.concatenate([np.full(20, 2 ** 30 - 2), np.full(20, -1)]), 2)
    ptr = np.array([0] + [n] * 31 + [2 * n], np.int64)
    cols = (ps, pi.astype(np.int32), gs, gi.astype(np.int32))
    want = _check(cols, ptr, 64, (0, 63), 1)
    assert want['tp'][63] == 4 and want['fp'][63] == 0 and want['iou'][63] == 0.0 + 15 / 20 + 20 / 25 + 15 / 20 + 20 / 25
    merged = R.panoptic_ref(*cols, np.array([0, 2 * n], np.int64), 64, (0, 63), 1)
    assert merged['tp'][63] == 2                                           # what one scan would give
    _check(cols, ptr, 64, (), 1)                                           # ... and with class 63 as stuff
    ptr2 = np.array([0] * 31 + [n, 2 * n], np.int64)                       # the rows in the last two scans
    _check(cols, ptr2, 64, (63,), 1)


def test_nothing_to_score():
    from lidal_amd.evaluate import panoptic_accumulate
    case = R.random_case(6)
    ps, pi, gs, gi, ptr = case
    want = _check((ps, pi, np.full_like(gs, 255), gi), ptr)                # every row void
    assert want['tp'].sum() == want['fp'].sum() == want['fn'].sum() == 0
    want = _check((np.full_like(ps, -1), pi, gs, gi), ptr, min_points=1)   # no row with a predicted segment
    assert want['tp'].sum() == want['fp'].sum() == 0 and want['fn'].sum() > 0
    stats = _accumulate(case[:4], ptr)                                     # p = 0: the stats stay as they are
    before = _host(stats)
    none64, none32 = torch.empty(0, dtype=torch.int64, device=DEV), torch.empty(0, dtype=torch.int32, device=DEV)
    panoptic_accumulate(stats, none64, none32, none64, none32, THINGS)
    panoptic_accumulate(stats, [none64] * 3, [none32] * 3, [none64] * 3, [none32] * 3, THINGS)
    assert R.same(_host(stats), before)


def test_bad_ids_raise_and_count_as_the_definition_says():
    from lidal_amd.evaluate import panoptic_quality
    ps, pi, gs, gi, ptr = R.random_case(9)
    thing_g = np.nonzero(np.isin(gs, THINGS))[0]
    thing_p = np.nonzero(np.isin(gs, THINGS) & np.isin(ps, THINGS))[0]
    gi[thing_g[3]], pi[thing_p[5]] = 2 ** 30 - 1, -2
    want = R.panoptic_ref(ps, pi, gs, gi, ptr, C, THINGS, 1)
    assert want['status'][0] == 1
    stats = _accumulate((ps, pi, gs, gi), ptr, min_points=1)
    assert R.same(_host(stats), want)
    with pytest.raises(ValueError, match='outside'):
        panoptic_quality(stats, THINGS)
    stats = _accumulate(R.random_case(10)[:4], R.random_case(10)[4], stats=stats)    # the word stays set
    assert _host(stats)['status'][0] == 1


def test_instance_columns_of_stuff_rows_are_not_looked_at(scene):
    ps, pi, gs, gi = (c.copy() for c in scene['cols'])
    rng = np.random.RandomState(12)
    stuff_g, stuff_p = ~np.isin(gs, THINGS), ~np.isin(ps, THINGS)
    gi[stuff_g] = rng.randint(-2 ** 31, 2 ** 31 - 1, int(stuff_g.sum()))
    pi[stuff_p] = rng.randint(-2 ** 31, 2 ** 31 - 1, int(stuff_p.sum()))
    assert not np.array_equal(gi, scene['cols'][3]) and not np.array_equal(pi, scene['cols'][1])
    got = _host(_accumulate((ps, pi, gs, gi), scene['ptr']))
    assert R.same(got, scene['want']) and got['status'][0] == 0


def test_a_row_permutation_gives_the_same_bits(scene):
    for seed in (5, 6):
        cols = R.permuted(scene['cols'], scene['ptr'], seed)
        assert R.same(_host(_accumulate(cols, scene['ptr'])), scene['want'])


# ---- 5. exactly-sized scratch ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['scene', 'one row', 'tile'])
def test_exact_scratch_between_guards(scene, case):
    from lidal_amd import backend as B
    from lidal_amd.evaluate import PanopticStats
    if case == 'scene':
        cols, ptr, n_classes, things = scene['cols'], scene['ptr'], C, THINGS
    else:
        p = 1 if case == 'one row' else 2048
        rng = np.random.RandomState(3)
        (cols, ptr), n_classes, things = _one(np.zeros(p), rng.randint(0, 9, p), np.zeros(p), rng.randint(0, 9, p)), 1, (0,)
    want = R.panoptic_ref(*cols, ptr, n_classes, things, 5)
    mask = sum(1 << t for t in things)
    ps, pi, gs, gi = (_g(c) for c in cols)
    p, n = len(cols[0]), len(ptr) - 1
    L = B.lib()
    nbytes = L.lidal_panoptic_accumulate_workspace_bytes(p, n)
    guarded = Guarded()
    ws = guarded(nbytes)
    stats = PanopticStats(n_classes, DEV)
    rc = L.lidal_panoptic_accumulate(B.ptr(ps), B.ptr(pi), B.ptr(gs), B.ptr(gi), p, ptr.ctypes.data, n, n_classes, mask, 5,
                                     B.ptr(stats.tp), B.ptr(stats.fp), B.ptr(stats.fn), B.ptr(stats.iou),
                                     B.ptr(stats.status), B.ptr(ws), nbytes, B.stream())
    assert rc == 0, L.lidal_last_error()
    guarded.check()
    assert R.same(_host(stats), want)
    rc = L.lidal_panoptic_accumulate(B.ptr(ps), B.ptr(pi), B.ptr(gs), B.ptr(gi), p, ptr.ctypes.data, n, n_classes, mask, 5,
                                     B.ptr(stats.tp), B.ptr(stats.fp), B.ptr(stats.fn), B.ptr(stats.iou),
                                     B.ptr(stats.status), B.ptr(ws), nbytes - 1, B.stream())
    assert rc == 2 and b'workspace' in L.lidal_last_error()


# ---- 6. end to end -------------------------------------------------------------------------------------------------------
def _blobs():
    """Two scans of well separated objects, 5 m apart: cubes of 0.1 m (every two points of one nearer than 0.18 m) of
    classes 0 and 1, one dumbbell per scan -- two such cubes of 60 points whose centres are 0.4 m apart, so every
    distance across is in [0.3, 0.53] -- and a stuff class 2 far below.  -> per-scan points, labels, gt ids, objects."""
    rng = np.random.RandomState(8)
    scans, n_objects = [], np.zeros(3, np.int64)
    for s in range(2):
        xyz, sem, inst = [], [], []
        for k in range(9 + s):
            centre = np.array([5.0 * (k % 4), 5.0 * (k // 4), 1.0])
            n = int(rng.randint(55, 90))
            xyz.append(centre + rng.uniform(-0.05, 0.05, (n, 3)))
            sem.append(np.full(n, k % 2)); inst.append(np.full(n, k + 1))
            n_objects[k % 2] += 1
        for half in (-0.2, 0.2):
            xyz.append(np.array([20.0 + half, 20.0, 1.0]) + rng.uniform(-0.05, 0.05, (60, 3)))
            sem.append(np.zeros(60, np.int64)); inst.append(np.full(60, 40))
        n_objects[0] += 1
        ground = np.concatenate([rng.uniform(0, 25, (300, 2)), np.full((300, 1), -5.0)], 1)
        xyz.append(ground); sem.append(np.full(300, 2)); inst.append(np.zeros(300, np.int64))
        n_objects[2] += 1
        order = rng.permutation(sum(len(x) for x in xyz))
        scans.append((np.concatenate(xyz).astype(np.float32)[order], np.concatenate(sem).astype(np.int64)[order],
                      np.concatenate(inst).astype(np.int32)[order]))
    return scans, n_objects


def test_clusters_of_separated_objects_score_one():
    from lidal_amd import data
    from lidal_amd.evaluate import PanopticStats, panoptic_accumulate, panoptic_quality
    scans, n_objects = _blobs()
    pts, sem, gt = ([_g(sc[j]) for sc in scans] for j in range(3))
    ptr = np.concatenate([[0], np.cumsum([len(sc[0]) for sc in scans])]).astype(np.int64)
    host = lambda j: np.concatenate([sc[j] for sc in scans])
    for tol, split in ((0.5, False), (0.25, True)):
        found = data.euclidean_clusters(pts, sem, tolerance={0: tol, 1: tol}, min_points=1)
        stats = PanopticStats(3, DEV)
        panoptic_accumulate(stats, sem, list(torch.split(found.inst, [len(sc[0]) for sc in scans])), sem, gt, things=(0, 1))
        got = _host(stats)
        assert R.same(got, R.panoptic_ref(host(1), found.inst.cpu().numpy(), host(1), host(2), ptr, 3, (0, 1), 50))
        q = panoptic_quality(stats, (0, 1))
        if not split:
            assert np.array_equal(got['tp'], n_objects) and got['fp'].sum() == got['fn'].sum() == 0
            assert np.array_equal(got['iou'], got['tp'].astype(np.float64))
            assert q['PQ'] == q['PQ_th'] == q['PQ_st'] == q['SQ'] == q['RQ'] == 1.0 and q['present'].all()
        else:                                                              # the dumbbells fall in two halves of exactly 1/2
            assert got['tp'].tolist() == [n_objects[0] - 2, n_objects[1], 2]
            assert got['fp'].tolist() == [4, 0, 0] and got['fn'].tolist() == [2, 0, 0]
            assert q['pq'][0] == (n_objects[0] - 2) / (n_objects[0] - 2 + 3.0) and q['PQ_st'] == 1.0


def test_evaluate_panoptic_batches():
    """An untrained SPVCNN over two synthetic validation batches: the sums are the reference's on the model's own argmax
    and the clusters' ids (both computed again and read back), the confusion is evaluate_batches'."""
    from lidal_amd import SparseTensor, data, synth
    from lidal_amd.evaluate import evaluate_batches, evaluate_panoptic_batches, panoptic_quality
    from lidal_amd.network import SPVCNN
    torch.manual_seed(3)
    model = SPVCNN(19).to(DEV).eval()
    table = data.sk_label_map()
    ids = np.nonzero(table != 255)[0]
    rng = np.random.default_rng(23)
    world = synth.make_world(5)
    scans, raws = [], []
    for i in range(3):
        pts, inten = synth.raycast_scan(world, (18.0 + 2 * i, 0.0), np.random.default_rng([21, i]), n_beams=16, n_az=256)
        p = pts.shape[0]
        raw = (rng.choice(np.concatenate([ids, [0]]), p) | (rng.integers(0, 4, p) << 16)).astype(np.uint32)
        raw[:3] |= np.uint32(0x80000000)                                   # ids with the top bit set
        scans.append((_g(pts), _g(inten)))
        raws.append(_g(raw.view(np.int32)))
    rs = np.random.RandomState(10)
    batches = [data.val_batch(scans[:2], raws[:2], table, rng=rs, with_instances=True),
               data.val_batch(scans[2:], raws[2:], table, rng=rs, with_instances=True)]
    assert [len(b['points']) for b in batches] == [2, 1] and batches[0]['gt_inst'][0].dtype == torch.int32
    assert int(batches[0]['gt_inst'][0][0]) >= 32768
    plain = data.val_batch(scans[:2], raws[:2], table, rng=np.random.RandomState(10))
    assert 'points' not in plain and 'gt_inst' not in plain and torch.equal(plain['labels_p_b'], batches[0]['labels_p_b'])
    tol = {c: 0.5 for c in data.SK_THINGS}
    stats, quality, conf, miou = evaluate_panoptic_batches(model, batches, data.SK_THINGS, tol, min_points=5)
    want = None
    with torch.no_grad():
        for b in batches:
            logits, _ = model(SparseTensor(b['feats_v_b'], b['coords_v_b']))
            pred = logits.argmax(1)[b['inverse_indices_b'].long()]
            sizes = [x.shape[0] for x in b['points']]
            inst = data.euclidean_clusters(b['points'], list(torch.split(pred, sizes)), tolerance=tol, min_points=1)
            ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
            want = R.panoptic_ref(pred.cpu().numpy(), inst.inst.cpu().numpy(), b['labels_p_b'].cpu().numpy(),
                                  torch.cat(b['gt_inst']).cpu().numpy(), ptr, 19, data.SK_THINGS, 5, acc=want)
    got = {k: getattr(stats, k).numpy() for k in R.KEYS}
    assert not stats.tp.is_cuda and R.same(got, want), (got, want)
    assert want['tp'].sum() + want['fp'].sum() + want['fn'].sum() > 0
    again = panoptic_quality(stats, data.SK_THINGS)
    assert all(np.array_equal(quality[k], again[k], equal_nan=True) for k in quality)
    conf2, _, miou2 = evaluate_batches(model, batches)
    assert np.array_equal(conf, conf2) and (miou == miou2 or (np.isnan(miou) and np.isnan(miou2)))
