"""Panoptic quality without a GPU: the two restatements of tests/panoptic_ref.py against each other bit for bit, what
the scene is built to contain, the arithmetic of evaluate.panoptic_quality, data.instance_ids and SK_THINGS, the header
against backend.SIGNATURES and the refusals that come before the device is touched."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import panoptic_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C, THINGS = R.SCENE_C, R.SCENE_THINGS


@pytest.fixture(scope='module')
def scene():
    return R.scene()


@pytest.mark.parametrize('min_points', [1, 50])
def test_the_two_restatements_agree_on_the_scene(scene, min_points):
    a = R.panoptic_ref(*scene, C, THINGS, min_points)
    b = R.panoptic_brute(*scene, C, THINGS, min_points)
    assert R.same(a, b), (a, b)
    assert a['status'][0] == 0 and a['tp'].sum() > 0


@pytest.mark.parametrize('seed', [1, 2, 3])
def test_the_two_restatements_agree_on_random_rows(seed):
    case = R.random_case(seed)
    for min_points in (1, 20, 50):
        assert R.same(R.panoptic_ref(*case, C, THINGS, min_points), R.panoptic_brute(*case, C, THINGS, min_points))
    rare = R.random_case(100 + seed, agree=0.55, n_ids=3)          # near the threshold: pairs at and around 1/2
    assert R.same(R.panoptic_ref(*rare, C, THINGS, 1), R.panoptic_brute(*rare, C, THINGS, 1))


def test_bad_ids_void_the_row_or_its_prediction_in_both():
    ps, pi, gs, gi, ptr = R.random_case(9)
    thing_g, thing_p = np.nonzero(np.isin(gs, THINGS))[0], np.nonzero(np.isin(gs, THINGS) & np.isin(ps, THINGS))[0]
    gi[thing_g[3]], pi[thing_p[5]] = 2 ** 30 - 1, -2
    a, b = R.panoptic_ref(ps, pi, gs, gi, ptr, C, THINGS, 1), R.panoptic_brute(ps, pi, gs, gi, ptr, C, THINGS, 1)
    assert R.same(a, b) and a['status'][0] == 1
    gs2, ps2 = gs.copy(), ps.copy()
    gs2[thing_g[3]], ps2[thing_p[5]] = 255, 255                    # the same rows made void / unpredicted by hand
    c = R.panoptic_ref(ps2, pi, gs2, gi, ptr, C, THINGS, 1)
    assert all(np.array_equal(a[k], c[k]) for k in ('tp', 'fp', 'fn')) and np.array_equal(a['iou'].view(np.int64),
                                                                                          c['iou'].view(np.int64))


def test_the_scene_holds_what_it_is_built_for(scene):
    ps, pi, gs, gi, ptr = scene
    assert len(ptr) == 4 and all(2500 <= n <= 3500 for n in np.diff(ptr))
    out = R.panoptic_ref(*scene, C, THINGS, 50)
    full = lambda c: out['tp'][c] >= 1 and out['fp'][c] >= 1 and out['fn'][c] >= 1
    assert any(full(c) for c in THINGS) and any(full(c) for c in range(C) if c not in THINGS), out
    ga, pa, it, gm, pm = R.segments(*scene, C, THINGS)
    unmatched = [n for g, n in ga.items() if g not in gm] + [n for p, n in pa.items() if p not in pm]
    assert 49 in unmatched and 50 in unmatched
    halves = [(g, p) for (g, p), n in it.items() if 2 * n == ga[g] + pa[p] - n]
    assert any(g[0] in THINGS for g, _ in halves) and any(g[0] not in THINGS for g, _ in halves)
    assert not any(g in gm or p in pm for g, p in halves)          # exactly 1/2 is no match (nor does either match elsewhere)
    small = R.panoptic_ref(*scene, C, THINGS, 1)                   # the threshold moves the misses only
    assert np.array_equal(small['tp'], out['tp']) and (small['fp'] > out['fp']).any() and (small['fn'] > out['fn']).any()
    assert np.array_equal(small['iou'].view(np.int64), out['iou'].view(np.int64))


def test_two_calls_accumulate(scene):
    other = R.random_case(4)
    first = R.panoptic_ref(*scene, C, THINGS, 50)
    both = R.panoptic_ref(*other, C, THINGS, 50, acc=first)
    fresh = R.panoptic_ref(*other, C, THINGS, 50)
    for k in ('tp', 'fp', 'fn'):
        assert np.array_equal(both[k], first[k] + fresh[k])
    assert np.array_equal(both['iou'].view(np.int64), (first['iou'] + fresh['iou']).view(np.int64))
    assert R.same(both, R.panoptic_brute(*other, C, THINGS, 50, acc=first))


def test_a_row_permutation_changes_nothing(scene):
    ptr = scene[4]
    want = R.panoptic_ref(*scene, C, THINGS, 50)
    cols = R.permuted(scene[:4], ptr, 5)
    assert not np.array_equal(cols[2], scene[2])
    assert R.same(R.panoptic_ref(*cols, ptr, C, THINGS, 50), want)
    assert R.same(R.panoptic_brute(*cols, ptr, C, THINGS, 50), want)


def _stats(tp, fp, fn, iou, status=0):
    from lidal_amd.evaluate import PanopticStats
    st = PanopticStats(len(tp), 'cpu')
    st.tp, st.fp, st.fn = (torch.tensor(v, dtype=torch.int64) for v in (tp, fp, fn))
    st.iou = torch.tensor(iou, dtype=torch.float64)
    st.status = torch.tensor([status], dtype=torch.int64)
    return st


def test_panoptic_quality_arithmetic():
    from lidal_amd.evaluate import panoptic_quality
    # class 0: a thing with matches; 1: a thing, absent; 2: stuff with tp = 0; 3: stuff, perfect
    q = panoptic_quality(_stats([3, 0, 0, 2], [1, 0, 2, 0], [2, 0, 1, 0], [2.25, 0.0, 0.0, 2.0]), things=(0, 1))
    assert q['present'].tolist() == [True, False, True, True]
    assert q['sq'].tolist() == [0.75, 0.0, 0.0, 1.0]
    assert q['rq'].tolist() == [3 / 4.5, 0.0, 0.0, 1.0]
    assert q['pq'].tolist() == [0.75 * (3 / 4.5), 0.0, 0.0, 1.0]
    assert q['PQ'] == float(np.mean(q['pq'])) and q['SQ'] == 1.75 / 4 and q['RQ'] == float(np.mean(q['rq']))
    assert q['PQ_th'] == q['pq'][0] / 2 and q['PQ_st'] == 0.5 and q['SQ_th'] == 0.375 and q['RQ_st'] == 0.5
    only = panoptic_quality(_stats([1], [0], [0], [0.625]), things=(0,))
    assert only['PQ'] == only['PQ_th'] == 0.625 and np.isnan(only['PQ_st'])
    with pytest.raises(ValueError, match='outside'):
        panoptic_quality(_stats([1], [0], [0], [1.0], status=1), things=(0,))
    with pytest.raises(ValueError):
        panoptic_quality(_stats([1], [0], [0], [1.0]), things=(1,))


def test_instance_ids_and_the_thing_classes():
    from lidal_amd import data
    words = np.array([0x0000000A, 0x0001000A, 0xFFFF001E, 0x8000FFFF, 0x7FFF0000], dtype=np.uint32)
    want = [0, 1, 65535, 32768, 32767]
    for raw in (words, words.view(np.int32), torch.from_numpy(words.view(np.int32))):
        got = data.instance_ids(raw)
        assert got.dtype == torch.int32 and got.tolist() == want
    if hasattr(torch, 'uint32'):
        assert data.instance_ids(torch.from_numpy(words.view(np.int32)).view(torch.uint32)).tolist() == want
    with pytest.raises(TypeError):
        data.instance_ids(words.astype(np.int64))
    assert data.SK_THINGS == (0, 1, 2, 3, 4, 5, 6, 7)
    assert [data._SK_CLASS_IDS[c] for c in data.SK_THINGS] == [10, 11, 15, 18, 20, 30, 31, 32]
    assert all(data._SK_MOVING[m] in data._SK_THING_IDS + (13, 16) for m in data._SK_MOVING)   # only things move


def test_refusals_before_the_device_is_touched():
    """Every one of these raises ValueError although nothing here is on a GPU: the checks come first."""
    from lidal_amd.evaluate import PanopticStats, panoptic_accumulate
    st = PanopticStats(8, 'cpu')
    sem, inst = torch.zeros(10, dtype=torch.int64), torch.zeros(10, dtype=torch.int32)
    with pytest.raises(ValueError, match='n_classes'):
        PanopticStats(65, 'cpu')
    with pytest.raises(ValueError, match='n_classes'):
        PanopticStats(0, 'cpu')
    wide = PanopticStats(8, 'cpu')
    wide.n_classes = 65
    with pytest.raises(ValueError, match='classes'):
        panoptic_accumulate(wide, sem, inst, sem, inst, things=(0,))
    with pytest.raises(ValueError, match='thing class'):
        panoptic_accumulate(st, sem, inst, sem, inst, things=(8,))
    with pytest.raises(ValueError, match='thing class'):
        panoptic_accumulate(st, sem, inst, sem, inst, things=(-1,))
    for bad in (0, -3, 1.5):
        with pytest.raises(ValueError, match='min_points'):
            panoptic_accumulate(st, sem, inst, sem, inst, things=(0,), min_points=bad)
    with pytest.raises(ValueError, match='same lengths'):
        panoptic_accumulate(st, sem, inst[:9], sem, inst, things=(0,))
    with pytest.raises(ValueError, match='same lengths'):
        panoptic_accumulate(st, [sem[:4], sem[4:]], [inst[:5], inst[5:]], [sem[:4], sem[4:]], [inst[:4], inst[4:]], things=(0,))
    with pytest.raises(ValueError, match='same lengths'):
        panoptic_accumulate(st, [sem], [inst], [sem[:5], sem[5:]], [inst], things=(0,))
    with pytest.raises(ValueError, match='scans'):
        panoptic_accumulate(st, [sem[:0]] * 33, [inst[:0]] * 33, [sem[:0]] * 33, [inst[:0]] * 33, things=(0,))
    with pytest.raises(ValueError, match='integer tensor'):
        panoptic_accumulate(st, sem.float(), inst, sem, inst, things=(0,))
    assert int(st.tp.sum()) == 0
    with pytest.raises(RuntimeError):                              # ... and what passes them all wants a GPU: no fallback
        panoptic_accumulate(st, sem, inst, sem, inst, things=(0,))


def test_header_signatures_and_refusals_of_the_entry_point():
    """The two symbols are declared, exported and in the ctypes table with the header's argument counts; the library
    refuses a bad c, n_scans, min_points, point_ptr, thing mask or workspace before any launch, and p = 0 is a no-op."""
    from lidal_amd import backend as B
    header = open(os.path.join(ROOT, 'include', 'lidal_amd.h')).read()
    for name, n_args in (('lidal_panoptic_accumulate_workspace_bytes', 2), ('lidal_panoptic_accumulate', 18)):
        m = re.search(r'\b(?:int|int64_t)\s+%s\s*\(([^)]*)\)\s*;' % name, header)
        assert m and len(m.group(1).split(',')) == n_args == len(B.SIGNATURES[name][1]), name
    assert re.search(r'LIDAL_PANOPTIC_BAD_ID = 1\b', header)
    L = B.lib()
    nbytes = L.lidal_panoptic_accumulate_workspace_bytes(100, 2)
    assert nbytes > 0 and L.lidal_panoptic_accumulate_workspace_bytes(200000, 2) > nbytes
    ptr = (ctypes.c_int64 * 3)(0, 40, 100)
    P = ctypes.addressof(ptr)

    def call(p=100, point_ptr=P, n=2, c=8, things=0xF, mp=50, ws=nbytes):
        return L.lidal_panoptic_accumulate(None, None, None, None, p, point_ptr, n, c, things, mp, None, None, None, None,
                                           None, None, ws, None)

    for kw, word in ((dict(c=0), b'classes'), (dict(c=65), b'classes'), (dict(n=0), b'scans'), (dict(n=33), b'scans'),
                     (dict(mp=0), b'min_points'), (dict(point_ptr=None), b'point_ptr'), (dict(p=99), b'end at'),
                     (dict(things=1 << 8), b'thing class'), (dict(ws=nbytes - 1), b'workspace'),
                     (dict(), b'null array')):
        assert call(**kw) == 2 and word in L.lidal_last_error(), (kw, L.lidal_last_error())
    down = (ctypes.c_int64 * 3)(0, 60, 40)
    assert call(p=40, point_ptr=ctypes.addressof(down)) == 2 and b'ascend' in L.lidal_last_error()
    empty = (ctypes.c_int64 * 3)(0, 0, 0)
    assert call(p=0, point_ptr=ctypes.addressof(empty), things=(1 << 64) - 1, c=64) == 0     # nothing to launch
