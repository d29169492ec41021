"""Labels and predictions carried across registered frames (lidal_amd/score/transfer.py, csrc/transfer.hip; DESIGN.md
section 21) against a numpy restatement that lives here: a brute-force nearest neighbour in f64, the vote rules and the
fused probability row, all to exact equality."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
C = 19
IGN = 255
STATS = ('own', 'none', 'weak', 'gated', 'confirmed', 'contradicted', 'invalid')


def _g(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- the restatement ----------------------------------------------------------------------------------------------------
def ref_match_one(q, pts, r):
    """Nearest point of pts to every row of q: d2 = ((ex^2 + ey^2) + ez^2) in f64, first minimum, sqrt(d2) <= r, else -1.
    A query that is not finite, or whose cube [q - r, q + r]^3 leaves the 2^20 - 1 cells (of 2 r) either side of the
    origin, matches nothing (include/lidal_amd.h at lidal_nn_grid_build)."""
    out = np.full(q.shape[0], -1, np.int32)
    if pts.shape[0] == 0:
        return out
    px, py, pz = (np.ascontiguousarray(pts[:, k])[None, :] for k in range(3))       # (finite: the tests' neighbours are)
    for a in range(0, q.shape[0], 128):
        qq = q[a:a + 128]
        with np.errstate(invalid='ignore', over='ignore'):
            d2 = np.square(px - qq[:, 0:1])
            d2 += np.square(py - qq[:, 1:2])
            d2 += np.square(pz - qq[:, 2:3])                                        # ((ex^2 + ey^2) + ez^2)
        j = d2.argmin(1)
        best = d2[np.arange(len(qq)), j]
        with np.errstate(invalid='ignore'):
            inside = ((np.floor((qq - r) / (2 * r)) >= -(2 ** 20 - 1)) & (np.floor((qq + r) / (2 * r)) <= 2 ** 20 - 1)).all(1)
        ok = np.isfinite(qq).all(1) & inside & np.isfinite(best)
        ok[ok] &= np.sqrt(best[ok]) <= r
        out[a:a + 128] = np.where(ok, j, -1)
    return out


def ref_match(q, neis, r):
    return np.stack([ref_match_one(q, n, r) for n in neis]) if neis else np.zeros((0, q.shape[0]), np.int32)


def ref_transfer(match, nei_labels, c, q_labels=None, gate=None, ignore=IGN, min_votes=1, min_agree=1.0):
    """(out, votes, agree, stats) by the rules of include/lidal_amd.h."""
    p = match.shape[1]
    hist = np.zeros((p, c), np.int64)
    invalid = 0
    rows = np.arange(p)
    for n, lab in enumerate(nei_labels):
        if lab is None:
            continue
        ok = match[n] >= 0
        l = np.full(p, ignore, np.int64)
        l[ok] = lab[match[n][ok]]
        ok &= l != ignore
        bad = ok & ((l < 0) | (l >= c))
        invalid += int(bad.sum())
        ok &= ~bad
        np.add.at(hist, (rows[ok], l[ok]), 1)
    winner = hist.argmax(1)                      # the first maximum
    agree = hist.max(1)
    nv = hist.sum(1)
    none = nv == 0
    weak = ~none & ((nv < min_votes) | (agree.astype(np.float64) < min_agree * nv.astype(np.float64)))
    gated = ~none & ~weak & (gate != winner if gate is not None else np.zeros(p, bool))
    passes = ~none & ~weak & ~gated
    own = (q_labels != ignore) if q_labels is not None else np.zeros(p, bool)
    out = np.where(passes, winner, ignore).astype(np.int64)
    if q_labels is not None:
        out = np.where(own, q_labels, out)
    stats = np.zeros(c + 7, np.int64)
    stats[:c] = np.bincount(winner[passes & ~own], minlength=c)
    stats[c + 0] = own.sum()
    stats[c + 1] = (~own & none).sum()
    stats[c + 2] = (~own & weak).sum()
    stats[c + 3] = (~own & gated).sum()
    if q_labels is not None:
        stats[c + 4] = (own & passes & (winner == q_labels)).sum()
        stats[c + 5] = (own & passes & (winner != q_labels)).sum()
    stats[c + 6] = invalid
    return out, nv.astype(np.int32), agree.astype(np.int32), stats


def ref_fuse(match, q_prob, nei_prob):
    """f32 adds in neighbour order, f64 divide, f32 store; first maximum."""
    s = q_prob.astype(np.float32).copy()
    cnt = np.zeros(s.shape[0], np.int32)
    for n, pr in enumerate(nei_prob):
        ok = match[n] >= 0
        s[ok] = (s[ok] + pr[match[n][ok]]).astype(np.float32)
        cnt += ok
    fused = (s.astype(np.float64) / (cnt + 1).astype(np.float64)[:, None]).astype(np.float32)
    pred = fused.argmax(1).astype(np.int64)
    return fused, pred, fused[np.arange(len(pred)), pred], cnt


def np_entropy(pk):
    pk = pk.astype(np.float64)
    pk = pk / pk.sum(1, keepdims=True)
    with np.errstate(divide='ignore', invalid='ignore'):
        return -np.where(pk > 0, pk * np.log(pk), 0.0).sum(1)


# ---- the sequence of the issue: 9 frames, window 4, 6 of 20 supervoxels annotated per frame ---------------------------------
WINDOW, RADIUS, QUERY_FRAMES = 4, 0.1, (0, 4, 8)


def _cell_class(world):
    cell = np.floor(world / 2.0).astype(np.int64)
    return (7 * cell[:, 0] + 13 * cell[:, 1] + 5 * cell[:, 2]) % 19


@pytest.fixture(scope='module')
def seq():
    from lidal_amd import synth
    from lidal_amd.score import FrameBank, neighbour_ids
    frames = synth.make_sequence(9, n_points=None, seed=3, step=0.8, n_beams=24, n_az=256)
    rng = np.random.default_rng(0)
    worlds, labels, truth, probs = [], [], [], []
    prng = np.random.default_rng(11)
    for f in frames:
        w = f['world']
        cls = _cell_class(w)
        lab = np.full(w.shape[0], IGN, np.int64)
        for s in rng.choice(20, 6, replace=False):
            lab[f['sv2point'][s]] = cls[f['sv2point'][s]]
        lg = prng.standard_normal((w.shape[0], C)) + np.sin(w[:, :1] * 0.7) * 2
        e = np.exp(lg - lg.max(1, keepdims=True))
        worlds.append(w); labels.append(lab); truth.append(cls)
        probs.append((e / e.sum(1, keepdims=True)).astype(np.float32))
    assert all(6000 < w.shape[0] < 6150 for w in worlds)
    bank = FrameBank(RADIUS)
    for w, p in zip(worlds, probs):
        bank.add(_g(w), _g(p))
    nei = {i: neighbour_ids(i, 9, WINDOW) for i in QUERY_FRAMES}
    assert nei[0] == [3, 4, 1, 2]
    match = {i: ref_match(worlds[i], [worlds[n] for n in nei[i]], RADIUS) for i in QUERY_FRAMES}
    return {'worlds': worlds, 'labels': labels, 'truth': truth, 'probs': probs, 'bank': bank, 'nei': nei, 'match': match,
            'dev_labels': {f: _g(l) for f, l in enumerate(labels)}}


def test_match_table_equals_the_brute_force_search(seq):
    from lidal_amd.score import match_points
    from lidal_amd.score.interframe import score_points
    for i in QUERY_FRAMES:
        got = match_points(seq['bank'], i, nei_num=WINDOW)
        assert got.dtype == torch.int32 and tuple(got.shape) == (WINDOW, seq['worlds'][i].shape[0])
        assert np.array_equal(got.cpu().numpy(), seq['match'][i]), i
        assert torch.equal(match_points(seq['bank'], i, frames=seq['nei'][i]), got)
        _, _, cnt = score_points(seq['bank'], i, WINDOW)
        assert torch.equal((got >= 0).sum(0).to(torch.int32), cnt)
        assert int((got >= 0).sum()) > 1000


@pytest.mark.parametrize('min_votes,min_agree', [(1, 1.0), (2, 0.6), (1, 2 / 3)])
def test_annotation_group_equals_the_restatement_on_the_sequence(seq, min_votes, min_agree):
    from lidal_amd.score import transfer_labels
    for i in QUERY_FRAMES:
        match = seq['match'][i]
        nei_labels = [seq['labels'][n] for n in seq['nei'][i]]
        gate = seq['truth'][i].copy()
        gate[::7] = (gate[::7] + 1) % 19
        dmatch = _g(match)
        for use_gate in (False, True):
            for use_own in (True, False):
                labels = {f: l for f, l in seq['dev_labels'].items() if use_own or f != i}
                want = ref_transfer(match, nei_labels, C, seq['labels'][i] if use_own else None,
                                    gate if use_gate else None, IGN, min_votes, min_agree)
                for m in (None, dmatch):
                    out, stats, votes, agree = transfer_labels(seq['bank'], i, labels, C, nei_num=WINDOW,
                                                               min_votes=min_votes, min_agree=min_agree,
                                                               gate=_g(gate) if use_gate else None, match=m,
                                                               return_votes=True)
                    got = [t.cpu().numpy() for t in (out, votes, agree, stats)]
                    for name, a, b in zip(('out', 'votes', 'agree', 'stats'), got, want):
                        assert a.dtype == b.dtype and np.array_equal(a, b), (i, use_gate, use_own, name)
        # the rules really fire on this sequence (the restatement alone, counted when the issue was written:
        # 1037 / 1356 / 1310 unannotated points with votes, 140 / 211 / 391 with two or more, 5 / 8 / 41 split)
        st = ref_transfer(match, nei_labels, C, seq['labels'][i])[3]
        assert st[C + 4] > 0 and st[C + 5] > 0                   # confirmed and contradicted both occur
        _, nv, ag, _ = ref_transfer(match, nei_labels, C)
        free = seq['labels'][i] == IGN
        print('frame', i, 'voted', int((nv[free] > 0).sum()), 'twice', int((nv[free] >= 2).sum()), 'split',
              int((ag[free] < nv[free]).sum()))
        assert (nv[free] > 0).sum() >= 1000 and (nv[free] >= 2).sum() >= 100 and (ag[free] < nv[free]).sum() >= 1


# ---- the entry point itself, between guard bands --------------------------------------------------------------------------
GUARD = 256


class Guarded:
    """Device buffers of exactly the documented sizes, each between two bands of 0xA5 (and filled with 0xA5: garbage)."""

    def __init__(self):
        self.bufs = []

    def new(self, shape, dtype):
        n = int(np.prod(shape)) * dtype.itemsize
        pad = (-n) % 8
        raw = torch.full((GUARD + n + pad + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
        self.bufs.append((raw, n))
        return raw[GUARD:GUARD + n].view(dtype).view(shape)

    def check(self):
        for raw, n in self.bufs:
            assert bool((raw[:GUARD] == 0xA5).all()) and bool((raw[GUARD + n:] == 0xA5).all())


def lib_transfer(match, nei_p, c, nei_labels=None, q_labels=None, gate=None, ignore=IGN, min_votes=1, min_agree=1.0,
                 q_prob=None, nei_prob=None, annotate=True):
    """lidal_interframe_transfer on a given match table (numpy in, numpy out), every output guarded."""
    from lidal_amd import backend as B
    n, p = match.shape
    g = Guarded()
    keep = [_g(match.astype(np.int32))]
    ptr = lambda a: None if a is None else (keep.append(_g(a)) or keep[-1].data_ptr())
    n_arr = (ctypes.c_int64 * n)(*[int(v) for v in nei_p])
    res = {}
    args = [keep[0].data_ptr(), p, c, n, n_arr]
    if annotate:
        l_arr = (ctypes.c_void_p * n)(*[ptr(l) for l in nei_labels])
        outs = [g.new((p,), torch.int64), g.new((p,), torch.int32), g.new((p,), torch.int32), g.new((c + 7,), torch.int64)]
        args += [l_arr, ptr(q_labels), ptr(gate), ignore, min_votes, min_agree] + [o.data_ptr() for o in outs]
        res.update(zip(('out', 'votes', 'agree', 'stats'), outs))
    else:
        args += [None, None, None, ignore, min_votes, min_agree, None, None, None, None]
    if q_prob is not None:
        f_arr = (ctypes.c_void_p * n)(*[ptr(f) for f in nei_prob])
        outs = [g.new((p, c), torch.float32), g.new((p,), torch.int64), g.new((p,), torch.float32), g.new((p,), torch.int32)]
        args += [ptr(q_prob), f_arr] + [o.data_ptr() for o in outs]
        res.update(zip(('prob', 'pred', 'conf', 'count'), outs))
    else:
        args += [None] * 6
    B.check(B.lib().lidal_interframe_transfer(*args, B.stream()), 'interframe_transfer')
    torch.cuda.synchronize()
    g.check()
    return {k: v.cpu().numpy() for k, v in res.items()}


def _same(got, want, names):
    for name, b in zip(names, want):
        assert got[name].dtype == b.dtype and np.array_equal(got[name], b), name


ANN = ('out', 'votes', 'agree', 'stats')
FUSED = ('prob', 'pred', 'conf', 'count')


def test_vote_rules_at_their_edges():
    c = 5
    # one neighbour point per vote: neighbour n has one point, labelled as the column says
    def run(cols, **kw):
        match = np.array([[0 if v is not None else -1] for v in cols], np.int32).reshape(len(cols), 1)
        labs = [np.array([v if v is not None else 0], np.int64) for v in cols]
        got = lib_transfer(match, [1] * len(cols), c, labs, **kw)
        _same(got, ref_transfer(match, labs, c, **{k: v for k, v in kw.items()}), ANN)
        return got
    got = run([3, 1, 1, 3])                                  # a two-class tie goes to the lower class ...
    assert got['agree'][0] == 2 and got['votes'][0] == 4 and got['out'][0] == IGN and got['stats'][c + 2] == 1
    got = run([3, 1, 1, 3], min_agree=0.5)                   # ... and is taken when half is enough
    assert got['out'][0] == 1 and got['stats'][1] == 1
    got = run([2, 4, 2], min_agree=2 / 3)                    # 2 of 3 at 2/3: the same double product decides
    assert got['out'][0] == (2 if not 2.0 < (2 / 3) * 3.0 else IGN) and got['votes'][0] == 3
    got = run([2, 4, 2], min_agree=0.67)
    assert got['out'][0] == IGN and got['stats'][c + 2] == 1
    got = run([IGN, 2])                                      # an ignored neighbour label is no vote
    assert got['votes'][0] == 1 and got['out'][0] == 2 and got['stats'][c + 6] == 0
    got = run([-1, c, 300, 2])                               # labels outside [0, c): skipped and counted
    assert got['votes'][0] == 1 and got['out'][0] == 2 and got['stats'][c + 6] == 3
    got = run([-1, c, 300])
    assert got['votes'][0] == 0 and got['out'][0] == IGN and got['stats'][c + 1] == 1 and got['stats'][c + 6] == 3
    got = run([2, 2], min_votes=3)
    assert got['out'][0] == IGN and got['stats'][c + 2] == 1
    got = run([2, 2], gate=np.array([1], np.int64))          # the gate
    assert got['out'][0] == IGN and got['stats'][c + 3] == 1
    got = run([2, 2], gate=np.array([2], np.int64))
    assert got['out'][0] == 2
    got = run([2, 2], q_labels=np.array([4], np.int64))      # own label wins, and the vote is measured against it
    assert got['out'][0] == 4 and got['stats'][c + 0] == 1 and got['stats'][c + 5] == 1 and got['stats'][2] == 0
    got = run([2, 2], q_labels=np.array([2], np.int64))
    assert got['out'][0] == 2 and got['stats'][c + 4] == 1
    got = run([2, None], q_labels=np.array([IGN], np.int64))
    assert got['out'][0] == 2 and got['stats'][c + 0] == 0
    # confirmed and contradicted in one call
    match = np.zeros((2, 2), np.int32)
    labs = [np.array([2], np.int64)] * 2
    own = np.array([2, 4], np.int64)
    got = lib_transfer(match, [1, 1], c, labs, q_labels=own)
    _same(got, ref_transfer(match, labs, c, own), ANN)
    assert got['stats'].tolist() == [0] * c + [2, 0, 0, 0, 1, 1, 0]
    # a NULL label pointer votes nothing; an entry past the neighbour's size is no match
    match = np.array([[0], [0], [7]], np.int32)
    got = lib_transfer(match, [1, 1, 1], c, [None, np.array([3], np.int64), np.array([1], np.int64)])
    assert got['votes'][0] == 1 and got['out'][0] == 3


@pytest.mark.parametrize('p', [1, 255, 256, 257])
@pytest.mark.parametrize('c', [1, 19, 32])
def test_both_groups_on_random_tables_at_block_edges(p, c):
    rng = np.random.default_rng(p * 100 + c)
    n = 5
    nei_p = [40, 0, 17, 300, 1]
    match = np.stack([np.where(rng.random(p) < 0.6, rng.integers(0, max(q, 1), p), -1) if q else np.full(p, -1)
                      for q in nei_p]).astype(np.int32)
    pool = np.array(list(range(c)) * 4 + [IGN, IGN, -1, c, 300], np.int64)
    labs = [rng.choice(pool, max(q, 1)) for q in nei_p]
    own = np.where(rng.random(p) < 0.3, rng.integers(0, c, p), IGN).astype(np.int64)
    gate = rng.integers(0, c, p).astype(np.int64)

    def rows(q):
        x = rng.random((max(q, 1), c)).astype(np.float32)
        return x / x.sum(1, keepdims=True, dtype=np.float32)
    q_prob, nei_prob = rows(p), [rows(q) for q in nei_p]
    for kw in ({}, {'q_labels': own, 'min_agree': 0.5}, {'q_labels': own, 'gate': gate, 'min_votes': 2, 'min_agree': 0.6}):
        got = lib_transfer(match, nei_p, c, labs, q_prob=q_prob, nei_prob=nei_prob, **kw)
        _same(got, ref_transfer(match, labs, c, **kw), ANN)
        _same(got, ref_fuse(match, q_prob, nei_prob), FUSED)
    alone = lib_transfer(match, nei_p, c, q_prob=q_prob, nei_prob=nei_prob, annotate=False)
    _same(alone, ref_fuse(match, q_prob, nei_prob), FUSED)
    assert ref_transfer(match, labs, c)[3][c + 6] > 0 or p == 1


def test_geometry_edges_empty_neighbour_no_neighbour_nan_and_far_queries():
    from lidal_amd.score import FrameBank, fuse_predictions, match_points, transfer_labels
    rng = np.random.default_rng(5)
    base = rng.uniform(-20, 20, (300, 3))
    far = 0.2 * 2.0 ** 21 + 3.0                               # 2^21 cells of 0.2 m out
    q = base.copy()
    q[7] = [np.nan, 1.0, 2.0]
    q[8] = [far, 0.0, 0.0]
    q[9] = [np.inf, 0.0, 0.0]
    nb = base + rng.uniform(-0.03, 0.03, base.shape)
    nb[8] = [far, 0.0, 0.0]                                   # the same far place: still no match
    worlds = [q, nb, np.zeros((0, 3)), nb[::-1].copy()]
    c = 4
    probs = [rng.random((w.shape[0], c)).astype(np.float32) for w in worlds]
    bank = FrameBank(RADIUS)
    for w, pr in zip(worlds, probs):
        bank.add(_g(w), _g(pr))
    frames = [1, 2, 3]
    want = ref_match(q, [worlds[f] for f in frames], RADIUS)
    got = match_points(bank, 0, frames=frames)
    assert np.array_equal(got.cpu().numpy(), want)
    assert (want[1] == -1).all() and (want[:, 7:10] == -1).all() and (want[0] >= 0).sum() >= 290
    labs = {f: rng.integers(0, c, worlds[f].shape[0]) for f in frames}
    out, stats, votes, agree = transfer_labels(bank, 0, {f: _g(l) for f, l in labs.items()}, c, frames=frames,
                                               return_votes=True)
    ref = ref_transfer(want, [labs[f] for f in frames], c)
    for a, b in zip((out, votes, agree, stats), ref):
        assert np.array_equal(a.cpu().numpy(), b)
    assert (ref[0][7:10] == IGN).all()
    fused = fuse_predictions(bank, 0, frames=frames, match=got)
    for a, b in zip(fused, ref_fuse(want, probs[0], [probs[f] for f in frames])):
        assert np.array_equal(a.cpu().numpy(), b)
    # no neighbour at all: nobody votes, the fused row is the point's own
    m0 = match_points(bank, 0, frames=[])
    assert tuple(m0.shape) == (0, 300)
    out, stats = transfer_labels(bank, 0, {}, c, frames=[])
    assert bool((out == IGN).all()) and stats.tolist() == [0] * c + [0, 300, 0, 0, 0, 0, 0]
    prob, pred, conf, count = fuse_predictions(bank, 0, frames=[])
    assert torch.equal(prob, bank.prob[0]) and int(count.sum()) == 0
    assert torch.equal(pred, bank.prob[0].argmax(1)) and torch.equal(conf, bank.prob[0].max(1).values)
    # geometry alone is enough to carry labels; scoring it is refused
    bare = FrameBank(RADIUS)
    for w in worlds:
        bare.add(_g(w))
    assert torch.equal(match_points(bare, 0, frames=frames), got)
    with pytest.raises(ValueError, match='without probabilities'):
        fuse_predictions(bare, 0, frames=frames)
    from lidal_amd.score.interframe import score_points
    with pytest.raises(ValueError, match='without probabilities'):
        score_points(bare, 0, 2)


def test_prediction_group_equals_the_restatement_and_the_scorers_entropy(seq):
    from lidal_amd.score import fuse_predictions
    from lidal_amd.score.interframe import score_points
    for i in QUERY_FRAMES:
        prob, pred, conf, count = fuse_predictions(seq['bank'], i, nei_num=WINDOW)
        want = ref_fuse(seq['match'][i], seq['probs'][i], [seq['probs'][n] for n in seq['nei'][i]])
        for name, a, b in zip(FUSED, (prob, pred, conf, count), want):
            a = a.cpu().numpy()
            assert a.dtype == b.dtype and np.array_equal(a, b), (i, name)
        assert (want[3] >= 2).sum() > 100
        _, intere, cnt = score_points(seq['bank'], i, WINDOW)
        assert torch.equal(cnt, count)
        ent = np_entropy(want[0])
        assert np.abs(intere.cpu().numpy() - ent).max() <= 1e-4 * np.abs(ent).max()


def test_fused_pred_is_the_first_maximum_of_an_exact_tie():
    c = 6
    q_prob = np.array([[0.125, 0.25, 0.25, 0.125, 0.125, 0.125],          # point 0, unmatched: a tie in the row itself
                       [0.5, 0.125, 0.125, 0.125, 0.0625, 0.0625]], np.float32)
    # point 1, matched twice: 0.5 + 0 + 0.125 == 0.125 + 0.125 + 0.375 == 0.125 + 0.5 + 0, exact in every width
    nei_a = np.array([[0.0, 0.125, 0.5, 0.125, 0.125, 0.125]], np.float32)
    nei_b = np.array([[0.125, 0.375, 0.0, 0.25, 0.125, 0.125]], np.float32)
    match = np.array([[-1, 0], [-1, 0]], np.int32)
    got = lib_transfer(match, [1, 1], c, q_prob=q_prob, nei_prob=[nei_a, nei_b], annotate=False)
    _same(got, ref_fuse(match, q_prob, [nei_a, nei_b]), FUSED)
    assert got['pred'][0] == 1 and got['prob'][0][1] == got['prob'][0][2] and got['count'][0] == 0
    assert got['prob'][1][0] == got['prob'][1][1] == got['prob'][1][2] and got['pred'][1] == 0 and got['count'][1] == 2


def test_one_hop_whatever_the_order_of_the_frames(seq):
    from lidal_amd.score import match_points, transfer_sequence
    bank, given = seq['bank'], seq['dev_labels']
    up, stats_up = transfer_sequence(bank, given, C, nei_num=WINDOW, min_agree=0.6)
    down, stats_down = transfer_sequence(bank, given, C, order=list(range(8, -1, -1)), nei_num=WINDOW, min_agree=0.6,
                                         summary=True)
    assert sorted(up) == sorted(down) == list(range(9))
    for f in range(9):
        assert torch.equal(up[f], down[f])
    host = stats_up.tolist()
    assert host[:C] == stats_down['classes'] and host[C:] == [stats_down[k] for k in STATS]
    assert sum(host[:C]) >= 3000 and stats_down['own'] == int(sum((l != IGN).sum() for l in seq['labels']))
    for i in QUERY_FRAMES:
        want = ref_transfer(seq['match'][i], [seq['labels'][n] for n in seq['nei'][i]], C, seq['labels'][i], None, IGN, 1, 0.6)
        assert np.array_equal(up[i].cpu().numpy(), want[0])
    # a label that exists only as an OUTPUT of frame 4 (carried there from frame 3) is not seen by frame 5
    only3 = {3: given[3]}
    out, _ = transfer_sequence(bank, only3, C, nei_num=2)          # window 2: frame 4 reads 3 and 5, frame 5 reads 4 and 6
    carried = out[4] != IGN
    assert int(carried.sum()) > 300
    m54 = match_points(bank, 5, frames=[4])[0]
    reach = (m54 >= 0) & carried[m54.clamp(min=0).long()]
    assert int(reach.sum()) > 50                                    # a second hop would have had labels to take
    assert bool((out[5] == IGN).all())


def test_match_entry_point_writes_exactly_its_table(seq):
    from lidal_amd import backend as B
    bank, i = seq['bank'], 4
    frames = seq['nei'][i]
    p, n = seq['worlds'][i].shape[0], len(frames)
    g = Guarded()
    match = g.new((n, p), torch.int32)
    grids = [bank.grid(f) for f in frames]
    g_arr = (ctypes.c_void_p * n)(*[t.data_ptr() for t in grids])
    p_arr = (ctypes.c_void_p * n)(*[bank.world[f].data_ptr() for f in frames])
    n_arr = (ctypes.c_int64 * n)(*[bank.world[f].shape[0] for f in frames])
    B.check(B.lib().lidal_interframe_match(bank.world[i].data_ptr(), p, g_arr, p_arr, n_arr, n, RADIUS, match.data_ptr(),
                                           B.stream()), 'interframe_match')
    torch.cuda.synchronize()
    g.check()
    assert np.array_equal(match.cpu().numpy(), seq['match'][i])
    # ... and the transfer, on that table, with stats full of garbage before the call (lib_transfer guards every output)
    got = lib_transfer(seq['match'][i], [seq['worlds'][f].shape[0] for f in frames], C, [seq['labels'][f] for f in frames],
                       q_labels=seq['labels'][i], q_prob=seq['probs'][i], nei_prob=[seq['probs'][f] for f in frames])
    _same(got, ref_transfer(seq['match'][i], [seq['labels'][f] for f in frames], C, seq['labels'][i]), ANN)
    _same(got, ref_fuse(seq['match'][i], seq['probs'][i], [seq['probs'][f] for f in frames]), FUSED)


# ---- the data route --------------------------------------------------------------------------------------------------------
def _scans():
    from lidal_amd import data, synth
    from lidal_amd.score.interframe import sv_csr
    world = synth.make_world(5)
    host = [synth.raycast_scan(world, (18.0 + 3 * k, 0.0), np.random.default_rng([23, k]), n_beams=16, n_az=128, n_points=n)
            for k, n in enumerate((500, 700))]
    table = data.sk_label_map()
    ids = np.nonzero(table != 255)[0]
    rng = np.random.default_rng(24)
    raws, csrs, flags, extras = [], [], [], []
    for k, (pts, _) in enumerate(host):
        p = pts.shape[0]
        raw = (rng.choice(ids, p) | (rng.integers(1, 65536, p) << 16)).astype(np.uint32)
        raws.append(_g(raw.view(np.int32)))
        csrs.append(sv_csr(synth.angular_supervoxels(pts, 4), DEV)[:2])
        flags.append(np.array([[1, 0, 0, 1], [0, 1, 0, 0]][k]))
        extras.append(_g(np.where(rng.random(p) < 0.5, rng.integers(0, 19, p), 255).astype(np.int64)))
    return [(_g(p), _g(w)) for p, w in host], raws, table, csrs, flags, extras


def _batches_equal(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        if isinstance(a[k], torch.Tensor):
            assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k


def test_extra_labels_fill_what_train_labels_left_open():
    from lidal_amd import data
    pairs, raws, table, csrs, flags, extras = _scans()
    plain = data.train_batch(pairs, raws, table, csrs, flags, rng=np.random.RandomState(9))
    same = data.train_batch(pairs, raws, table, csrs, flags, rng=np.random.RandomState(9), extra_labels=None)
    _batches_equal(plain, same)
    got = data.train_batch(pairs, raws, table, csrs, flags, rng=np.random.RandomState(9), extra_labels=extras)
    lab = torch.where(plain['labels_p_b'] == 255, torch.cat(extras), plain['labels_p_b'])
    assert int((plain['labels_p_b'] == 255).sum()) > 300 and int((lab != plain['labels_p_b']).sum()) > 100
    assert int((plain['labels_p_b'] != 255).sum()) > 300
    assert torch.equal(got['labels_p_b'], lab) and torch.equal(got['labels_v_b'], lab[plain['unique_idxs_b']])
    for k in ('coords_v_b', 'feats_v_b', 'inverse_indices_b', 'unique_idxs_b'):
        assert torch.equal(got[k], plain[k]), k
    half = data.train_batch(pairs, raws, table, csrs, flags, rng=np.random.RandomState(9), extra_labels=[None, extras[1]])
    lab = torch.where(plain['labels_p_b'] == 255, torch.cat([torch.full_like(extras[0], 255), extras[1]]), plain['labels_p_b'])
    assert torch.equal(half['labels_p_b'], lab)
    # the mixed batch, identity mixes
    mixes = [data.identity_mix(j) for j in range(2)]
    mplain = data.mixed_train_batch(pairs, raws, table, mixes, csrs, flags, rng=np.random.RandomState(9))
    msame = data.mixed_train_batch(pairs, raws, table, mixes, csrs, flags, rng=np.random.RandomState(9), extra_labels=None)
    _batches_equal(mplain, msame)
    mgot = data.mixed_train_batch(pairs, raws, table, mixes, csrs, flags, rng=np.random.RandomState(9), extra_labels=extras)
    mlab = torch.where(mplain['labels_p_b'] == 255, torch.cat(extras), mplain['labels_p_b'])
    assert torch.equal(mgot['labels_p_b'], mlab) and torch.equal(mgot['labels_v_b'], mlab[mplain['unique_idxs_b']])
    assert torch.equal(mgot['labels_v_b'], got['labels_v_b'])
    with pytest.raises(ValueError, match='extra label arrays'):
        data.train_batch(pairs, raws, table, csrs, flags, extra_labels=extras[:1])
    with pytest.raises(ValueError, match='int64'):
        data.train_batch(pairs, raws, table, csrs, flags, extra_labels=[extras[0][:-1], None])
