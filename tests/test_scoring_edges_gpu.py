"""The inter-frame scorer and the small scoring kernels (csrc/score.hip) at their edges, against the plain restatement
tests/interframe_ref.py (brute force, nearest by (d2, index); pinned on the CPU by tests/test_scoring_cpu.py).

map_count, confusion counts, registration and cell-size invariance are exact.  interd and intere are compared PER POINT:
the GPU and scipy evaluate the same f64 expression and differ in the last bit of log, so every f32 term differs by at
most one f32 ulp and both sides sum in the same order -- |delta interd| <= SCORE_ULPS * 2^-24 * (sum over the matched
neighbours of sum_k |term_k|) / max(cnt, 1), |delta intere| <= SCORE_ULPS * 2^-24 * sum_k |entr_k|, the sums taken from the
restatement's own f32 terms.  Every check prints the largest multiple of 2^-24 * (that sum) it saw (pytest -s).
All inputs come from fixed seeds.

What each test is there to catch, as four one-line changes of csrc/score.hip (restated in numpy over these same inputs):
  sqrt(d2) <= dis_thresh -> <     map_count of the lattice at the origin (426 points) and of the margin pairs (12)
  tie j < arg -> j > arg          interd / intere of both lattices and of the coincident neighbours, by > 10^6 x the bound
  rr -> r, no margin on the cube  map_count of the margin pairs at cells of 0.25 and 0.5 radii (12 points), nothing else:
                                  lattices and clouds have e = n - q exact, and then n <= fl(q + r) follows from e <= r
  np_sum_f32 -> sequential sum    intere of the lattices (8.2 x 2^-24 x sum|terms|, the bound is 4), the sequence (7.4) and
                                  the class widths 9 / 19 / 32 (5.1 / 5.9 / 8.5); widths below 8 sum sequentially anyway"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import interframe_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SCORE_ULPS = 4          # as test_redal_edges_gpu.py: the one step not restated is the last bit of log
TRANSLATION = np.array([1234.5, -2345.25, 17.0])
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bank(probs, worlds, dis):
    from lidal_amd.score import FrameBank
    bank = FrameBank(dis)
    for p, w in zip(probs, worlds):
        bank.add(_t(np.asarray(w, np.float64).reshape(-1, 3)), _t(np.asarray(p, np.float32)))
    return bank


def _gpu(probs, worlds, i, nei, dis):
    from lidal_amd.score import interframe
    out = interframe.score_points(_bank(probs, worlds, dis), i, nei)
    torch.cuda.synchronize()
    return out


def _ref(probs, worlds, i, nei, dis):
    from lidal_amd.score import interframe
    return R.score_frame_points(i, probs, worlds, interframe.neighbour_ids(i, len(probs), nei), dis)


def _multiple(delta, unit):
    """max over the points of delta / unit; a point whose unit is 0 must have delta 0."""
    assert np.all(delta[unit == 0] == 0), 'a point without terms must be exact'
    nz = unit > 0
    return float((delta[nz] / unit[nz]).max()) if nz.any() else 0.0


def _check(got, ref, what):
    d, e, n = (t.cpu().numpy() for t in got)
    assert d.dtype == np.float64 and e.dtype == np.float32 and n.dtype == np.int32
    assert np.array_equal(n, ref['map_count']), (what, int((n != ref['map_count']).sum()))
    md = _multiple(np.abs(d - ref['interd']), R.interd_bound(ref, 1))
    me = _multiple(np.abs(e.astype(np.float64) - ref['intere'].astype(np.float64)), R.intere_bound(ref, 1))
    print('%s: points %d, matches %d, interd off by %.3f, intere by %.3f x 2^-24 x sum|terms|'
          % (what, n.size, int(n.sum()), md, me))
    assert md <= SCORE_ULPS, (what, md)
    assert me <= SCORE_ULPS, (what, me)
    return md, me


def _run(probs, worlds, i, nei, dis, what):
    ref = _ref(probs, worlds, i, nei, dis)
    got = _gpu(probs, worlds, i, nei, dis)
    _check(got, ref, what)
    return got, ref


# ------------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def _lattice_frames(translated, c=19):
    """Frame 0: the full lattice; frames 1 and 2: two seeded ~8 % subsets, each in a shuffled order.  neighbour_ids(0, 3, 2)
    is [2, 1]."""
    q, a = R.lattice(seed=0)
    _, b = R.lattice(seed=1)
    rs = np.random.RandomState(5)
    a, b = a[rs.permutation(a.shape[0])], b[rs.permutation(b.shape[0])]
    worlds = [q, a, b]
    if translated:
        worlds = [w + TRANSLATION for w in worlds]
    probs = [R.softmax_rows(rs, w.shape[0], c) for w in worlds]
    return probs, worlds


@functools.lru_cache(maxsize=None)
def _sequence():
    """A ragged synthetic sequence as tests/test_scoring_gpu.py makes it: 13 frames, each thinned by its own fraction."""
    from lidal_amd import synth
    frames = synth.make_sequence(13, n_points=None, seed=3, step=0.8, n_beams=16, n_az=256)
    rng = np.random.default_rng(0)
    probs, worlds = [], []
    for f in frames:
        keep = rng.random(f['world'].shape[0]) < rng.uniform(0.6, 1.0)
        w = f['world'][keep]
        lg = rng.standard_normal((w.shape[0], 19)) + np.sin(w[:, :1] * 0.7) * 2
        p = np.exp(lg - lg.max(1, keepdims=True))
        probs.append((p / p.sum(1, keepdims=True)).astype(np.float32))
        worlds.append(w)
    return probs, worlds


@functools.lru_cache(maxsize=None)
def _sequence_ref(i, nei, dis):
    probs, worlds = _sequence()
    return _ref(probs, worlds, i, nei, dis)


def _cloud_frames(rs, sizes, c, box=0.6, sharp=True):
    """Frames of the given sizes in one small box, so that most points have a neighbour within 0.1 in most frames; rows with
    exact one-hots and exact zeros."""
    worlds = [rs.uniform(0, box, size=(n, 3)) + TRANSLATION for n in sizes]
    probs = []
    for n in sizes:
        p = R.softmax_rows(rs, n, c)
        if sharp and n:
            hot = rs.random_sample(n) < 0.2
            p[hot] = 0.0
            p[hot, rs.randint(0, c, size=int(hot.sum()))] = 1.0
            if c > 1:
                zero = (rs.random_sample(n) < 0.2) & ~hot
                cut = rs.random_sample((n, c)) < 0.4
                cut[np.arange(n), p.argmax(1)] = False
                p = np.where(zero[:, None] & cut, np.float32(0), p)
                p = (p / p.sum(1, keepdims=True)).astype(np.float32)
        probs.append(p)
    return probs, worlds


# ------------------------------------------------------------------------------------------------ 3.1 matches, exactly
@pytest.mark.parametrize('translated', [False, True], ids=['origin', 'kitti_scale'])
def test_lattice_matches_exactly(translated):
    """Pairs at exactly 0.05, 0.1 and sqrt(2) * 0.05, points on cell faces of both 0.1 and 0.2, negative coordinates and
    -0.0; then the same lattice at KITTI-scale world coordinates, its expectation recomputed there."""
    probs, worlds = _lattice_frames(translated)
    got, ref = _run(probs, worlds, 0, 2, 0.1, 'lattice')
    n = got[2].cpu().numpy()
    assert (n == 2).sum() > 5000 and (n == 0).sum() > 10


def test_ragged_sequence_matches_exactly():
    probs, worlds = _sequence()
    matched = 0
    for i in (0, 6, 12):
        got = _gpu(probs, worlds, i, 10, 0.1)
        _check(got, _sequence_ref(i, 10, 0.1), 'sequence frame %d' % i)
        matched += int(got[2].sum())
    assert matched > 1000


# ------------------------------------------------------------------------------------------------ 3.2 cell size, radius
def test_outputs_do_not_depend_on_the_cell_size():
    from lidal_amd.score import FrameBank
    probs_l, worlds_l = _lattice_frames(False)
    probs_s, worlds_s = _sequence()
    saved = FrameBank.CELL
    outs = {}
    try:
        for cell in (0.5, 1.0, 2.0, 3.0, 7.3):
            FrameBank.CELL = cell
            outs[cell] = [_gpu(probs_l, worlds_l, 0, 2, 0.1)] + [_gpu(probs_s, worlds_s, i, 10, 0.1) for i in (0, 6, 12)]
    finally:
        FrameBank.CELL = saved
    for cell, runs in outs.items():
        for a, b in zip(runs, outs[2.0]):
            assert all(torch.equal(u, v) for u, v in zip(a, b)), cell
    assert int(outs[2.0][0][2].sum()) > 10000 and int(outs[2.0][1][2].sum()) > 300


def test_matches_at_the_radius_across_a_cell_face_need_the_margin_of_the_cube():
    """R.margin_pairs: neighbours exactly on the face of cell 1, queries below cell 0 whose fl(q + r) falls one ulp short
    of that face while fl(neighbour - query) == r.  The cube [q - r, q + r] misses the neighbour's cell at cells of
    0.25 and 0.5 radii (tests/test_scoring_cpu.py shows it on the CPU); the probed cube's margin must bring it in.  The
    second half of the queries is one ulp farther and matches nothing."""
    from lidal_amd.score import FrameBank
    rs = np.random.RandomState(6)
    q, nb = R.margin_pairs(0.1, 0.05)
    half = nb.shape[0]
    worlds = [np.concatenate([q, rs.uniform(3, 4, size=(500, 3))])]
    for n in (400, 450):
        w = np.concatenate([nb, rs.uniform(3, 4, size=(n, 3))])
        worlds.append(w[rs.permutation(w.shape[0])])
    probs = [R.softmax_rows(rs, w.shape[0], 19) for w in worlds]
    ref = _ref(probs, worlds, 0, 2, 0.1)
    assert np.all(ref['map_count'][:half] == 2) and np.all(ref['map_count'][half:2 * half] == 0)
    saved = FrameBank.CELL
    outs = {}
    try:
        for cell in (0.25, 0.5, 2.0):
            FrameBank.CELL = cell
            outs[cell] = _gpu(probs, worlds, 0, 2, 0.1)
    finally:
        FrameBank.CELL = saved
    for cell, got in outs.items():
        _check(got, ref, 'margin pairs, cell %g r' % cell)
        assert all(torch.equal(u, v) for u, v in zip(got, outs[2.0])), cell


def test_cell_ordered_queries_give_the_same_outputs():
    """lidal_interframe_score_ordered with the query frame's own grid (interframe.CELL_ORDER): the lattice, a sequence
    frame, frames with empty neighbours and a one-point query, each torch.equal to the scan-order run."""
    from lidal_amd.score import interframe
    rs = np.random.RandomState(14)
    cases = [(_lattice_frames(True), 0, 2), (_sequence(), 6, 10), (_cloud_frames(rs, [400, 0, 300, 350, 0], 7), 2, 4),
             (_cloud_frames(rs, [1, 300, 257], 32), 0, 2)]
    saved = interframe.CELL_ORDER
    try:
        for (probs, worlds), i, nei in cases:
            interframe.CELL_ORDER = False
            plain = _gpu(probs, worlds, i, nei, 0.1)
            interframe.CELL_ORDER = True
            ordered = _gpu(probs, worlds, i, nei, 0.1)
            assert all(torch.equal(u, v) for u, v in zip(plain, ordered)), (i, nei)
            assert plain[2].numel() == 1 or int(plain[2].sum()) > 100
    finally:
        interframe.CELL_ORDER = saved
    _check(ordered, _ref(*cases[-1][0], 0, 2, 0.1), 'cell order, p = 1')


@pytest.mark.parametrize('dis', [0.05, 0.3])
def test_other_radii_match_the_restatement(dis):
    probs, worlds = _lattice_frames(False)
    got, _ = _run(probs, worlds, 0, 2, dis, 'lattice, radius %g' % dis)
    assert int(got[2].sum()) > 1000
    probs, worlds = _sequence()
    _check(_gpu(probs, worlds, 6, 10, dis), _sequence_ref(6, 10, dis), 'sequence, radius %g' % dis)


# ------------------------------------------------------------------------------------------------ 3.3 the tie rule
def test_coincident_neighbours_with_different_rows_lowest_index_wins():
    rs = np.random.RandomState(7)
    base = rs.uniform(0, 1.0, size=(700, 3))
    query = base[:500] + rs.normal(0, 0.03, size=(500, 3))
    frames = [query]
    for _ in range(2):
        w = np.repeat(base, 3, axis=0)                 # every neighbour point three times, bit for bit
        frames.append(w[rs.permutation(w.shape[0])])
    probs = [R.softmax_rows(rs, w.shape[0], 19, scale=3.0) for w in frames]
    got, ref = _run(probs, frames, 0, 2, 0.1, 'coincident')
    assert int(got[2].sum()) > 600
    # the input tells the rule apart from its opposite: the highest index of a tie carries another row
    j = ref['ids'][0]
    m = j >= 0
    w = frames[2]
    last = np.array([np.flatnonzero((w == w[k]).all(1)).max() for k in j[m][:50]])
    assert np.all(last > j[m][:50]) and not np.array_equal(probs[2][last], probs[2][j[m][:50]])


def test_a_block_of_5000_coincident_points_inside_a_cloud():
    """The long in-cell scan: 5000 copies of one point among 3000 others; 64 queries within reach of the block (on both
    sides of the radius), 2000 out of its reach."""
    rs = np.random.RandomState(8)
    centre = np.array([2.0, 2.0, 2.0])
    others = rs.uniform(0, 4, size=(3000, 3))
    others = others[np.linalg.norm(others - centre, axis=1) > 0.5]
    nb = np.concatenate([others, np.repeat(centre[None], 5000, axis=0)])
    nb = nb[rs.permutation(nb.shape[0])]
    far = rs.uniform(0, 4, size=(2000, 3))
    far = far[np.linalg.norm(far - centre, axis=1) > 0.5]
    u = rs.normal(size=(64, 3))
    near = centre + u / np.linalg.norm(u, axis=1, keepdims=True) * rs.uniform(0.02, 0.13, size=(64, 1))
    query = np.concatenate([far, near])
    frames = [query, nb, nb[::-1].copy()]
    probs = [R.softmax_rows(rs, w.shape[0], 19) for w in frames]
    got, ref = _run(probs, frames, 0, 2, 0.1, 'block')
    first = np.flatnonzero((nb == centre).all(1)).min()
    hit = ref['ids'][1][-64:]
    assert 20 < (hit >= 0).sum() < 64 and np.all(hit[hit >= 0] == first)


# ------------------------------------------------------------------------------------------------ 3.4 empty and extreme shapes
def _own_entropy(prob):
    return R.score_points(np.zeros((prob.shape[0], 3)), prob, [], [], 0.1)['intere']


def test_empty_frames():
    rs = np.random.RandomState(9)
    probs, worlds = _cloud_frames(rs, [400, 0, 300, 350, 0], 19)
    # an empty query frame (frame 1 of 5, neighbours [0, 2])
    d, e, n = _gpu(probs, worlds, 1, 2, 0.1)
    assert d.shape == (0,) and e.shape == (0,) and n.shape == (0,)
    # one empty neighbour among full ones: frame 2's neighbours are [1, 0, 3, 4] -- 1 and 4 are empty
    got, _ = _run(probs, worlds, 2, 4, 0.1, 'empty neighbours among full ones')
    assert int(got[2].sum()) > 100
    # all neighbours empty
    probs, worlds = _cloud_frames(rs, [257, 0, 0], 19)
    got, ref = _run(probs, worlds, 0, 2, 0.1, 'all neighbours empty')
    assert int(got[2].abs().sum()) == 0 and float(got[0].abs().sum()) == 0.0
    assert np.array_equal(ref['intere'], _own_entropy(probs[0]))
    # no neighbours at all
    probs, worlds = _cloud_frames(rs, [300, 200, 200], 19)
    got, ref = _run(probs, worlds, 0, 0, 0.1, 'nei_num 0')
    assert int(got[2].abs().sum()) == 0 and float(got[0].abs().sum()) == 0.0
    assert np.array_equal(ref['intere'], _own_entropy(probs[0]))


def test_32_neighbours_on_34_tiny_frames_and_refusals():
    from lidal_amd.score import interframe
    rs = np.random.RandomState(10)
    sizes = [int(s) for s in rs.randint(20, 90, size=36)]
    probs, worlds = _cloud_frames(rs, sizes, 19, box=0.6)
    assert interframe.neighbour_ids(0, 36, 32)[:2] == [17, 18] and interframe.neighbour_ids(35, 36, 32)[-1] == 3
    for i in (0, 17, 35):
        got, _ = _run(probs, worlds, i, 32, 0.1, '32 neighbours, frame %d' % i)
        assert int(got[2].max()) > 16
    bank = _bank(probs, worlds, 0.1)
    with pytest.raises(RuntimeError, match='at most 32 neighbours'):
        interframe.score_points(bank, 17, 34)
    _check(interframe.score_points(bank, 17, 32), _ref(probs, worlds, 17, 32, 0.1), 'after the refusal')
    wide = [R.softmax_rows(rs, n, 33) for n in sizes[:3]]
    bank33 = _bank(wide, worlds[:3], 0.1)
    with pytest.raises(RuntimeError, match=r'classes must be in 1\.\.32'):
        interframe.score_points(bank33, 0, 2)
    _check(interframe.score_points(bank, 0, 32), _ref(probs, worlds, 0, 32, 0.1), 'after the second refusal')


@pytest.mark.parametrize('p', [1, 255, 256, 257])
def test_query_sizes_around_the_block(p):
    rs = np.random.RandomState(100 + p)
    probs, worlds = _cloud_frames(rs, [p, 300, 1, 257, 256], 19, box=0.4)
    got, _ = _run(probs, worlds, 0, 4, 0.1, 'p = %d' % p)
    assert p == 1 or int(got[2].sum()) > p


# ------------------------------------------------------------------------------------------------ 3.5 class widths
@pytest.mark.parametrize('c', [1, 2, 7, 8, 9, 16, 19, 24, 31, 32])
def test_class_widths_with_one_hots_and_zeros(c):
    """np_sum_f32's three branches (n < 8, whole blocks of 8, a remainder); rows with exact one-hots and exact zeros:
    q + eps, and the v > 0 branch of the entropy."""
    rs = np.random.RandomState(200 + c)
    probs, worlds = _cloud_frames(rs, [1500, 1300, 1400, 1200, 1350], c, box=0.6)
    assert any((p == 1).any() for p in probs) and (c == 1 or any((p == 0).any() for p in probs))
    got, _ = _run(probs, worlds, 2, 4, 0.1, 'c = %d' % c)
    assert int(got[2].sum()) > 1500


# ------------------------------------------------------------------------------------------------ 3.6 supervoxel means
def _sv_reduce(interd, intere, world, groups):
    from lidal_amd import backend as B
    from lidal_amd.score import interframe
    ptr, idx, _ = interframe.sv_csr(groups, DEV)
    s = len(groups)
    d, e, w = _t(interd), _t(intere), _t(world)
    sv_d = torch.empty(s, dtype=torch.float32, device=DEV)
    sv_e = torch.empty(s, dtype=torch.float32, device=DEV)
    sv_c = torch.empty((s, 3), dtype=torch.float32, device=DEV)
    B.check(B.lib().lidal_supervoxel_reduce(B.ptr(d), B.ptr(e), B.ptr(w), B.ptr(ptr), B.ptr(idx), s, B.ptr(sv_d),
                                            B.ptr(sv_e), B.ptr(sv_c), B.stream()), 'supervoxel_reduce')
    torch.cuda.synchronize()
    return sv_d.cpu().numpy(), sv_e.cpu().numpy(), sv_c.cpu().numpy()


def _within_ulps(got, want64, ulps):
    want = want64.astype(np.float32)
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) <= ulps * np.spacing(np.abs(want)).astype(np.float64)


def test_supervoxel_means_at_block_edges():
    """Supervoxels of 1, 255, 256, 257, 10000 points and the whole frame, ids repeated and unsorted, one empty: against the
    f64 mean (exactly rounded sums) rounded to f32 within 1 f32 ulp; sv_intere also within ceil(log2 n) + 1 ulps of numpy's
    own f32 mean, the reference's expression."""
    rs = np.random.RandomState(12)
    p = 20000
    interd = rs.gamma(2.0, 0.3, size=p)
    interd[rs.random_sample(p) < 0.3] = 0.0
    intere = rs.uniform(0, 2.9, size=p).astype(np.float32)
    world = rs.uniform(-40, 40, size=(p, 3)) + TRANSLATION
    perm = rs.permutation(p)
    groups = [perm[:1], perm[1:256], perm[256:512], perm[512:769], perm[1000:11000], np.arange(p), np.zeros(0, np.int64),
              rs.randint(0, p, size=3000), np.repeat(perm[:7], 40), np.sort(perm[:300])[::-1].copy()]
    sv_d, sv_e, sv_c = _sv_reduce(interd, intere, world, groups)
    ref_d, ref_e, ref_c = R.supervoxel_means(interd, intere, world, groups)
    empty = np.array([len(g) == 0 for g in groups])
    assert empty.sum() == 1
    for got, want in ((sv_d, ref_d), (sv_e, ref_e), (sv_c, ref_c)):
        assert np.array_equal(np.isnan(got).reshape(len(groups), -1).all(1), empty)
        assert np.array_equal(np.isnan(got), np.isnan(want.astype(np.float32)), equal_nan=True)
        ok = _within_ulps(got[~empty], want[~empty], 1)
        assert ok.all(), np.flatnonzero(~ok.reshape(ok.shape[0], -1).all(1))
    for k, g in enumerate(groups):
        if len(g):
            mean32 = intere[g].mean()
            assert mean32.dtype == np.float32
            ulps = int(np.ceil(np.log2(len(g)))) + 1
            assert abs(float(sv_e[k]) - float(mean32)) <= ulps * float(np.spacing(mean32)), (k, len(g))


# ------------------------------------------------------------------------------------------------ 3.7 view-mean softmax
TINY = 2.0 ** -126      # the smallest normal f32: below it the format has no relative precision


def _softmax_bound(ref):
    """1e-4 of the f64 value.  Only where that is less than an f32 can resolve at all -- a value below 2^-126 / 1e-4, such
    as the exp(-160) of a class 160 below the maximum, which f32 holds as a subnormal or as 0 -- the smallest normal f32
    is allowed on top."""
    return 1e-4 * ref + np.where(ref < TINY / 1e-4, TINY, 0.0)


@pytest.mark.parametrize('p', [1, 255, 257])
@pytest.mark.parametrize('c', [1, 16, 19, 32])
@pytest.mark.parametrize('reps', [1, 2, 8])
def test_view_mean_softmax_edges(reps, c, p):
    """Logits of magnitude +-80, one class at -inf, rows with exactly tied maxima.  Every probability within 1e-4 of its
    f64 value, relatively (_softmax_bound: the smallest normal f32 on top only below 2^-126 / 1e-4, where the format
    ends); pred equal on EVERY row whose two largest reference probabilities differ by more than twice that; on exact
    ties the lowest class."""
    from lidal_amd.score.prob_inference import view_mean_softmax
    rs = np.random.RandomState(1000 * reps + 10 * c + p % 10)
    nv = max(2, p // 2)
    logits = (rs.standard_normal((reps * nv, c)) * rs.choice([1.0, 3.0, 30.0], size=(reps * nv, 1))).astype(np.float32)
    logits = np.clip(logits, -80, 80)
    logits[rs.random_sample(reps * nv) < 0.1] *= 0          # identical logits: every probability 1 / c
    if c > 1:
        logits[::7, rs.randint(0, c)] = 80.0
        logits[3::7, rs.randint(0, c)] = -80.0
        logits[:, c // 2][rs.random_sample(reps * nv) < 0.3] = -np.inf
    inverse = np.concatenate([rs.randint(0, nv, size=p) + v * nv for v in range(reps)]).astype(np.int64)
    tied = np.zeros(p, bool)
    if c >= 16:                                                 # points whose classes 3 and 11 tie for the maximum in every view
        tied[::5] = True
        for v in range(reps):
            rows = np.unique(inverse[v * p:(v + 1) * p][tied])
            logits[rows, 3] = logits[rows, 11] = np.float32(81.0)
        tied = np.array([all(logits[inverse[v * p + k], 3] == 81.0 for v in range(reps)) for k in range(p)])
    prob, pred = view_mean_softmax(_t(logits), _t(inverse), reps)
    torch.cuda.synchronize()
    prob, pred = prob.cpu().numpy(), pred.cpu().numpy()
    ref, ref_pred = R.view_mean_softmax(logits, inverse, reps)
    assert prob.shape == (p, c) and np.isfinite(prob).all() and np.isfinite(ref).all()
    bound = _softmax_bound(ref)
    err = np.abs(prob.astype(np.float64) - ref)
    print('view mean softmax reps %d c %d p %d: largest error / bound %.4f' % (reps, c, p, (err / bound).max()))
    assert (err <= bound).all()
    if c > 1:
        top = np.sort(ref, axis=1)
        clear = (top[:, -1] - top[:, -2]) > 2 * _softmax_bound(top[:, -1])
        assert clear.sum() >= 0.5 * (~tied).sum()
        assert np.array_equal(pred[clear], ref_pred[clear])
        assert np.array_equal(pred[tied], np.full(int(tied.sum()), 3)) and np.array_equal(prob[tied, 3], prob[tied, 11])
        flat = (logits[inverse.reshape(reps, p)] == 0).all(axis=(0, 2))
        assert np.all(pred[flat] == 0)
    else:
        assert np.all(pred == 0) and np.all(prob == 1.0)


# ------------------------------------------------------------------------------------------------ 3.8 confusion matrix
@pytest.mark.parametrize('p', [0, 255, 256, 257])
@pytest.mark.parametrize('c', [16, 19])
def test_confusion_edges(c, p):
    """Labels -1, values in [c, 100), 100 and 255 are all left out; exact argmax ties go to the first index; two
    accumulating calls; exact equality with the bincount restatement."""
    from lidal_amd.evaluate import confusion_accumulate
    rs = np.random.RandomState(300 + c + p)
    nv = 200
    logits = rs.standard_normal((nv, c)).astype(np.float32)
    logits[::3, 5] = logits[::3, 9] = 7.0                      # ties of the maximum
    logits[1::3] = 0.0                                          # all equal: class 0
    inverse = rs.randint(0, nv, size=p).astype(np.int64)
    labels = rs.randint(0, c, size=p).astype(np.int64)
    odd = rs.random_sample(p) < 0.4
    labels[odd] = rs.choice([-1, c, c + 1, 57, 99, 100, 255], size=int(odd.sum()))
    ref = R.confusion(logits, inverse, labels, c)
    if p:
        assert ref.sum() < p and ref[5].sum() > 0 and ref[9].sum() < ref[5].sum() and ref[0].sum() > 0
    conf = torch.zeros((c, c), dtype=torch.int32, device=DEV)
    confusion_accumulate(conf, _t(logits), _t(inverse), _t(labels))
    assert np.array_equal(conf.cpu().numpy(), ref)
    confusion_accumulate(conf, _t(logits), _t(inverse), _t(labels))
    assert np.array_equal(conf.cpu().numpy(), 2 * ref)


# ------------------------------------------------------------------------------------------------ 3.9 registration
@pytest.mark.parametrize('p', [1, 255, 257, 50001])
def test_registration_bit_for_bit(p):
    from lidal_amd.data import register_scan
    rs = np.random.RandomState(400 + p % 1000)
    for _ in range(3):
        a = rs.normal(size=(3, 3))
        rot, _ = np.linalg.qr(a)
        pose = np.eye(4)
        pose[:3, :3] = rot
        pose[:3, 3] = rs.uniform(-5000, 5000, size=3)
        pts = (rs.standard_normal((p, 3)) * [30, 30, 3]).astype(np.float32)
        want = R.register(pts, pose)
        got = register_scan(_t(pts), pose).cpu().numpy()
        assert want.dtype == np.float64 and got.shape == want.shape
        assert np.array_equal(got.view(np.int64), want.view(np.int64))


# ------------------------------------------------------------------------------------------------ 4. out-of-range points
_POISON = r'''
import os, sys
import numpy as np, torch
sys.path.insert(0, %(root)r)
sys.path.insert(0, os.path.join(%(root)r, 'tests'))
import interframe_ref as R
from lidal_amd.score import FrameBank, interframe
nan, inf = float('nan'), float('inf')
poison = np.array([[nan, 0, 0], [0, inf, 0], [0, 0, -inf], [1e300, 0, 0], [-1e300, 1, 1], [3e5, 0, 0], [0, -3e5, 0.1],
                   [nan, nan, nan], [inf, -inf, nan], [0.1, 0.1, 2.5e5]])
rs = np.random.RandomState(13)
sizes = [3000, 2600, 2800]
worlds = [rs.uniform(0, 1.0, size=(n, 3)) for n in sizes]
probs = [R.softmax_rows(rs, n, 19) for n in sizes]
extra = [R.softmax_rows(rs, poison.shape[0], 19) for _ in sizes]
bad_w = [np.concatenate([w, poison[rs.permutation(poison.shape[0])]]) for w in worlds]
bad_p = [np.concatenate([p, e]) for p, e in zip(probs, extra)]

def run(pr, wo):
    bank = FrameBank(0.1)
    for p, w in zip(pr, wo):
        bank.add(torch.from_numpy(w).cuda(), torch.from_numpy(p).cuda())
    out = [interframe.score_points(bank, i, 2) for i in range(3)]
    torch.cuda.synchronize()
    return out

clean, dirty = run(probs, worlds), run(bad_p, bad_w)
interframe.CELL_ORDER = True            # lidal_interframe_score_ordered: the poisoned queries sorted by their parked keys
for a, b in zip(dirty, run(bad_p, bad_w)):
    assert all(torch.equal(u, v) for u, v in zip(a, b))
for i, (a, b) in enumerate(zip(clean, dirty)):
    n = sizes[i]
    assert all(torch.equal(u, v[:n]) for u, v in zip(a, b)), i
    d, e, c = (t[n:].cpu().numpy() for t in b)
    assert np.all(c == 0) and np.all(d == 0.0), (i, c, d)
    own = R.score_points(np.zeros((poison.shape[0], 3)), extra[i], [], [], 0.1)
    assert np.all(np.abs(e.astype(np.float64) - own['intere']) <= R.intere_bound(own, 4)), i
    # the restatement knows no key range (its finite poisoned points find their own copies in the other frames), so it
    # speaks for the valid points only: poisoned neighbours are matched by none of them there either
    ref = R.score_frame_points(i, bad_p, bad_w, interframe.neighbour_ids(i, 3, 2), 0.1)
    assert np.array_equal(b[2][:n].cpu().numpy(), ref['map_count'][:n])
assert int(clean[0][2].sum()) > 1000
print('POISON_OK')
'''


def test_out_of_range_points_match_nothing_and_disturb_nothing(tmp_path):
    """A handful of poisoned points (NaN, +-Inf, 1e300, 3e5 m) appended to every frame: the valid points' outputs are
    torch.equal to the run without them, the poisoned queries get cnt = 0, interd = 0 and the entropy of their own row;
    the same through the cell-ordered entry point.
    Run in a process of its own under a time limit: before the range predicate of csrc/grid.h such a query could loop
    without end."""
    r = subprocess.run([sys.executable, '-c', _POISON % {'root': ROOT}], capture_output=True, text=True, timeout=300,
                       cwd=str(tmp_path))
    assert r.returncode == 0 and 'POISON_OK' in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
