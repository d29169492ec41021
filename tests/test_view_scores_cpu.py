"""The view-disagreement scores on the host: the restatement tests/view_ref.py pinned against scipy as LiDAL.py:71,76
applies it, the exact zeros of the definition, and the flow of view_sequence's tuples through the collection, the
score board and the selection."""
import numpy as np
import torch

import view_ref as V


def _view_probs(rs, reps, p, c, zero_rows=True):
    lg = rs.standard_normal((reps, p, c)) * rs.choice([0.5, 2.0, 6.0], size=(1, p, 1))
    e = np.exp(lg - lg.max(axis=2, keepdims=True))
    if zero_rows:
        e[:, ::5, 7] = 0.0                      # one class exactly 0 in every view of every fifth point
    return (e / e.sum(axis=2, keepdims=True)).astype(np.float32)


def test_restatement_agrees_with_scipy_applied_as_the_reference_applies_it():
    """LiDAL.py:61-81 with the view mean as query_prob and every view matched: sum_prob accumulates in f32 and is
    divided by the count, interd_points += np.sum(kl_div(query + eps, view + eps), axis=1), entropy(sum_prob / count).
    The mean is the same f32 operations (exact); the divergence and the entropy differ from scipy only in the last bit
    of log before each f32 rounding: 1e-6, relatively (every term of either sum is >= 0)."""
    from scipy.special import kl_div
    from scipy.stats import entropy
    reps, p, c = 8, 257, 19
    pv = _view_probs(np.random.RandomState(5), reps, p, c)
    assert (pv[:, ::5, 7] == 0).all() and (pv[:, 1::5] > 0).all()
    m, viewd, viewe = V.scores_from_view_probs(pv)
    sum_prob = pv[0].copy()
    map_count = np.ones(p)
    for v in range(1, reps):
        sum_prob += pv[v]
        map_count += 1
    sum_prob /= np.expand_dims(map_count, 1)
    assert sum_prob.dtype == np.float32 and np.array_equal(m, sum_prob)
    epsilon = 0.00001
    interd_points = np.zeros(p)
    for v in range(reps):
        terms = kl_div(m + epsilon, pv[v] + epsilon)
        assert terms.dtype == np.float32
        interd_points += np.sum(terms, axis=1)
    interd_points /= reps
    intere_points = entropy(sum_prob, axis=1)
    assert viewd.dtype == np.float64 and viewe.dtype == np.float32 and intere_points.dtype == np.float32
    assert (interd_points > 0).all()
    assert np.allclose(viewd, interd_points, rtol=1e-6, atol=0)
    assert np.allclose(viewe, intere_points, rtol=1e-6, atol=0)


def test_one_view_and_two_identical_views_give_exactly_zero_divergence():
    """reps 1: m is p_0 / 1.  reps 2, the same view twice: p + p and / 2 are exact, m is p again; the KL term of x == y
    is x * log(1) - x + y = 0.  (Eight identical views do NOT give 0: the running f32 sum rounds at 3 p.)"""
    rs = np.random.RandomState(6)
    pv = _view_probs(rs, 1, 257, 19)
    for reps in (1, 2):
        m, viewd, viewe = V.scores_from_view_probs(np.repeat(pv, reps, axis=0))
        assert np.array_equal(m, pv[0])
        assert np.array_equal(viewd, np.zeros(257))
        assert (viewe > 0).all()
    lg = rs.standard_normal((257, 19)) * 3
    for reps in (1, 2):
        ref = V.scores_from_logits(lg, np.tile(np.arange(257), reps), reps)
        assert np.array_equal(ref['viewd'], np.zeros(257))
        assert np.array_equal(ref['view_arg'], np.tile(lg.argmax(1), (reps, 1)))


def test_view_tuples_flow_through_collection_board_and_selection():
    """view_sequence returns score_sequence's tuples: collect_sequence (one rank), ScoreBoard.add_sequence with every
    frame under its own sequence index (the unposed case: no two frames' supervoxels within 5 m) and .select reproduce
    select() on the same host arrays."""
    from lidal_amd.score import ScoreBoard, collect_sequence, select
    rs = np.random.RandomState(7)
    n_frames, n_sv = 6, 20
    n = n_frames * n_sv
    d = rs.gamma(2.0, 0.2, size=n).astype(np.float32)
    e = rs.uniform(0, 2.9, size=n).astype(np.float32)
    centres = rs.uniform(-30, 30, size=(n, 3)).astype(np.float32)
    pnums = rs.randint(50, 4000, size=n)
    board = ScoreBoard(n)
    for f in range(n_frames):
        sl = slice(f * n_sv, (f + 1) * n_sv)
        scores = [(torch.from_numpy(d[sl]), torch.from_numpy(e[sl]), torch.from_numpy(centres[sl]))]
        ptrs = [torch.from_numpy(np.concatenate([[0], np.cumsum(pnums[sl])]))]
        board.add_sequence(f, collect_sequence(scores, [np.arange(sl.start, sl.stop)], ptrs, 0, 1))
    offset = (np.repeat(np.arange(n_frames), n_sv) * 1000.0)[:, None]
    assert np.array_equal(board.sv_interds, d) and np.array_equal(board.sv_interes, e)
    assert np.array_equal(board.sv_pnums, pnums)
    assert np.array_equal(board.sv_centers, (centres + offset).astype(np.float32))
    flags = np.zeros(n, int)
    flags[rs.choice(n, 10, replace=False)] = 1
    total = int(pnums.sum())
    got = board.select(flags, total)
    want = select(flags, d, e, pnums, (centres + offset).astype(np.float32), total)
    assert np.array_equal(got, want)
    assert (got != flags).any()


def test_view_metrics_are_frame_level_metrics_largest_first():
    from lidal_amd.score import FrameBoard
    from lidal_amd.score.frame_level import LARGEST, METRICS, num_to_add
    for name in ('VIEWD', 'VIEWE', 'VOTE'):
        assert name in METRICS and LARGEST[name] is True
    rs = np.random.RandomState(8)
    lens = (120, 180)
    board = FrameBoard([np.zeros(n, bool) for n in lens])
    scores = [rs.uniform(0, 1, size=n).astype(np.float32) for n in lens]
    for s, sc in enumerate(scores):
        board.add(s, 'VIEWD', list(sc))
    new = board.select('VIEWD')
    k = num_to_add(sum(lens))
    assert k == 3 and new.sum() == k
    assert set(np.flatnonzero(new)) == set(np.argsort(-np.concatenate(scores), kind='stable')[:k])
