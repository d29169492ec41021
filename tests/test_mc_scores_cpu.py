"""The MC-dropout scores without a GPU: tests/mc_ref.py's restatement of the kernel's number widths against the f64
definition at the shapes the GPU tests use (how far f32 probabilities alone are from the definition), its exact
identities, and the new frame-level metric names."""
import numpy as np
import pytest

import mc_ref as M


@pytest.mark.parametrize('sigma', M.SIGMAS)
@pytest.mark.parametrize('reps,c,p', M.SHAPES)
def test_f32_probabilities_stay_two_orders_inside_the_bar(reps, c, p, sigma):
    """The bar of the GPU tests is 1e-4 x max|reference| (tests/test_view_scores_gpu.py:62-63).  A pipeline that only
    shares the kernel's number widths -- f32 soft-max rows, f32 mean, f64 entropies -- has to be far inside it, or the
    bar would be testing the format and not the kernel."""
    logits, inverse = M.inputs(reps, c, p, sigma)
    ref = M.scores_from_logits(logits, inverse, reps)
    pv = M.softmax_f32(logits[inverse].reshape(reps, p, c))
    m, bald, ment, _ = M.scores_from_pass_probs(pv)
    assert bald.dtype == np.float64 and ment.dtype == np.float32
    err_b, bar_b = np.abs(bald - ref['bald']).max(), 1e-4 * np.abs(ref['bald']).max()
    err_e, bar_e = np.abs(ment - ref['ment']).max(), 1e-4 * np.abs(ref['ment']).max()
    print('reps %d c %d p %d sigma %d: bald error %.2e (bar %.2e)  ment error %.2e (bar %.2e)'
          % (reps, c, p, sigma, err_b, bar_b, err_e, bar_e))
    assert err_e <= bar_e / 100
    if reps > 1:
        assert err_b <= bar_b / 100
    else:
        assert np.all(bald == 0.0) and np.all(ref['bald'] == 0.0)       # one pass: m is p_0
    assert np.abs(m - ref['prob']).max() < 1e-6
    assert ref['bald'].min() > -1e-12                                   # (Jensen: the mutual information is >= 0)


@pytest.mark.parametrize('reps', [1, 2, 4, 8, 3, 5, 7])
def test_a_repeated_row_gives_exactly_zero_in_the_restatement(reps):
    """The f64 sum of up to 2^29 equal f32 addends is exact and (n p) / n rounds back to p, so m is the row; the two-sum
    of equal entropies returns n H whenever that is a double, as it is for n a power of two, and S / n is H."""
    rs = np.random.RandomState(reps)
    row = M.softmax_f32((rs.standard_normal((500, 19)) * 3).astype(np.float32))
    _, bald, ment, m = M.scores_from_pass_probs(np.stack([row] * reps))
    assert np.array_equal(m, row)
    if reps in (1, 2, 4, 8):
        assert np.all(bald == 0.0)
        assert np.array_equal(ment, M.scores_from_pass_probs(row[None])[2])
    else:
        assert np.abs(bald).max() < 1e-15


def test_why_the_entropy_is_not_taken_of_the_f32_chain():
    """Five, six and seven equal f32 addends round away from the exact multiple in a chain of adds, so the view mean of
    8 equal rows as lidal_view_mean_softmax forms it -- prob, whose bytes are kept -- is not the row; its entropy would
    leave a bald of about 1e-7 where the passes agree exactly.  Likewise a plain f64 chain of 8 equal entropies."""
    rs = np.random.RandomState(8)
    row = M.softmax_f32((rs.standard_normal((500, 19)) * 3).astype(np.float32))
    prob, bald, _, m = M.scores_from_pass_probs(np.stack([row] * 8))
    assert not np.array_equal(prob, row) and np.abs(prob - row).max() <= 2 * np.spacing(row.max())
    assert np.array_equal(m, row) and np.all(bald == 0.0)
    chain = 0 < np.abs(M.entropy(prob) - M.entropy(row)).max() < 1e-6
    h = M.entropy(row)
    s = np.zeros_like(h)
    for _ in range(8):
        s = s + h
    assert chain and (s / 8 != h).any()


def test_a_one_hot_row_has_zero_entropy_and_no_nan():
    logits = np.full((4, 19), -250.0, np.float32)
    logits[np.arange(4), [0, 5, 18, 7]] = 0.0
    pv = M.softmax_f32(logits)[None].repeat(2, axis=0)
    assert np.array_equal(np.sort(pv[0], axis=1)[:, -1], np.ones(4, np.float32)) and pv[0].sum() == 4.0
    m, bald, ment, _ = M.scores_from_pass_probs(pv)
    assert np.all(ment == 0.0) and np.all(bald == 0.0) and not np.isnan(m).any()
    ref = M.scores_from_logits(logits, np.tile(np.arange(4), 2), 2)
    assert np.all(ref['ment'] < 1e-100) and np.all(ref['bald'] == 0.0)       # (exp(-250) is not 0 in f64)


def test_the_frame_level_metrics_keep_their_order():
    from lidal_amd.score.frame_level import LARGEST, MC_METRICS, METRICS
    assert METRICS == ('ENT', 'MAR', 'CONF', 'SEGENT', 'CSET', 'VIEWD', 'VIEWE', 'VOTE', 'BALD', 'MCENT')
    assert MC_METRICS == ('BALD', 'MCENT')
    assert LARGEST['BALD'] is True and LARGEST['MCENT'] is True
    assert LARGEST['CONF'] is False and LARGEST['VOTE'] is True


def test_mc_scoring_needs_a_counter_dropout_before_anything_runs():
    from lidal_amd.network import MinkUNet, SPVCNN
    from lidal_amd.score import frame_sequence, mc_sequence
    for model in (MinkUNet(19), SPVCNN(19)):
        with pytest.raises(ValueError, match='no lidal_amd.nn.Dropout'):
            mc_sequence(model, [{}])
        with pytest.raises(ValueError, match='no lidal_amd.nn.Dropout'):
            frame_sequence(model, [{}], metrics=('BALD',))
