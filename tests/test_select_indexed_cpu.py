"""select_indexed (lidal_amd/score/selection.py) against select on the host: with a neighbour table from the numpy
restatement (tests/pairs_ref.py) the table-driven loop must write the flags of the reference's loop, array_equal, at
every budget -- and must have gone through its fallback (a candidate with two or more added neighbours, where the first
hit depends on the set's iteration order) while doing so."""
import os

import numpy as np
import pytest

from pairs_ref import pairs_ref, within


@pytest.fixture(scope='module')
def board(golden_dir):
    g = np.load(os.path.join(golden_dir, 'selection_small.npz'))
    b = {k: g[k] for k in ('flags_in', 'sv_interds', 'sv_interes', 'sv_pnums', 'sv_centers', 'flags_out')}
    b['train_point_num'] = int(g['train_point_num'])
    b['pairs'] = pairs_ref(b['sv_centers'], 5.0)
    return b


def _both(b, budget):
    from lidal_amd.score import select, select_indexed
    args = (b['flags_in'], b['sv_interds'], b['sv_interes'], b['sv_pnums'], b['sv_centers'], budget)
    want = select(*args)
    got, counts = select_indexed(*args, pairs=b['pairs'], details=True)
    return want, got, counts


def test_restatement_is_the_loops_expression(board):
    """pairs_ref evaluates a row at a time; the loop evaluates one pair at a time.  Same booleans, boundary included."""
    c = board['sv_centers']
    rs = np.random.RandomState(3)
    for i in rs.randint(0, c.shape[0], 40):
        row = within(c, i, 5.0)
        for j in rs.randint(0, c.shape[0], 200):
            assert bool(np.sqrt(np.square(c[i] - c[j]).sum()) < 5.0) == bool(row[j])
    four = np.nextafter(np.float32(4), np.float32(0))
    trio = np.array([[0, 0, 0], [3, 4, 0], [3, four, 0], [3, np.nextafter(four, np.float32(0)), 0]], np.float32)
    assert float(np.square(trio[2]).sum()) < 25.0                       # the squared distance is below 25 ...
    assert within(trio, 0, 5.0).tolist() == [True, False, False, True]  # ... the rounded root is 5.0: not within
    row_ptr, col = pairs_ref(trio, 5.0)
    assert col[row_ptr[0]:row_ptr[1]].tolist() == [3]
    assert row_ptr.dtype == np.int64 and col.dtype == np.int32


def test_table_of_fixture_is_symmetric_and_dense_enough(board):
    row_ptr, col = board['pairs']
    n = board['sv_centers'].shape[0]
    rows = np.repeat(np.arange(n), np.diff(row_ptr))
    assert not (rows == col).any()
    fwd = set(zip(rows.tolist(), col.tolist()))
    assert fwd == set(zip(col.tolist(), rows.tolist()))
    assert np.diff(row_ptr).max() >= 2                  # a candidate can have several added neighbours at all


@pytest.mark.parametrize('which', ['own', 'binding', 'ten_times_all'])
def test_select_indexed_equals_select(board, which):
    budget = {'own': board['train_point_num'], 'binding': int(board['sv_pnums'][:40].sum() * 100),
              'ten_times_all': int(board['sv_pnums'].sum() * 10)}[which]
    want, got, counts = _both(board, budget)
    assert np.array_equal(got, want)
    assert got.dtype == want.dtype
    if which == 'own':
        assert np.array_equal(got, board['flags_out'])  # the flags the reference's own run wrote
    if which == 'binding':
        assert (want == 1).sum() < (board['flags_out'] == 1).sum()      # the budget branch did bind
    else:
        # the fallback was exercised: candidates whose first hit only the set's iteration order decides
        assert counts['multi_hit'] >= 1, counts
    assert counts['free'] >= 1


def test_multi_hit_counter_counts(board):
    """details=False returns the flags alone; the counters add up to the candidates visited."""
    from lidal_amd.score import select_indexed
    args = (board['flags_in'], board['sv_interds'], board['sv_interes'], board['sv_pnums'], board['sv_centers'],
            int(board['sv_pnums'][:40].sum() * 100))
    flags = select_indexed(*args, pairs=board['pairs'])
    flags2, counts = select_indexed(*args, pairs=board['pairs'], details=True)
    assert isinstance(flags, np.ndarray) and np.array_equal(flags, flags2)
    assert set(counts) == {'free', 'one_hit', 'multi_hit'} and sum(counts.values()) > 0


def _small_board(n, seed, coincide=False, flags=None):
    rs = np.random.RandomState(seed)
    centers = (np.tile(np.float32([12.5, -3.25, 1.0]), (n, 1)) if coincide
               else rs.uniform(-12, 12, (n, 3)).astype(np.float32))
    return dict(flags_in=np.zeros(n, dtype=np.int64) if flags is None else flags,
                sv_interds=rs.uniform(0, 1, n).astype(np.float32), sv_interes=rs.uniform(0, 2, n).astype(np.float32),
                sv_pnums=rs.randint(50, 500, n), sv_centers=centers, pairs=pairs_ref(centers, 5.0))


def test_all_labelled_board():
    b = _small_board(60, 5, flags=np.ones(60, dtype=np.int64))
    want, got, counts = _both(b, 10 ** 9)
    assert np.array_equal(got, want) and (got == 1).all() and sum(counts.values()) == 0


def test_empty_board():
    b = _small_board(0, 6)
    want, got, counts = _both(b, 10 ** 9)
    assert got.shape == (0,) and np.array_equal(got, want) and sum(counts.values()) == 0


def test_every_centre_coincides():
    """One cluster: every candidate after the first hits the single added member; the flags move along the entropies."""
    b = _small_board(80, 7, coincide=True)
    assert np.diff(b['pairs'][0]).tolist() == [79] * 80
    want, got, counts = _both(b, 10 ** 9)
    assert np.array_equal(got, want)
    assert (got == 1).sum() == 1 and (got == 2).sum() == 1 and counts['free'] == 2


def test_crowded_board_with_old_pseudo_labels():
    """Dense centres (a dozen neighbours each) and a board that carries flags 1 and 2 of an earlier round."""
    rs = np.random.RandomState(8)
    b = _small_board(400, 9, flags=rs.choice([0, 0, 0, 1, 2], 400).astype(np.int64))
    multi = 0
    for budget in (10 ** 9, int(b['sv_pnums'].sum()) * 10):
        want, got, counts = _both(b, budget)
        assert np.array_equal(got, want)
        multi += counts['multi_hit']
    assert multi >= 1


def test_table_of_another_board_is_refused(board):
    from lidal_amd.score import select_indexed
    b = _small_board(10, 1)
    with pytest.raises(ValueError):
        select_indexed(b['flags_in'], b['sv_interds'], b['sv_interes'], b['sv_pnums'], b['sv_centers'], 10 ** 9,
                       pairs=board['pairs'])


def test_centre_pairs_refuses_before_touching_the_device():
    from lidal_amd.score import centre_pairs
    c = np.zeros((4, 3), np.float32)
    for bad in ([[0.0, 0.0, 0.0]], c.astype(np.float64), c[:, :2], c.reshape(-1)):
        with pytest.raises(TypeError):
            centre_pairs(bad)
    for radius in (0.1, 0.0, -5.0, float('inf'), float('nan'), 1e39):
        with pytest.raises(ValueError):
            centre_pairs(c, radius)
