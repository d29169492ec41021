"""centre_pairs (csrc/neighbours.hip: lidal_radius_pairs_count / _fill) against the brute-force numpy restatement of
the selection loop's expression (tests/pairs_ref.py), array_equal on both arrays of the table: at the rounding boundary
of the radius, on either side of cell borders, with the sequence offsets, with rows longer than a workgroup and than the
LDS staging of the row sort, with centres that have no pairs or are refused, and at other radii -- and then the flags of
select_indexed on that table against select."""
import os

import numpy as np
import pytest
import torch

from guarded_ws import Guarded
from pairs_ref import pairs_ref

pytestmark = pytest.mark.gpu
F0 = np.float32(0)


def _check(centers, radius=5.0, as_tensor=False):
    from lidal_amd.score import centre_pairs
    centers = np.ascontiguousarray(centers, dtype=np.float32)
    got = centre_pairs(torch.from_numpy(centers).cuda() if as_tensor else centers, radius)
    want = pairs_ref(centers, radius)
    assert got[0].dtype == np.int64 and got[1].dtype == np.int32
    assert got[0].shape == (centers.shape[0] + 1,)
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1], want[1])
    return got


@pytest.fixture(scope='module')
def board(golden_dir):
    from lidal_amd.score import centre_pairs
    g = np.load(os.path.join(golden_dir, 'selection_small.npz'))
    b = {k: g[k] for k in ('flags_in', 'sv_interds', 'sv_interes', 'sv_pnums', 'sv_centers', 'flags_out')}
    b['train_point_num'] = int(g['train_point_num'])
    b['want'] = pairs_ref(b['sv_centers'], 5.0)
    b['got'] = centre_pairs(b['sv_centers'], 5.0)
    return b


def test_fixture_centres(board):
    from lidal_amd import backend as B
    assert np.array_equal(board['got'][0], board['want'][0])
    assert np.array_equal(board['got'][1], board['want'][1])
    assert B.HITS.get('radius_pairs_count', 0) >= 1 and B.HITS.get('radius_pairs_fill', 0) >= 1
    assert np.diff(board['got'][0]).max() > 64          # rows longer than one wave of candidates


def test_table_is_symmetric_ascending_without_self_pairs(board):
    row_ptr, col = board['got']
    n = row_ptr.size - 1
    rows = np.repeat(np.arange(n), np.diff(row_ptr))
    assert not (rows == col).any()
    inside = np.ones(col.size, dtype=bool)
    inside[row_ptr[:-1][np.diff(row_ptr) > 0]] = False  # first entry of every row
    assert (np.diff(col.astype(np.int64))[inside[1:]] > 0).all()
    key = rows.astype(np.int64) * n + col
    assert np.array_equal(np.sort(key), np.sort(col.astype(np.int64) * n + rows))


def test_table_is_deterministic_and_takes_a_device_tensor(board):
    again = _check(board['sv_centers'], as_tensor=True)
    assert np.array_equal(again[0], board['got'][0]) and np.array_equal(again[1], board['got'][1])


def test_rounded_root_decides_at_the_radius():
    """From (0,0,0): (3,4,0) is at 5.0; (3, 4-, 0) has a squared distance below 25 whose rounded root is 5.0 -- not a
    pair either; one step further it is."""
    four = np.nextafter(np.float32(4), F0)
    trio = np.array([[0, 0, 0], [3, 4, 0], [3, four, 0], [3, np.nextafter(four, F0), 0]], np.float32)
    assert float(np.square(trio[2]).sum()) < 25.0
    row_ptr, col = _check(trio)
    assert col[row_ptr[0]:row_ptr[1]].tolist() == [3]
    # the same boundary away from the origin, across a cell border, and on the other axes
    for shift in ([5.0, 4.0, -3.0], [-11.0, -12.0, 7.0]):
        for perm in ([0, 1, 2], [2, 0, 1], [1, 2, 0]):
            _check((trio + np.float32(shift))[:, perm])


def test_either_side_of_cell_borders():
    """Coordinates at, just below and just above the borders of the 8 m cells at 0, +-8, +-16: floor, not truncation,
    and every neighbour cell a pair can straddle."""
    vals = []
    for b in (-16.0, -8.0, 0.0, 8.0, 16.0):
        b = np.float32(b)
        vals += [b, np.nextafter(b, np.float32(-100)), np.nextafter(b, np.float32(100)), b - np.float32(0.5),
                 b + np.float32(0.5), b - np.float32(4.75), b + np.float32(2.5)]
    vals = np.array(vals + [-0.0], np.float32)
    rs = np.random.RandomState(21)
    _check(vals[rs.randint(0, vals.size, (700, 3))])
    line = np.zeros((vals.size, 3), np.float32)         # all on one axis: pairs straddle the border cell by cell
    line[:, 2] = vals
    _check(line)


def test_sequence_offsets():
    """LiDAL.py:218: the centres of sequence k are shifted by 1000 k metres, which keeps sequences apart."""
    rs = np.random.RandomState(22)
    c = np.concatenate([rs.uniform(-20, 20, (150, 3)).astype(np.float32) + np.float32(k * 1000.0) for k in range(11)])
    row_ptr, col = _check(c[rs.permutation(c.shape[0])])
    assert row_ptr[-1] > 0


def test_coincident_centres_in_one_cell():
    """1 500 equal centres: every row has 1 499 entries, more than a workgroup and more than the LDS staging of the row
    sort; a few distinct centres around them keep the rows from being all alike."""
    rs = np.random.RandomState(23)
    c = np.tile(np.float32([3.5, -2.25, 1.0]), (1500, 1))
    c = np.concatenate([c, rs.uniform(-6, 10, (40, 3)).astype(np.float32)])
    row_ptr, _ = _check(c[rs.permutation(c.shape[0])])
    assert np.diff(row_ptr).max() >= 1499


@pytest.mark.parametrize('n', [0, 1, 2])
def test_tiny_boards(n):
    c = np.array([[1, 2, 3], [1, 2, 6]], np.float32)[:n]
    row_ptr, col = _check(c.reshape(n, 3))
    assert col.size == (2 if n == 2 else 0)
    if n == 2:
        assert _check(np.array([[1, 2, 3], [1, 2, 8]], np.float32))[1].size == 0


def test_centres_without_pairs_and_centres_refused():
    from lidal_amd.score import centre_pairs
    rs = np.random.RandomState(24)
    c = rs.uniform(-9, 9, (300, 3)).astype(np.float32)
    c[17, 1] = np.nan
    c[130, 0] = np.inf
    c[131] = [-np.inf, np.nan, 0]
    row_ptr, col = _check(c)
    for i in (17, 130, 131):
        assert row_ptr[i] == row_ptr[i + 1] and not (col == i).any()
    assert row_ptr[-1] > 0
    # the last cells of the key range are served: |index| = 2^20 - 1, probes stop at the range's edge
    edge = np.float32(8 * (2 ** 20 - 1))
    far = np.array([[edge, 0, 0], [edge + 3, 1, 0], [edge + 7, 0, 0], [-edge, 0, -edge], [-edge + 2, 0, 3 - edge],
                    [0, edge + 1, 0], [0, edge + 5, 1]], np.float32)
    assert _check(np.concatenate([c, far]))[0][-1] > row_ptr[-1]
    # one cell further is refused, on either side
    for bad in (np.float32(8 * 2 ** 20), -edge - np.float32(4), np.float32(1e30)):
        d = c.copy()
        d[200, 2] = bad
        with pytest.raises(ValueError):
            centre_pairs(d)


@pytest.mark.parametrize('radius,box', [(0.5, 3.0), (8.0, 40.0), (5.0, 25.0), (0.5, 40.0)])
def test_other_radii(radius, box):
    rs = np.random.RandomState(25)
    c = rs.uniform(-box, box, (900, 3)).astype(np.float32)
    c[::7] = np.round(c[::7] / np.float32(radius)) * np.float32(radius)        # centres exactly `radius` apart
    _check(c, radius)


@pytest.mark.parametrize('n', [2047, 2048, 2049, 524288, 524289, 2097153])
def test_lattice_at_the_edges_of_the_scan(n):
    """Sizes chosen for the scan of the row lengths (8 x 256 = 2048 lengths per tile): one tile and its neighbours, one
    256-wide step of tile sums (256 x 2048) and one more, and one element past 1024 tiles.  Centres on a 1 m lattice,
    4096 to a row, radius 1.25 m: the neighbours of i are i - 4096, i - 1, i + 1, i + 4096 where they exist, so the
    lengths are 2, 3 or 4 and the table is index arithmetic.  Every value is exact in f32; the cell edge is 2 m."""
    from lidal_amd.score import centre_pairs
    i = np.arange(n, dtype=np.int64)
    centers = np.stack([i % 4096, i // 4096, np.zeros(n, np.int64)], axis=1).astype(np.float32)
    cand = np.stack([i - 4096, i - 1, i + 1, i + 4096], axis=1)
    there = np.stack([i >= 4096, i % 4096 != 0, (i % 4096 != 4095) & (i + 1 < n), i + 4096 < n], axis=1)
    row_ptr, col = centre_pairs(centers, 1.25)
    assert row_ptr.dtype == np.int64 and col.dtype == np.int32
    assert np.array_equal(row_ptr, np.concatenate([[0], np.cumsum(there.sum(axis=1))]))
    assert np.array_equal(col, cand[there].astype(np.int32))


def test_radius_float32_cannot_hold_is_refused():
    from lidal_amd.score import centre_pairs
    with pytest.raises(ValueError):
        centre_pairs(np.zeros((3, 3), np.float32), 0.1)


def test_scratch_is_what_the_library_says(board, monkeypatch):
    from lidal_amd import backend as B
    from lidal_amd.score import centre_pairs
    g = Guarded()
    monkeypatch.setattr(B, 'workspace', g)
    got = centre_pairs(board['sv_centers'][:1234], 5.0)
    g.check()
    want = pairs_ref(board['sv_centers'][:1234], 5.0)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_select_indexed_on_the_device_table_equals_select(board):
    from lidal_amd.score import select, select_indexed
    args = (board['flags_in'], board['sv_interds'], board['sv_interes'], board['sv_pnums'], board['sv_centers'],
            board['train_point_num'])
    want = select(*args)
    got, counts = select_indexed(*args, pairs=board['got'], details=True)
    assert np.array_equal(got, want) and np.array_equal(got, board['flags_out'])
    assert counts['multi_hit'] >= 1
    assert np.array_equal(select_indexed(*args), want)  # pairs=None: the table is made on the way


def test_scoreboard_select_indexed(board):
    from lidal_amd.score import ScoreBoard
    sb = ScoreBoard(board['flags_in'].size, sv_pnums=board['sv_pnums'], sv_centers=board['sv_centers'])
    sb.sv_interds[:] = board['sv_interds']
    sb.sv_interes[:] = board['sv_interes']
    budget = int(board['sv_pnums'][:400].sum() * 100)
    want = sb.select(board['flags_in'], budget)
    assert np.array_equal(sb.select(board['flags_in'], budget, indexed=True), want)
    assert np.array_equal(sb.select(board['flags_in'], budget, indexed=True, pairs=board['got']), want)
    assert (want == 1).sum() > 0 and (want == 2).sum() > 0
