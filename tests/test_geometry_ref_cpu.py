"""tests/geometry_ref.py held to the oracle (oracle.tsref) on every input family of the geometry edge tests, and the
input generators held to what they claim: distinct hashes, slot collisions at the end of a table, bitmap aliases.
Also the sensitivity list of those tests: each mutation of the kernels, restated in numpy on the tests' own inputs,
must change an answer that tests/test_geometry_edges_gpu.py compares.  No GPU."""
import numpy as np
import pytest
import torch

import geometry_ref as G
from oracle.tsref.nn import functional as RF
from oracle.tsref.nn.utils import get_kernel_offsets


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def test_sphash_known_answers_and_the_oracle_on_edge_coordinates():
    c = np.array([[0, 0, 0, 0], [1, 2, 3, 0], [4095, 4096, 8191, 4], [100, 200, 300, 7]], dtype=np.int32)
    assert G.sphash(c).tolist() == [947293587111810033, 1043245732202901914, 482871551030584986, 15305659009498132]
    edge = G.hash_edge_coords()
    assert np.array_equal(G.sphash(edge), RF.sphash(_t(edge)).numpy())
    for ks, st in ((3, 1), (2, 2), (3, 8)):
        off = get_kernel_offsets(ks, st)
        assert np.array_equal(G.sphash(edge, off.numpy()), RF.sphash(_t(edge), off).numpy())      # offsets that wrap


def test_hashquery_equals_the_oracle_over_the_whole_i64_range():
    rng = np.random.default_rng(2)
    for nr in (0, 1, 513, 5000):
        refs = rng.integers(G.INT64_MIN, G.INT64_MAX, size=nr, dtype=np.int64)
        if nr > 10:
            refs[3], refs[7], refs[9] = -1, G.INT64_MIN, -1
            refs[nr // 2:] = refs[:nr - nr // 2]              # duplicates: the first occurrence wins
        q = np.concatenate([refs[::3], rng.integers(G.INT64_MIN, G.INT64_MAX, size=200, dtype=np.int64),
                            np.array([-1, G.INT64_MIN, G.INT64_MAX, 0], dtype=np.int64)])
        assert np.array_equal(G.hashquery(q, refs), RF.sphashquery(_t(q), _t(refs)).numpy())
    same = np.full(5000, 77, dtype=np.int64)
    assert G.hashquery(np.array([77]), same).tolist() == [0]
    assert G.hashquery(np.array([77]), same, last_wins=True).tolist() == [4999]      # (sensitivity: last-wins is seen)


def test_the_end_of_table_chain_is_one():
    keys, absent = G.end_of_table_chain()
    assert np.unique(keys).size == 64 and (keys < 0).any() and (keys > 0).any()
    assert G.table_capacity(64) == 1024
    assert (G.slot_of(keys, 1024) == 1023).all()              # one slot, the last: the chain runs 1023, 0, 1, .. 62
    s = G.slot_of(absent, 1024)
    assert ((s == 1023) | (s < 63)).all() and not np.isin(absent, keys).any()
    assert (s == 1023).any() and (s < 63).any()


def test_table_capacity_steps_and_bitmap_dims():
    assert [G.table_capacity(n) for n in (0, 512, 513, 8192, 8193, 16384, 16385)] == \
        [1024, 1024, 2048, 16384, 32768, 32768, 65536]
    assert [G.table_spatial_dims(G.table_capacity(n)) for n in (1, 8192, 8193, 16384, 16385)] == \
        [(5, 5), (5, 5), (6, 5), (6, 5), (6, 6)]


@pytest.mark.parametrize('ks,st', G.SHAPES)
def test_kernel_offsets_equal_the_oracle(ks, st):
    """Every shape of the edge tests is defined by the oracle's get_kernel_offsets (none had to be dropped)."""
    for ts in (1, 4):
        assert np.array_equal(G.kernel_offsets(ks, (ts,) * 3), get_kernel_offsets(ks, ts).numpy())
    off = G.kernel_offsets(ks, (1, 1, 1))
    if off.shape[0] % 2 == 1:
        assert np.array_equal(off[::-1], -off)                # what the mirror writes of the symmetric probe assume


@pytest.mark.parametrize('name,ks,st', G.kmap_case_ids(), ids=lambda v: str(v).replace(' ', ''))
def test_kernel_map_equals_the_oracle(name, ks, st):
    c = G.case_coords(name)
    ts = G.kmap_cases()[name][1]
    assert np.unique(c, axis=0).shape[0] == c.shape[0]        # precondition of build_kernel_map: unique rows
    m = G.case_map(name, ks, st)                              # (raises if two probed coordinates share a hash)
    if c.shape[0] == 0:
        assert m.total == 0 and m.results.shape == (np.prod(ks), 0)
        return
    nbmaps, nbsizes, sizes, out_coords, results = RF.build_kmap(_t(c), (ts,) * 3, ks, (st,) * 3)
    assert m.sizes == sizes
    assert np.array_equal(m.out_coords, out_coords.numpy())
    assert np.array_equal(m.results, results.numpy())
    assert np.array_equal(m.nbmaps, nbmaps.numpy())
    assert np.array_equal(m.nbsizes, nbsizes.numpy())
    if st == 1 and m.results.shape[0] % 2 == 1:
        assert np.array_equal(m.nbr_in, m.results[::-1])


def test_families_contain_what_they_claim():
    # the sheets straddle the origin in all three axes
    for ts in (1, 2, 4, 8):
        c = G.case_coords('sheet_origin_ts%d' % ts)
        assert (c[:, :3].min(0) < 0).all() and (c[:, :3].max(0) > 0).all() and (c[:, :3] % ts == 0).all()
        assert c.shape[0] <= 17000
    # row counts are exact, and the x-runs cross the word boundaries of the bitmap with a real neighbour on the other side
    for n in (8192, 8193, 16384, 16385, 0, 1, 2, 1023, 1024, 1025):
        c = G.case_coords('rows_%d' % n)
        assert c.shape[0] == n
        if n >= 1023:
            m = G.case_map('rows_%d' % n, (3, 3, 3), 1)
            for edge in (31, 63):
                left = np.nonzero(c[:, 0] == edge)[0]
                assert (m.results[14, left] >= 0).sum() > 0   # offset 14 = (+1, 0, 0): a hit across x' = edge | edge + 1
    # batches 0 and 4 share a column and a bitmap bit but not their neighbourhoods
    c = G.case_coords('batches8')
    assert sorted(set(c[:, 3].tolist())) == list(range(8))
    m = G.case_map('batches8', (3, 3, 3), 1)
    r0 = int(np.nonzero((c == [5, 5, 5, 0]).all(1))[0][0])
    r4 = int(np.nonzero((c == [5, 5, 5, 4]).all(1))[0][0])
    assert G.sbit_of(c[r0], 0, 5, 5) == G.sbit_of(c[r4], 0, 5, 5)
    assert m.results[14, r0] >= 0 and m.results[14, r4] < 0 and m.results[12, r4] >= 0 and m.results[12, r0] < 0


@pytest.mark.parametrize('ts', [1, 4])
def test_aliased_voxels_share_a_bit_and_differ_in_a_neighbour(ts):
    c, pairs = G.aliased(ts)
    xb, yb = G.table_spatial_dims(G.table_capacity(c.shape[0]))
    assert (xb, yb) == (5, 5)
    m = G.case_map('aliased_ts%d' % ts, (3, 3, 3), 1)
    shift = ts.bit_length() - 1
    row = {tuple(r): i for i, r in enumerate(c.tolist())}
    for a, b in pairs:
        assert tuple(a) != tuple(b) and G.sbit_of(a, shift, xb, yb) == G.sbit_of(b, shift, xb, yb)
        ra, rb = m.results[:, row[tuple(a)]] >= 0, m.results[:, row[tuple(b)]] >= 0
        assert (ra & ~rb).any() and (rb & ~ra).any()          # each has a neighbour the other lacks
    # and the probe of a LACKING neighbour really meets a set bit: the +x neighbour of a's aliases does not exist, its bit does
    bits = set(G.sbit_of(c, shift, xb, yb).tolist())
    for a, b in pairs:
        p = np.array(b) + np.array([ts, 0, 0, 0])
        assert tuple(p) not in row and int(G.sbit_of(p, shift, xb, yb)[0]) in bits


def test_downsample_equals_the_oracle_negative_coordinates_included():
    rng = np.random.default_rng(4)
    c = rng.integers(-300, 300, size=(3000, 4)).astype(np.int32)
    c[:, 3] = rng.integers(-2, 3, size=3000)
    for ts in (1, 2, 3, 8):
        ct = c.copy()
        ct[:, :3] *= ts
        assert np.array_equal(G.downsample(ct, (2 * ts,) * 3), RF.spdownsample(_t(ct), 2, 2, ts).numpy())
    pos = np.abs(c)
    chain, cur = G.pyramid(pos, 4, 1), _t(pos)
    for l in range(4):
        cur = RF.spdownsample(cur, 2, 2, 2 ** l)
        assert np.array_equal(chain[l], cur.numpy())
        assert np.array_equal(chain[l], G.downsample(pos, (2 ** (l + 1),) * 3))      # floor of a floor
    # (sensitivity: truncating division differs from floor only on negative coordinates -- which the GPU entry points
    # now refuse, so no accepted input can tell the two apart; the refusal tests stand guard instead)
    assert not np.array_equal(G.downsample(c, (2, 2, 2), trunc=True), G.downsample(c, (2, 2, 2)))
    assert np.array_equal(G.downsample(pos, (2, 2, 2), trunc=True), G.downsample(pos, (2, 2, 2)))


def test_row_order_restatement():
    assert G.bit_rank(8) == list(range(32))
    r = G.bit_rank(27)
    assert sorted(r[:27]) == list(range(27)) and r[13] == 0 and r[0] == 26 and r[26] == 19
    nbr = np.full((27, 5), -1, dtype=np.int32)
    nbr[13] = np.arange(5)
    nbr[0, 1] = 3
    nbr[0, 3] = 1
    perm, table, tm = G.row_order(nbr)
    assert perm.tolist() == [0, 2, 4, 1, 3] and np.array_equal(table, nbr[:, perm])
    assert tm.tolist() == [(1 << 13) | 1]
    # Gray rank: consecutive ranks are masks that differ in one bit
    k = G.row_keys(np.where(((np.arange(8)[None] ^ (np.arange(8)[None] >> 1)) >> np.arange(3)[:, None]) & 1, 0, -1))
    assert k.tolist() == list(range(8))


# ---------------------------------------------------------------- sensitivity: every mutation changes a compared answer
def _model(name, **kw):
    ts = G.kmap_cases()[name][1]
    m = G.case_map(name, (3, 3, 3), 1)
    return G.symmetric_probe_model(G.case_coords(name), ts, (3, 3, 3), m.results, **kw), m.results


@pytest.mark.parametrize('name', ['sheet_origin_ts1', 'sheet_origin_ts8', 'batches8', 'aliased_ts1', 'aliased_ts4',
                                  'rows_8192', 'rows_8193', 'rows_16385', 'rows_1025', 'dense12'])
def test_the_probe_model_is_the_map(name):
    got, want = _model(name)
    assert np.array_equal(got, want)


def test_mutations_of_the_probe_change_the_maps_the_gpu_tests_compare():
    def differs(name, **kw):
        got, want = _model(name, **kw)
        return not np.array_equal(got, want)
    # the probe reading shift 0 instead of the header's: every family at a tensor stride > 1
    assert differs('sheet_origin_ts2', shift_probe=0) and differs('sheet_origin_ts8', shift_probe=0)
    assert differs('aliased_ts4', shift_probe=0) and differs('rows_8193_ts2', shift_probe=0)
    # the batch bits dropped on the insert side only: any family with a batch id that is not 0 mod 4
    assert differs('batches8', insert_batch_mask=0) and differs('sheet_origin_ts1', insert_batch_mask=0)
    # xb and yb swapped on one side: only where they differ (8193 .. 16384 rows)
    assert differs('rows_8193', swap_xy=True) and differs('rows_16384', swap_xy=True)
    assert not differs('rows_8192', swap_xy=True)
    # the mirror entry written to K - k instead of K - 1 - k
    assert differs('dense12', mirror_shift=1) and differs('rows_2', mirror_shift=1)


def test_mutations_of_the_row_order_change_what_the_gpu_tests_compare():
    m = G.case_map('rows_1025', (3, 3, 3), 1)
    perm, table, tm = G.row_order(m.results)
    keys = G.row_keys(m.results)
    assert (np.diff(keys[perm].astype(np.int64)) == 0).any()                  # there are ties ...
    perm_u = G.row_order(m.results, stable=False)[0]
    assert not np.array_equal(perm_u, perm)                                   # ... so an unstable sort is seen
    tm256 = G.row_order(m.results, tile_rows=256)[2]
    wide = np.repeat(tm256, 2)[:tm.size]
    assert not np.array_equal(wide, tm)                                       # a mask OR-ed over 256 rows has extra bits
    assert ((wide & tm) == tm).all()                                          # (extra only: every convolution still passes)
