"""The geometry builders (csrc/hash.hip, csrc/kmap.hip, nn/functional/{hash,query,downsample,conv}.py) at their edges,
against the plain restatement in tests/geometry_ref.py (itself held to the oracle in tests/test_geometry_ref_cpu.py,
where the input families also prove what they contain).  Everything is integer work and compared exactly."""
import numpy as np
import pytest
import torch

import geometry_ref as G

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _F():
    from lidal_amd.nn import functional as F
    return F


def _conv():
    from lidal_amd.nn.functional import conv
    return conv


def _g(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _eq(got, want):
    got = got.cpu().numpy()
    want = np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(got.astype(np.int64), want.astype(np.int64)), int((got != want).sum())


# ---------------------------------------------------------------- tables
def test_sphash_on_negative_extreme_and_wrapping_coordinates():
    F = _F()
    c = G.hash_edge_coords()
    _eq(F.sphash(_g(c)), G.sphash(c))
    for ks, st in (((3, 3, 3), 1), ((2, 2, 2), 2), ((3, 3, 3), 8), ((5, 5, 5), 1)):
        off = G.kernel_offsets(ks, (st,) * 3)
        _eq(F.sphash(_g(c), _g(off)), G.sphash(c, off))


def _i64_keys(n, seed):
    return np.random.default_rng(seed).integers(G.INT64_MIN, G.INT64_MAX, size=n, dtype=np.int64)


@pytest.mark.parametrize('nr', [512, 513, 8192, 8193])
@pytest.mark.parametrize('minus_one', [True, False])
def test_sphashquery_over_the_whole_i64_range(nr, minus_one):
    """Capacity steps at 512|513 and 8192|8193 references; negative keys, INT64_MIN; the all-ones key -1 (the empty mark
    of a slot) present in the references -- twice: the first index wins -- or absent from them."""
    F = _F()
    refs = _i64_keys(nr, nr)
    refs[refs == -1] = 5
    refs[11] = G.INT64_MIN
    refs[nr - 1] = refs[4]                                        # a duplicate: first wins
    if minus_one:
        refs[7] = refs[300] = -1
    q = np.concatenate([refs, _i64_keys(2000, nr + 1), np.array([-1, G.INT64_MIN, G.INT64_MAX, 0, -2], dtype=np.int64)])
    want = G.hashquery(q, refs)
    assert want[nr + 2000] == (7 if minus_one else -1)
    got = F.sphashquery(_g(q), _g(refs))
    _eq(got, want)
    assert int(got.max()) < nr and int(got.min()) >= -1           # nothing but row indices and -1


def test_sphashquery_identical_references_and_empty_tables():
    F = _F()
    same = np.full(5000, -1234567890123, dtype=np.int64)
    _eq(F.sphashquery(_g(np.array([-1234567890123, 5, -1], dtype=np.int64)), _g(same)), [0, -1, -1])
    ones = np.full(5000, -1, dtype=np.int64)
    _eq(F.sphashquery(_g(np.array([-1, 5, -2], dtype=np.int64)), _g(ones)), [0, -1, -1])
    none = torch.zeros(0, dtype=torch.int64, device=DEV)
    _eq(F.sphashquery(_g(np.array([-1, 0], dtype=np.int64)), none), [-1, -1])


def test_sphashquery_probe_chain_wraps_at_the_end_of_the_table():
    F = _F()
    keys, absent = G.end_of_table_chain()                         # 64 keys on the LAST slot of 1024: the chain wraps to slot 0
    q = np.concatenate([keys[::-1], absent, keys])
    _eq(F.sphashquery(_g(q), _g(keys)), G.hashquery(q, keys))
    refs = np.concatenate([keys, keys[:5], np.array([-1], dtype=np.int64)])        # duplicates inside the chain, and -1
    q = np.concatenate([q, np.array([-1], dtype=np.int64)])
    _eq(F.sphashquery(_g(q), _g(refs)), G.hashquery(q, refs))


@pytest.mark.parametrize('s', [1, 2, 8])
def test_table_from_coords_equals_table_from_hashes(s):
    from lidal_amd.nn.functional.query import HashTable
    F = _F()
    c = G.sheet_origin(s, seed=20 + s)[:6000]
    rng = np.random.default_rng(s)
    qc = np.concatenate([c[rng.permutation(c.shape[0])[:3000]], c[:3000] + np.array([s, 0, 0, 0], dtype=np.int32),
                         c[:50] + np.array([0, 0, 0, 4], dtype=np.int32)])
    q = F.sphash(_g(qc))
    a = HashTable.from_coords(_g(c), s).query(q)
    b = HashTable(F.sphash(_g(c))).query(q)
    want = G.hashquery(G.sphash(qc), G.sphash(c))
    row = {t: i for i, t in enumerate(map(tuple, c.tolist()))}
    assert want.tolist() == [row.get(t, -1) for t in map(tuple, qc.tolist())]     # (no hash collision in this input)
    _eq(a, want)
    _eq(b, want)


# ---------------------------------------------------------------- kernel maps
def _check_map(kmap, out_coords, m, route):
    assert tuple(kmap.sizes) == tuple(m.sizes), route
    _eq(out_coords, m.out_coords)
    _eq(kmap.nbr_out, m.results)
    _eq(kmap.nbsizes, m.nbsizes)
    _eq(kmap.koff, m.koff)
    assert kmap.total == m.total, route
    _eq(kmap.nbmaps, m.nbmaps)
    _eq(kmap.nbr_in, m.nbr_in)
    if kmap.symmetric:
        assert torch.equal(kmap.nbr_in, kmap.nbr_out.flip(0)), route


def _three_routes(c, ts, ks, st, m):
    """-> the maps of build_kernel_map with gradients (table + rules in one call), under no_grad (rules built lazily)
    and of the batched builder, each checked against the reference map m."""
    conv = _conv()
    ins, stv = (ts,) * 3, (st,) * 3
    with torch.enable_grad():
        km, oc = conv.build_kernel_map(_g(c), ins, ks, stv)
        assert km._rules is not None
        _check_map(km, oc, m, 'grad')
    with torch.no_grad():
        km, oc = conv.build_kernel_map(_g(c), ins, ks, stv)
        assert km._rules is None
        _check_map(km, oc, m, 'no_grad')
    oc = _g(c) if st == 1 else _g(m.out_coords)
    for grad in (True, False):
        with torch.set_grad_enabled(grad):
            km, = conv.build_kernel_maps([(_g(c), ins, ks, stv, oc)], {})
            assert (km._rules is not None) == grad
            _check_map(km, oc, m, 'batch')


@pytest.mark.parametrize('name,ks,st', G.kmap_case_ids(), ids=lambda v: str(v).replace(' ', ''))
def test_kernel_map_three_routes(name, ks, st):
    c = G.case_coords(name)
    ts = G.kmap_cases()[name][1]
    _three_routes(c, ts, ks, st, G.case_map(name, ks, st))


def test_batched_builder_with_an_empty_level_and_mixed_shapes():
    """One call over maps of odd sizes and every kernel volume, an EMPTY level among them: each equals the single build,
    the empty one included (nbsizes and koff all zero)."""
    conv = _conv()
    names = [('rows_1025', (3, 3, 3), 1), ('rows_0', (3, 3, 3), 1), ('rows_1023', (2, 2, 2), 2), ('rows_0', (2, 2, 2), 2),
             ('batches8', (5, 5, 5), 1), ('rows_1', (1, 1, 1), 1), ('rows_2', (3, 1, 1), 1), ('dense12_pos', (1, 3, 3), 1)]
    for grad in (True, False):
        jobs, maps = [], []
        for name, ks, st in names:
            m = G.case_map(name, ks, st)
            c = _g(G.case_coords(name))
            jobs.append((c, (1, 1, 1), ks, (st,) * 3, c if st == 1 else _g(m.out_coords)))
            maps.append(m)
        with torch.set_grad_enabled(grad):
            out = conv.build_kernel_maps(jobs, {})
            single, oc1 = conv.build_kernel_map(jobs[1][0], (1, 1, 1), (3, 3, 3), (1, 1, 1))
        for km, job, m in zip(out, jobs, maps):
            _check_map(km, job[4], m, 'batch')
        for a, b in ((out[1].nbr_out, single.nbr_out), (out[1].nbsizes, single.nbsizes), (out[1].koff, single.koff)):
            assert torch.equal(a, b)
        assert out[1].total == 0 and out[1].nbmaps.shape == (0, 2) and oc1.shape == (0, 4)
    with torch.no_grad():                                         # nothing but empty levels
        e = _g(G.case_coords('rows_0'))
        km, = conv.build_kernel_maps([(e, (1, 1, 1), (3, 3, 3), (1, 1, 1), e)], {})
        assert km.total == 0 and km.nbsizes.tolist() == [0] * 27


# ---------------------------------------------------------------- downsampling
def _down_inputs():
    rng = np.random.default_rng(6)
    out = {}
    for n in (1, 1023, 1024, 1025):
        c = rng.integers(0, 40, size=(n, 4)).astype(np.int32)
        c[:, 3] = rng.integers(0, 3, size=n)
        out['n%d' % n] = c
    out['all_equal'] = np.repeat(np.array([[9, 4, 7, 2]], dtype=np.int32), 1500, 0)
    out['sorted'] = G.downsample(rng.integers(0, 64, size=(3000, 4)).astype(np.int32), (1, 1, 1))
    hi = rng.integers(65000, 65536, size=(1200, 4)).astype(np.int32)
    hi[:, 3] = rng.integers(8185, 8192, size=1200)
    hi[:5] = [65535, 65535, 65535, 8191]
    hi[5] = [0, 65535, 0, 0]
    out['top_of_range'] = hi
    return out


@pytest.mark.parametrize('name', ['n1', 'n1023', 'n1024', 'n1025', 'all_equal', 'sorted', 'top_of_range'])
@pytest.mark.parametrize('ts', [1, 3, 8])
def test_spdownsample_and_pyramid_at_the_edges(name, ts):
    F = _F()
    c = _down_inputs()[name].copy()
    if name != 'top_of_range':
        c[:, :3] *= ts
    _eq(F.spdownsample(_g(c), 2, 2, ts), G.downsample(c, (2 * ts,) * 3))
    for levels in (1, 4):
        got = F.downsample_pyramid(_g(c), levels, ts)
        want = G.pyramid(c, levels, ts)
        assert len(got) == levels
        for a, b in zip(got, want):
            _eq(a, b)
    b15 = c.copy()
    b15[:, 3] = 32767 - (b15[:, 3] % 3)                         # the single downsampler takes 15 batch bits
    _eq(F.spdownsample(_g(b15), 2, 2, ts), G.downsample(b15, (2 * ts,) * 3))


@pytest.mark.parametrize('n,levels', [(256, 4), (257, 4), (341, 3), (342, 3), (1, 4), (512, 2), (513, 2)])
def test_pyramid_rows_times_levels_across_a_tile_edge(n, levels):
    F = _F()
    rng = np.random.default_rng(n)
    c = rng.integers(0, 200, size=(n, 4)).astype(np.int32) * np.array([8, 8, 8, 1], dtype=np.int32)
    c[:, 3] %= 2
    for a, b in zip(F.downsample_pyramid(_g(c), levels, 8), G.pyramid(c, levels, 8)):
        _eq(a, b)


@pytest.mark.parametrize('n', [1, 1023, 1024, 1025])
def test_unique_sorted_at_the_edges(n):
    F = _F()
    rng = np.random.default_rng(n)
    k = rng.integers(0, G.INT64_MAX, size=n, dtype=np.int64)
    k[n // 2:] = k[:n - n // 2]
    k[0] = G.INT64_MAX
    if n > 2:
        k[1] = 0
    _eq(F.unique_sorted(_g(k)), np.unique(k))
    _eq(F.unique_sorted(_g(np.sort(k))), np.unique(k))          # already sorted
    _eq(F.unique_sorted(_g(np.full(n, 42, dtype=np.int64))), [42])


def _row(x=0, y=0, z=0, b=0, n=700):
    rng = np.random.default_rng(9)
    c = rng.integers(0, 100, size=(n, 4)).astype(np.int32)
    c[:, 3] %= 2
    c[n // 2] = [x, y, z, b]
    return c


@pytest.mark.parametrize('bad', [dict(x=65536), dict(z=65536), dict(b=8192)])
def test_pyramid_refuses_what_its_key_cannot_hold(bad):
    with pytest.raises(ValueError, match='65536.*8192'):
        _F().downsample_pyramid(_g(_row(**bad)), 2, 1)


@pytest.mark.parametrize('bad', [dict(x=-1), dict(y=-2), dict(z=G.INT32_MIN), dict(y=65536), dict(z=1 << 20), dict(b=-1),
                                 dict(b=32768)])
def test_spdownsample_refuses_what_its_key_cannot_hold(bad):
    """Garbage was returned before: a negative coordinate was divided by truncation and sign-extended over the
    neighbouring key fields, 65536 or a batch id of 32768 spilled out of its field."""
    c = _row(**bad)
    with pytest.raises(ValueError, match='65536.*32768'):
        _F().spdownsample(_g(c), 2, 2, 1)
    with pytest.raises(ValueError, match='65536.*32768'):
        _conv().build_kernel_map(_g(np.unique(c, axis=0)), (1, 1, 1), (2, 2, 2), (2, 2, 2))
    ok = _row(x=65535, y=65535, z=65535, b=32767)
    _eq(_F().spdownsample(_g(ok), 2, 2, 1), G.downsample(ok, (2, 2, 2)))


@pytest.mark.parametrize('n,at', [(1, 0), (1025, 0), (1025, 1024), (3000, 1500)])
def test_unique_sorted_refuses_a_negative_key(n, at):
    k = np.random.default_rng(n).integers(0, G.INT64_MAX, size=n, dtype=np.int64)
    k[at] = -1 if n == 1 else G.INT64_MIN + at
    with pytest.raises(ValueError, match='2\\^63'):
        _F().unique_sorted(_g(k))


# ---------------------------------------------------------------- occupancy row order
def _random_table(K, n, seed, fill=0.4):
    rng = np.random.default_rng(seed)
    t = rng.integers(0, max(n, 1), size=(K, n)).astype(np.int32)
    t[rng.random((K, n)) > fill] = -1
    if n > 3:
        t[:, 1] = -1                                              # rows with no neighbour at all
        t[:, n - 1] = -1
    return t


def _check_order(order, nbr):
    """perm is a permutation; table == nbr[:, perm]; the restated key is non-decreasing along perm and ties keep
    ascending row order (which pins perm down completely); tile masks == OR of their 128 rows, no bit more or less."""
    n = nbr.shape[1]
    perm, table, tm = G.row_order(nbr)
    assert order.n_rows == n
    got = order.perm[:n].cpu().numpy()
    assert sorted(got.tolist()) == list(range(n))
    keys = G.row_keys(nbr)[got].astype(np.int64)
    assert (np.diff(keys) >= 0).all()
    tie = np.diff(keys) == 0
    assert (np.diff(got)[tie] > 0).all()
    _eq(order.perm[:n], perm)
    _eq(order.table, table)
    assert np.array_equal(order.tile_masks[:tm.size].cpu().numpy().view(np.uint32), tm)


ORDER_K = [1, 8, 27, 32]
ORDER_N = [0, 1, 127, 128, 129, 1025]


@pytest.mark.parametrize('K', ORDER_K)
@pytest.mark.parametrize('n', ORDER_N)
def test_row_order_of_random_tables(K, n):
    conv = _conv()
    for nbr in (_random_table(K, n, K * 7 + n), np.full((K, n), -1, dtype=np.int32)):
        _check_order(conv.RowOrder(_g(nbr)), nbr)
        if K == 32 and n:
            top = np.full((K, n), -1, dtype=np.int32)
            top[31, ::3] = 0                                      # bit 31 alone
            _check_order(conv.RowOrder(_g(top)), top)


@pytest.mark.parametrize('name,ks,st', [('rows_1025', (3, 3, 3), 1), ('batches8', (3, 3, 3), 1), ('rows_1023', (2, 2, 2), 2),
                                       ('aliased_ts1', (1, 3, 3), 1)])
def test_row_order_of_real_tables(name, ks, st):
    conv = _conv()
    m = G.case_map(name, ks, st)
    for nbr in (m.results, m.nbr_in):
        _check_order(conv.RowOrder(_g(nbr)), nbr)
    a, b = conv.RowOrder.build_many([_g(m.results), _g(m.nbr_in)])
    _check_order(a, m.results)
    _check_order(b, m.nbr_in)


@pytest.mark.parametrize('count', [2, 16, 17])
@pytest.mark.parametrize('K', [8, 27])
def test_build_many_equals_the_single_builds(count, K):
    conv = _conv()
    sizes = [129, 0, 1025, 1, 127, 128, 300, 2, 64, 257, 5, 1000, 130, 126, 3, 511, 640][:count]
    tabs = [_random_table(K, n, 100 * K + i) for i, n in enumerate(sizes)]
    many = conv.RowOrder.build_many([_g(t) for t in tabs])
    assert len(many) == count
    for o, t in zip(many, tabs):
        _check_order(o, t)
        one = conv.RowOrder(_g(t))
        n = t.shape[1]
        assert torch.equal(o.perm[:n], one.perm[:n]) and torch.equal(o.table, one.table)
        assert torch.equal(o.tile_masks[:-(-n // 128)], one.tile_masks[:-(-n // 128)])


def test_kmap_invert_of_a_non_symmetric_map():
    from lidal_amd import backend as B
    m = G.case_map('rows_1025', (2, 2, 2), 2)
    n_in, n_out = m.sizes
    assert n_in != n_out
    nbr_out = _g(m.results)
    t = torch.empty((8, n_in), dtype=torch.int, device=DEV)
    B.check(B.lib().lidal_kmap_invert(B.ptr(nbr_out), n_out, 8, B.ptr(t), n_in, B.stream()), 'kmap_invert')
    _eq(t, G.invert(m.results, n_in))
