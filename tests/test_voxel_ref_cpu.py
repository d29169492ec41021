"""The case builder of the exact point-voxel tests (tests/voxel_ref.py) checked without a GPU: every case reaches the
kernel form it names (asked of the library's own query), its operands meet the exactness precondition, the oracle does
not depend on the order of summation, and the scratch size follows the form."""
import numpy as np
import pytest
import torch

import voxel_ref as R

IDS = [R.case_id(c) for c in R.CASES]


@pytest.mark.parametrize('op', ['vox', 'devox'])
@pytest.mark.parametrize('case', R.CASES, ids=IDS)
def test_every_case_reaches_the_form_it_names(case, op):
    lay = R.layout(case, op)
    assert R.lib().lidal_segment_form(lay.n_entries, case.m, case.c, case.dtype) == case.form
    # the ladder is there, once each at least, and the exactness precondition holds for the longest list
    want = R.ladder(lay.rpw, case.form - 10 if case.form > 10 else 0) + ([R.BIG] if case.big else [])
    have = np.bincount(lay.lengths)
    assert all(have[n] >= 1 for n in want)
    assert 64 * 8 * int(lay.lengths.max()) < 2 ** 24
    if case.avg is not None:
        assert case.avg[0] <= lay.n_entries // case.m <= case.avg[1]


def test_each_form_is_reached_for_both_element_types():
    reached = {(c.form, c.dtype) for c in R.CASES}
    assert reached == {(f, d) for f in (R.GROUP, R.WAVE, R.WG1, R.WG2, R.WG4) for d in (R.F32, R.BF16)}
    assert sum(c.big for c in R.CASES if c.form == R.WAVE) >= 1 and sum(c.big for c in R.CASES if c.form > 10) >= 1
    for form, pair in R.SMALL.items():
        assert [c.form for c in pair] == [form, form] and [c.dtype for c in pair] == [R.F32, R.BF16]


def test_the_query_refuses_what_the_sums_refuse():
    q = R.lib().lidal_segment_form
    assert q(1000, 0, 32, R.F32) == -1 and q(1000, 10, 0, R.F32) == -1
    assert q(1000, 10, 6, R.F32) == -1 and q(1000, 10, 30, R.BF16) == -1           # channels: multiples of 4
    assert q(1000, 10, 256, R.F32) >= 0 and q(1000, 10, 260, R.F32) == -1          # 64 lanes of 4
    assert q(1000, 10, 512, R.BF16) >= 0 and q(1000, 10, 520, R.BF16) == -1        # 64 lanes of 8
    assert q(1000, 10, 260, R.BF16) == -1                                          # 4-element steps: 256 at most
    assert q(1000, 10, 32, 2) == -1


@pytest.mark.parametrize('op', ['vox', 'devox'])
@pytest.mark.parametrize('form', sorted(R.SMALL))
def test_the_oracle_does_not_depend_on_the_order(form, op):
    """f32 sums of the terms, entry by entry in three shuffled orders, equal the f64 reference bit for bit."""
    case = R.SMALL[form][0]
    ops = R.build_case(case, op)
    m, c = case.m, case.c
    if op == 'vox':
        ref = R.ref_voxelize(ops['rows'], ops['idx'], ops['counts'], m)
        idx = ops['idx'].numpy()
        e = np.nonzero((idx >= 0) & (idx < m))[0]
        v = idx[e]
        terms = ops['rows'].numpy()[e] / ops['counts'].numpy()[v].astype(np.float32)[:, None]
    else:
        ref = R.ref_devoxelize_bwd(ops['rows'], ops['idx'], ops['w'], m)
        idx, w = ops['idx'].numpy().reshape(-1), ops['w'].numpy().reshape(-1)
        e = np.nonzero((idx >= 0) & (idx < m) & (w != 0))[0]
        v = idx[e]
        terms = ops['rows'].numpy()[e >> 3] * w[e][:, None]
    assert terms.dtype == np.float32
    assert np.array_equal(np.bincount(v, minlength=m), R.layout(case, op).lengths)
    ref = ref.numpy()
    assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref)          # the exact sums are f32 numbers
    rng = np.random.default_rng(form)
    for _ in range(3):
        p = rng.permutation(len(e))
        out = np.zeros((m, c), dtype=np.float32)
        np.add.at(out, v[p], terms[p])
        assert out.dtype == np.float32 and np.array_equal(out.astype(np.float64), ref)


@pytest.mark.parametrize('dtype,c', R.CELLS)
def test_cell_cases_have_the_structure_the_cell_form_relies_on(dtype, c):
    ops = R.build_cells(dtype, c)
    idx8, points, m = ops['idx'].numpy(), ops['points'], ops['m']
    assert np.array_equal(np.bincount(idx8[:, 0], minlength=m), points)
    assert points[m - 1] == 0 and (points == 0).sum() >= 4
    lad = R.ladder(64 // (c // (4 if dtype == R.F32 else 8)), 1)
    assert set(lad) <= set(points.tolist())
    first = {}
    for i, row in enumerate(idx8):
        assert np.array_equal(idx8[first.setdefault(int(row[0]), i)], row)         # one corner row per cell
    assert (idx8 == -1).any() and (ops['w'].numpy() == 0).any() and idx8.max() < m


@pytest.mark.parametrize('case', R.CASES, ids=IDS)
def test_segment_workspace_follows_the_forms(case):
    """lidal_segment_workspace_bytes: zero exactly when neither element type takes more than one part, else the
    partial rows of the larger part count."""
    L = R.lib()
    for op in ('vox', 'devox'):
        ne = R.layout(case, op).n_entries
        for ne_ in (ne, ne + case.m, max(ne - case.m, 0), 1, 40 * case.m, 300 * case.m, 3000 * case.m):
            parts = max(max(L.lidal_segment_form(ne_, case.m, case.c, d) - 10, 0) for d in (R.F32, R.BF16))
            want = case.m * parts * case.c * 4 if parts > 1 else 0
            assert L.lidal_segment_workspace_bytes(ne_, case.m, case.c) == want, (ne_, parts)
    assert L.lidal_segment_workspace_bytes(1000, 0, case.c) == 0
