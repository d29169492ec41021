"""tests/interframe_ref.py pinned on the CPU: against the reference's own scoring fixtures, against sklearn's KDTree on
the inputs whose matches the GPU tests demand exactly, and the range predicate of csrc/grid.h driven on the host."""
import math
import os
import subprocess

import numpy as np
import pytest

import interframe_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRANSLATION = np.array([1234.5, -2345.25, 17.0])


def _kdtree_query(query, pts):
    """The matching step of oracle/scoring_ref.py (LiDAL.py:63-66)."""
    from sklearn.neighbors import KDTree
    dists, nearest = KDTree(pts).query(query, k=1, return_distance=True, dualtree=False, breadth_first=False)
    return dists.reshape(-1), nearest.reshape(-1)


def test_restatement_reproduces_the_reference_fixtures(golden_dir):
    """tests/golden/scoring_small.npz holds outputs of the reference's own worker_func: the brute-force restatement gives
    the same per-point and per-supervoxel values as exactly as oracle.scoring_ref does (tests/test_oracle_cpu.py:
    array_equal), and the map_count that the KDTree matching yields."""
    from oracle import scoring_ref
    g = np.load(os.path.join(golden_dir, 'scoring_small.npz'))
    probs, worlds = list(g['probs']), list(g['worlds'])
    nei, dis = int(g['nei_num']), float(g['dis_thresh'])
    matched = 0
    for i in (0, 5, 13, 26):
        ids = scoring_ref.neighbour_ids(i, len(probs), nei)
        out = R.score_frame_points(i, probs, worlds, ids, dis)
        kd_count = np.zeros(worlds[i].shape[0], np.int64)
        for n, mine in zip(ids, out['ids']):
            dists, nearest = _kdtree_query(worlds[i], worlds[n])
            kd_count += dists <= dis
            assert np.array_equal(mine >= 0, dists <= dis)
        assert np.array_equal(out['map_count'], kd_count)
        matched += int(kd_count.sum())
        if i == 0:
            assert np.array_equal(out['interd'], g['interd_points_f0'])
            assert np.array_equal(out['intere'], g['intere_points_f0'])
        sv2point = list(g['sv2point'][i])
        sv_d = np.array([out['interd'][s].mean() for s in sv2point], np.float32)
        sv_e = np.array([out['intere'][s].mean() for s in sv2point], np.float32)
        assert np.array_equal(sv_d, g['sv_interds'][i]) and np.array_equal(sv_e, g['sv_interes'][i])
    assert matched > 200


@pytest.mark.parametrize('shift', [np.zeros(3), TRANSLATION], ids=['origin', 'kitti_scale'])
def test_lattice_matches_are_kdtrees_up_to_exact_ties(shift):
    """The lattice input of the GPU tests is well posed by the reference alone: brute force (d2, index) and KDTree agree
    on WHICH queries match, bit for bit on the distances, and pick a different point only where both are exactly as far.
    The input really has ties and really has pairs at the threshold on both sides of `<=`."""
    q, nb = R.lattice()
    if shift.any():                     # (-0.0 + 0.0 is +0.0: the untranslated lattice keeps its negative zeros)
        q, nb = q + shift, nb + shift
    dis = 0.1
    ids, d2 = R.match(q, nb, dis)
    dists, nearest = _kdtree_query(q, nb)
    assert np.array_equal(ids >= 0, dists <= dis)
    assert np.array_equal(np.sqrt(d2), dists)
    m = ids >= 0
    assert m.sum() > 10000 and (~m).sum() > 100
    differ = m & (ids != nearest)
    e = nb[nearest] - q
    d2_kd = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
    assert np.array_equal(d2_kd[differ], d2[differ])          # exact ties, every one
    assert np.all(ids[differ] < nearest[differ])              # ... and the restatement holds the lower index
    assert differ.sum() > 50
    close = np.abs(np.sqrt(d2) - dis) < 1e-12
    assert (close & m).sum() > 50 and (close & ~m).sum() > 20
    # cell faces: nodes exactly on multiples of 0.1 and 0.2, on the negative side too, and a negative zero
    if not shift.any():
        assert np.any(q[:, 0] == -0.2) and np.any(q[:, 0] == 0.2) and np.any(q[:, 1] == -0.1)
        assert np.any((q == 0) & np.signbit(q))


def test_nearest_prefers_the_lowest_index_and_ignores_nan():
    pts = np.array([[1.0, 0, 0], [0, 1.0, 0], [np.nan, 0, 0], [0, 1.0, 0], [np.inf, 0, 0]])
    idx, d2 = R.nearest(np.array([[0.0, 0, 0], [0, 0.9, 0], [np.nan, 0, 0], [np.inf, 0, 0], [1e300, 0, 0]]), pts)
    assert idx.tolist() == [0, 1, -1, -1, -1] and d2[0] == 1.0
    assert R.nearest(np.zeros((2, 3)), np.zeros((0, 3)))[0].tolist() == [-1, -1]


def _probed(q, r, cell):
    """The cell box that grid_nearest probes for the cube [q - r, q + r]: (lo, hi) as floor() gives them."""
    return np.floor((q - r) / cell), np.floor((q + r) / cell)


def test_margin_pairs_match_at_r_and_fall_off_a_cube_without_margin():
    """R.margin_pairs is well posed by the arithmetic alone: the first half matches at sqrt(d2) == r exactly, the second
    half misses by one ulp; the cube of r itself misses the neighbour's cell on the pair's axis, the cube of
    rr = r (1 + 1e-9) + 1e-12 that csrc/score.hip probes holds it.  No lattice or cloud input has such a pair: there the
    cube of r already holds every matched neighbour's cell (checked below on the lattice), so only this input tells
    whether the margin is there."""
    r, cell = 0.1, 0.05
    q, nb = R.margin_pairs(r, cell)
    half = nb.shape[0]
    assert q.shape[0] == 2 * half and half == 12
    ids, d2 = R.match(q, nb, r)
    assert np.array_equal(ids[:half], np.arange(half)) and np.all(ids[half:] == -1)
    assert np.all(np.sqrt(d2[:half]) == r)
    near, _ = R.nearest(q[half:], nb)
    assert np.array_equal(near, np.arange(half)) and np.all(np.sqrt(d2[half:]) == np.nextafter(r, 1.0))
    for grid_cell in (cell, cell / 2):                                       # FrameBank.CELL 0.5 and 0.25
        home = np.floor(nb / grid_cell)
        lo, hi = _probed(q[:half], r, grid_cell)
        assert np.all(((home < lo) | (home > hi)).sum(axis=1) == 1)          # off the cube of r, on the pair's own axis
        lo, hi = _probed(q[:half], r * (1.0 + 1e-9) + 1e-12, grid_cell)
        assert np.all((home >= lo) & (home <= hi))
    # the lattice does not tell: every matched neighbour's cell is inside the cube of r, at every cell size in use
    ql, nl = R.lattice()
    for shift in (np.zeros(3), TRANSLATION):
        j, _ = R.match(ql + shift, nl + shift, r)
        m = j >= 0
        for cells in (0.5, 1.0, 2.0, 3.0, 7.3):
            lo, hi = _probed((ql + shift)[m], r, cells * r)
            home = np.floor((nl + shift)[j[m]] / (cells * r))
            assert np.all((home >= lo) & (home <= hi))


_HOST_PROGRAM = r'''
#include <cstdio>
#include <cstdlib>
#include "grid.h"
int main(int argc, char** argv) {
  for (int i = 1; i + 1 < argc; i += 2) {
    const double v = strtod(argv[i], nullptr), cell = strtod(argv[i + 1], nullptr);
    printf("%d %lld\n", (int)lidal::grid::cell_in_range(floor(v / cell)), (long long)lidal::grid::cell_index(v, cell));
  }
  return 0;
}
'''


def test_grid_range_predicate_on_the_host(tmp_path):
    """csrc/grid.h's cell_in_range / cell_index, compiled for the host: NaN, +-Inf, +-1e300, +-0.0, and coordinates one
    cell inside and one cell outside +-2^20 cells, at cell 0.05 / 0.1 / 0.2.  Out of range gives the parking index
    -2^20, never a cast of an unrepresentable value."""
    src = tmp_path / 'range.cpp'
    src.write_text(_HOST_PROGRAM)
    exe = str(tmp_path / 'range')
    r = subprocess.run(['hipcc', '-x', 'hip', '--offload-host-only', '-O1', '-std=c++17', '-ffp-contract=off',
                        '-I', os.path.join(ROOT, 'lidal_amd', 'csrc'), str(src), '-o', exe],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    big = 1 << 20
    cases = []          # (v, cell, must be in range or None = as the host arithmetic says)
    for cell in (0.05, 0.1, 0.2):
        for v in (math.nan, math.inf, -math.inf, 1e300, -1e300, 3e5, -3e5, 2.0 ** 63 * cell, -2.0 ** 63 * cell,
                  (big + 1) * cell, -(big + 1) * cell, big * cell * 1.000001, 1.9e18 * cell):
            cases.append((v, cell, False))
        for v in (0.0, -0.0, 17.0, -2345.25, (big - 2) * cell, -(big - 2) * cell):
            cases.append((v, cell, True))
        for v in ((big - 1) * cell, -(big - 1) * cell, big * cell, -big * cell):
            cases.append((v, cell, None))
    argv = []
    for v, cell, _ in cases:
        argv += ['nan' if math.isnan(v) else ('inf' if v == math.inf else ('-inf' if v == -math.inf else v.hex())),
                 cell.hex()]
    out = subprocess.run([exe] + argv, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.split('\n')[:len(cases)]
    assert len(lines) == len(cases)
    for (v, cell, must), line in zip(cases, lines):
        ok, index = (int(t) for t in line.split())
        f = math.floor(v / cell) if math.isfinite(v) else None
        want = f is not None and -(big - 1) <= f <= big - 1
        if must is not None:
            assert want == must, (v, cell)
        assert bool(ok) == want, (v, cell, line)
        assert index == (f if want else -big), (v, cell, line)
    # +-0.0 are cell 0; 3e5 m is out of range at every cell size a 0.1 m radius uses
    assert (3e5 / 0.2) > big
