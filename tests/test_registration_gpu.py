"""Point-to-plane ICP on the GPU (lidal_amd/score/registration.py, csrc/icp.hip) against the numpy
restatement of icp_ref.py: the normals bit for bit, the sums of an iteration to the rigorous bound of a reordered f64
sum, the solve and the pose update bit for bit on the GPU's own sums, the stopping rules at their edges, and two
synthetic scans brought together end to end."""
import ctypes
import math

import numpy as np
import pytest
import torch

import icp_ref as R
from guarded_ws import Guarded

pytestmark = pytest.mark.gpu
DEV = 'cuda'
T = R.TRACE


def _g(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


# ---- the entry points themselves, outputs and scratch between guard bands ------------------------------------------------
def lib_normals(xyz, k, max_variation, cell=0.5):
    from lidal_amd import backend as B
    p = xyz.shape[0]
    g = Guarded()
    d_xyz = _g(xyz.astype(np.float32))
    out = g(p * 3 * 8).view(torch.float64).view(p, 3)
    nbytes = B.lib().lidal_point_normals_workspace_bytes(p, k)
    ws = g(nbytes)
    B.check(B.lib().lidal_point_normals(d_xyz.data_ptr(), p, k, cell, max_variation, out.data_ptr(), ws.data_ptr(), nbytes,
                                        B.stream()), 'point_normals')
    g.check()
    return out.cpu().numpy()


def build_grid(pts, cell):
    from lidal_amd import backend as B
    p = pts.shape[0]
    nbytes, ws_bytes = B.lib().lidal_nn_grid_bytes(p), B.lib().lidal_nn_grid_workspace_bytes(p)
    buf = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    B.check(B.lib().lidal_nn_grid_build(pts.data_ptr(), p, cell, buf.data_ptr(), nbytes, ws.data_ptr(), ws_bytes, B.stream()),
            'nn_grid_build')
    return buf


def lib_icp(src, tgt_pts, tgt_normals, pose, radii, stride=1, min_pairs=6, eps_rot=1e-6, eps_trans=1e-5, cell=None):
    """lidal_icp_run (numpy in, numpy out): (pose 4x4, trace [n_iters, 64])."""
    from lidal_amd import backend as B
    g = Guarded()
    d_src, d_pts, d_nrm = _g(src.astype(np.float32).reshape(-1, 3)), _g(tgt_pts.astype(np.float64)), _g(tgt_normals.astype(np.float64))
    grid = build_grid(d_pts, float(cell if cell is not None else max(radii)))
    n = len(radii)
    d_pose = g(16 * 8).view(torch.float64)
    d_pose.copy_(_g(np.asarray(pose, dtype=np.float64).reshape(16)))
    trace = g(n * T['width'] * 8).view(torch.float64).view(n, T['width'])
    nbytes = B.lib().lidal_icp_workspace_bytes(d_src.shape[0], stride)
    ws = g(nbytes)
    arr = (ctypes.c_double * n)(*radii)
    B.check(B.lib().lidal_icp_run(d_src.data_ptr(), d_src.shape[0], stride, grid.data_ptr(), d_pts.data_ptr(), d_nrm.data_ptr(),
                                  d_pts.shape[0], d_pose.data_ptr(), arr, n, min_pairs, eps_rot, eps_trans, trace.data_ptr(),
                                  ws.data_ptr(), nbytes, B.stream()), 'icp_run')
    g.check()
    return d_pose.cpu().numpy().reshape(4, 4), trace.cpu().numpy()


def _status(trace):
    return trace[:, T['status']].astype(int).tolist()


# ---- normals ---------------------------------------------------------------------------------------------------------------
def _cloud(seed=1, p=300):
    return np.random.default_rng(seed).uniform(-3.0, 3.0, (p, 3)).astype(np.float32) + np.float32(5.0)


@pytest.mark.parametrize('case', ['random', 'zeroed', 'plane', 'k_plus_1'])
def test_normals_equal_the_restatement_bit_for_bit(case):
    k = 10
    if case == 'random':                    # the variation never exceeds 1/3: every point keeps its normal
        xyz, max_variation = _cloud(), 1.0
    elif case == 'zeroed':
        xyz, max_variation = _cloud(), 0.12
    elif case == 'plane':                   # the ground 2 m under the sensor, exactly: variation 0
        xyz = _cloud(2)
        xyz[:, 2] = -2.0
        max_variation = 0.05
    else:
        xyz, max_variation = _cloud(3, k + 1), 1.0
    want = R.ref_normals(xyz, k, max_variation)
    got = lib_normals(xyz, k, max_variation)
    assert _same_bits(got, want)
    zero = (want == 0.0).all(1)
    facing = (want * xyz.astype(np.float64)).sum(1)
    assert (facing[~zero] <= 0.0).all() and np.abs(np.linalg.norm(want[~zero], axis=1) - 1.0).max() < 1e-12
    if case == 'random' or case == 'k_plus_1':
        assert not zero.any()
    elif case == 'zeroed':
        assert 20 < zero.sum() < 280                 # both kinds occur
        assert _same_bits(got[~zero], R.ref_normals(xyz, k, 1.0)[~zero])
    else:
        assert np.array_equal(want, np.tile([0.0, 0.0, 1.0], (300, 1)))
    assert _same_bits(lib_normals(xyz, k, max_variation, cell=1.7), got)          # the search cell does not matter
    from lidal_amd.score import point_normals
    assert _same_bits(point_normals(_g(xyz), k, max_variation).cpu().numpy(), got)


# ---- one iteration ---------------------------------------------------------------------------------------------------------
def _room(rng, p):
    """p points on a floor and two walls (1 cm of noise): normals everywhere but at the edges, all six motions held."""
    n = p // 3
    u = rng.uniform(0.0, 1.0, (p, 2))
    pts = np.empty((p, 3))
    pts[:n] = np.stack([2.0 + 8.0 * u[:n, 0], -4.0 + 8.0 * u[:n, 1], np.full(n, -1.5)], 1)
    pts[n:2 * n] = np.stack([np.full(n, 10.0), -4.0 + 8.0 * u[n:2 * n, 0], -1.5 + 4.0 * u[n:2 * n, 1]], 1)
    m = p - 2 * n
    pts[2 * n:] = np.stack([2.0 + 8.0 * u[2 * n:, 0], np.full(m, 4.0), -1.5 + 4.0 * u[2 * n:, 1]], 1)
    pts += rng.normal(0.0, 0.01, pts.shape)
    return rng.permutation(pts).astype(np.float32)


def _rigid(rx, ry, rz, t):
    cx, sx, cy, sy, cz, sz = math.cos(rx), math.sin(rx), math.cos(ry), math.sin(ry), math.cos(rz), math.sin(rz)
    m = np.eye(4)
    m[:3, :3] = (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1.0]]) @ np.array([[cy, 0, sy], [0, 1.0, 0], [-sy, 0, cy]]) @
                 np.array([[1.0, 0, 0], [0, cx, -sx], [0, sx, cx]]))
    m[:3, 3] = t
    return m


@pytest.fixture(scope='module')
def room():
    rng = np.random.default_rng(22)
    tgt32 = _room(rng, 600)
    tgt = tgt32.astype(np.float64)
    normals = R.ref_normals(tgt32, 10, 0.05)
    assert 400 < (normals != 0.0).any(1).sum() < 600
    move = _rigid(0.004, -0.003, 0.006, (0.03, -0.02, 0.015))            # source -> target
    inv = np.linalg.inv(move)
    src = ((tgt @ inv[:3, :3].T + inv[:3, 3]) + rng.normal(0.0, 0.005, tgt.shape)).astype(np.float32)
    return {'tgt32': tgt32, 'tgt': tgt, 'normals': normals, 'src': src, 'move': move}


@pytest.mark.parametrize('stride', [1, 3])
@pytest.mark.parametrize('p_src', [1, 255, 256, 257, 600])
def test_one_iteration_sums_within_the_bound_and_update_bit_for_bit(room, p_src, stride):
    src = room['src'][:p_src]
    init = _rigid(0.0, 0.0, 0.001, (0.005, 0.0, -0.004))
    pose, trace = lib_icp(src, room['tgt'], room['normals'], init, (1.0,), stride=stride)
    row = trace[0]
    terms = R.ref_terms(src, stride, init, room['tgt'], room['normals'], 1.0)
    n = terms.shape[0]
    assert row[T['pairs']] == float(n)                                   # the pair count is exact
    assert n >= (p_src + stride - 1) // stride * 0.6
    for q in range(29):
        exact = math.fsum(terms[:, q])
        bound = 2.0 * n * 2.0 ** -53 * math.fsum(np.abs(terms[:, q]))
        print('p_src %d stride %d sum %d: error %.3g, bound %.3g' % (p_src, stride, q, abs(row[q] - exact), bound))
        assert abs(row[q] - exact) <= bound, q
    status, xi, new_pose = R.ref_finish(row[:29], init, 6, 1e-6, 1e-5)
    assert status == (R.OK if n >= 6 else R.FEW_PAIRS)
    assert _status(trace) == [status]
    assert _same_bits(row[T['xi']:T['xi'] + 6], xi)
    assert _same_bits(pose, new_pose)
    assert _same_bits(row[T['pose']:T['pose'] + 16], init.reshape(16)) and row[T['max_dist']] == 1.0
    assert not row[53:].any()
    if n >= 6:
        assert not _same_bits(pose, init)
        # the step goes the right way: one iteration takes most of the 3 cm / 0.006 rad out
        before, after = R.pose_errors(init, room['move']), R.pose_errors(pose, room['move'])
        if p_src == 600 and stride == 1:
            assert after[0] < 0.4 * before[0] and after[1] < 0.4 * before[1]
    pose2, trace2 = lib_icp(src, room['tgt'], room['normals'], init, (1.0,), stride=stride)
    assert _same_bits(pose2, pose) and _same_bits(trace2, trace)         # a second run: the same bits everywhere
    pose3, trace3 = lib_icp(src, room['tgt'], room['normals'], init, (1.0,), stride=stride, cell=0.37)
    assert _same_bits(pose3, pose) and _same_bits(trace3, trace)         # and whatever the cell of the grid


# ---- edges -----------------------------------------------------------------------------------------------------------------
def test_no_match_and_no_normal_fail_and_leave_the_pose(room):
    init = _rigid(0.0, 0.0, 0.001, (0.005, 0.0, -0.004))
    far = room['src'] + np.float32(100.0)
    for src, normals in ((far, room['normals']), (room['src'], np.zeros_like(room['normals'])),
                         (np.zeros((0, 3), np.float32), room['normals'])):
        pose, trace = lib_icp(src, room['tgt'], normals, init, (1.0, 1.0, 0.5))
        assert _status(trace) == [R.FEW_PAIRS, R.AFTER_FAILURE, R.AFTER_FAILURE]
        assert _same_bits(pose, init)
        assert not trace[:, :T['status']].any()                              # no pair, no sum, no step
        for it in range(3):
            assert _same_bits(trace[it, T['pose']:T['pose'] + 16], init.reshape(16))
    # enough pairs for the solve, too few for the caller
    pose, trace = lib_icp(room['src'], room['tgt'], room['normals'], init, (1.0, 1.0), min_pairs=601)
    assert _status(trace) == [R.FEW_PAIRS, R.AFTER_FAILURE] and _same_bits(pose, init) and trace[0, T['pairs']] > 400


def test_nan_and_out_of_range_source_points_are_skipped(room):
    init = np.eye(4)
    base = room['src'].copy()
    base[[5, 300, 599]] = [[500.0, 0.0, 0.0], [0.0, -500.0, 0.0], [0.0, 0.0, 500.0]]        # matched by nothing
    bad = base.copy()
    bad[5] = [np.nan, 1.0, 2.0]
    bad[300] = [1e12, 0.0, 0.0]                                                             # beyond 2^20 cells of 1 m
    bad[599] = [0.0, -np.inf, 0.0]
    want = lib_icp(base, room['tgt'], room['normals'], init, (1.0, 0.5))
    got = lib_icp(bad, room['tgt'], room['normals'], init, (1.0, 0.5))
    assert _status(got[1]) == [R.OK, R.OK]
    assert _same_bits(got[0], want[0]) and _same_bits(got[1], want[1])
    assert got[1][0, T['pairs']] == float(R.ref_terms(bad, 1, init, room['tgt'], room['normals'], 1.0).shape[0])


def test_an_exact_plane_is_degenerate_and_leaves_the_pose():
    ij = np.stack(np.meshgrid(np.arange(20.0), np.arange(20.0), indexing='ij'), -1).reshape(-1, 2)
    tgt = np.concatenate([0.5 * ij + 1.0, np.zeros((400, 1))], 1)                 # z = 0
    normals = np.tile([0.0, 0.0, 1.0], (400, 1))
    src = tgt.astype(np.float32)
    src[:, :2] += np.float32(0.125)
    pose, trace = lib_icp(src, tgt, normals, np.eye(4), (1.0, 1.0))
    assert trace[0, T['pairs']] == 400.0
    assert _status(trace) == [R.DEGENERATE, R.AFTER_FAILURE]
    assert _same_bits(pose, np.eye(4)) and not trace[:, T['xi']:T['xi'] + 6].any()
    assert R.ref_finish(trace[0, :29], np.eye(4), 6, 1e-6, 1e-5)[0] == R.DEGENERATE
    assert trace[0, 11] == 0.0 and trace[0, 20] == 400.0                          # A[2][2] = 0: the pivot is exactly 0


def test_an_aligned_source_skips_the_rest_of_every_level(room):
    radii = (1.0, 1.0, 1.0, 0.5, 0.5, 0.2)
    pose, trace = lib_icp(room['tgt32'], room['tgt'], room['normals'], np.eye(4), radii)
    assert _status(trace) == [R.CONVERGED, R.SKIPPED, R.SKIPPED, R.CONVERGED, R.SKIPPED, R.CONVERGED]
    assert _same_bits(pose, np.eye(4))
    assert trace[:, T['max_dist']].tolist() == list(radii)
    for it in (1, 2, 4):
        assert not trace[it, :T['status']].any()
    for it in (0, 3, 5):
        assert trace[it, T['pairs']] > 400 and trace[it, T['rr']] == 0.0 and not trace[it, T['xi']:T['xi'] + 6].any()
    # the same through the restatement
    assert _status(R.ref_icp(room['tgt32'], room['tgt'], room['normals'], None, radii, min_pairs=6)[1]) == _status(trace)


# ---- end to end ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def scans():
    host, truth = R.make_scans(4)
    assert all(7500 < s.shape[0] < 8500 for s in host)
    return [_g(s) for s in host], truth


def test_two_scans_end_to_end(scans):
    """16 x 512 scans from (10, 0) and (11, 0.3), the second yawed by 2 degrees; identity start, default schedule.
    The restatement alone: 1.6 mm, 1.5e-4 (test_registration_cpu.py)."""
    from lidal_amd.score import IcpTarget, icp
    dev, truth = scans
    target = IcpTarget(dev[0])
    assert target.points.dtype == torch.float64 and target.normals.dtype == torch.float64 and len(target) == dev[0].shape[0]
    pose, trace = icp(dev[1], target)
    assert pose.is_cuda and pose.dtype == torch.float64 and tuple(pose.shape) == (4, 4)
    assert not trace.is_cuda and tuple(trace.shape) == (30, 64)
    dt, dr = R.pose_errors(pose.cpu().numpy(), truth[1])
    print('GPU: translation error %.3g m, rotation error %.3g' % (dt, dr))
    assert dt <= 0.01 and dr <= 5e-4
    status = trace[:, T['status']].to(torch.int64).tolist()
    assert R.SKIPPED in status and not set(status) & {R.FEW_PAIRS, R.DEGENERATE, R.AFTER_FAILURE}
    # without the read-back: the same run, the trace left on the GPU; and a subsampled source lands in the same place
    pose2, trace2 = icp(dev[1], target, check=False)
    assert trace2.is_cuda and torch.equal(pose2, pose) and torch.equal(trace2.cpu(), trace)
    pose4, _ = icp(dev[1], target, stride=4)
    dt4, dr4 = R.pose_errors(pose4.cpu().numpy(), truth[1])
    print('GPU, stride 4: translation error %.3g m, rotation error %.3g' % (dt4, dr4))
    assert dt4 <= 0.01 and dr4 <= 5e-4
    # a run that cannot work says so
    with pytest.raises(RuntimeError, match='too few pairs'):
        icp(dev[1] + 500.0, target)


def test_a_sequence_of_four_scans_and_the_products_that_ride_on_it(scans):
    from lidal_amd import data
    from lidal_amd.score import FrameBank, match_points, register_sequence
    dev, truth = scans
    poses, report = register_sequence(dev)
    assert poses.dtype == np.float64 and poses.shape == (4, 4, 4) and np.array_equal(poses[0], np.eye(4))
    assert len(report) == 3 and all(r['pairs'] > 1000 and 0.0 < r['rms'] < 0.1 and 1 <= r['iterations'] <= 30 for r in report)
    for f in range(4):
        dt, dr = R.pose_errors(poses[f], truth[f])
        print('frame %d: translation error %.3g m, rotation error %.3g' % (f, dt, dr))
    for f in range(4):
        dt, dr = R.pose_errors(poses[f], truth[f])
        assert dt <= 0.03 and dr <= 1e-3, f
    # refinement: coarse poses in, the same chain out
    coarse = [t.copy() for t in truth]
    for f in range(1, 4):
        coarse[f][:3, 3] += (0.2 * f, -0.1 * f, 0.0)
    refined, _ = register_sequence(dev, init_poses=coarse)
    for f in range(4):
        dt, dr = R.pose_errors(refined[f], truth[f])
        assert dt <= 0.03 and dr <= 1e-3, f
    bank = FrameBank(0.1)
    for f in range(4):
        bank.add(data.register_scan(dev[f], poses[f]))
    match = match_points(bank, 1, frames=[0, 2])
    assert match.dtype == torch.int32 and tuple(match.shape) == (2, dev[1].shape[0])
