"""Poses for sequences that have none: scan-to-scan point-to-plane ICP on the GPU.

The inter-frame scorer, the selection radius and the label / prediction carry all match points across frames at 0.1 m in
a world frame, and until here that frame came from a pose file (`data.parse_poses`, `data.register_scan`).  This module
makes the poses, or refines coarse ones:

  * `point_normals`: the normal of every point of a raw scan (k nearest other points, covariance, Jacobi), facing the
    sensor; (0,0,0) where the neighbourhood is no surface;
  * `IcpTarget`: a scan as something to register onto -- its f64 points, normals and one nearest-neighbour grid;
  * `icp`: `n_iters` iterations of point-to-plane ICP, enqueued without a read-back; the pose stays on the GPU;
  * `register_sequence`: frame i onto frame i - 1 along a sequence, the relative poses chained in f64 into the pose
    array `data.register_scan` and `FrameBank.add` take.

Odometry only: no loop closure, no robust kernel, moving objects are met by the distance gate alone.  The definitions
are this project's own (include/lidal_amd.h at lidal_icp_run); tests/icp_ref.py restates them in numpy.
"""
import ctypes
import math

import numpy as np
import torch

from .. import backend as B
from .redal import KNN_CELL, _xyz

__all__ = ['point_normals', 'IcpTarget', 'icp', 'register_sequence', 'ICP_STATUS', 'DEFAULT_SCHEDULE', 'TRACE']

MAX_ITERS = 256
MAX_K = 64
DEFAULT_SCHEDULE = (1.0,) * 10 + (0.5,) * 10 + (0.2,) * 10
# a trace row (f64 [64], include/lidal_amd.h LIDAL_ICP_TRACE_*): where its parts start
TRACE = {'width': 64, 'sums': 0, 'pairs': 28, 'rr': 27, 'xi': 29, 'status': 35, 'max_dist': 36, 'pose': 37}
ICP_STATUS = ('updated', 'converged', 'skipped', 'too few pairs', 'degenerate', 'after a failure')
_FAILED = (3, 4, 5)


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def _is_number(v):
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool)


def _check_points(points, what, name):
    if not isinstance(points, torch.Tensor):
        raise TypeError('%s: %s must be a tensor' % (what, name))
    if points.ndim != 2 or points.shape[1] != 3:
        raise ValueError('%s: %s must be a [P, 3] tensor, got %s' % (what, name, tuple(points.shape)))
    if not points.dtype.is_floating_point:
        raise TypeError('%s: %s must be a floating-point tensor' % (what, name))


def _check_normal_arguments(points, k, max_variation, what):
    _check_points(points, what, 'points')
    if not _is_int(k):
        raise TypeError('%s: k must be an int' % what)
    if not 1 <= k <= MAX_K:
        raise ValueError('%s: k must be in 1..%d, got %d' % (what, MAX_K, k))
    if not _is_number(max_variation):
        raise TypeError('%s: max_variation must be a number' % what)
    if math.isnan(float(max_variation)):
        raise ValueError('%s: max_variation is NaN' % what)
    if points.shape[0] < k + 1:
        raise ValueError('%s: %d points cannot have %d nearest other points (need at least k + 1)'
                         % (what, points.shape[0], k))


def point_normals(points, k=10, max_variation=0.05, cell=KNN_CELL):
    """Normals f64 [P,3] of a raw scan f32 [P,3] (GPU): the eigenvector of the smallest eigenvalue of the covariance of
    the k nearest other points, facing the sensor origin; (0,0,0) where the surface variation lambda_min / (l1 + l2 + l3)
    exceeds max_variation or nothing finite comes out.  cell: the search grid's cell (the normals do not depend on it)."""
    _check_normal_arguments(points, k, max_variation, 'point_normals')
    xyz = _xyz(points, cell)
    p = xyz.shape[0]
    out = torch.empty((p, 3), dtype=torch.float64, device=xyz.device)
    nbytes = B.lib().lidal_point_normals_workspace_bytes(p, int(k))
    ws = B.workspace(nbytes, xyz.device)
    B.check(B.lib().lidal_point_normals(B.ptr(xyz), p, int(k), float(cell), float(max_variation), B.ptr(out), B.ptr(ws),
                                        nbytes, B.stream()), 'point_normals')
    return out


class IcpTarget:
    """A scan to register onto: points f32 [P,3] (GPU, the scan's own sensor frame) -> .points f64 [P,3], .normals f64
    [P,3] (point_normals(points, k, max_variation)) and one grid of lidal_nn_grid_build, built at the first icp() that
    asks.  cell None: the largest max_dist of that first call; the answers do not depend on the cell."""

    def __init__(self, points, cell=None, k=10, max_variation=0.05):
        _check_normal_arguments(points, k, max_variation, 'IcpTarget')
        if cell is not None:
            if not _is_number(cell):
                raise TypeError('IcpTarget: cell must be a number or None')
            if not 0.0 < float(cell) < float('inf'):
                raise ValueError('IcpTarget: cell must be finite and positive, got %r' % (cell,))
        self.cell = None if cell is None else float(cell)
        self.normals = point_normals(points, k, max_variation)
        self.points = points.detach().to(torch.float64).contiguous()
        self._grid = None

    def __len__(self):
        return self.points.shape[0]

    def grid(self, max_dist):
        if self._grid is None:
            pts = self.points
            p = pts.shape[0]
            nbytes = B.lib().lidal_nn_grid_bytes(p)
            ws_bytes = B.lib().lidal_nn_grid_workspace_bytes(p)
            buf = torch.empty(nbytes, dtype=torch.uint8, device=pts.device)
            ws = B.workspace(ws_bytes, pts.device)
            B.check(B.lib().lidal_nn_grid_build(B.ptr(pts), p, self.cell if self.cell is not None else float(max_dist),
                                                B.ptr(buf), nbytes, B.ptr(ws), ws_bytes, B.stream()), 'nn_grid_build')
            self._grid = buf
        return self._grid


def _check_pose(pose, what, name):
    """A 4x4 pose as host f64, or the GPU tensor itself."""
    if isinstance(pose, torch.Tensor) and pose.is_cuda:
        if pose.dtype != torch.float64 or tuple(pose.shape) != (4, 4):
            raise ValueError('%s: %s must be a float64 [4, 4] tensor' % (what, name))
        return pose
    try:
        host = np.array(pose.cpu() if isinstance(pose, torch.Tensor) else pose, dtype=np.float64)
    except (TypeError, ValueError):
        raise TypeError('%s: %s must be a 4x4 array of numbers' % (what, name))
    if host.shape != (4, 4):
        raise ValueError('%s: %s must be 4x4, got %s' % (what, name, host.shape))
    if not np.isfinite(host).all():
        raise ValueError('%s: %s is not finite' % (what, name))
    return host


def _check_icp_arguments(max_dist, stride, min_pairs, eps_rot, eps_trans, what):
    try:
        schedule = [v for v in max_dist]
    except TypeError:
        raise TypeError('%s: max_dist must be a sequence of radii, one per iteration' % what)
    if not all(_is_number(v) for v in schedule):
        raise TypeError('%s: max_dist must hold numbers' % what)
    if not 1 <= len(schedule) <= MAX_ITERS:
        raise ValueError('%s: max_dist must hold 1..%d iterations, got %d' % (what, MAX_ITERS, len(schedule)))
    schedule = [float(v) for v in schedule]
    if not all(0.0 < v < float('inf') for v in schedule):
        raise ValueError('%s: every max_dist must be finite and positive' % what)
    if not _is_int(stride):
        raise TypeError('%s: stride must be an int' % what)
    if stride < 1:
        raise ValueError('%s: stride must be at least 1, got %d' % (what, stride))
    if not _is_int(min_pairs):
        raise TypeError('%s: min_pairs must be an int' % what)
    if min_pairs < 6:
        raise ValueError('%s: min_pairs must be at least 6, got %d' % (what, min_pairs))
    for name, v in (('eps_rot', eps_rot), ('eps_trans', eps_trans)):
        if not _is_number(v):
            raise TypeError('%s: %s must be a number' % (what, name))
        if not float(v) >= 0.0:
            raise ValueError('%s: %s must not be negative or NaN, got %r' % (what, name, v))
    return schedule


def icp(source_points, target, init=None, max_dist=DEFAULT_SCHEDULE, stride=1, min_pairs=100, eps_rot=1e-6,
        eps_trans=1e-5, check=True):
    """Point-to-plane ICP of source_points f32 [P,3] (GPU, sensor frame) onto `target` (an IcpTarget): the pose that
    takes source coordinates into the target's frame.  init: the starting estimate (4x4, host or GPU f64; default the
    identity).  max_dist: the match radius of every iteration; once an update is below eps_rot (radians, about) and
    eps_trans (metres) the rest of the run of equal radii is skipped.  Every stride-th source point takes part.
    Returns (pose f64 [4,4] on the GPU, trace f64 [n_iters, 64]: TRACE, ICP_STATUS).  check=True reads the trace back
    (the one synchronisation; the trace returned is the host copy) and raises RuntimeError when the run failed: fewer
    than min_pairs pairs, or normal equations that do not determine the pose.  check=False returns at once, the trace on
    the GPU."""
    what = 'icp'
    _check_points(source_points, what, 'source_points')
    if not isinstance(target, IcpTarget):
        raise TypeError('%s: target must be an IcpTarget' % what)
    schedule = _check_icp_arguments(max_dist, stride, min_pairs, eps_rot, eps_trans, what)
    start = _check_pose(init, what, 'init') if init is not None else np.eye(4)
    B.require_gpu(source_points, target.points)
    src = source_points.detach().float().contiguous()
    dev = src.device
    if isinstance(start, torch.Tensor):
        B.require_gpu(start)
        pose = start.detach().clone().contiguous()
    else:
        pose = torch.from_numpy(np.ascontiguousarray(start)).to(dev)
    n = len(schedule)
    trace = torch.empty((n, TRACE['width']), dtype=torch.float64, device=dev)
    radii = (ctypes.c_double * n)(*schedule)
    p = src.shape[0]
    nbytes = B.lib().lidal_icp_workspace_bytes(p, int(stride))
    grid = target.grid(max(schedule))
    ws = B.workspace(nbytes, dev)
    B.check(B.lib().lidal_icp_run(B.ptr(src), p, int(stride), B.ptr(grid), B.ptr(target.points), B.ptr(target.normals),
                                  len(target), B.ptr(pose), radii, n, int(min_pairs), float(eps_rot), float(eps_trans),
                                  B.ptr(trace), B.ptr(ws), nbytes, B.stream()), 'icp_run')
    if not check:
        return pose, trace
    host = trace.cpu()
    status = host[:, TRACE['status']].to(torch.int64).tolist()
    for it, st in enumerate(status):
        if st in _FAILED:
            raise RuntimeError('icp: iteration %d (max_dist %g) failed: %s (%d pairs, min_pairs %d)'
                               % (it, schedule[it], ICP_STATUS[st], int(host[it, TRACE['pairs']]), min_pairs))
    return pose, host


def _report(trace):
    """pairs and rms residual of the last iteration that ran (as it found them), and how many ran."""
    status = trace[:, TRACE['status']].to(torch.int64).tolist()
    ran = [it for it, st in enumerate(status) if st in (0, 1)]
    last = ran[-1]
    pairs = int(trace[last, TRACE['pairs']])
    return {'pairs': pairs, 'rms': math.sqrt(float(trace[last, TRACE['rr']]) / pairs), 'iterations': len(ran)}


def register_sequence(scans, init_poses=None, k=10, max_variation=0.05, **icp_args):
    """World poses of a sequence of scans (f32 [P,3] GPU tensors, sensor frames) by registering frame i onto frame i - 1.
    init_poses None: every pair starts from the previous pair's relative pose (constant velocity; the first from the
    identity).  init_poses [F] 4x4: the relative poses they imply are the starting estimates -- pose refinement.  The
    relative poses are chained in f64 on the host: world_i = world_{i-1} * relative_i, frame 0 at init_poses[0] or the
    identity.  icp_args: max_dist, stride, min_pairs, eps_rot, eps_trans of icp().
    Returns (poses f64 [F,4,4] numpy -- what data.register_scan takes --, report: one {'pairs', 'rms', 'iterations'}
    per pair).  Odometry: the error accumulates along the chain."""
    what = 'register_sequence'
    try:
        scans = list(scans)
    except TypeError:
        raise TypeError('%s: scans must be a sequence of [P, 3] tensors' % what)
    if not scans:
        raise ValueError('%s: no scans' % what)
    for f, s in enumerate(scans):
        _check_normal_arguments(s, k, max_variation, '%s: scan %d' % (what, f))
    unknown = set(icp_args) - {'max_dist', 'stride', 'min_pairs', 'eps_rot', 'eps_trans'}
    if unknown:
        raise TypeError('%s: unexpected arguments %s' % (what, sorted(unknown)))
    _check_icp_arguments(icp_args.get('max_dist', DEFAULT_SCHEDULE), icp_args.get('stride', 1),
                         icp_args.get('min_pairs', 100), icp_args.get('eps_rot', 1e-6), icp_args.get('eps_trans', 1e-5),
                         what)
    starts = None
    if init_poses is not None:
        try:
            init_poses = list(init_poses)
        except TypeError:
            raise TypeError('%s: init_poses must be a sequence of 4x4 poses' % what)
        if len(init_poses) != len(scans):
            raise ValueError('%s: %d init_poses for %d scans' % (what, len(init_poses), len(scans)))
        starts = []
        for f, m in enumerate(init_poses):
            m = _check_pose(m, what, 'init_poses[%d]' % f)
            starts.append(m.cpu().numpy() if isinstance(m, torch.Tensor) else m)
    B.require_gpu(*scans)
    poses = np.empty((len(scans), 4, 4), np.float64)
    poses[0] = starts[0] if starts is not None else np.eye(4)
    report = []
    rel = np.eye(4)
    for f in range(1, len(scans)):
        target = IcpTarget(scans[f - 1], k=k, max_variation=max_variation)
        if starts is not None:
            rel = np.linalg.solve(starts[f - 1], starts[f])
        try:
            pose, trace = icp(scans[f], target, init=rel, **icp_args)
        except RuntimeError as e:
            raise RuntimeError('%s: frame %d onto frame %d: %s' % (what, f, f - 1, e))
        rel = pose.cpu().numpy()
        poses[f] = np.matmul(poses[f - 1], rel)
        report.append(_report(trace))
    return poses, report
