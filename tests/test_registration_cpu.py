"""The registration (lidal_amd/score/registration.py, csrc/icp.hip) without a GPU: the entry points
exist as documented and refuse every limit themselves before a device is touched, the Python functions raise their
argument errors, and the numpy restatement (icp_ref.py) alone meets the end-to-end condition of the GPU test."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import icp_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {'lidal_point_normals_workspace_bytes': 2, 'lidal_point_normals': 9, 'lidal_icp_workspace_bytes': 2,
       'lidal_icp_run': 17}


def test_entry_points_exist_with_the_documented_signatures():
    from lidal_amd import backend as B
    header = open(os.path.join(ROOT, 'include', 'lidal_amd.h')).read()
    handle = ctypes.CDLL(B.LIB_PATH)
    for name, n_args in NEW.items():
        assert hasattr(handle, name), name
        m = re.search(r'\b(?:int|int64_t)\s+%s\s*\(([^)]*)\)\s*;' % name, header)
        assert m is not None, name
        assert len([a for a in m.group(1).split(',') if a.strip()]) == n_args, name
        assert name in B.SIGNATURES and len(B.SIGNATURES[name][1]) == n_args, name
    consts = dict((k, int(v)) for k, v in re.findall(r'LIDAL_ICP_([A-Z_]+) = (\d+)', header))
    assert consts['TRACE'] == R.TRACE['width'] and consts['TRACE_XI'] == R.TRACE['xi']
    assert consts['TRACE_STATUS'] == R.TRACE['status'] and consts['TRACE_POSE'] == R.TRACE['pose']
    assert consts['TRACE_MAX_DIST'] == R.TRACE['max_dist'] and consts['TRACE_SUMS'] == 0
    assert [consts[k] for k in ('OK', 'CONVERGED', 'SKIPPED', 'FEW_PAIRS', 'DEGENERATE', 'AFTER_FAILURE')] == list(range(6))
    from lidal_amd.score import registration
    assert registration.TRACE == R.TRACE and len(registration.ICP_STATUS) == 6
    L = B.lib_handle()
    # the workgroups, and so the workspace, follow p_src and stride alone: 256 B of state + 256 B per workgroup
    assert L.lidal_icp_workspace_bytes(0, 1) == 512 and L.lidal_icp_workspace_bytes(256, 1) == 512
    assert L.lidal_icp_workspace_bytes(257, 1) == 768 and L.lidal_icp_workspace_bytes(769, 3) == 768
    assert L.lidal_icp_workspace_bytes(10 ** 7, 1) == 256 + 1024 * 256
    assert L.lidal_point_normals_workspace_bytes(300, 10) == -(-300 * 10 * 4 // 256) * 256 + L.lidal_knn_workspace_bytes(300)


def test_entry_points_refuse_every_limit_before_any_launch():
    """Host memory behind every pointer: a call that got past its LIDAL_REQUIREs would have to touch a device."""
    from lidal_amd import backend as B
    L = B.lib_handle()
    mem = (ctypes.c_double * 64)()
    a = ctypes.addressof(mem)
    good = (ctypes.c_double * 3)(1.0, 0.5, 0.5)

    def run(src=a, p_src=100, stride=1, grid=a, pts=a, nrm=a, p_tgt=100, pose=a, radii=good, n_iters=3, min_pairs=6,
            eps_rot=1e-6, eps_trans=1e-5, trace=a, ws=a, ws_bytes=1 << 20):
        rc = L.lidal_icp_run(src, p_src, stride, grid, pts, nrm, p_tgt, pose, radii, n_iters, min_pairs, eps_rot, eps_trans,
                             trace, ws, ws_bytes, None)
        return rc, L.lidal_last_error().decode()

    def radii(*v):
        return (ctypes.c_double * len(v))(*v)

    for kw, text in ((dict(stride=0), 'stride'), (dict(stride=-3), 'stride'),
                     (dict(n_iters=0), 'n_iters'), (dict(n_iters=257), 'n_iters'), (dict(n_iters=-1), 'n_iters'),
                     (dict(radii=radii(1.0, 0.0, 0.5)), r'max_dist[1]'), (dict(radii=radii(-1.0, 1.0, 1.0)), 'max_dist[0]'),
                     (dict(radii=radii(1.0, 1.0, float('nan'))), 'max_dist[2]'),
                     (dict(radii=radii(float('inf'), 1.0, 1.0)), 'max_dist[0]'), (dict(radii=None), 'max_dist_host'),
                     (dict(min_pairs=5), 'min_pairs'), (dict(min_pairs=0), 'min_pairs'),
                     (dict(p_src=-1), 'negative'), (dict(p_tgt=-1), 'negative'),
                     (dict(src=None), 'NULL'), (dict(grid=None), 'NULL'), (dict(pts=None), 'NULL'), (dict(nrm=None), 'NULL'),
                     (dict(pose=None), 'NULL'), (dict(trace=None), 'NULL'), (dict(ws=None), 'NULL'),
                     (dict(ws_bytes=511), 'workspace too small')):
        rc, err = run(**kw)
        assert rc == 2 and text in err, (kw, rc, err)

    def normals(xyz=a, p=300, k=10, cell=0.5, max_variation=0.05, out=a, ws=a, ws_bytes=1 << 30):
        rc = L.lidal_point_normals(xyz, p, k, cell, max_variation, out, ws, ws_bytes, None)
        return rc, L.lidal_last_error().decode()

    for kw, text in ((dict(p=10), 'need at least k + 1'), (dict(p=0), 'need at least k + 1'), (dict(k=0), 'k must be in 1..64'),
                     (dict(k=65, p=1000), 'k must be in 1..64'), (dict(cell=0.0), 'cell'),
                     (dict(max_variation=float('nan')), 'max_variation'), (dict(xyz=None), 'NULL'), (dict(out=None), 'NULL'),
                     (dict(ws=None), 'NULL'), (dict(ws_bytes=1000), 'workspace too small')):
        rc, err = normals(**kw)
        assert rc == 2 and text in err, (kw, rc, err)


def _host_target(p=50):
    """An IcpTarget of host tensors, filled behind __init__ (which takes GPU tensors only): argument errors come first."""
    from lidal_amd.score import IcpTarget
    t = IcpTarget.__new__(IcpTarget)
    t.cell, t._grid = None, None
    t.points = torch.zeros((p, 3), dtype=torch.float64)
    t.normals = torch.zeros((p, 3), dtype=torch.float64)
    return t


def test_icp_and_register_sequence_raise_their_argument_errors_before_the_device():
    from lidal_amd.score import IcpTarget, icp, point_normals, register_sequence
    src = torch.zeros((40, 3))
    tgt = _host_target()
    for kw, err, text in (
            (dict(source_points=np.zeros((4, 3))), TypeError, 'source_points'),
            (dict(source_points=torch.zeros((4, 4))), ValueError, 'source_points'),
            (dict(source_points=torch.zeros((4, 3), dtype=torch.int64)), TypeError, 'source_points'),
            (dict(target=torch.zeros((4, 3))), TypeError, 'IcpTarget'),
            (dict(init=np.eye(3)), ValueError, 'init'), (dict(init='pose'), TypeError, 'init'),
            (dict(init=np.full((4, 4), np.nan)), ValueError, 'init'),
            (dict(max_dist=1.0), TypeError, 'max_dist'), (dict(max_dist=()), ValueError, 'max_dist'),
            (dict(max_dist=(1.0,) * 257), ValueError, 'max_dist'), (dict(max_dist=(1.0, 0.0)), ValueError, 'max_dist'),
            (dict(max_dist=(1.0, float('inf'))), ValueError, 'max_dist'), (dict(max_dist=(1.0, float('nan'))), ValueError, 'max_dist'),
            (dict(max_dist=('1',)), TypeError, 'max_dist'),
            (dict(stride=0), ValueError, 'stride'), (dict(stride=1.5), TypeError, 'stride'),
            (dict(min_pairs=5), ValueError, 'min_pairs'), (dict(min_pairs=100.0), TypeError, 'min_pairs'),
            (dict(eps_rot=-1.0), ValueError, 'eps_rot'), (dict(eps_trans=float('nan')), ValueError, 'eps_trans'),
            (dict(eps_rot='small'), TypeError, 'eps_rot')):
        args = dict(source_points=src, target=tgt)
        args.update(kw)
        with pytest.raises(err, match=text):
            icp(**args)
    scans = [torch.zeros((30, 3))] * 3
    for kw, err, text in (
            (dict(scans=[]), ValueError, 'no scans'), (dict(scans=5), TypeError, 'scans'),
            (dict(scans=[scans[0], np.zeros((30, 3))]), TypeError, 'scan 1'),
            (dict(scans=[scans[0], torch.zeros((5, 3))]), ValueError, 'scan 1'),
            (dict(init_poses=[np.eye(4)] * 2), ValueError, 'init_poses'), (dict(init_poses=7), TypeError, 'init_poses'),
            (dict(init_poses=[np.eye(4), np.eye(3), np.eye(4)]), ValueError, r'init_poses\[1\]'),
            (dict(k=0), ValueError, 'k must be'), (dict(k=2.0), TypeError, 'k must be'),
            (dict(max_variation=float('nan')), ValueError, 'max_variation'),
            (dict(stride=0), ValueError, 'stride'), (dict(min_pairs=3), ValueError, 'min_pairs'),
            (dict(max_dist=(-1.0,)), ValueError, 'max_dist'), (dict(check=False), TypeError, 'unexpected'),
            (dict(radius=1.0), TypeError, 'unexpected')):
        args = dict(scans=scans)
        args.update(kw)
        with pytest.raises(err, match=text):
            register_sequence(**args)
    for kw, err, text in ((dict(k=65), ValueError, 'k must be'), (dict(k=10, points=torch.zeros((10, 3))), ValueError, 'k \\+ 1'),
                          (dict(max_variation='0.05'), TypeError, 'max_variation'), (dict(points=[[0.0] * 3] * 20), TypeError, 'points')):
        args = dict(points=torch.zeros((40, 3)))
        args.update(kw)
        with pytest.raises(err, match=text):
            point_normals(**args)
        with pytest.raises(err, match=text):
            IcpTarget(**args)
    with pytest.raises(ValueError, match='cell'):
        IcpTarget(torch.zeros((40, 3)), cell=0.0)
    # and past the argument checks, host tensors are refused like everywhere else: no CPU path
    with pytest.raises(RuntimeError, match='GPU only'):
        icp(src, tgt)
    with pytest.raises(RuntimeError, match='GPU only'):
        register_sequence(scans)
    with pytest.raises(RuntimeError, match='GPU only'):
        point_normals(torch.zeros((40, 3)))


def test_the_restatement_alone_meets_the_end_to_end_condition():
    """The two scans of the GPU test through icp_ref alone: identity start, default schedule, k = 10, max_variation 0.05.
    Measured when written: 1.6 mm in translation, 1.5e-4 in rotation (the bound: 1 cm, 5e-4)."""
    scans, truth = R.make_scans(2)
    assert all(7500 < s.shape[0] < 8500 for s in scans)
    normals = R.ref_normals(scans[0], 10, 0.05)
    zero = (normals == 0.0).all(1)
    assert 0.0 < zero.mean() < 0.2
    assert np.abs(np.linalg.norm(normals[~zero], axis=1) - 1.0).max() < 1e-12
    assert ((normals * scans[0].astype(np.float64)).sum(1) <= 0.0).all()           # every normal faces the sensor
    pose, trace = R.ref_icp(scans[1], scans[0].astype(np.float64), normals)
    status = trace[:, R.TRACE['status']].astype(int)
    assert not np.isin(status, (R.FEW_PAIRS, R.DEGENERATE, R.AFTER_FAILURE)).any()
    assert (status == R.SKIPPED).any() and status[20] == R.OK                       # a level converges early; the next runs
    dt, dr = R.pose_errors(pose, truth[1])
    print('restatement: translation error %.3g m, rotation error %.3g' % (dt, dr))
    assert dt <= 0.01 and dr <= 5e-4
    t0, r0 = R.pose_errors(np.eye(4), truth[1])
    assert t0 >= 1.0 and r0 >= 0.03                                                 # and the start was nowhere near
