"""Restatement of csrc/icp.hip (include/lidal_amd.h at lidal_point_normals and lidal_icp_run) in
numpy and Python floats: a brute-force nearest neighbour in f64 as in test_transfer_gpu.py, jacobi_ref.py for the
eigenvectors, and the Cholesky solve and quaternion update operation by operation.  Every product and sum is rounded on
its own, as in the kernels.  Also the synthetic scans the registration tests share."""
import math

import numpy as np

from jacobi_ref import jacobi3

TRACE = {'width': 64, 'sums': 0, 'rr': 27, 'pairs': 28, 'xi': 29, 'status': 35, 'max_dist': 36, 'pose': 37}
OK, CONVERGED, SKIPPED, FEW_PAIRS, DEGENERATE, AFTER_FAILURE = range(6)
DEFAULT_SCHEDULE = (1.0,) * 10 + (0.5,) * 10 + (0.2,) * 10


# ---- normals -------------------------------------------------------------------------------------------------------------
def ref_knn(xyz, k):
    """The k nearest OTHER points of every point, sorted by (d2, index); d2 = ((ex^2 + ey^2) + ez^2) in f64."""
    pts = xyz.astype(np.float64)
    p = pts.shape[0]
    out = np.empty((p, k), np.int64)
    for a in range(0, p, 256):
        q = pts[a:a + 256]
        d2 = np.square(pts[None, :, 0] - q[:, 0:1])
        d2 += np.square(pts[None, :, 1] - q[:, 1:2])
        d2 += np.square(pts[None, :, 2] - q[:, 2:3])
        d2[np.arange(len(q)), np.arange(a, a + len(q))] = np.inf
        out[a:a + 256] = np.argsort(d2, axis=1, kind='stable')[:, :k]
    return out


def ref_normal(nb, point, max_variation):
    """One normal from the neighbours nb [k][3] (Python floats, in neighbour order) of `point`."""
    k = len(nb)
    mx = my = mz = 0.0
    for x, y, z in nb:
        mx += x; my += y; mz += z
    inv = 1.0 / float(k)
    mx *= inv; my *= inv; mz *= inv
    a00 = a01 = a02 = a11 = a12 = a22 = 0.0
    for x, y, z in nb:
        dx, dy, dz = x - mx, y - my, z - mz
        a00 += dx * dx; a01 += dx * dy; a02 += dx * dz
        a11 += dy * dy; a12 += dy * dz; a22 += dz * dz
    a = [[a00 * inv, a01 * inv, a02 * inv], [a01 * inv, a11 * inv, a12 * inv], [a02 * inv, a12 * inv, a22 * inv]]
    e = jacobi3(a)
    lam = [a[0][0], a[1][1], a[2][2]]
    c, lmin = 0, lam[0]
    for j in (1, 2):
        if lam[j] < lmin:
            c, lmin = j, lam[j]
    n = [e[0][c], e[1][c], e[2][c]]
    total = lam[0] + lam[1] + lam[2]
    if total == 0.0:
        return [0.0, 0.0, 0.0]
    var = lmin / total
    facing = (n[0] * point[0] + n[1] * point[1]) + n[2] * point[2]
    if facing > 0.0:
        n = [-v for v in n]
    if not all(math.isfinite(v) for v in n + [var, facing]) or var > max_variation:
        return [0.0, 0.0, 0.0]
    return n


def ref_normals(xyz, k, max_variation):
    """normals f64 [p,3] of xyz f32 [p,3]."""
    pts = xyz.astype(np.float64)
    knn = ref_knn(xyz, k)
    out = np.empty((pts.shape[0], 3), np.float64)
    rows = pts.tolist()
    for i, nb in enumerate(knn.tolist()):
        out[i] = ref_normal([rows[j] for j in nb], rows[i], max_variation)
    return out


# ---- one iteration -------------------------------------------------------------------------------------------------------
def ref_transform(src, pose):
    """s = pose * src in f64, ((h0*P[j][0] + h1*P[j][1]) + h2*P[j][2]) + P[j][3]."""
    h = src.astype(np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        return np.stack([((h[:, 0] * pose[j, 0] + h[:, 1] * pose[j, 1]) + h[:, 2] * pose[j, 2]) + pose[j, 3]
                         for j in range(3)], axis=1)


def ref_nearest(q, pts, r):
    """Index of the nearest row of pts to every row of q with sqrt(d2) <= r (first minimum), else -1."""
    out = np.full(q.shape[0], -1, np.int64)
    if pts.shape[0] == 0:
        return out
    px, py, pz = (np.ascontiguousarray(pts[:, k])[None, :] for k in range(3))
    for a in range(0, q.shape[0], 256):
        qq = q[a:a + 256]
        with np.errstate(invalid='ignore', over='ignore'):
            d2 = np.square(px - qq[:, 0:1])
            d2 += np.square(py - qq[:, 1:2])
            d2 += np.square(pz - qq[:, 2:3])
        j = d2.argmin(1)
        best = d2[np.arange(len(qq)), j]
        ok = np.isfinite(qq).all(1) & np.isfinite(best)
        ok[ok] &= np.sqrt(best[ok]) <= r
        out[a:a + 256] = np.where(ok, j, -1)
    return out


def ref_terms(src, stride, pose, tgt_pts, tgt_normals, max_dist):
    """The 29 terms of every source point that takes part: f64 [pairs, 29], in source order."""
    s = ref_transform(src[::stride], pose)
    j = ref_nearest(s, tgt_pts, max_dist)
    ok = j >= 0
    ok[ok] &= (tgt_normals[j[ok]] != 0.0).any(1)
    s, n, t = s[ok], tgt_normals[j[ok]], tgt_pts[j[ok]]
    r = ((s[:, 0] - t[:, 0]) * n[:, 0] + (s[:, 1] - t[:, 1]) * n[:, 1]) + (s[:, 2] - t[:, 2]) * n[:, 2]
    J = [s[:, 1] * n[:, 2] - s[:, 2] * n[:, 1], s[:, 2] * n[:, 0] - s[:, 0] * n[:, 2], s[:, 0] * n[:, 1] - s[:, 1] * n[:, 0],
         n[:, 0], n[:, 1], n[:, 2]]
    cols = [J[u] * J[v] for u in range(6) for v in range(u, 6)] + [-(J[u] * r) for u in range(6)] + [r * r, np.ones_like(r)]
    return np.stack(cols, axis=1) if len(r) else np.zeros((0, 29))


def ref_finish(sums, pose, min_pairs, eps_rot, eps_trans):
    """(status, xi [6], new pose 4x4) from the 29 sums, operation by operation as icp_finish_kernel."""
    sums = [float(v) for v in sums]
    P = [[float(v) for v in row] for row in np.asarray(pose).reshape(4, 4)]
    A = [[0.0] * 6 for _ in range(6)]
    q = 0
    for u in range(6):
        for v in range(u, 6):
            A[u][v] = A[v][u] = sums[q]
            q += 1
    b = sums[21:27]
    zero = [0.0] * 6
    if not sums[28] >= float(min_pairs):
        return FEW_PAIRS, zero, np.array(P)
    dmax = max(A[u][u] for u in range(6)) if all(A[u][u] == A[u][u] for u in range(6)) else float('nan')
    floor = 1e-12 * dmax
    L = [[0.0] * 6 for _ in range(6)]
    for j in range(6):
        d = A[j][j]
        for k in range(j):
            d = d - L[j][k] * L[j][k]
        if not d > floor or not d < math.inf:
            return DEGENERATE, zero, np.array(P)
        L[j][j] = math.sqrt(d)
        for i in range(j + 1, 6):
            s = A[i][j]
            for k in range(j):
                s = s - L[i][k] * L[j][k]
            L[i][j] = s / L[j][j]
    y = [0.0] * 6
    for i in range(6):
        s = b[i]
        for k in range(i):
            s = s - L[i][k] * y[k]
        y[i] = s / L[i][i]
    xi = [0.0] * 6
    for i in range(5, -1, -1):
        s = y[i]
        for k in range(i + 1, 6):
            s = s - L[k][i] * xi[k]
        xi[i] = s / L[i][i]
    if not all(math.isfinite(v) for v in xi):
        return DEGENERATE, zero, np.array(P)
    qx, qy, qz = 0.5 * xi[0], 0.5 * xi[1], 0.5 * xi[2]
    nrm = math.sqrt(((1.0 + qx * qx) + qy * qy) + qz * qz)
    qw = 1.0 / nrm
    qx, qy, qz = qx / nrm, qy / nrm, qz / nrm
    xx, yy, zz = qx * qx, qy * qy, qz * qz
    xy, xz, yz = qx * qy, qx * qz, qy * qz
    wx, wy, wz = qw * qx, qw * qy, qw * qz
    R = [[1.0 - 2.0 * (yy + zz), 2.0 * (xy - wz), 2.0 * (xz + wy)],
         [2.0 * (xy + wz), 1.0 - 2.0 * (xx + zz), 2.0 * (yz - wx)],
         [2.0 * (xz - wy), 2.0 * (yz + wx), 1.0 - 2.0 * (xx + yy)]]
    N = [row[:] for row in P]
    for i in range(3):
        for j in range(4):
            N[i][j] = ((R[i][0] * P[0][j] + R[i][1] * P[1][j]) + R[i][2] * P[2][j]) + xi[3 + i] * P[3][j]
    rot = max(abs(xi[0]), abs(xi[1]), abs(xi[2]))
    tra = max(abs(xi[3]), abs(xi[4]), abs(xi[5]))
    return (CONVERGED if rot < eps_rot and tra < eps_trans else OK), xi, np.array(N)


def ref_icp(src, tgt_pts, tgt_normals, init=None, max_dist=DEFAULT_SCHEDULE, stride=1, min_pairs=100, eps_rot=1e-6,
            eps_trans=1e-5):
    """(pose 4x4, trace [n_iters, 64]) of lidal_icp_run; the sums of an iteration are math.fsum's (the kernel's order is
    its own: the sums agree to the bound of the GPU test, not bit for bit)."""
    pose = np.eye(4) if init is None else np.array(init, dtype=np.float64)
    trace = np.zeros((len(max_dist), TRACE['width']))
    failed, converged, level = False, None, 0
    for it, r in enumerate(max_dist):
        if it > 0 and max_dist[it] != max_dist[it - 1]:
            level = it
        row = trace[it]
        row[TRACE['max_dist']] = r
        row[TRACE['pose']:TRACE['pose'] + 16] = pose.reshape(16)
        if failed or converged == level:
            row[TRACE['status']] = AFTER_FAILURE if failed else SKIPPED
            continue
        terms = ref_terms(src, stride, pose, tgt_pts, tgt_normals, r)
        sums = [math.fsum(terms[:, q]) for q in range(29)]
        status, xi, pose = ref_finish(sums, pose, min_pairs, eps_rot, eps_trans)
        row[:29] = sums
        row[TRACE['xi']:TRACE['xi'] + 6] = xi
        row[TRACE['status']] = status
        failed = status in (FEW_PAIRS, DEGENERATE)
        if status == CONVERGED:
            converged = level
    return pose, trace


# ---- the scans of the end-to-end tests -----------------------------------------------------------------------------------
WORLD_SEED, BEAMS, AZIMUTHS, YAW_STEP = 7122, 16, 512, math.radians(2.0)


def rot_z(theta):
    c, s = math.cos(theta), math.sin(theta)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def make_scans(n_frames):
    """n_frames scans of synth's world (seed 7122), 16 beams x 512 azimuths, from (10 + f, 0.3 f), frame f expressed in
    a sensor frame yawed by 2 f degrees.  Returns ([points f32 [P,3]], [true pose 4x4 of frame f in frame 0's frame])."""
    from lidal_amd import synth
    world = synth.make_world(WORLD_SEED)
    scans, truth = [], []
    for f in range(n_frames):
        pts, _ = synth.raycast_scan(world, (10.0 + f, 0.3 * f), np.random.default_rng([WORLD_SEED, f]), n_beams=BEAMS,
                                    n_az=AZIMUTHS)
        rz = rot_z(YAW_STEP * f)
        scans.append(np.ascontiguousarray((pts.astype(np.float64) @ rz).astype(np.float32)))       # rows: Rz(-yaw) p
        t = np.eye(4)
        t[:3, :3] = rz
        t[:3, 3] = (float(f), 0.3 * f, 0.0)
        truth.append(t)
    return scans, truth


def pose_errors(pose, truth):
    """(largest translation entry error, largest rotation entry error)."""
    d = np.abs(np.asarray(pose) - truth)
    return float(d[:3, 3].max()), float(d[:3, :3].max())
