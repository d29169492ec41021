"""Seeded inputs of the supervoxel fixtures, shared by make_golden_supervoxel.py and the tests (regenerated, never
stored twice: the fixture keeps their sha256)."""
import hashlib

import numpy as np

from lidal_amd import synth

# (name, P, K): the assignment problems of tests/test_supervoxel_gpu.py, bounds of slack 0.05
ASSIGN_CASES = (('p20_k20', 20, 20), ('p44_k4', 44, 4), ('p400_k20', 400, 20), ('p777_k7', 777, 7),
                ('p1030_k20', 1030, 20), ('p3000_k20', 3000, 20))
FRAMES = (('small', 8, 256), ('medium', 16, 768))         # raycast scans: (name, beams, azimuth steps)
BATCH_EXTRA = (6, 200)                                     # a third scan for the batch test


def sha256(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def scan(n_beams, n_az, seed=31):
    world = synth.make_world(seed=seed, length=200.0)
    pts, _ = synth.raycast_scan(world, (40.0, 0.0), np.random.default_rng(seed), n_beams=n_beams, n_az=n_az)
    return np.ascontiguousarray(pts, dtype=np.float32)


def full_scan():
    """One scan of the benchmark's size (64 beams x 2048 azimuth steps, about 130 k points)."""
    return scan(64, 2048, seed=7122)


def assign_case(p, k, seed):
    """A flat point cloud and k centres that are not among its points: (xyz f32 [p,3], centres f64 [k,3])."""
    rng = np.random.RandomState(seed)
    xyz = (rng.randn(p, 3) * [20.0, 20.0, 1.0]).astype(np.float32)
    centers = rng.randn(k, 3) * [15.0, 15.0, 1.0]
    return xyz, centers


def clumps(sizes, seed, spread=1.0):
    """len(sizes) centres on a circle and sizes[c] points around centre c: the unconstrained cluster sizes are `sizes`."""
    rng = np.random.RandomState(seed)
    k = len(sizes)
    ang = 2 * np.pi * np.arange(k) / k
    centers = np.stack([40 * np.cos(ang), 40 * np.sin(ang), np.zeros(k)], axis=1)
    xyz = np.concatenate([centers[c] + rng.randn(n, 3) * spread for c, n in enumerate(sizes)]).astype(np.float32)
    perm = rng.permutation(len(xyz))
    return np.ascontiguousarray(xyz[perm]), centers


def shaped_cases():
    """name -> (xyz, centres, size_min, size_max)."""
    out = {}
    # every point nearest to centre 0: the largest excess, the longest paths
    rng = np.random.RandomState(3)
    xyz = (rng.randn(2000, 3) * 0.5).astype(np.float32)
    ang = 2 * np.pi * np.arange(19) / 19
    far = np.stack([60 + 5 * np.arange(19), 30 * np.cos(ang), 30 * np.sin(ang)], axis=1)
    out['one_centre'] = (xyz, np.concatenate([np.zeros((1, 3)), far]), 95, 105)
    # all points identical: every arc is a tie, zero-cost cycles
    out['identical'] = (np.full((600, 3), 1.25, dtype=np.float32),
                        np.random.RandomState(4).randn(20, 3) * 10, 28, 31)
    # size_min == size_max (slack 0, P a multiple of K)
    xyz, centers = assign_case(1200, 20, 5)
    out['exact_sizes'] = (xyz, centers, 60, 60)
    # the clamped sizes sum to less than P: the clusters -> sink arcs carry flow
    xyz, centers = clumps([30, 5, 5, 4], 6)
    out['sink_deficit'] = (xyz, centers, 10, 12)
    # ... and to more than P: the sink -> cluster arcs carry flow
    xyz, centers = clumps([14, 14, 14, 2], 7)
    out['sink_excess'] = (xyz, centers, 10, 15)
    return out
