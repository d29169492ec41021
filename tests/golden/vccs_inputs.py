"""Seeded inputs of the VCCS fixtures, shared by make_golden_vccs.py and the tests (regenerated, never stored twice:
the fixture keeps their sha256).  Each is the smallest cloud at which its path can still go wrong; all use the default
resolutions (voxel 0.5 m, seed 10 m: 35 rounds, more than 15.7 voxels within 5 m of a seed) unless they say otherwise."""
import hashlib

import numpy as np

from lidal_amd import synth

BATCH = ('ground_chain_row', 'flat_plane', 'three_collinear')       # three different fixtures in one call
SMALL = ('ground_chain_row', 'ground_wall', 'flat_plane', 'one_point', 'identical', 'two_points', 'faces_negative',
         'three_collinear')                                         # the CPU test runs the restatement on these
ALL = SMALL + ('scan_20k',)


def sha256(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def _grid(x0, x1, y0, y1, step):
    x, y = np.meshgrid(np.arange(x0, x1, step), np.arange(y0, y1, step), indexing='ij')
    return x.reshape(-1), y.reshape(-1)


def ground_chain_row():
    """A noisy 24 m x 24 m ground patch at 0.25 m spacing (supervoxels that steal voxels from one another), an 80-voxel
    chain of single points stepping (0.5, 0.5, 0.5) off its corner (its far end is beyond the reach of 35 rounds), and
    a detached row of 8 points 60 m away (its seed candidate sees 8 voxels, not more than 15.7)."""
    rng = np.random.RandomState(12)
    x, y = _grid(-12.0, 12.0, -12.0, 12.0, 0.25)
    ground = np.stack([x + rng.uniform(-0.05, 0.05, x.size), y + rng.uniform(-0.05, 0.05, x.size),
                       -1.7 + rng.normal(0.0, 0.04, x.size)], axis=1)
    i = np.arange(1, 81, dtype=np.float64)
    chain = np.stack([11.8 + 0.5 * i, 11.8 + 0.5 * i, -1.7 + 0.5 * i], axis=1)
    row = np.stack([72.25 + 0.5 * np.arange(8), np.full(8, 0.25), np.full(8, -1.75)], axis=1)
    pts = np.concatenate([ground, chain, row])
    return np.ascontiguousarray(pts[rng.permutation(len(pts))], dtype=np.float32), {}


def ground_wall():
    """Ground and a perpendicular wall rising from it, seed resolution 4 m (13 rounds): along the crease the normal term
    decides."""
    rng = np.random.RandomState(13)
    x, y = _grid(-8.0, 8.0, -8.0, 8.0, 0.25)
    ground = np.stack([x, y, -1.7 + rng.normal(0.0, 0.02, x.size)], axis=1)
    y2, z2 = _grid(-8.0, 8.0, -1.7, 6.3, 0.25)
    wall = np.stack([3.1 + rng.normal(0.0, 0.02, y2.size), y2, z2], axis=1)
    pts = np.concatenate([ground, wall])
    return np.ascontiguousarray(pts[rng.permutation(len(pts))], dtype=np.float32), dict(seed_resolution=4.0)


def flat_plane():
    """Exactly flat, grid aligned, 20 m x 20 m, one point per voxel centre: four seeds, four supervoxels of exactly 400
    voxels, and exact ties in D that the lower label takes."""
    x, y = _grid(-10.0, 10.0, -10.0, 10.0, 0.5)
    pts = np.stack([x + 0.25, y + 0.25, np.full(x.size, 0.25)], axis=1)
    return np.ascontiguousarray(pts, dtype=np.float32), {}


def degenerate():
    out = {}
    out['one_point'] = np.array([[1.0, 2.0, 3.0]], dtype=np.float32)
    out['identical'] = np.full((130, 3), -3.3, dtype=np.float32)
    out['two_points'] = np.array([[0.2, 0.2, 0.2], [0.7, 0.2, 0.2]], dtype=np.float32)
    # exactly on cell faces, and at negative coordinates: floor, not truncation (-0.25 is in cell -1, -0.5 opens -1)
    out['faces_negative'] = np.array([[-0.5, -0.25, 0.0], [-0.25, -0.5, -0.0], [0.0, 0.5, -0.5], [-1.0, -1.0, -1.0],
                                      [-0.75, 0.25, -1.25], [0.5, 0.0, 1.0], [-1.5, -0.5, 0.5], [0.49999997, -1e-7, 1e-7]],
                                     dtype=np.float32)
    # a voxel with 3 collinear neighbours: a rank-one covariance
    out['three_collinear'] = np.array([[0.25 + 0.5 * i, 0.25, 0.25] for i in range(4)], dtype=np.float32)
    return out


def scan_20k():
    """One raycast scan of the synthetic world, cut to about 20 k points."""
    world = synth.make_world(seed=31, length=200.0)
    pts, _ = synth.raycast_scan(world, (40.0, 0.0), np.random.default_rng(31), n_beams=16, n_az=1536)
    return np.ascontiguousarray(pts[:20000], dtype=np.float32), {}


def fixture(name):
    """(xyz f32 [P,3], keyword arguments of vccs_supervoxels)."""
    if name in ('ground_chain_row', 'ground_wall', 'flat_plane', 'scan_20k'):
        return globals()[name]()
    return degenerate()[name], {}
