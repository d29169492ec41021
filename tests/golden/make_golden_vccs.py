"""Writes tests/golden/vccs_small.npz from the numpy restatement (tests/vccs_ref.py) of DESIGN.md section 12:

  python tests/golden/make_golden_vccs.py

Per fixture of vccs_inputs.ALL: the sha256 of the input, labels, seed voxels, voxel owners, the number of voxels, the
restatement's counts of steals and ties, and the mask of the voxels within `rounds` adjacency steps of a seed voxel --
taken with scipy.sparse.csgraph, which shares nothing with the restatement's rounds.  The GPU tests read only this file.
"""
import os
import sys

import numpy as np
from scipy import sparse
from scipy.sparse import csgraph

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE), HERE]

import vccs_inputs as VI     # noqa: E402
import vccs_ref as R         # noqa: E402


def ball(nbr, seed_voxels, rounds):
    v = nbr.shape[1]
    if len(seed_voxels) == 0:
        return np.zeros(v, dtype=bool)
    rows = np.tile(np.arange(v), 27)
    cols = nbr.reshape(-1)
    ok = cols >= 0
    graph = sparse.csr_matrix((np.ones(int(ok.sum())), (rows[ok], cols[ok])), shape=(v, v))
    steps = csgraph.dijkstra(graph, unweighted=True, indices=np.asarray(seed_voxels), min_only=True)
    return steps <= rounds


def main():
    out = {}
    for name in VI.ALL:
        xyz, kw = VI.fixture(name)
        r = R.vccs(xyz, **kw)
        mask = ball(r['nbr'], r['seed_voxels'], r['rounds'])
        out[name + '_sha'] = VI.sha256(xyz)
        out[name + '_labels'] = r['labels'].astype(np.int32)
        out[name + '_seed_voxels'] = r['seed_voxels'].astype(np.int32)
        out[name + '_owners'] = r['owners'].astype(np.int32)
        out[name + '_ball'] = np.packbits(mask)
        out[name + '_stats'] = np.array([len(r['owners']), r['steals'], r['ties'], r['rounds']], dtype=np.int64)
        unl = r['owners'] == 0
        print('%-18s P %6d V %6d seeds %3d steals %5d ties %5d unlabelled voxels %4d points at 0: %d  ball==labelled %s'
              % (name, len(xyz), len(r['owners']), len(r['seed_voxels']), r['steals'], r['ties'], int(unl.sum()),
                 int((r['labels'] == 0).sum()), bool((mask == ~unl).all())))
    path = os.path.join(HERE, 'vccs_small.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
