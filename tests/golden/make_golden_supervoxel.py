"""Generate tests/golden/supervoxel_small.npz on the CPU (numpy and scipy; no GPU, no reference code: the reference's
k_means_constrained dependency is not available, so the fixture pins this project's own definition).

  python tests/golden/make_golden_supervoxel.py

What the fixture pins
  assign_*     per assignment problem (supervoxel_inputs.ASSIGN_CASES and shaped_cases()): the labels and objective of
               the numpy restatement (tests/supervoxel_ref.py), its augmentation count, and the optimum of the
               transportation LP found independently by scipy.optimize.linprog(method='highs'); sha256 of the inputs
  frame_*      per raycast scan (about 2 k and 12 k points): the restatement's seeds, first labels, centres and final
               labels, both objectives with their LP optima, and (small scan only) both cost matrices
  full_*       one scan of about 130 k points: both objectives, augmentation counts and the CRC of the final labels of
               the restatement (no LP: HiGHS does not hold 2.6 M variables in reasonable time)
"""
import os
import sys
import time
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, 'tests'), HERE):
    sys.path.insert(0, p)

import supervoxel_inputs as SI  # noqa: E402
import supervoxel_ref as R  # noqa: E402


def _assign(out, name, xyz, centers, lo, hi):
    cost = R.costs(xyz, centers)
    labels, obj, aug = R.balanced_assign(cost, lo, hi)
    lp = R.lp_optimum(cost, lo, hi)
    assert obj == lp, (name, obj, lp)
    sizes = np.bincount(labels, minlength=cost.shape[1])
    assert sizes.min() >= lo and sizes.max() <= hi
    out['assign_%s_labels' % name] = labels.astype(np.int8)
    out['assign_%s_objective' % name] = np.int64(obj)
    out['assign_%s_lp' % name] = np.int64(lp)
    out['assign_%s_aug' % name] = np.int64(aug)
    out['assign_%s_bounds' % name] = np.array([lo, hi], dtype=np.int64)
    out['assign_%s_sha' % name] = SI.sha256(xyz, centers)
    print('assign %-14s P %5d K %2d [%d, %d]: objective %d = LP, %d augmentations' % (
        name, cost.shape[0], cost.shape[1], lo, hi, obj, aug))


def main():
    out = {}
    for i, (name, p, k) in enumerate(SI.ASSIGN_CASES):
        xyz, centers = SI.assign_case(p, k, 100 + i)
        _assign(out, name, xyz, centers, *R.bounds(p, k))
    for name, (xyz, centers, lo, hi) in SI.shaped_cases().items():
        _assign(out, name, xyz, centers, lo, hi)
    for name, beams, az in SI.FRAMES:
        xyz = SI.scan(beams, az)
        r = R.supervoxel_kmeans(xyz, 20, 0.05, 0)
        t0 = time.time()
        lp1, lp2 = R.lp_optimum(r['cost1'], r['lo'], r['hi']), R.lp_optimum(r['cost2'], r['lo'], r['hi'])
        assert (r['objective1'], r['objective2']) == (lp1, lp2)
        out['frame_%s_sha' % name] = SI.sha256(xyz)
        out['frame_%s_seeds' % name] = r['seeds']
        out['frame_%s_labels1' % name] = r['labels1'].astype(np.int8)
        out['frame_%s_centers' % name] = r['centers']
        out['frame_%s_labels' % name] = r['labels'].astype(np.int8)
        out['frame_%s_objectives' % name] = np.array([r['objective1'], r['objective2']], dtype=np.int64)
        out['frame_%s_lp' % name] = np.array([lp1, lp2], dtype=np.int64)
        out['frame_%s_aug' % name] = np.array(r['augmentations'], dtype=np.int64)
        if name == 'small':
            out['frame_small_cost1'], out['frame_small_cost2'] = r['cost1'], r['cost2']
        print('frame %-7s P %6d [%d, %d]: objectives %s = LP (%.0f s), augmentations %s' % (
            name, len(xyz), r['lo'], r['hi'], (r['objective1'], r['objective2']), time.time() - t0, r['augmentations']))
    xyz = SI.full_scan()
    t0 = time.time()
    r = R.supervoxel_kmeans(xyz, 20, 0.05, 0)
    out['full_sha'] = SI.sha256(xyz)
    out['full_objectives'] = np.array([r['objective1'], r['objective2']], dtype=np.int64)
    out['full_aug'] = np.array(r['augmentations'], dtype=np.int64)
    out['full_labels_crc'] = np.int64(zlib.crc32(r['labels'].astype(np.int8).tobytes()))
    print('full scan P %d [%d, %d]: objectives %s, augmentations %s, %.0f s of numpy' % (
        len(xyz), r['lo'], r['hi'], (r['objective1'], r['objective2']), r['augmentations'], time.time() - t0))
    path = os.path.join(HERE, 'supervoxel_small.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
