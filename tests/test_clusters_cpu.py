"""Euclidean clustering without a GPU: the numpy reference of tests/cluster_ref.py against scipy in f64, the header
against backend.SIGNATURES, the refusals and no-ops of lidal_euclidean_clusters (all before any launch) and the draw of
draw_instance_paste."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import cluster_ref as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {'lidal_euclidean_clusters_workspace_bytes': 2, 'lidal_euclidean_clusters': 17}


def test_the_reference_names_the_partition_of_scipy_in_f64():
    """query_pairs + connected_components per (scan, class) in f64 give the partition of the f32 reference: no pair of
    the scene lies within 1e-5 m of its tolerance (f32 rounding moves a distance of tens of metres' coordinates by
    about 1e-6), which the test asserts.  The scene has a component that min_points drops and one that spans more than
    two cells."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    from scipy.spatial import cKDTree
    xyz, ptr, lab = C.scene()
    assert 2500 <= len(xyz) <= 3500 and len(ptr) == 3
    tol = C.tolerance_table(C.SCENE_TOL)
    root = C.components(xyz, ptr, lab, tol)
    want = np.full(len(xyz), -1, dtype=np.int64)
    for s in range(2):
        for c, t in C.SCENE_TOL.items():
            rows = np.nonzero((lab == c) & (np.arange(len(xyz)) >= ptr[s]) & (np.arange(len(xyz)) < ptr[s + 1]))[0]
            tree = cKDTree(xyz[rows].astype(np.float64))
            pairs = tree.query_pairs(float(np.float32(t)), output_type='ndarray')
            near, far = tree.query_pairs(float(np.float32(t)) - 1e-5), tree.query_pairs(float(np.float32(t)) + 1e-5)
            assert len(near) == len(far) == len(pairs), 'a pair lies within 1e-5 m of the tolerance: pick another seed'
            graph = coo_matrix((np.ones(len(pairs)), (pairs[:, 0], pairs[:, 1])), shape=(len(rows), len(rows)))
            _, comp = connected_components(graph, directed=False)
            first = np.full(comp.max() + 1, len(xyz), dtype=np.int64)
            np.minimum.at(first, comp, rows)                       # a component is named by its smallest row
            want[rows] = first[comp]
    assert np.array_equal(root, want)
    assert (want[np.isin(lab, (0, 5))] == -1).all() and (want[np.isin(lab, (1, 2, 3, 4))] >= 0).all()
    sizes = np.bincount(root[root >= 0], minlength=len(xyz))
    assert ((sizes > 0) & (sizes < C.SCENE_MIN)).any(), 'no component for min_points to drop'
    cells = np.floor(xyz / 1.0).astype(np.int64)                    # the cell edge: the power of two above 0.7
    assert max(len(np.unique(cells[root == r], axis=0)) for r in np.nonzero(sizes >= C.SCENE_MIN)[0]) > 2
    ref = C.clusters_ref(xyz, ptr, lab, C.SCENE_TOL, C.SCENE_MIN, C.SCENE_MAX)
    k = len(ref['cls'])
    assert k >= 20 and ref['inst_ptr'][0] == 0 and ref['inst_ptr'][-1] == k and 0 < ref['inst_ptr'][1] < k
    assert (ref['sizes'] >= C.SCENE_MIN).all() and ref['members'].size == (ref['inst'] >= 0).sum()
    starts = ref['members'][ref['member_ptr'][:-1]]
    assert (np.diff(starts) > 0).all()                              # ids ascend with the smallest member row


def test_header_and_signatures_agree():
    from lidal_amd import backend as B
    header = open(os.path.join(ROOT, 'include', 'lidal_amd.h')).read()
    handle = ctypes.CDLL(B.LIB_PATH)
    for name, n_args in NEW.items():
        assert hasattr(handle, name), name
        m = re.search(r'\b(?:int|int64_t)\s+%s\s*\(([^)]*)\)\s*;' % name, header)
        assert m is not None, name
        assert len([a for a in m.group(1).split(',') if a.strip()]) == n_args, name
        assert name in B.SIGNATURES and len(B.SIGNATURES[name][1]) == n_args, name
    consts = dict((k, int(v)) for k, v in re.findall(r'LIDAL_CLUSTERS_([A-Z_]+) = (\d+)', header))
    assert consts == {'CELL_RANGE': 1, 'WALK': 2}
    from lidal_amd import data
    assert set(data._CLUSTER_ERRORS) == set(consts.values())


def _call(L, p, ptr, n_scans, tol, min_points=1, max_points=10, ws_bytes=None):
    ok = 0x10000                                                    # a fake device address: a launch would fault on it
    ptr_a = (ctypes.c_int64 * 40)(*ptr)
    tol_a = (ctypes.c_float * 64)(*tol)
    if ws_bytes is None:
        ws_bytes = L.lidal_euclidean_clusters_workspace_bytes(p, n_scans)
    return L.lidal_euclidean_clusters(None if p == 0 else ok, None, p, ctypes.addressof(ptr_a), n_scans,
                                      ctypes.addressof(tol_a), min_points, max_points, None, None, None, None, None, None,
                                      None, ws_bytes, None)


def test_refusals_come_before_any_launch():
    """No GPU here: a call that got as far as a launch or a copy would fail with another message."""
    from lidal_amd import backend as B
    L = B.lib()
    half = [0.5] * 64
    one = lambda v: [v] + [0.0] * 63
    need = L.lidal_euclidean_clusters_workspace_bytes(100, 2)
    assert need > 0 and L.lidal_euclidean_clusters_workspace_bytes(1000, 2) > need
    cases = [(dict(p=100, ptr=[0, 100], n_scans=0, tol=half), b'scans'),
             (dict(p=100, ptr=[0] + [100] * 33, n_scans=33, tol=half), b'scans'),
             (dict(p=100, ptr=[0, 40, 100], n_scans=2, tol=one(-0.5)), b'negative or NaN'),
             (dict(p=100, ptr=[0, 40, 100], n_scans=2, tol=one(float('nan'))), b'negative or NaN'),
             (dict(p=100, ptr=[0, 40, 100], n_scans=2, tol=[0.5] * 63 + [2.0 ** -11]), b'outside [2^-10, 2^10]'),
             (dict(p=100, ptr=[0, 40, 100], n_scans=2, tol=one(1025.0)), b'outside [2^-10, 2^10]'),
             (dict(p=100, ptr=[0, 40, 100], n_scans=2, tol=one(float('inf'))), b'outside [2^-10, 2^10]'),
             (dict(p=100, ptr=[0, 40, 100], n_scans=2, tol=half, min_points=0), b'min_points'),
             (dict(p=100, ptr=[0, 40, 100], n_scans=2, tol=half, min_points=5, max_points=4), b'min_points'),
             (dict(p=100, ptr=[0, 60, 40, 100], n_scans=3, tol=half), b'ascend'),
             (dict(p=100, ptr=[1, 40, 100], n_scans=2, tol=half), b'start at 0'),
             (dict(p=100, ptr=[0, 40, 99], n_scans=2, tol=half), b'end at p'),
             (dict(p=100, ptr=[0, 40, 101], n_scans=2, tol=half), b'end at p'),
             (dict(p=2 ** 30, ptr=[0, 2 ** 30], n_scans=1, tol=half), b'fewer than 2^30'),
             (dict(p=100, ptr=[0, 40, 100], n_scans=2, tol=half, ws_bytes=need - 1), b'workspace too small')]
    for kw, what in cases:
        assert _call(L, **kw) != 0, kw
        assert what in L.lidal_last_error(), (kw, L.lidal_last_error())


def test_nothing_to_cluster_is_a_clean_no_op():
    """p = 0, or a table without a positive tolerance: 0, and nothing launched (there is no device here to launch on)."""
    from lidal_amd import backend as B
    L = B.lib()
    assert _call(L, p=0, ptr=[0, 0, 0], n_scans=2, tol=[0.5] * 64) == 0
    assert _call(L, p=100, ptr=[0, 40, 100], n_scans=2, tol=[0.0] * 64) == 0
    # ... and the limits hold for them as well
    assert _call(L, p=0, ptr=[0, 0, 0], n_scans=2, tol=[0.5] * 64, min_points=0) != 0


def test_the_wrapper_refuses_before_the_device_is_touched():
    from lidal_amd import data
    x = torch.zeros((4, 3))
    for kw in (dict(tolerance=-1.0), dict(tolerance=float('nan')), dict(tolerance={3: 2000.0}), dict(tolerance={64: 0.5}),
               dict(tolerance=1e-4), dict(min_points=0), dict(min_points=3, max_points=2)):
        with pytest.raises(ValueError):
            data.euclidean_clusters(x, **kw)
    with pytest.raises(ValueError):
        data.euclidean_clusters([x] * 33)
    with pytest.raises(ValueError):
        data.euclidean_clusters(x, labels=torch.zeros(3, dtype=torch.int64))


class _CountingRng:
    """Stands in for a generator: records every call, answers choice with what it was told to."""

    def __init__(self, answer):
        self.calls, self.answer = [], answer

    def choice(self, n, size=None, replace=True):
        self.calls.append((n, size, replace))
        return np.asarray(self.answer)

    def __getattr__(self, name):
        raise AssertionError('draw_instance_paste called rng.%s' % name)


def _instances():
    """Two scans of 6 and 8 rows; ids 0, 1 in scan 0 (classes 1, 2), ids 2..5 in scan 1 (classes 2, 1, 3, 1)."""
    from lidal_amd.data import Instances
    inst = torch.tensor([0, -1, 1, 0, 1, -1, 2, 3, -1, 4, 5, 3, 5, 2], dtype=torch.int32)
    cls = torch.tensor([1, 2, 2, 1, 3, 1], dtype=torch.int32)
    members = torch.tensor([0, 3, 2, 4, 6, 13, 7, 11, 9, 10, 12], dtype=torch.int32)
    member_ptr = torch.tensor([0, 2, 4, 6, 8, 9, 11])
    return Instances(inst=inst, inst_ptr=np.array([0, 2, 6]), cls=cls, member_ptr=member_ptr, members=members,
                     bbox=torch.zeros((6, 6)), sizes=member_ptr[1:] - member_ptr[:-1], point_ptr=np.array([0, 6, 14]),
                     member_start=np.array([0, 4, 11]))


def test_draw_instance_paste_draws_once_among_the_candidates_in_id_order():
    from lidal_amd.data import draw_instance_paste
    ins = _instances()
    # scan 1, classes {1, 3}: the candidates are ids 3, 4, 5 in that order; the answer (2, 0) picks ids 5 and 3
    rng = _CountingRng([2, 0])
    mask = draw_instance_paste(ins, 1, rng, classes=(3, 1), n_inst=2)
    assert rng.calls == [(3, 2, False)]
    assert mask.dtype == torch.bool and mask.tolist() == [False, True, False, False, True, True, True, False]
    # more asked for than there are: every candidate, still one draw
    rng = _CountingRng([1, 0, 2])
    assert draw_instance_paste(ins, 1, rng, classes=(1, 3), n_inst=9).tolist() == \
        [False, True, False, True, True, True, True, False]
    assert rng.calls == [(3, 3, False)]
    # no candidates (no such class in the scan; no class asked for; nothing asked for): nothing is drawn
    for kw in (dict(classes=(3,), scan=0), dict(classes=(), scan=1), dict(classes=(1,), scan=1, n_inst=0)):
        rng = _CountingRng([0])
        scan = kw.pop('scan')
        mask = draw_instance_paste(ins, scan, rng, **kw)
        assert rng.calls == [] and not mask.any() and mask.numel() == (6, 8)[scan]
    # a real generator is left where a hand count says: one choice without replacement among 3, nothing else
    rng, twin = np.random.RandomState(11), np.random.RandomState(11)
    mask = draw_instance_paste(ins, 1, rng, classes=(1, 3), n_inst=1)
    picked = (3, 4, 5)[int(twin.choice(3, size=1, replace=False)[0])]
    assert mask.tolist() == (ins.inst[6:] == picked).tolist()
    assert rng.rand() == twin.rand()
    # as_csr: scan-local rows in the form train_labels takes
    ptr, rows = ins.as_csr(1)
    assert ptr.tolist() == [0, 2, 4, 5, 7] and rows.tolist() == [0, 7, 1, 5, 3, 4, 6] and rows.dtype == torch.int64
    ptr, rows = ins.as_csr(0)
    assert ptr.tolist() == [0, 2, 4] and rows.tolist() == [0, 3, 2, 4]
