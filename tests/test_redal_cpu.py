"""ReDAL region selection: the host side (select_redal, the k-means definition's numpy restatement, curvature files,
the C-ABI surface) against the reference's own outputs and scikit-learn's (tests/golden/make_golden_redal.py)."""
import os
import re

import numpy as np

import redal_inputs as RI
import redal_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fixture(golden_dir):
    return np.load(os.path.join(golden_dir, 'redal_small.npz'))


def test_select_redal_reproduces_reference_main(golden_dir):
    """ReDAL.py's __main__ on a 10-sequence Processing_files tree: given the cluster labels its KMeans produced,
    select_redal writes the same flags (importance decay, both argsorts, the first-overrun break)."""
    from lidal_amd.score.redal import select_redal
    g = _fixture(golden_dir)
    n = g['main_flags_in'].shape[0]
    flags = select_redal(g['main_flags_in'], g['main_sv_scores'], np.zeros((n, RI.FT_DIM), np.float32),
                         g['main_sv_pnums'], int(g['main_train_point_num']), labels=g['main_kmeans_labels'])
    assert np.array_equal(flags, g['main_flags_out'])
    new = (flags == 1).sum() - (g['main_flags_in'] == 1).sum()
    assert 0 < new < g['main_kmeans_labels'].size           # the 1 % point budget ran out inside the candidates
    assert set(np.unique(flags)) <= {0, 1}


def test_select_redal_leaves_input_untouched(golden_dir):
    from lidal_amd.score.redal import select_redal
    g = _fixture(golden_dir)
    flags_in, scores = g['main_flags_in'].copy(), g['main_sv_scores'].copy()
    select_redal(flags_in, scores, np.zeros((flags_in.size, RI.FT_DIM), np.float32), g['main_sv_pnums'],
                 int(g['main_train_point_num']), labels=g['main_kmeans_labels'])
    assert np.array_equal(flags_in, g['main_flags_in']) and np.array_equal(scores, g['main_sv_scores'])


def test_regenerated_inputs_match_fixture(golden_dir):
    g = _fixture(golden_dir)
    assert RI.sha256(RI.blobs()) == str(g['km_blobs_sha'])
    assert RI.sha256(RI.overlapping()) == str(g['km_overlap_sha'])
    frames = RI.worker_frames()
    assert RI.sha256(*[a for f in frames for a in (f['prob'], f['outfeat'], f['curvature'])],
                     *[p for f in frames for p in f['sv2point']]) == str(g['worker_inputs_sha'])


def test_kmeans_restatement_matches_sklearn_on_blobs(golden_dir):
    """The project's k-means definition (greedy k-means++, Lloyd, restarts), restated in numpy, splits the 150
    separable blobs exactly as sklearn.cluster.KMeans(150, random_state=0, n_init=10) did."""
    g = _fixture(golden_dir)
    labels, _ = redal_ref.kmeans(RI.blobs(), 150, random_state=0, n_init=10)
    assert redal_ref.same_partition(labels, g['km_blobs_labels'])
    assert len(np.unique(labels)) == 150


def test_scan_and_pairwise_restatement():
    """The restatement's building blocks: the chunked scan's total equals its last prefix, prefixes never decrease
    across chunk borders, and the written-out pairwise distance agrees with numpy's own row sum."""
    rs = np.random.RandomState(0)
    d = rs.uniform(0, 1, size=(2, 1000))
    pot, cs = redal_ref.scan(d)
    assert np.array_equal(pot, cs[:, -1]) and (np.diff(cs, axis=1) >= 0).all()
    assert np.allclose(pot, d.sum(1), rtol=1e-12)
    x = rs.normal(size=(50, 96))
    assert np.array_equal(redal_ref.d2(x, x[3]), ((x - x[3]) ** 2).sum(axis=1))


def test_curvature_files_round_trip(tmp_path):
    from lidal_amd import io
    curv = np.random.RandomState(1).uniform(0, 0.1, 1000).astype(np.float32)
    path = str(tmp_path / 'boundary' / '00' / '000000.npy')
    io.save_curvature(path, curv)
    back = io.load_curvature(path)
    assert back.dtype == np.float32 and np.array_equal(back, curv)
    np.save(path, curv.astype(np.float64))          # a file written in another width is read as ReDAL.py:57 reads it
    assert io.load_curvature(path).dtype == np.float32


def test_redal_symbols_declared_and_exported():
    from lidal_amd import backend as B
    header = open(os.path.join(ROOT, 'include', 'lidal_amd.h')).read()
    names = ['lidal_knn_workspace_bytes', 'lidal_knn', 'lidal_surface_variation', 'lidal_region_scores_workspace_bytes',
             'lidal_region_scores', 'lidal_kmeans_workspace_bytes', 'lidal_kmeans']
    for n in names:
        assert re.search(r'\b%s\(' % n, header), n
        assert n in B.SIGNATURES, n
        assert getattr(B.lib_handle(), n) is not None
    assert B.lib().lidal_version() >= 162
    assert B.lib().lidal_knn_workspace_bytes(1000) > 0
    assert B.lib().lidal_kmeans_workspace_bytes(1000, 96, 150, 7) > 0


def test_product_path_imports_no_sklearn_scipy_or_oracle():
    import subprocess
    import sys
    code = ('import sys; import lidal_amd.score, lidal_amd.score.redal, lidal_amd.io; '
            'bad = [m for m in sys.modules if m.split(".")[0] in ("sklearn", "scipy", "oracle")]; '
            'print(bad); sys.exit(1 if bad else 0)')
    r = subprocess.run([sys.executable, '-c', code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
