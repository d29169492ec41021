"""Generate the ReDAL fixtures under tests/golden/.  Runs ONLY in the build container: it imports the reference's own
score/sv_level/ReDAL.py from /root/reference and runs it unchanged (nuscenes stubbed, as make_golden.py does), and it
needs scikit-learn and scipy; neither the reference nor those packages exist on the GPU box.

  python tests/golden/make_golden_redal.py

What each fixture pins
  redal_small.npz  worker_func outputs (sv_id, sv_scores, sv_feats, sv_pnums) on the seeded frames of
                   redal_inputs.worker_frames(); the flags ReDAL.py's __main__ writes in a temporary Processing_files
                   tree (10 sequences, 1 600 regions, sv_pnums.npy pre-written so that the 1 % point budget binds), with
                   the labels its sklearn KMeans produced and the scikit-learn version; sklearn
                   KMeans(150, random_state=0, n_init=10) labels and inertia on redal_inputs.blobs() and
                   .overlapping(); sha256 of every regenerated input.
  redal_sv.npz     a raycast scan (~20 k points) with the surface-variation restatement (scipy cKDTree, k + 1 neighbours
                   with the point itself dropped, f64 population covariance, eigvalsh), and the 52 nearest points
                   (the point itself first) of 300 sampled points with their distances.
"""
import os
import pickle
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = '/root/reference'
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import redal_inputs as RI  # noqa: E402

TRAIN_POINT_NUM = 2349559532       # ReDAL.py:104


def _stub_nuscenes(tmp):
    d = os.path.join(tmp, 'stubs', 'nuscenes', 'utils')
    os.makedirs(d)
    open(os.path.join(tmp, 'stubs', 'nuscenes', '__init__.py'), 'w').close()
    open(os.path.join(d, '__init__.py'), 'w').close()
    with open(os.path.join(d, 'splits.py'), 'w') as f:
        f.write('def create_splits_scenes():\n    return {"train": []}\n')
    return os.path.join(tmp, 'stubs')


def _write_frame(base, seq, i, f, sv_id, prob_dir, feat_dir):
    name = '%06d' % i
    for d in (prob_dir, feat_dir, 'boundary', 'super_voxel/VCCS'):
        os.makedirs(os.path.join(base, d, seq), exist_ok=True)
    paths = (os.path.join(base, prob_dir, seq, name + '.npy'), os.path.join(base, feat_dir, seq, name + '.npy'),
             os.path.join(base, 'boundary', seq, name + '.npy'),
             os.path.join(base, 'super_voxel/VCCS', seq, name + '.pickle'))
    np.save(paths[0], f['prob'])
    np.save(paths[1], f['outfeat'])
    np.save(paths[2], f['curvature'])
    with open(paths[3], 'wb') as fh:
        pickle.dump((sv_id, f['sv2point']), fh)
    return paths


def _import_redal(tmp):
    stubs = _stub_nuscenes(tmp)
    sys.path.insert(0, stubs)
    if REF not in sys.path:
        sys.path.insert(0, REF)
    import score.sv_level.ReDAL as R          # the reference file, unchanged
    return R, stubs


def make_worker(out):
    tmp = tempfile.mkdtemp()
    R, _ = _import_redal(tmp)
    frames = RI.worker_frames()
    base = os.path.join(tmp, 'Processing_files', 'SK')
    files = [_write_frame(base, '00', i, f, f['sv_id'], 'prob_map/SPVCNN/fr/0r', 'outfeat/SPVCNN/fr/0r')
             for i, f in enumerate(frames)]
    R.init_worker(False, '00', [p[0] for p in files], [p[1] for p in files], [p[2] for p in files],
                  [p[3] for p in files])
    ids, sc, ft, pn = [], [], [], []
    for i, f in enumerate(frames):
        sv_id, s, fe, n = R.worker_func(i)
        assert np.array_equal(sv_id, f['sv_id'])
        ids.append(sv_id), sc.append(s), ft.append(fe), pn.append(n)
    out.update(worker_sv_id=np.concatenate(ids), worker_sv_scores=np.concatenate(sc),
               worker_sv_feats=np.concatenate(ft), worker_sv_pnums=np.concatenate(pn).astype(np.int64),
               worker_inputs_sha=RI.sha256(*[a for f in frames for a in (f['prob'], f['outfeat'], f['curvature'])],
                                           *[p for f in frames for p in f['sv2point']]))
    print('worker_func: %d frames, %d regions, largest %d points' % (len(frames), len(out['worker_sv_id']),
                                                                     int(out['worker_sv_pnums'].max())))


_DRIVER = '''import runpy, sys
import numpy as np
import sklearn.cluster
_KMeans = sklearn.cluster.KMeans


class RecordingKMeans(_KMeans):
    """records labels_ of every fit; the fit itself is sklearn's"""
    def fit(self, X, y=None, sample_weight=None):
        r = super().fit(X, y=y, sample_weight=sample_weight)
        np.save(%r, self.labels_)
        return r


sklearn.cluster.KMeans = RecordingKMeans
sys.argv = ['ReDAL.py', '--dataset_name', 'SK', '--model_name', 'SPVCNN', '--r_id', '1']
runpy.run_module('score.sv_level.ReDAL', run_name='__main__', alter_sys=True)
'''


def make_main(out):
    import sklearn
    from lidal_amd.score.redal import select_redal
    tmp = tempfile.mkdtemp()
    R, stubs = _import_redal(tmp)
    base = os.path.join(tmp, 'Processing_files', 'SK')
    rng = np.random.RandomState(9)
    gid = 0
    all_flags, files = [], []
    for s_i, seq in enumerate(RI.MAIN_SEQS):
        os.makedirs(os.path.join(base, 'sv_flag/VCCS/0r', seq))
        for i, f in enumerate(RI.main_frames(s_i)):
            sv_id = np.arange(gid, gid + RI.MAIN_SV, dtype=np.int64)
            gid += RI.MAIN_SV
            files.append(_write_frame(base, seq, i, f, sv_id, 'prob_map/SPVCNN/fr/0r', 'outfeat/SPVCNN/fr/0r'))
            flags = (rng.random_sample(RI.MAIN_SV) < 0.03).astype(np.int64)
            np.save(os.path.join(base, 'sv_flag/VCCS/0r', seq, '%06d.npy' % i), flags)
            all_flags.append(flags)
    # the cached point counts (`sv_pre`): large enough that 1 % of 2 349 559 532 points runs out inside the candidates
    sv_pnums = rng.randint(100000, 600000, size=gid).astype(np.int64)
    np.save(os.path.join(base, 'super_voxel/VCCS/sv_pnums.npy'), sv_pnums)
    labels_path = os.path.join(tmp, 'kmeans_labels.npy')
    driver = os.path.join(tmp, 'run_redal.py')
    with open(driver, 'w') as fh:
        fh.write(_DRIVER % labels_path)
    env = dict(os.environ, PYTHONPATH=stubs + ':' + REF)
    r = subprocess.run([sys.executable, driver], cwd=tmp, env=env, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    flags_out = []
    for seq in RI.MAIN_SEQS:
        for i in range(RI.MAIN_FRAMES):
            flags_out.append(np.load(os.path.join(base, 'sv_flag/VCCS/SPVCNN/ReDAL/1r', seq, '%06d.npy' % i)))
    flags_out = np.concatenate(flags_out)
    labels = np.load(labels_path)
    # the scores __main__ gathered, recomputed with the same worker_func (sv_pre: three outputs)
    sv_scores = np.zeros(gid, dtype=np.float32)
    R.init_worker(True, '00', [p[0] for p in files], [p[1] for p in files], [p[2] for p in files],
                  [p[3] for p in files])
    for i in range(len(files)):
        sv_id, s, _ = R.worker_func(i)
        sv_scores[sv_id] = s
    flags_in = np.concatenate(all_flags)
    mine = select_redal(flags_in, sv_scores, np.zeros((gid, RI.FT_DIM), np.float32), sv_pnums, TRAIN_POINT_NUM,
                        labels=labels)
    assert np.array_equal(mine, flags_out), 'select_redal != reference __main__'
    out.update(main_flags_in=flags_in, main_flags_out=flags_out, main_sv_scores=sv_scores, main_sv_pnums=sv_pnums,
               main_kmeans_labels=labels.astype(np.int16), main_train_point_num=TRAIN_POINT_NUM,
               sklearn_version=sklearn.__version__)
    print('__main__: %d regions, %d unlabeled, %d clustered, %d newly labelled (sklearn %s)' % (
        gid, int((flags_in == 0).sum()), labels.size, int((flags_out == 1).sum() - (flags_in == 1).sum()),
        sklearn.__version__))


def make_kmeans(out):
    from sklearn.cluster import KMeans
    for name, x in (('blobs', RI.blobs()), ('overlap', RI.overlapping())):
        m = KMeans(n_clusters=150, random_state=0, n_init=10).fit(x)
        out['km_%s_sha' % name] = RI.sha256(x)
        out['km_%s_labels' % name] = m.labels_.astype(np.int16)
        out['km_%s_inertia' % name] = float(m.inertia_)
        print('sklearn KMeans on %s %s: inertia %.6g, %d iterations' % (name, x.shape, m.inertia_, m.n_iter_))


def make_sv():
    from scipy.spatial import cKDTree
    from lidal_amd import synth
    k = 50
    world = synth.make_world(seed=31, length=200.0)
    pts, _ = synth.raycast_scan(world, (40.0, 0.0), np.random.default_rng(31), n_beams=32, n_az=640)
    xyz = pts.astype(np.float32)
    x64 = xyz.astype(np.float64)
    dist, idx = cKDTree(x64).query(x64, k=k + 1)
    nb = np.empty((len(x64), k), dtype=np.int64)
    for i in range(len(x64)):                    # drop the point itself (the first column unless a duplicate ties it)
        row = idx[i]
        nb[i] = row[row != i][:k] if (row == i).any() else row[:k]
    q = x64[nb]                                   # [P, k, 3]
    c = q - q.mean(1, keepdims=True)
    cov = np.einsum('pki,pkj->pij', c, c) / k
    w = np.linalg.eigvalsh(cov)
    sigma = w[:, 0] / w.sum(1)
    sigma_clip = np.minimum(sigma, 0.1)
    sample = np.random.RandomState(5).choice(len(x64), size=300, replace=False)
    sdist, sidx = cKDTree(x64).query(x64[sample], k=k + 2)      # the point itself, its k neighbours, the next one
    np.savez_compressed(os.path.join(HERE, 'redal_sv.npz'), xyz=xyz, sigma=sigma_clip, sigma_raw=sigma, k=k,
                        sample=sample.astype(np.int32), sample_knn=sidx.astype(np.int32), sample_dist=sdist,
                        own_first=(sidx[:, 0] == sample).astype(np.int8))
    print('surface variation: %d points, sigma < 0.01 (planar) for %.0f %%, clipped for %.0f %%' % (
        len(xyz), 100 * (sigma < 0.01).mean(), 100 * (sigma > 0.1).mean()))


if __name__ == '__main__':
    out = {}
    make_worker(out)
    make_main(out)
    make_kmeans(out)
    np.savez_compressed(os.path.join(HERE, 'redal_small.npz'), **out)
    make_sv()
    for f in ('redal_small.npz', 'redal_sv.npz'):
        print(f, os.path.getsize(os.path.join(HERE, f)), 'bytes')
