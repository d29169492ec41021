"""Generate the frame-level fixtures under tests/golden/.  Runs ONLY in the build container: it imports the reference's
own score/frame_level/*.py from /root/reference and runs them unchanged (nuscenes stubbed, as make_golden_redal.py
does), and it needs scipy and scikit-learn; neither the reference nor those packages exist on the GPU box.

  python tests/golden/make_golden_frame.py

frame_small.npz pins
  worker_*        worker_func of softmax_entropy.py, margin_sampling.py, least_confidence_sampling.py and
                  segment_entropy.py on frame_inputs.worker_frame(k) for every size of WORKER_SIZES, and segment_entropy
                  on frame_inputs.empty_sv_frame() (NaN)
  main_*          the flags each __main__ (ENT, MAR, CONF, SEGENT, RAND with np.random.seed(RAND_SEED)) writes in a
                  temporary Processing_files tree of 10 sequences x 30 frames (num_add = 3), the per-frame scores, and
                  this host's np.argpartition on the zero half (the flags rest on it: DESIGN.md section 9)
  cset_*          core_set.py's flags on 10 x 200 frames (num_add = 20); the generator reseeds until the relative gap
                  between the chosen and the next candidate exceeds 1e-5 at every step
  *_sha, versions sha256 of every regenerated input, the scipy and scikit-learn versions
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
sys.path.insert(0, os.path.dirname(HERE))

import frame_inputs as FI  # noqa: E402
import frame_ref  # noqa: E402

RAND_SEED = 11
MODULES = {'ENT': 'softmax_entropy', 'MAR': 'margin_sampling', 'CONF': 'least_confidence_sampling',
           'SEGENT': 'segment_entropy', 'CSET': 'core_set', 'RAND': 'RAND'}


def _stub_nuscenes(tmp):
    d = os.path.join(tmp, 'stubs', 'nuscenes', 'utils')
    os.makedirs(d)
    open(os.path.join(tmp, 'stubs', 'nuscenes', '__init__.py'), 'w').close()
    open(os.path.join(d, '__init__.py'), 'w').close()
    with open(os.path.join(d, 'splits.py'), 'w') as f:
        f.write('def create_splits_scenes():\n    return {"train": []}\n')
    return os.path.join(tmp, 'stubs')


def _import(tmp, name):
    stubs = _stub_nuscenes(tmp) if not os.path.exists(os.path.join(tmp, 'stubs')) else os.path.join(tmp, 'stubs')
    for p in (stubs, REF):
        if p not in sys.path:
            sys.path.insert(0, p)
    import importlib
    return importlib.import_module('score.frame_level.' + name)        # the reference file, unchanged


def _write(path, obj):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    if path.endswith('.pickle'):
        with open(path, 'wb') as f:
            pickle.dump(obj, f)
    else:
        np.save(path, obj)


def make_worker(out):
    tmp = tempfile.mkdtemp()
    frames = [FI.worker_frame(k) for k in range(len(FI.WORKER_SIZES))] + [FI.empty_sv_frame()]
    probs, preds, svs = [], [], []
    for k, f in enumerate(frames):
        probs.append(os.path.join(tmp, 'prob', '%06d.npy' % k))
        preds.append(os.path.join(tmp, 'pred', '%06d.npy' % k))
        svs.append(os.path.join(tmp, 'sv', '%06d.pickle' % k))
        _write(probs[-1], f['prob'])
        _write(preds[-1], f['pred'])
        _write(svs[-1], (np.arange(len(f['sv2point'])), f['sv2point']))
    vals = {}
    for m in ('ENT', 'MAR', 'CONF'):
        mod = _import(tmp, MODULES[m])
        mod.init_worker('00', probs)
        vals[m] = np.array([mod.worker_func(k) for k in range(len(FI.WORKER_SIZES))], dtype=np.float32)
    seg = []
    mod = _import(tmp, MODULES['SEGENT'])
    for k, f in enumerate(frames):          # class_num differs per frame: one init per frame
        mod.init_worker(f['class_num'], '00', preds, svs)
        with np.errstate(all='ignore'):
            seg.append(np.float64(mod.worker_func(k)))
    out.update(worker_ent=vals['ENT'], worker_mar=vals['MAR'], worker_conf=vals['CONF'],
               worker_segent=np.array(seg[:-1]), worker_segent_empty=np.float64(seg[-1]),
               worker_sizes=np.array(FI.WORKER_SIZES), worker_inputs_sha=FI.sha256(
                   *[a for f in frames for a in (f['prob'], f['pred'])], *[p for f in frames for p in f['sv2point']]))
    # the restatement is what the kernels are held to; it must reproduce the reference here
    for k, f in enumerate(frames[:-1]):
        e, ma, c = frame_ref.uncertainty(f['prob'])
        assert ma == vals['MAR'][k] and c == vals['CONF'][k], k
        assert e == vals['ENT'][k], (k, e, vals['ENT'][k])
        assert frame_ref.segment_entropy(f['pred'], f['sv2point'], f['class_num']) == seg[k], k
    assert np.isnan(seg[-1])
    print('worker_func: %d frames up to %d points' % (len(frames), max(FI.WORKER_SIZES)))


_DRIVER = '''import runpy, sys
import numpy as np
np.random.seed(%d)
sys.argv = ['x.py', '--dataset_name', 'SK', '--r_id', '1'] + (['--model_name', 'SPVCNN'] if %r else [])
runpy.run_module('score.frame_level.%s', run_name='__main__', alter_sys=True)
'''


def _run_main(tmp, module):
    driver = os.path.join(tmp, 'run_%s.py' % module)
    with open(driver, 'w') as fh:
        fh.write(_DRIVER % (RAND_SEED, module != 'RAND', module))
    env = dict(os.environ, PYTHONPATH=os.path.join(tmp, 'stubs') + ':' + REF)
    r = subprocess.run([sys.executable, driver], cwd=tmp, env=env, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-3000:]


def _flags_out(base, sub):
    return np.concatenate([np.load(os.path.join(base, 'frame_flag', sub, '%s.npy' % s)) for s in FI.SEQS]) != 0


def make_main(out):
    tmp = tempfile.mkdtemp()
    _stub_nuscenes(tmp)
    base = os.path.join(tmp, 'Processing_files', 'SK')
    flags = FI.main_flags_in()
    scores = {m: [] for m in ('ENT', 'MAR', 'CONF', 'SEGENT')}
    shas = []
    for s_i, seq in enumerate(FI.SEQS):
        _write(os.path.join(base, 'frame_flag', '0r', seq + '.npy'), flags[s_i])
        for i in range(FI.MAIN_FRAMES):
            f = FI.main_frame(s_i, i)
            shas += [f['prob'], f['pred']] + f['sv2point']
            _write(os.path.join(base, 'prob_map/SPVCNN/fr/0r', seq, '%06d.npy' % i), f['prob'])
            _write(os.path.join(base, 'pred/SPVCNN/fr/0r', seq, '%06d.npy' % i), f['pred'])
            _write(os.path.join(base, 'super_voxel', seq, '%06d.pickle' % i), (np.arange(4), f['sv2point']))
            e, ma, c = frame_ref.uncertainty(f['prob'])
            scores['ENT'].append(e), scores['MAR'].append(ma), scores['CONF'].append(c)
            scores['SEGENT'].append(frame_ref.segment_entropy(f['pred'], f['sv2point'], FI.MAIN_C))
    for m in ('ENT', 'MAR', 'CONF', 'SEGENT', 'RAND'):
        _run_main(tmp, MODULES[m])
        out['main_flags_' + m] = _flags_out(base, 'RAND/1r' if m == 'RAND' else 'SPVCNN/%s/1r' % m)
    flags_in = np.concatenate(flags)
    n = flags_in.size
    num_add = int(round(0.01 * n))
    u = int((~flags_in).sum())
    big, small = frame_ref.argpartition_probe(u, num_add)
    out.update(main_flags_in=flags_in, main_probe_largest=big, main_probe_smallest=small, main_num_add=num_add,
               main_rand_seed=RAND_SEED, main_inputs_sha=FI.sha256(*shas),
               **{'main_scores_' + m: np.array(v, dtype=np.float32) for m, v in scores.items()})
    for m in ('ENT', 'MAR', 'CONF', 'SEGENT'):
        assert (out['main_flags_' + m] & ~flags_in).sum() == num_add, m
    print('__main__: %d frames, %d unlabeled, num_add %d' % (n, u, num_add))


def _gaps(x, labeled, num_add):
    """f64 greedy k-center on the true distances: the smallest relative gap between the chosen and the next candidate"""
    x64 = x.astype(np.float64)
    lab = np.where(labeled)[0]
    md = np.min(np.sqrt(((x64[:, None, :] - x64[None, lab, :]) ** 2).sum(-1)), axis=1)
    gap = np.inf
    for _ in range(num_add):
        top2 = np.sort(md)[-2:]
        gap = min(gap, (top2[1] - top2[0]) / top2[1])
        ind = int(np.argmax(md))
        md = np.minimum(md, np.sqrt(((x64 - x64[ind]) ** 2).sum(-1)))
    return gap


def make_cset(out):
    import sklearn
    seed = 1
    while True:
        feats = FI.cset_feats(seed)
        flags_in = np.concatenate(FI.cset_flags_in(seed))
        gap = _gaps(feats, flags_in, int(round(0.01 * flags_in.size)))
        if gap > 1e-5:
            break
        seed += 1
    tmp = tempfile.mkdtemp()
    _stub_nuscenes(tmp)
    base = os.path.join(tmp, 'Processing_files', 'SK')
    flags = FI.cset_flags_in(seed)
    for s_i, seq in enumerate(FI.SEQS):
        _write(os.path.join(base, 'frame_flag', '0r', seq + '.npy'), flags[s_i])
        for i in range(FI.CSET_FRAMES):
            _write(os.path.join(base, 'outfeat/SPVCNN/fr/0r', seq, '%06d.npy' % i), FI.cset_outfeat(seed, s_i, i))
    _run_main(tmp, MODULES['CSET'])
    flags_out = _flags_out(base, 'SPVCNN/CSET/1r')
    picks, _ = frame_ref.coreset(feats, flags_in, int(round(0.01 * flags_in.size)))
    mine = flags_in.copy()
    mine[picks] = True
    assert np.array_equal(mine, flags_out), 'restated core-set != core_set.py'
    out.update(cset_seed=seed, cset_flags_in=flags_in, cset_flags_out=flags_out, cset_min_gap=gap,
               cset_feats_sha=FI.sha256(feats), sklearn_version=sklearn.__version__)
    print('core_set: seed %d, %d frames, %d picked, smallest relative gap %.3g (sklearn %s)' % (
        seed, flags_in.size, int((flags_out & ~flags_in).sum()), gap, sklearn.__version__))


if __name__ == '__main__':
    import scipy
    out = {'scipy_version': scipy.__version__, 'numpy_version': np.__version__}
    make_worker(out)
    make_main(out)
    make_cset(out)
    path = os.path.join(HERE, 'frame_small.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')
