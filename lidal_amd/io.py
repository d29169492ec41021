"""On-disk formats shared with an existing LiDAL `Processing_files/` tree and the reference's
checkpoints.  Plain host I/O: the formats are numpy .npy, pickles of
numpy arrays and torch.save dicts, so files written here are readable by the reference scripts and
vice versa.

  prob_map/.../<frame>.npy     f32 [P, C]    score/prob_inference.py:129 -> LiDAL.py:45-49
  pred/.../<frame>.npy         i64 [P]       score/prob_inference.py:130
  super_voxel/.../<frame>.pickle (sv_id i64 [S], sv2point list of i64 arrays)
                                              dataset/prepare_supervoxel_kmeans_sk.py:62-74
  super_voxel/KMeans/<seq>/<frame>.npy        [P] the cluster of every point (`clf.labels_`)
                                              dataset/prepare_supervoxel_kmeans_sk.py:21-22
  super_voxel/KMeans/id2sv.pickle             list of (sequence, frame name, supervoxel of the frame), by sv_id
                                              dataset/prepare_supervoxel_kmeans_sk.py:77-80
  super_voxel/VCCS/...                        the same three formats (dataset/prepare_supervoxel_VCCS_sk.py:27-28,
                                              79-92): the functions of the KMeans tree serve it, nothing is VCCS-only
  sv_flag/.../<frame>.npy      i64 [S] in {0,1,2}   LiDAL.py:328-330
  super_voxel/KMeans/sv_pnums.npy, sv_centers.npy   i64 [sum S]; f32 [sum S, 3] with the
                               +1000 * sequence-index offset      LiDAL.py:173-177,220-222
  frame_flag/0r/<seq>.npy, frame_flag/<model>/<METRIC>/<r>r/<seq>.npy, frame_flag/RAND/<r>r/<seq>.npy
                               bool [frames of the sequence]   score/frame_level/*.py (RAND.py writes float)
  boundary/<seq>/<frame>.npy   f32 [P]       the surface variation of a raw scan
                               dataset/ReDAL/gen_surface_variation_sk.py -> ReDAL.py:57
  <dir>/current.pt             {'model_state_dict', 'iteration', 'ep_id'}   train.py:151-155
  sequences/<seq>/velodyne/<frame>.bin   f32 [P, 4] (x, y, z, intensity)      dataset/sk_dataset.py:101
  samples/LIDAR_TOP/<token>.pcd.bin      f32 [P, 5], the first 4 used         dataset/nu_dataset.py:122-123
  sequences/<seq>/labels/<frame>.label   u32 [P], class in the low 16 bits    dataset/sk_dataset.py:108-111
  lidarseg/.../<token>_lidarseg.bin      u8 [P]                               dataset/nu_dataset.py:130
  pred/.../<frame>.npy (read back as pseudo labels)   i64 [P]                 dataset/sk_dataset.py:119
"""
import os
import pickle

import numpy as np
import torch

__all__ = ['save_prob_pred', 'load_prob', 'load_supervoxels', 'save_supervoxels', 'save_sv_labels', 'load_sv_labels',
           'save_id2sv', 'load_id2sv', 'load_sv_flag',
           'save_sv_flag', 'load_sv_stats', 'save_sv_stats', 'load_curvature', 'save_curvature', 'frame_flag_path', 'load_frame_flag',
           'save_frame_flag', 'save_checkpoint', 'load_checkpoint', 'load_scan', 'load_labels', 'load_pred']


def _mkdir_for(path):
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)


def save_prob_pred(prob_path, pred_path, prob, pred):
    """prob f32 [P,C] / pred i64 [P] (tensors or arrays) -> the two .npy files of prob_inference."""
    prob = prob.detach().cpu().numpy() if torch.is_tensor(prob) else np.asarray(prob)
    pred = pred.detach().cpu().numpy() if torch.is_tensor(pred) else np.asarray(pred)
    _mkdir_for(prob_path), _mkdir_for(pred_path)
    np.save(prob_path, prob.astype(np.float32, copy=False))
    np.save(pred_path, pred.astype(np.int64, copy=False))


def load_prob(path, device=None):
    prob = np.load(path)
    assert prob.dtype == np.float32 and prob.ndim == 2, (prob.dtype, prob.shape)
    t = torch.from_numpy(prob)
    return t.to(device) if device is not None else t


def load_supervoxels(path):
    """-> (sv_id i64 [S], sv2point list of i64 index arrays) exactly as LiDAL.py:84-85 reads it."""
    with open(path, 'rb') as f:
        sv_id, sv2point = pickle.load(f)
    return np.asarray(sv_id), [np.asarray(p) for p in sv2point]


def save_supervoxels(path, sv_id, sv2point):
    _mkdir_for(path)
    with open(path, 'wb') as f:
        pickle.dump((np.asarray(sv_id), [np.asarray(p) for p in sv2point]), f)


def save_sv_labels(path, labels):
    """The cluster of every point of one scan (lidal_amd.data.kmeans_supervoxels' labels, a tensor or an array) ->
    super_voxel/KMeans/<seq>/<frame>.npy, the file prepare_supervoxel_kmeans_sk.py:21-22 writes from `clf.labels_`
    (int32, scikit-learn's label type)."""
    labels = labels.detach().cpu().numpy() if torch.is_tensor(labels) else np.asarray(labels)
    _mkdir_for(path)
    np.save(path, labels.reshape(-1).astype(np.int32))


def load_sv_labels(path):
    """-> i64 [P], read as prepare_supervoxel_kmeans_sk.py:59 reads it."""
    labels = np.load(path)
    assert labels.ndim == 1 and labels.dtype.kind in 'iu', (labels.dtype, labels.shape)
    return labels.astype(np.int64)


def save_id2sv(path, id2sv):
    """The list of (sequence, frame name, supervoxel of the frame) indexed by sv_id -> super_voxel/KMeans/id2sv.pickle
    (prepare_supervoxel_kmeans_sk.py:77-80)."""
    _mkdir_for(path)
    with open(path, 'wb') as f:
        pickle.dump(list(id2sv), f)


def load_id2sv(path):
    with open(path, 'rb') as f:
        return [tuple(entry) for entry in pickle.load(f)]


def load_sv_flag(path):
    return np.load(path)


def save_sv_flag(path, flags):
    _mkdir_for(path)
    np.save(path, np.asarray(flags))


def load_sv_stats(pnums_path, centers_path):
    """The cached per-supervoxel statistics of LiDAL.py:173-177: (sv_pnums i64 [N], sv_centers f32
    [N,3]) -- feed them to score.ScoreBoard(n, sv_pnums, sv_centers) (the reference's `sv_pre`)."""
    pn, ce = np.load(pnums_path), np.load(centers_path)
    assert pn.ndim == 1 and ce.shape == (pn.shape[0], 3), (pn.shape, ce.shape)
    return pn, ce


def save_sv_stats(pnums_path, centers_path, sv_pnums, sv_centers):
    """LiDAL.py:220-222 (written once, by the first scoring round)."""
    _mkdir_for(pnums_path), _mkdir_for(centers_path)
    np.save(pnums_path, np.asarray(sv_pnums))
    np.save(centers_path, np.asarray(sv_centers))


def load_curvature(path):
    """boundary/<seq>/<frame>.npy -> f32 [P], read as ReDAL.py:57 reads it (`.astype(np.float32)`)."""
    curv = np.load(path).astype(np.float32)
    assert curv.ndim == 1, curv.shape
    return curv


def save_curvature(path, curvature):
    """f32 [P] (a tensor or an array: score.surface_variation's output) -> boundary/<seq>/<frame>.npy, the file
    gen_surface_variation_sk.py writes."""
    curvature = curvature.detach().cpu().numpy() if torch.is_tensor(curvature) else np.asarray(curvature)
    _mkdir_for(path)
    np.save(path, curvature.astype(np.float32, copy=False))


def _dataset_kind(dataset):
    kind = str(dataset).upper()
    if kind in ('SK', 'SEMANTICKITTI'):
        return 'SK'
    if kind in ('NU', 'NUSCENES'):
        return 'NU'
    raise ValueError("dataset must be 'SK' or 'NU', not %r" % (dataset,))


def load_scan(path, dataset, device=None):
    """A LiDAR sweep -> (points f32 [P,3], intensity f32 [P]): 4 floats per point for SemanticKITTI
    (sk_dataset.py:101), 5 per point with the first 4 used for nuScenes (nu_dataset.py:122-123)."""
    width = 4 if _dataset_kind(dataset) == 'SK' else 5
    raw = np.fromfile(path, dtype=np.float32).reshape(-1, width)
    points = torch.from_numpy(np.ascontiguousarray(raw[:, :3]))
    intensity = torch.from_numpy(np.ascontiguousarray(raw[:, 3]))
    return (points.to(device), intensity.to(device)) if device is not None else (points, intensity)


def load_labels(path, dataset, device=None):
    """An annotation file as lidal_amd.data.train_labels takes it: SemanticKITTI u32 [P] (sk_dataset.py:108-109) as an
    int32 tensor of the same bits (instance id in the high half, masked on the device), nuScenes u8 [P]
    (nu_dataset.py:130) as a uint8 tensor."""
    if _dataset_kind(dataset) == 'SK':
        t = torch.from_numpy(np.fromfile(path, dtype=np.uint32).reshape(-1).view(np.int32))
    else:
        t = torch.from_numpy(np.fromfile(path, dtype=np.uint8).reshape(-1))
    return t.to(device) if device is not None else t


def load_pred(path, device=None):
    """pred/.../<frame>.npy of save_prob_pred -> i64 [P], last round's predictions (the pseudo labels of
    sk_dataset.py:119)."""
    pred = np.load(path)
    assert pred.ndim == 1 and pred.dtype.kind in 'iu', (pred.dtype, pred.shape)
    t = torch.from_numpy(pred.astype(np.int64, copy=False))
    return t.to(device) if device is not None else t


def frame_flag_path(root, dataset_name, seq, r_id, metric=None, model_name=None):
    """The frame flags of sequence `seq` after round r_id, under root (the directory holding Processing_files):
    frame_flag/0r for r_id == 0, frame_flag/RAND/<r>r for RAND, else frame_flag/<model>/<metric>/<r>r
    (score/frame_level/*.py)."""
    base = os.path.join(root, 'Processing_files', dataset_name, 'frame_flag')
    if r_id == 0:
        return os.path.join(base, '0r', '%s.npy' % seq)
    if metric == 'RAND':
        return os.path.join(base, 'RAND', '%dr' % r_id, '%s.npy' % seq)
    return os.path.join(base, model_name, metric, '%dr' % r_id, '%s.npy' % seq)


def load_frame_flag(path):
    """-> bool [frames]; RAND.py's float files read as its `== False` reads them."""
    return np.load(path) != 0


def save_frame_flag(path, flags):
    flags = flags.detach().cpu().numpy() if torch.is_tensor(flags) else np.asarray(flags)
    _mkdir_for(path)
    np.save(path, flags.astype(bool))


def save_checkpoint(directory, model, iteration, ep_id):
    """train.py:150-155 (rank 0 only in the reference); unwraps DistributedDataParallel."""
    os.makedirs(directory, exist_ok=True)
    module = model.module if hasattr(model, 'module') else model
    torch.save({'model_state_dict': module.state_dict(), 'iteration': iteration, 'ep_id': ep_id},
               os.path.join(directory, 'current.pt'))


def load_checkpoint(path, model, strict=True, map_location='cpu'):
    """train.py:63-72 / prob_inference.py:65-71: load a reference-format checkpoint (keys may carry
    DDP's 'module.' prefix); returns (iteration, ep_id)."""
    ckpt = torch.load(path, map_location=map_location)
    sd = {k[len('module.'):] if k.startswith('module.') else k: v
          for k, v in ckpt['model_state_dict'].items()}
    (model.module if hasattr(model, 'module') else model).load_state_dict(sd, strict=strict)
    return ckpt.get('iteration', 0), ckpt.get('ep_id', 0)
