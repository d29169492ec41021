"""Input voxelisation and collation on the GPU: the host-side mirror of the reference's
dataset/sk_dataset.py:143-171 (per-scan augmentation + voxelisation) and :188-242 (collate_fn).
SURVEY.md section 8f, row 1: the step immediately before the hot path.

The random draws stay on the host in the reference's order (`draw_augmentation`), so a seeded
numpy generator reproduces the reference's augmentation; everything per point runs in
lidal_voxelize_points (affine in f64, x20, translation, int cast, unique rows with first-occurrence
index and inverse map).

Training labels (sk_dataset.py:106-141,170-171; nu_dataset.py:128-160,189-190): `train_labels` turns
the raw annotation words, the round's supervoxel flags, the supervoxel membership lists and last round's predictions
into labels_p / labels_v in lidal_train_labels, and `train_sample` composes the three steps into the dict `collate`
takes.  The frame filters of the loaders (`labeled_frames`, `frames_from_flag`) stay on the host: they pick files.

Supervoxels (dataset/prepare_supervoxel_kmeans_{sk,nu}.py): `kmeans_supervoxels` clusters raw scans
into size-constrained k-means supervoxels in lidal_supervoxel_kmeans and returns the labels with the device CSR the
scorers and `train_labels` take; `supervoxel_tables` turns the labels into the (sv_id, sv2point) pickles and the id2sv
list of an existing Processing_files tree; `balanced_assign` is the exact size-constrained assignment on its own.

Whole batches: `voxelize_batch` voxelises and collates up to 32 samples -- the scans of a batch, or
the augmented views of one scan -- in lidal_voxelize_batch with one read-back; `train_batch`, `val_batch` and
`score_sample` / `score_frame_inputs` compose it into the three __getitem__ + collate_fn modes of the reference, ending
in what train_step, evaluate_batches and score_sequence take.

Mixed batches (the project's own definition, nothing of the reference): `mix_scans` builds up to 32
mixed samples -- inclination bands or an azimuth sector of two scans interleaved, rotated copies of the rows of chosen
classes pasted -- in lidal_mix_scans with one read-back; `draw_lasermix` / `draw_polarmix` make the `Mix` records on the
host and `mixed_train_batch` puts the step in front of voxelize_batch.

Instances (the project's own definition): `euclidean_clusters` turns labels or predictions into
instance ids -- the connected components of the fixed-radius graph per scan and class -- in lidal_euclidean_clusters
with one read-back; `Instances.as_csr` hands a scan's instances to `train_labels` as regions, `draw_instance_paste`
picks instances for a paste and `mix_scans(paste_masks=...)` pastes those rows only.  `instance_ids` reads the annotated
instances out of SemanticKITTI label words and `val_batch(with_instances=True)` carries them, with the raw points, to
evaluate.evaluate_panoptic_batches.
"""
import math

import numpy as np
import torch

from . import backend as B

__all__ = ['draw_augmentation', 'voxelize_scan', 'collate', 'parse_calibration', 'parse_poses',
           'register_scan', 'sk_label_map', 'nu_label_map', 'train_labels', 'train_sample', 'check_labels',
           'labeled_frames', 'frames_from_flag', 'kmeans_supervoxels', 'supervoxel_tables', 'balanced_assign',
           'supervoxel_bounds', 'supervoxel_costs', 'voxelize_batch', 'score_sample', 'mc_sample', 'val_batch', 'train_batch',
           'score_frame_inputs', 'class_weights', 'Mix', 'identity_mix', 'wedge_vectors', 'class_mask', 'draw_lasermix',
           'draw_polarmix', 'mix_scans', 'mixed_train_batch', 'Instances', 'euclidean_clusters', 'draw_instance_paste',
           'instance_ids', 'SK_THINGS']

SCALE = 20                # sk_dataset.py:56
FULL_SCALE = 8192


def draw_augmentation(rng=np.random):
    """sk_dataset.py:144-147 and :156 -- the five random draws of one __getitem__ call, in order.
    `rng` is the numpy global module (as the reference uses) or a RandomState."""
    trans_m = np.eye(3) + rng.randn(3, 3) * 0.1
    trans_m[0][0] *= rng.randint(0, 2) * 2 - 1
    theta = rng.rand() * 2 * math.pi
    trans_m = np.matmul(trans_m, [[math.cos(theta), math.sin(theta), 0],
                                  [-math.sin(theta), math.cos(theta), 0], [0, 0, 1]])
    rnd = np.concatenate([rng.rand(3), rng.rand(3)])
    return trans_m, rnd


def voxelize_scan(points, intensity, trans_m, rnd, scale=SCALE, full_scale=FULL_SCALE):
    """points f32 [P,3], intensity f32 [P] on the GPU; trans_m 3x3 and rnd [6] host float64.
    Returns (coords_v i32 [N,3], feats_v f32 [N,4], unique_idxs i64 [N], inverse_idxs i64 [P])
    with numpy's np.unique(axis=0) semantics (rows sorted lexicographically, first occurrence)."""
    B.require_gpu(points, intensity)
    points = points.contiguous().float()
    intensity = intensity.contiguous().float()
    p = points.shape[0]
    dev = points.device
    m_dev = torch.from_numpy(np.ascontiguousarray(trans_m, dtype=np.float64).reshape(9)).to(dev)
    r_dev = torch.from_numpy(np.ascontiguousarray(rnd, dtype=np.float64).reshape(6)).to(dev)
    feats_p = B.empty((p, 4), torch.float32, dev)
    coords_v = B.empty((max(p, 1), 3), torch.int, dev)
    uniq = B.empty(max(p, 1), torch.int64, dev)
    inverse = B.empty(p, torch.int64, dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)          # [n_out, n_invalid (i32 view)]
    n_invalid = counts[1:].view(torch.int32)[:1]
    ws_bytes = B.lib().lidal_voxelize_points_workspace_bytes(p)
    ws = B.workspace(ws_bytes, dev)
    B.check(B.lib().lidal_voxelize_points(B.ptr(points), B.ptr(intensity), p, B.ptr(m_dev),
                                          B.ptr(r_dev), float(scale), int(full_scale),
                                          B.ptr(feats_p), B.ptr(coords_v), B.ptr(uniq),
                                          B.ptr(inverse), B.ptr(counts), B.ptr(n_invalid), B.ptr(ws),
                                          ws_bytes, B.stream()), 'voxelize_points')
    host = counts.cpu()
    n_out, bad = int(host[0]), int(host[1:].view(torch.int32)[0])
    assert bad == 0, 'input voxels are not valid'            # sk_dataset.py:161
    uniq = uniq[:n_out]
    return coords_v[:n_out], feats_p[uniq], uniq, inverse


def collate(samples):
    """sk_dataset.py:188-242 on device tensors.  samples: dicts with coords_v [N,3], feats_v and
    optionally labels_v / labels_p / inverse_idxs.  The batch index becomes the 4th coordinate column and the
    inverse indices are offset by the voxels of the preceding samples."""
    coords, feats, labels, inverse, labels_p = [], [], [], [], []
    off = 0
    for b, s in enumerate(samples):
        c = s['coords_v'].int()
        coords.append(torch.cat([c, torch.full((c.shape[0], 1), b, dtype=torch.int, device=c.device)], 1))
        feats.append(s['feats_v'].float())
        if 'labels_v' in s:
            labels.append(s['labels_v'].long())
        if 'labels_p' in s:          # val / score modes: per-POINT labels (sk_dataset.py:236-238)
            labels_p.append(s['labels_p'].long())
        if 'inverse_idxs' in s:
            inverse.append(s['inverse_idxs'].long() + off)
            off += c.shape[0]        # == max(inverse) + 1: every voxel is hit by some point
    return {'coords_v_b': torch.cat(coords, 0), 'feats_v_b': torch.cat(feats, 0),
            'labels_v_b': torch.cat(labels, 0) if labels else None,
            'labels_p_b': torch.cat(labels_p, 0) if labels_p else None,
            'inverse_indices_b': torch.cat(inverse, 0) if inverse else None}


# ---- training labels (sk_dataset.py:106-141,170-171) ------------------------------------------
IGNORE = 255              # train.py:136 ignore_index

# SemanticKITTI (semantic-kitti-api, config/semantic-kitti.yaml): the raw ids of the 19 evaluated classes in the
# order of the benchmark's class list minus its 'unlabeled' entry, the raw ids the reference leaves out of training,
# and the moving variants with the static id they fold into.
_SK_CLASS_IDS = (10, 11, 15, 18, 20, 30, 31, 32, 40, 44, 48, 49, 50, 51, 70, 71, 72, 80, 81)
_SK_IGNORED_IDS = (0, 1, 13, 16, 52, 60, 99)     # unlabeled, outlier, bus, on-rails, other-structure, lane-marking, other-object
_SK_MOVING = {252: 10, 253: 31, 254: 30, 255: 32, 256: 16, 257: 13, 258: 18, 259: 20}
# the classes with annotated instances (the 'things' of the panoptic benchmark): car, bicycle, motorcycle, truck,
# other-vehicle, person, bicyclist, motorcyclist -- as training classes, the other eleven being 'stuff'
_SK_THING_IDS = (10, 11, 15, 18, 20, 30, 31, 32)
SK_THINGS = tuple(_SK_CLASS_IDS.index(raw) for raw in _SK_THING_IDS)

# nuScenes-lidarseg: the 32 annotated categories folded into the 16 classes of the lidarseg challenge, by class
# (barrier, bicycle, bus, car, construction_vehicle, motorcycle, pedestrian, traffic_cone, trailer, truck,
#  driveable_surface, other_flat, sidewalk, terrain, manmade, vegetation); every other category is ignored.
_NU_CLASS_IDS = ((9,), (14,), (15, 16), (17,), (18,), (21,), (2, 3, 4, 6), (12,), (22,), (23,), (24,), (25,), (26,), (27,),
                 (28,), (30,))


def sk_label_map():
    """i64 [260]: raw SemanticKITTI id -> training class 0..18 or 255, the table sk_dataset.py:66-92 builds.  An id
    the dataset does not define maps to class 0, not to 255: the reference's table starts as np.zeros(260)."""
    table = np.zeros(260, dtype=np.int64)
    for raw in _SK_IGNORED_IDS:
        table[raw] = IGNORE
    for cls, raw in enumerate(_SK_CLASS_IDS):
        table[raw] = cls
    for raw, static in _SK_MOVING.items():
        table[raw] = table[static]
    return table


def nu_label_map():
    """i64 [100]: nuScenes-lidarseg category -> training class 0..15 or 255 (nu_dataset.py:111-113)."""
    table = np.full(100, IGNORE, dtype=np.int64)
    for cls, raws in enumerate(_NU_CLASS_IDS):
        for raw in raws:
            table[raw] = cls
    return table


def _to_i64(x, dev):
    """A host array or a tensor of any integer / bool type -> i64 on dev (round-0 flag files hold bool,
    sk_dataloader.py:115-118)."""
    if not torch.is_tensor(x):
        x = torch.from_numpy(np.ascontiguousarray(np.asarray(x)).astype(np.int64))
    return x.to(device=dev, dtype=torch.int64).contiguous()


def train_labels(raw_labels, label_map, sv_csr=None, sv_flag=None, pseudo=None, unique_idxs=None, check=True):
    """sk_dataset.py:106-141,170-171 / nu_dataset.py:128-160,189-190 for one scan, on the GPU.
      raw_labels   the annotation file as a GPU tensor: uint8 [P] (nuScenes) or int32 / uint32 [P] holding the u32
                   words of a SemanticKITTI .label file (lidal_amd.io.load_labels returns either)
      label_map    i64 table (sk_label_map() / nu_label_map(); a host array is uploaded)
      sv_csr       (sv_ptr i64 [S+1], sv_idx i64) on the GPU (lidal_amd.score.interframe.sv_csr; a third element is ignored) and
      sv_flag      [S] in {0, 1, 2} (any integer or bool type, host or GPU): the modes 'train_sv' and, with
      pseudo       i64 [P] last round's predictions, 'train_sv_pseudo'.  Without flags every point keeps its label
                   ('train', 'train_frame', 'val').
      unique_idxs  i64 [N] of voxelize_scan, or None for labels_p alone ('val').
    Returns (labels_p i64 [P], labels_v i64 [N] or None).  A raw id beyond the table (numpy's IndexError in the
    reference) or an index outside its array raises; check=False skips that read-back -- the only synchronisation here
    -- and returns (labels_p, labels_v, n_invalid i32 [1] on the GPU) for check_labels to look at later."""
    B.require_gpu(raw_labels)
    dev = raw_labels.device
    if raw_labels.dtype == torch.uint8:
        raw_bytes = 1
    elif raw_labels.dtype in (torch.int32, getattr(torch, 'uint32', torch.int32)):
        raw_bytes = 4
    else:
        raise TypeError('raw_labels must be uint8 (nuScenes) or int32 / uint32 (SemanticKITTI), not %s' % raw_labels.dtype)
    raw_labels = raw_labels.contiguous().reshape(-1)
    p = raw_labels.shape[0]
    label_map = _to_i64(label_map, dev)
    if (sv_csr is None) != (sv_flag is None):
        raise ValueError('sv_csr and sv_flag come together')
    sv_ptr = sv_idx = flags = None
    s = nnz = 0
    if sv_flag is not None:
        sv_ptr, sv_idx = _to_i64(sv_csr[0], dev), _to_i64(sv_csr[1], dev)
        flags = _to_i64(sv_flag, dev)
        s, nnz = flags.shape[0], sv_idx.shape[0]
        if sv_ptr.shape[0] != s + 1:
            raise ValueError('%d flags for %d supervoxels' % (s, sv_ptr.shape[0] - 1))
        if s == 0:                       # an empty tensor has no address: flags present, none set
            flags = torch.zeros(1, dtype=torch.int64, device=dev)
        B.require_gpu(sv_ptr, sv_idx, flags)
    if pseudo is not None:
        B.require_gpu(pseudo)
        pseudo = pseudo.to(torch.int64).contiguous()
        assert pseudo.shape[0] == p                                  # sk_dataset.py:120
    n = 0
    labels_v = None
    if unique_idxs is not None:
        B.require_gpu(unique_idxs)
        unique_idxs = unique_idxs.to(torch.int64).contiguous()
        n = unique_idxs.shape[0]
        labels_v = B.empty(n, torch.int64, dev)
    labels_p = B.empty(p, torch.int64, dev)
    n_invalid = torch.empty(1, dtype=torch.int32, device=dev)
    ws_bytes = B.lib().lidal_train_labels_workspace_bytes(p)
    ws = B.workspace(ws_bytes, dev)
    B.check(B.lib().lidal_train_labels(B.ptr(raw_labels), raw_bytes, p, B.ptr(label_map), label_map.shape[0],
                                       B.ptr(sv_ptr), B.ptr(sv_idx) if nnz else None, nnz, s, B.ptr(flags),
                                       B.ptr(pseudo), B.ptr(unique_idxs) if n else None, n, B.ptr(labels_p),
                                       B.ptr(labels_v) if n else None, B.ptr(n_invalid), B.ptr(ws), ws_bytes,
                                       B.stream()), 'train_labels')
    if not check:
        return labels_p, labels_v, n_invalid
    check_labels(n_invalid)
    return labels_p, labels_v


def instance_ids(raw_labels):
    """The annotated instance ids of a SemanticKITTI scan: the upper 16 bits of its .label words (train_labels reads the
    lower 16) as i32 [P] in 0..65535, on the tensor's device.  raw_labels: int32 or uint32 storage of the u32 words, a
    tensor or a host array; a word with the top bit set is not sign-extended.  Ids are per scan and per class: 0 is
    'no instance annotated', the id of stuff points."""
    if not torch.is_tensor(raw_labels):
        raw = np.ascontiguousarray(np.asarray(raw_labels))
        if raw.dtype not in (np.int32, np.uint32):
            raise TypeError('instance_ids: the label words must be int32 or uint32, not %s' % raw.dtype)
        raw_labels = torch.from_numpy(raw.view(np.int32))
    elif raw_labels.dtype == getattr(torch, 'uint32', None):
        raw_labels = raw_labels.contiguous().view(torch.int32)
    elif raw_labels.dtype != torch.int32:
        raise TypeError('instance_ids: the label words must be int32 or uint32, not %s' % raw_labels.dtype)
    return ((raw_labels.reshape(-1) >> 16) & 0xFFFF).to(torch.int32)      # the shift is arithmetic: the mask undoes it


def check_labels(n_invalid):
    """Raises if any of the counters (an i32 [1] GPU tensor of train_labels(check=False), a sample of
    train_sample(check=False), or a list of either) is not zero.  One read-back for all of them."""
    items = n_invalid if isinstance(n_invalid, (list, tuple)) else [n_invalid]
    counters = [c['labels_invalid'] if isinstance(c, dict) else c for c in items]
    if not counters:
        return
    bad = int(torch.stack([c.reshape(()) for c in counters]).sum().item())
    if bad != 0:
        raise IndexError('train_labels: %d raw label ids beyond the label table or indices outside their array' % bad)


def train_sample(points, intensity, raw_labels, label_map, sv_csr=None, sv_flag=None, pseudo=None, rng=np.random,
                 scale=SCALE, full_scale=FULL_SCALE, check=True):
    """One training __getitem__ (sk_dataset.py:98-178) on the GPU: draw_augmentation(rng), voxelize_scan and
    train_labels -> {'coords_v', 'feats_v', 'labels_v'}, the sample `collate` takes; collate(...) of the
    batch's samples is what train_step takes.  check=False leaves the invalid-id counter in the sample
    ('labels_invalid', ignored by collate) for one check_labels(samples) per batch."""
    trans_m, rnd = draw_augmentation(rng)
    coords_v, feats_v, uniq, _ = voxelize_scan(points, intensity, trans_m, rnd, scale, full_scale)
    out = train_labels(raw_labels, label_map, sv_csr, sv_flag, pseudo, uniq, check=check)
    sample = {'coords_v': coords_v, 'feats_v': feats_v, 'labels_v': out[1]}
    if not check:
        sample['labels_invalid'] = out[2]
    return sample


# ---- a whole batch in one call (sk_dataset.py:143-171 per sample + collate_fn :188-242) --------
MAX_BATCH_SAMPLES = 32    # csrc/kmap.hip: the sample index rides above the 39 coordinate bits of one sort key
MAX_BATCH_POINTS = 2 ** 30 - 1            # csrc/sort.hip: fewer than 2^30 items in one sort


def _batch_arguments(points, intensity, trans_ms, rnds, full_scale):
    """The checks of voxelize_batch that need no device -> (shared, points list, intensity list, m f64 [S,9],
    r f64 [S,6], n_points list).  Everything refused here raises ValueError."""
    what = 'voxelize_batch'
    s = len(trans_ms)
    if s == 0:
        raise ValueError('%s: no samples' % what)
    if s > MAX_BATCH_SAMPLES:
        raise ValueError('%s: %d samples in one call (at most %d)' % (what, s, MAX_BATCH_SAMPLES))
    if len(rnds) != s:
        raise ValueError('%s: %d matrices and %d sets of draws' % (what, s, len(rnds)))
    shared = torch.is_tensor(points)
    if shared != torch.is_tensor(intensity):
        raise ValueError('%s: points and intensity are both one tensor (views of one scan) or both lists' % what)
    pts = [points] if shared else list(points)
    inten = [intensity] if shared else list(intensity)
    if not shared and (len(pts) != s or len(inten) != s):
        raise ValueError('%s: %d point tensors and %d intensity tensors for %d matrices' % (what, len(pts), len(inten), s))
    for j, (x, w) in enumerate(zip(pts, inten)):
        if not torch.is_tensor(x) or x.ndim != 2 or x.shape[1] != 3:
            raise ValueError('%s: sample %d: points must be [P, 3], not %s' % (what, j, tuple(getattr(x, 'shape', ()))))
        if not torch.is_tensor(w) or w.numel() != x.shape[0]:
            raise ValueError('%s: sample %d: %d intensities for %d points'
                             % (what, j, w.numel() if torch.is_tensor(w) else -1, x.shape[0]))
    m, r = np.empty((s, 9), dtype=np.float64), np.empty((s, 6), dtype=np.float64)
    for j in range(s):
        mj, rj = np.asarray(trans_ms[j], dtype=np.float64), np.asarray(rnds[j], dtype=np.float64)
        if mj.shape != (3, 3):
            raise ValueError('%s: sample %d: the matrix must be 3 x 3, not %s' % (what, j, mj.shape))
        if rj.shape != (6,):
            raise ValueError('%s: sample %d: six uniform draws, not %s' % (what, j, rj.shape))
        m[j], r[j] = mj.reshape(9), rj
    if not 0 < int(full_scale) <= 8192:
        raise ValueError('%s: full_scale=%r must be in 1..8192 (13 bits per axis)' % (what, full_scale))
    n_points = [pts[0].shape[0]] * s if shared else [x.shape[0] for x in pts]
    if sum(n_points) > MAX_BATCH_POINTS:
        raise ValueError('%s: %d points in one call (at most %d)' % (what, sum(n_points), MAX_BATCH_POINTS))
    return shared, pts, inten, m, r, n_points


def voxelize_batch(points, intensity, trans_ms, rnds, scale=SCALE, full_scale=FULL_SCALE):
    """S = len(trans_ms) samples voxelised AND collated in one library call with one read-back: what S calls of
    voxelize_scan followed by collate return, bit for bit.
      points / intensity   lists of S GPU tensors f32 [P_s,3] / [P_s] (the scans of a batch), or ONE tensor each: S views
                           of the same scan (the score mode, sk_dataloader.py:199-203)
      trans_ms / rnds      S host matrices 3x3 and S x six draws (draw_augmentation), one pair per sample
    Returns the dict of collate -- coords_v_b i32 [N,4], feats_v_b f32 [N,4], inverse_indices_b i64 [sum P] (labels_v_b and
    labels_p_b None) -- plus unique_idxs_b i64 [N] (first occurrences as rows of the concatenated point list) and, on
    the host, voxel_ptr i64 [S+1] and point_ptr i64 [S+1]: sample s owns voxels voxel_ptr[s]:voxel_ptr[s+1] and points
    point_ptr[s]:point_ptr[s+1].  ValueError, before anything touches the device, for no samples, more than 32, lengths
    that do not match and matrices or draws of the wrong shape; AssertionError naming the sample for points outside the
    grid (sk_dataset.py:161)."""
    shared, pts, inten, m, r, n_points = _batch_arguments(points, intensity, trans_ms, rnds, full_scale)
    B.require_gpu(*pts, *inten)
    s = len(n_points)
    pts = [x.contiguous().float() for x in pts]
    inten = [w.contiguous().float().reshape(-1) for w in inten]
    point_ptr = np.concatenate([[0], np.cumsum(n_points)]).astype(np.int64)
    p_total = int(point_ptr[-1])
    src = pts[0] if len(pts) == 1 else torch.cat(pts)
    src_i = inten[0] if len(inten) == 1 else torch.cat(inten)
    src_row0 = np.zeros(s, dtype=np.int64) if shared else point_ptr[:-1].copy()
    n_rows = np.array(n_points, dtype=np.int64)
    dev = src.device
    aug = torch.from_numpy(np.concatenate([m.reshape(-1), r.reshape(-1)])).to(dev)          # one upload: [S,9] | [S,6]
    cap = max(p_total, 1)
    coords = B.empty((cap, 4), torch.int, dev)
    feats = B.empty((cap, 4), torch.float32, dev)
    uniq = B.empty(cap, torch.int64, dev)
    inverse = B.empty(p_total, torch.int64, dev)
    counts = torch.empty(s + 1 + (s + 1) // 2, dtype=torch.int64, device=dev)        # voxel_ptr [S+1] | n_invalid i32 [S]
    ws_bytes = B.lib().lidal_voxelize_batch_workspace_bytes(p_total, s)
    ws = B.workspace(ws_bytes, dev)
    B.check(B.lib().lidal_voxelize_batch(B.ptr(src), B.ptr(src_i), src_row0.ctypes.data, n_rows.ctypes.data, s,
                                         B.ptr(aug), B.ptr(aug[9 * s:]), float(scale), int(full_scale), B.ptr(coords),
                                         B.ptr(feats), B.ptr(uniq), B.ptr(inverse), B.ptr(counts), B.ptr(ws), ws_bytes,
                                         B.stream()), 'voxelize_batch')
    host = counts.cpu().numpy()                                                        # the one read-back
    voxel_ptr, bad = host[:s + 1].copy(), host[s + 1:].view(np.int32)[:s]
    if bad.any():                                                                      # sk_dataset.py:161
        j = int(np.nonzero(bad)[0][0])
        raise AssertionError('input voxels are not valid: sample %d has %d points outside the grid' % (j, int(bad[j])))
    n = int(voxel_ptr[-1])
    return {'coords_v_b': coords[:n], 'feats_v_b': feats[:n], 'labels_v_b': None, 'labels_p_b': None,
            'inverse_indices_b': inverse, 'unique_idxs_b': uniq[:n], 'voxel_ptr': voxel_ptr, 'point_ptr': point_ptr}


def score_sample(points, intensity, inf_reps=8, rng=np.random):
    """The reference's score batch (sk_dataloader.py:199-203): `inf_reps` __getitem__ calls on ONE scan, each with its
    own draws (draw_augmentation(rng), in order), collated -- one voxelize_batch of views.  What infer_frame takes."""
    draws = [draw_augmentation(rng) for _ in range(int(inf_reps))]
    return voxelize_batch(points, intensity, [d[0] for d in draws], [d[1] for d in draws])


def mc_sample(points, intensity, passes=8, rng=np.random, augment=False):
    """The batch of an MC-dropout scoring pass (score/mc_dropout.py): ONE draw_augmentation(rng) repeated `passes`
    times through voxelize_batch, so the collated copies of the scan are the same voxels and their rows differ by their
    dropout masks alone (an element's mask depends on its index in the batch).  augment=True: score_sample -- every
    pass its own view, the masks on top."""
    if augment:
        return score_sample(points, intensity, passes, rng)
    trans_m, rnd = draw_augmentation(rng)
    return voxelize_batch(points, intensity, [trans_m] * int(passes), [rnd] * int(passes))


def _batch_scans(scans, others, what):
    scans = list(scans)
    for name, other in others:
        if other is not None and len(other) != len(scans):
            raise ValueError('%s: %d scans and %d %s' % (what, len(scans), len(other), name))
    return scans


def val_batch(scans, raw_labels, label_map, rng=np.random, with_instances=False):
    """The reference's validation batch (mode 'val' + collate_fn): scans is a list of (points, intensity) GPU pairs and
    raw_labels their annotation arrays (train_labels).  Draws per scan in order, one voxelize_batch, train_labels per
    scan for labels_p, one check_labels -> the batch of evaluate_batches (labels_p_b beside inverse_indices_b).
    with_instances (SemanticKITTI label words): the batch of evaluate_panoptic_batches, which carries in addition
    'points', the scans' raw f32 [P,3] rows, and 'gt_inst', instance_ids of every scan, as lists."""
    scans = _batch_scans(scans, [('label arrays', raw_labels)], 'val_batch')
    draws = [draw_augmentation(rng) for _ in scans]
    batch = voxelize_batch([x for x, _ in scans], [w for _, w in scans], [d[0] for d in draws], [d[1] for d in draws])
    out = [train_labels(raw, label_map, check=False) for raw in raw_labels]
    batch['labels_p_b'] = torch.cat([o[0] for o in out])
    check_labels([o[2] for o in out])
    if with_instances:
        batch['points'] = [x.float().contiguous() for x, _ in scans]
        batch['gt_inst'] = [instance_ids(raw) for raw in raw_labels]
    return batch


def _fill_extra(labels_p, extra_labels, what):
    """labels_p per scan with extra_labels[j] (i64 [P_j] or None: transfer_labels of score/transfer.py) where
    train_labels left `ignore` (255)."""
    if extra_labels is None:
        return labels_p
    out = []
    for j, (lab, extra) in enumerate(zip(labels_p, extra_labels)):
        if extra is not None:
            if not isinstance(extra, torch.Tensor):
                raise TypeError('%s: extra_labels[%d] must be a tensor or None' % (what, j))
            if extra.dtype != torch.int64 or extra.shape != lab.shape:
                raise ValueError('%s: extra_labels[%d] must be int64 [%d]' % (what, j, lab.shape[0]))
            B.require_gpu(extra)
            lab = torch.where(lab == 255, extra, lab)
        out.append(lab)
    return out


def train_batch(scans, raw_labels, label_map, sv_csrs=None, sv_flags=None, pseudos=None, rng=np.random, check=True,
                extra_labels=None):
    """The reference's training batch (modes 'train', 'train_sv', 'train_sv_pseudo' + collate_fn): scans is a list of
    (points, intensity) GPU pairs; raw_labels, sv_csrs, sv_flags and pseudos hold one entry per scan, as train_labels
    takes them.  Draws per scan in order, one voxelize_batch, train_labels per scan for labels_p (no read-back),
    labels_v_b = labels_p_b[unique_idxs_b], one check_labels for the batch (check=False: the counters stay in
    'labels_invalid') -> the batch of train_step.  extra_labels: one i64 [P] tensor or None per scan (labels carried over
    from neighbour frames, score.transfer_labels); it fills labels_p where train_labels left 255, before labels_v_b is
    taken."""
    if (sv_csrs is None) != (sv_flags is None):
        raise ValueError('train_batch: sv_csrs and sv_flags come together')
    scans = _batch_scans(scans, [('label arrays', raw_labels), ('supervoxel lists', sv_csrs), ('flag arrays', sv_flags),
                                 ('pseudo label arrays', pseudos), ('extra label arrays', extra_labels)], 'train_batch')
    draws = [draw_augmentation(rng) for _ in scans]
    batch = voxelize_batch([x for x, _ in scans], [w for _, w in scans], [d[0] for d in draws], [d[1] for d in draws])
    out = [train_labels(raw_labels[j], label_map, sv_csrs[j] if sv_csrs is not None else None,
                        sv_flags[j] if sv_flags is not None else None, pseudos[j] if pseudos is not None else None,
                        check=False) for j in range(len(scans))]
    batch['labels_p_b'] = torch.cat(_fill_extra([o[0] for o in out], extra_labels, 'train_batch'))
    batch['labels_v_b'] = batch['labels_p_b'][batch['unique_idxs_b']]
    if check:
        check_labels([o[2] for o in out])
    else:
        batch['labels_invalid'] = [o[2] for o in out]
    return batch


def score_frame_inputs(points, intensity, pose, sv2point, inf_reps=8, rng=np.random):
    """One frame of score_sequence from a raw scan: score_sample for the `inf_reps` collated views, register_scan for
    the world-frame points and sv_csr for the supervoxel lists -> {'coords', 'feats', 'inverse', 'world', 'sv_ptr',
    'sv_idx'}."""
    from .score.interframe import sv_csr
    batch = score_sample(points, intensity, inf_reps, rng)
    sv_ptr, sv_idx, _ = sv_csr(sv2point, points.device)
    return {'coords': batch['coords_v_b'], 'feats': batch['feats_v_b'], 'inverse': batch['inverse_indices_b'],
            'world': register_scan(points, pose), 'sv_ptr': sv_ptr, 'sv_idx': sv_idx}


# ---- mixed training batches: LaserMix / PolarMix style (csrc/mix.hip) -------------------------
MAX_MIXES = 32            # include/lidal_amd.h LIDAL_MIX_MAX
MAX_MIX_TANS = 31
MAX_MIX_ROT = 4
MAX_MIX_SLOTS = 2 ** 30 - 1
_MIX_DESC = np.dtype([('a0', '<i8'), ('na', '<i8'), ('b0', '<i8'), ('nb', '<i8'), ('take_a', '<u8'), ('take_b', '<u8'),
                      ('paste_classes', '<u8'), ('n_tans', '<i4'), ('has_wedge', '<i4'), ('n_rot', '<i4'),
                      ('reserved', '<i4'), ('wedge', '<f4', 4), ('rot', '<f4', 2 * MAX_MIX_ROT),
                      ('tans', '<f4', MAX_MIX_TANS), ('pad', '<i4', 3)])          # lidal_mix_desc, 256 bytes
_ALL_CELLS = 2 ** 64 - 1


class Mix:
    """One mixed sample of mix_scans.  Every float is an f32 value made on the host.
      a, b            the two scans (indices into the call's lists; they may be equal)
      tans            0..31 ascending finite tangents of the pitch boundaries: band = #{j : z >= tans[j] * r}
      wedge           None, or (d0x, d0y, d1x, d1y): the sector from direction d0 (included) to d1 (excluded), of width
                      in (0, pi] (wedge_vectors)
      take_a, take_b  64-bit masks over the cells, cell = band + (len(tans) + 1) * in_sector
      paste_classes   64-bit mask over the class ids 0..63 whose rows of B are pasted
      paste_rot       0..4 pairs (cos, sin): one rotated copy of those rows each"""
    __slots__ = ('a', 'b', 'tans', 'wedge', 'take_a', 'take_b', 'paste_classes', 'paste_rot')

    def __init__(self, a, b, tans=(), wedge=None, take_a=0, take_b=0, paste_classes=0, paste_rot=()):
        self.a, self.b = int(a), int(b)
        self.tans = np.asarray(tans, dtype=np.float32).reshape(-1)
        self.wedge = None if wedge is None else np.asarray(wedge, dtype=np.float32).reshape(-1)
        self.take_a, self.take_b, self.paste_classes = int(take_a), int(take_b), int(paste_classes)
        self.paste_rot = np.asarray(paste_rot, dtype=np.float32).reshape(-1, 2)

    def __eq__(self, other):
        return isinstance(other, Mix) and all(
            np.array_equal(getattr(self, k), getattr(other, k)) if isinstance(getattr(self, k), np.ndarray)
            else getattr(self, k) == getattr(other, k) for k in Mix.__slots__)

    __hash__ = None

    def __repr__(self):
        return 'Mix(%s)' % ', '.join('%s=%r' % (k, getattr(self, k)) for k in Mix.__slots__)


def identity_mix(a):
    """The mix that returns scan `a` unchanged: no boundaries, every cell of A, nothing else."""
    return Mix(a, a, take_a=1)


def wedge_vectors(alpha, width=math.pi):
    """The f32 direction vectors (cos a, sin a, cos(a + w), sin(a + w)) of the sector [alpha, alpha + width), taken in
    f64 and then cast; 0 < width <= pi."""
    if not 0.0 < width <= math.pi:
        raise ValueError('wedge_vectors: width=%r must be in (0, pi]' % (width,))
    return np.array([math.cos(alpha), math.sin(alpha), math.cos(alpha + width), math.sin(alpha + width)],
                    dtype=np.float64).astype(np.float32)


def class_mask(classes):
    """Class ids 0..63 -> the 64-bit mask of Mix.paste_classes."""
    mask = 0
    for c in classes:
        if not 0 <= int(c) < 64:
            raise ValueError('class_mask: class id %r is outside 0..63' % (c,))
        mask |= 1 << int(c)
    return mask


def draw_lasermix(a, b, rng=np.random, areas=(3, 4, 5, 6), pitch_deg=(-25.0, 3.0)):
    """Two twin mixes that interleave the inclination bands of scans a and b.  ONE draw: rng.randint(len(areas)) picks
    the number of areas n.  The n - 1 boundaries are equally spaced in pitch strictly inside pitch_deg; their tangents
    are taken in f64 and cast to f32.  Mix 1 takes A's even areas (0 = the lowest) and B's odd ones, the twin the
    complement: together they hold every row of A and of B once."""
    n = int(areas[int(rng.randint(len(areas)))])
    if not 1 <= n <= MAX_MIX_TANS + 1:
        raise ValueError('draw_lasermix: %d areas (1..%d)' % (n, MAX_MIX_TANS + 1))
    lo, hi = float(pitch_deg[0]), float(pitch_deg[1])
    pitch = lo + (hi - lo) * np.arange(1, n, dtype=np.float64) / n
    tans = np.tan(np.deg2rad(pitch)).astype(np.float32)
    even = sum(1 << c for c in range(0, n, 2))
    odd = sum(1 << c for c in range(1, n, 2))
    return Mix(a, b, tans, take_a=even, take_b=odd), Mix(a, b, tans, take_a=odd, take_b=even)


def draw_polarmix(a, b, rng=np.random, paste_classes=(), n_rot=3):
    """Two twin mixes that swap an azimuth sector of scans a and b.  Draws, in order: ONE rng.rand() u, alpha = 2 pi u,
    the sector is [alpha, alpha + pi); then, only with paste_classes, n_rot further rng.rand() u_k, rotation k =
    (k + u_k) * 2 pi / n_rot.  Mix 1 takes A outside the sector and B inside and pastes the rotated rows of B's
    paste_classes; the twin is the same mix of (b, a): B outside, A inside, pastes from A.  Without paste the twins
    hold every row of A and of B once."""
    alpha = 2.0 * math.pi * float(rng.rand())
    wedge = wedge_vectors(alpha, math.pi)
    mask, rot = class_mask(paste_classes), []
    if mask:
        if not 0 <= int(n_rot) <= MAX_MIX_ROT:
            raise ValueError('draw_polarmix: n_rot=%r (0..%d)' % (n_rot, MAX_MIX_ROT))
        for k in range(int(n_rot)):
            ang = (k + float(rng.rand())) * 2.0 * math.pi / int(n_rot)
            rot.append((math.cos(ang), math.sin(ang)))
    rot = np.array(rot, dtype=np.float64).astype(np.float32).reshape(-1, 2)
    kw = dict(wedge=wedge, take_a=0b01, take_b=0b10, paste_classes=mask if len(rot) else 0, paste_rot=rot)
    return Mix(a, b, **kw), Mix(b, a, **kw)


def _mix_arguments(n_points, mixes, has_labels):
    """The checks of mix_scans that need no device -> (descriptors as a _MIX_DESC array, slots, point_ptr of the
    input).  Everything refused here raises ValueError."""
    what = 'mix_scans'
    mixes = list(mixes)
    if not mixes:
        raise ValueError('%s: no mixes' % what)
    if len(mixes) > MAX_MIXES:
        raise ValueError('%s: %d mixes in one call (at most %d)' % (what, len(mixes), MAX_MIXES))
    s = len(n_points)
    ptr = np.concatenate([[0], np.cumsum(n_points)]).astype(np.int64)
    desc = np.zeros(len(mixes), dtype=_MIX_DESC)
    slots = 0
    for j, m in enumerate(mixes):
        if not (0 <= m.a < s and 0 <= m.b < s):
            raise ValueError('%s: mix %d: scans %d and %d of %d' % (what, j, m.a, m.b, s))
        t = np.asarray(m.tans, dtype=np.float32).reshape(-1)
        if len(t) > MAX_MIX_TANS:
            raise ValueError('%s: mix %d: %d boundaries (at most %d)' % (what, j, len(t), MAX_MIX_TANS))
        if not np.isfinite(t).all() or (np.diff(t) < 0).any():
            raise ValueError('%s: mix %d: the boundaries must be finite and ascending' % (what, j))
        w = None if m.wedge is None else np.asarray(m.wedge, dtype=np.float32).reshape(-1)
        if w is not None and (w.shape != (4,) or not np.isfinite(w).all()):
            raise ValueError('%s: mix %d: the sector takes four finite numbers (d0x, d0y, d1x, d1y)' % (what, j))
        cells = (len(t) + 1) * (1 if w is None else 2)
        for name in ('take_a', 'take_b', 'paste_classes'):
            if not 0 <= getattr(m, name) <= _ALL_CELLS:
                raise ValueError('%s: mix %d: %s is not a 64-bit mask' % (what, j, name))
        if (m.take_a | m.take_b) >> cells:
            raise ValueError('%s: mix %d: a mask bit at or above the %d cells' % (what, j, cells))
        rot = np.asarray(m.paste_rot, dtype=np.float32).reshape(-1, 2)
        if len(rot) > MAX_MIX_ROT:
            raise ValueError('%s: mix %d: %d rotations (at most %d)' % (what, j, len(rot), MAX_MIX_ROT))
        if not np.isfinite(rot).all():
            raise ValueError('%s: mix %d: the rotations must be finite' % (what, j))
        if len(rot) and not has_labels:
            raise ValueError('%s: mix %d: a paste needs labels' % (what, j))
        d = desc[j]
        d['a0'], d['na'], d['b0'], d['nb'] = ptr[m.a], n_points[m.a], ptr[m.b], n_points[m.b]
        d['take_a'], d['take_b'], d['paste_classes'] = m.take_a, m.take_b, m.paste_classes
        d['n_tans'], d['has_wedge'], d['n_rot'] = len(t), w is not None, len(rot)
        d['tans'][:len(t)] = t
        if w is not None:
            d['wedge'][:] = w
        d['rot'][:2 * len(rot)] = rot.reshape(-1)
        slots += int(n_points[m.a]) + int(n_points[m.b]) * (1 + len(rot))
        if slots > MAX_MIX_SLOTS:
            raise ValueError('%s: %d slots in one call (fewer than 2^30)' % (what, slots))
    return desc, slots, ptr


def _paste_key(labs, paste_masks, what):
    """The labels the mix is steered with: the label where a scan's mask is set, 255 (never pasted) elsewhere."""
    masks = list(paste_masks)
    if len(masks) != len(labs):
        raise ValueError('%s: %d paste masks for %d scans' % (what, len(masks), len(labs)))
    keys = []
    for j, (l, m) in enumerate(zip(labs, masks)):
        if m is None:
            keys.append(l)
            continue
        if not torch.is_tensor(m) or m.dtype != torch.bool or m.numel() != l.numel():
            raise ValueError('%s: scan %d: the paste mask must be a bool tensor over its %d rows' % (what, j, l.numel()))
        B.require_gpu(m)
        keys.append(torch.where(m.reshape(-1), l, torch.full_like(l, 255)))
    return keys


def mix_scans(points, intensity, labels, mixes, paste_masks=None):
    """M = len(mixes) mixed samples from S scans in ONE library call (lidal_mix_scans: three launches, no atomics) with
    one read-back.
      points / intensity   lists of S GPU tensors f32 [P_s,3] / [P_s], as voxelize_batch takes them
      labels               list of S i64 [P_s] (the labels_p of train_labels; 255 = ignored), or None: then no label
                           output and no paste
      mixes                1..32 Mix records
    Returns {'points' f32 [N,3], 'intensity' f32 [N], 'labels' i64 [N] or None, 'src' i64 [N]} on the device -- the
    samples laid end to end; src is the row of the concatenated input list each row was taken from (the B row for a
    paste), so any other per-point array follows with array[src] -- and on the host 'point_ptr' i64 [M+1] (sample m owns
    rows point_ptr[m]:point_ptr[m+1]) and 'parts' i64 [M,6], the row counts of A, B and the four pastes.  The outputs are
    allocated at the slot bound sum(n_a + n_b (1 + rotations)) and returned as slices.  ValueError, before anything
    touches the device, for no mixes or more than 32, a scan index out of range, more than 31 boundaries or boundaries
    that are not finite and ascending, a sector that is not finite, mask bits at or above the cell count, more than 4
    rotations, a paste without labels and 2^30 or more slots.

    paste_masks (a list with one bool tensor [P_s] on the device, or None, per scan) restricts the pastes to the rows
    whose mask is set -- the rows of chosen instances (draw_instance_paste): the call is steered with the label where
    the mask is set and 255 elsewhere, and the labels returned are labels[src].  A scan with None pastes as before."""
    what = 'mix_scans'
    pts, inten = list(points), list(intensity)
    labs = None if labels is None else list(labels)
    if len(inten) != len(pts) or (labs is not None and len(labs) != len(pts)):
        raise ValueError('%s: %d point tensors, %d intensity tensors and %s label tensors'
                         % (what, len(pts), len(inten), 'no' if labs is None else len(labs)))
    for j, x in enumerate(pts):
        if not torch.is_tensor(x) or x.ndim != 2 or x.shape[1] != 3:
            raise ValueError('%s: scan %d: points must be [P, 3], not %s' % (what, j, tuple(getattr(x, 'shape', ()))))
        for name, other in (('intensities', inten), ('labels', labs)):
            if other is not None and (not torch.is_tensor(other[j]) or other[j].numel() != x.shape[0]):
                raise ValueError('%s: scan %d: %d %s for %d points'
                                 % (what, j, other[j].numel() if torch.is_tensor(other[j]) else -1, name, x.shape[0]))
    if paste_masks is not None and labs is None:
        raise ValueError('%s: paste masks need labels' % what)
    desc, slots, _ = _mix_arguments([x.shape[0] for x in pts], mixes, labs is not None)
    m = len(desc)
    B.require_gpu(*pts, *inten, *(labs or []))
    pts = [x.contiguous().float() for x in pts]
    inten = [w.contiguous().float().reshape(-1) for w in inten]
    xyz = pts[0] if len(pts) == 1 else torch.cat(pts)
    w_all = inten[0] if len(inten) == 1 else torch.cat(inten)
    lab_all = None
    if labs is not None:
        labs = [l.to(torch.int64).contiguous().reshape(-1) for l in labs]
        lab_all = labs[0] if len(labs) == 1 else torch.cat(labs)
    key_all = lab_all
    if paste_masks is not None:
        keys = _paste_key(labs, paste_masks, what)
        key_all = keys[0] if len(keys) == 1 else torch.cat(keys)
    dev = xyz.device
    cap = max(slots, 1)
    out_xyz = B.empty((cap, 3), torch.float32, dev)
    out_w = B.empty(cap, torch.float32, dev)
    out_lab = B.empty(cap, torch.int64, dev) if lab_all is not None else None
    out_src = B.empty(cap, torch.int64, dev)
    counts = torch.empty(m + 1 + 6 * m, dtype=torch.int64, device=dev)               # point_ptr [M+1] | parts [M,6]
    ws_bytes = B.lib().lidal_mix_scans_workspace_bytes(slots, m)
    ws = B.workspace(ws_bytes, dev)
    B.check(B.lib().lidal_mix_scans(B.ptr(xyz), B.ptr(w_all), B.ptr(key_all), xyz.shape[0], desc.ctypes.data, m,
                                    B.ptr(out_xyz), B.ptr(out_w), B.ptr(out_lab), B.ptr(out_src), B.ptr(counts),
                                    B.ptr(ws), ws_bytes, B.stream()), 'mix_scans')
    host = counts.cpu().numpy()                                                       # the one read-back
    point_ptr, parts = host[:m + 1].copy(), host[m + 1:].reshape(m, 6).copy()
    n = int(point_ptr[-1])
    if paste_masks is not None:
        out_lab = lab_all[out_src[:n]]                                                # the labels behind the steering key
    return {'points': out_xyz[:n], 'intensity': out_w[:n], 'labels': out_lab[:n] if out_lab is not None else None,
            'src': out_src[:n], 'point_ptr': point_ptr, 'parts': parts}


def mixed_train_batch(scans, raw_labels, label_map, mixes, sv_csrs=None, sv_flags=None, pseudos=None, rng=np.random,
                      check=True, extra_labels=None, paste_masks=None):
    """train_batch over mixed samples: scans, raw_labels, sv_csrs, sv_flags and pseudos as train_batch takes them, and
    one Mix per sample of the batch.  train_labels per scan (no read-back), mix_scans of the scans and their labels_p,
    ONE draw_augmentation(rng) per mix in order, voxelize_batch over the mixed samples, labels_v_b = the mixed
    labels[unique_idxs_b], one check_labels (check=False: the counters stay in 'labels_invalid') -> the batch of
    train_step.  Beside it: labels_p_b and src_p_b per mixed point, src_b per voxel (rows of the concatenated input list:
    any per-point array of the scans follows the batch with array[src]) and parts of mix_scans.  Two read-backs: the
    mix's row counts and the batch's voxel counts.  identity_mix(j) for every scan gives train_batch's batch.
    extra_labels as train_batch takes them: they fill the scans' labels_p before the scans are mixed.  paste_masks as
    mix_scans takes them."""
    if (sv_csrs is None) != (sv_flags is None):
        raise ValueError('mixed_train_batch: sv_csrs and sv_flags come together')
    scans = _batch_scans(scans, [('label arrays', raw_labels), ('supervoxel lists', sv_csrs), ('flag arrays', sv_flags),
                                 ('pseudo label arrays', pseudos), ('extra label arrays', extra_labels)],
                        'mixed_train_batch')
    mixes = list(mixes)
    _mix_arguments([x.shape[0] for x, _ in scans], mixes, True)         # refused before anything is launched
    out = [train_labels(raw_labels[j], label_map, sv_csrs[j] if sv_csrs is not None else None,
                        sv_flags[j] if sv_flags is not None else None, pseudos[j] if pseudos is not None else None,
                        check=False) for j in range(len(scans))]
    mixed = mix_scans([x for x, _ in scans], [w for _, w in scans],
                      _fill_extra([o[0] for o in out], extra_labels, 'mixed_train_batch'), mixes, paste_masks=paste_masks)
    draws = [draw_augmentation(rng) for _ in mixes]
    ptr = mixed['point_ptr']
    cut = [(int(ptr[j]), int(ptr[j + 1])) for j in range(len(mixes))]
    batch = voxelize_batch([mixed['points'][a:b] for a, b in cut], [mixed['intensity'][a:b] for a, b in cut],
                           [d[0] for d in draws], [d[1] for d in draws])
    batch['labels_p_b'], batch['src_p_b'], batch['parts'] = mixed['labels'], mixed['src'], mixed['parts']
    batch['labels_v_b'] = mixed['labels'][batch['unique_idxs_b']]
    batch['src_b'] = mixed['src'][batch['unique_idxs_b']]
    if check:
        check_labels([o[2] for o in out])
    else:
        batch['labels_invalid'] = [o[2] for o in out]
    return batch


def class_weights(labels_v_b, n_classes, ignore=255, kind='inverse'):
    """Per-class weights f32 [n_classes] for nn.functional.cross_entropy(weight=...) from the histogram of a label
    tensor (any shape, integer, on the device; `ignore` and labels outside [0, n_classes) are not counted).  With
    n_k the count of class k and f_k = n_k / sum_j n_j:
        'inverse'       w_k = 1 / f_k
        'inverse_sqrt'  w_k = 1 / sqrt(f_k)
        'log'           w_k = 1 / log(1.02 + f_k)              (Paszke et al., ENet)
    A class without a label gets weight 0 under the two inverse kinds (no row carries it anyway) and the formula's
    finite 1 / log(1.02) under 'log'.  The inverse kinds are then scaled so that the weights of the classes that occur
    average 1; 'log' is left as the formula gives it.  Computed in f64 from exact counts (lidal_count)."""
    from .nn.functional.count import spcount
    if kind not in ('inverse', 'inverse_sqrt', 'log'):
        raise ValueError("kind must be 'inverse', 'inverse_sqrt' or 'log', got %r" % (kind,))
    B.require_gpu(labels_v_b)
    flat = labels_v_b.reshape(-1)
    idx = torch.where(flat == ignore, torch.full_like(flat, -1), flat).clamp(-1, n_classes).int()
    counts = spcount(idx, n_classes).double()
    f = counts / counts.sum().clamp_min(1.0)
    if kind == 'log':
        return (1.0 / torch.log(1.02 + f)).float()
    has = counts > 0
    w = torch.where(has, 1.0 / f.clamp_min(1e-300), torch.zeros_like(f))
    if kind == 'inverse_sqrt':
        w = w.sqrt()
    return (w / (w.sum() / has.sum().clamp_min(1)).clamp_min(1e-300)).float()


def labeled_frames(sv_flags_per_frame):
    """sk_dataloader.py:279-290: the indices of the frames with at least one flagged supervoxel (`flag.sum() != 0`;
    a frame with pseudo-labeled supervoxels only counts, as there).  Host arrays in, i64 indices out."""
    return np.array([i for i, flag in enumerate(sv_flags_per_frame) if np.asarray(flag).sum() != 0], dtype=np.int64)


def frames_from_flag(frame_flag):
    """sk_dataloader.py:160-172: frame flags (one array, or one per sequence in sequence order) -> the indices of the
    selected frames in the concatenated frame list."""
    if isinstance(frame_flag, (list, tuple)):
        flat = np.array([])
        for f in frame_flag:
            flat = np.append(flat, np.asarray(f))
    else:
        flat = np.asarray(frame_flag).reshape(-1)
    return np.nonzero(flat.astype(bool))[0].astype(np.int64)


# ---- world-frame registration (dataset/prepare_kdtree_sk.py) ---------------------
def _mat_from_values(values):
    pose = np.zeros((4, 4))
    pose[0, 0:4] = values[0:4]
    pose[1, 0:4] = values[4:8]
    pose[2, 0:4] = values[8:12]
    pose[3, 3] = 1.0
    return pose


def parse_calibration(filename):
    """prepare_kdtree_sk.py:39-62: `key: 12 floats` lines -> dict of 4x4 matrices."""
    calib = {}
    with open(filename) as f:
        for line in f:
            key, content = line.strip().split(':')
            calib[key] = _mat_from_values([float(v) for v in content.strip().split()])
    return calib


def parse_poses(filename, calibration):
    """prepare_kdtree_sk.py:10-36: per-scan camera poses -> LiDAR poses Tr^-1 * pose * Tr."""
    tr = calibration['Tr']
    tr_inv = np.linalg.inv(tr)
    poses = []
    with open(filename) as f:
        for line in f:
            pose = _mat_from_values([float(v) for v in line.strip().split()])
            poses.append(np.matmul(tr_inv, np.matmul(pose, tr)))
    return poses


def register_scan(points, pose):
    """prepare_kdtree_sk.py:76-80: sensor-frame points f32 [P,3] (GPU) + 4x4 pose (host f64) ->
    world-frame f64 [P,3], the data the reference hands to sklearn's KDTree (:83); here it goes to
    lidal_amd.score.FrameBank.add, which builds the uniform NN grid."""
    B.require_gpu(points)
    points = points.contiguous().float()
    p = points.shape[0]
    pose_dev = torch.from_numpy(np.ascontiguousarray(pose, dtype=np.float64).reshape(16)).to(points.device)
    world = torch.empty((p, 3), dtype=torch.float64, device=points.device)
    B.check(B.lib().lidal_register_points(B.ptr(points), p, B.ptr(pose_dev), B.ptr(world), B.stream()),
            'register_points')
    return world


# ---- size-constrained k-means supervoxels (dataset/prepare_supervoxel_kmeans_sk.py) ---------
SV_KMAX = 64              # csrc/supervoxel.hip: one bit per cluster in the 64-bit masks
SV_REACH = 5e5            # metres: 1000 * the largest distance between two points stays inside an int32 cost
_FLOW_ERRORS = {1: 'the size bounds admit no assignment', 2: 'no deficit node can be reached',
                3: 'the path walk does not end at an excess node', 4: 'the distances did not settle',
                5: 'an arc of the path has no point'}


def supervoxel_bounds(p, n_clusters=20, slack=0.05):
    """(size_min, size_max) of prepare_supervoxel_kmeans_sk.py:17 for a scan of p points: int(p / k * 0.95) and
    int(p / k * 1.05) in Python floats."""
    return int(p / n_clusters * (1 - slack)), int(p / n_clusters * (1 + slack))


def _check_bounds(p, k, lo, hi, what):
    if not 1 <= k <= SV_KMAX:
        raise ValueError('%s: n_clusters=%d must be in 1..%d' % (what, k, SV_KMAX))
    if p < k:
        raise ValueError('%s: %d points for %d clusters' % (what, p, k))
    if lo < 0 or lo > hi or k * hi < p or k * lo > p:
        raise ValueError('%s: no assignment of %d points to %d clusters has every size in [%d, %d]'
                         % (what, p, k, lo, hi))


def _raise_flow_errors(status, what):
    """status: host i32 [..., n_frames, 2] = (error word, augmentations)."""
    bad = np.argwhere(status[..., 0] != 0)
    if len(bad):
        where = tuple(int(v) for v in bad[0])
        code = int(status[where + (0,)])
        raise RuntimeError('%s: frame %d: %s (error word %d)' % (what, where[-1], _FLOW_ERRORS.get(code, '?'), code))


def _finite_points(xyz, what):
    reach = float(xyz.abs().max()) if xyz.numel() else 0.0      # (NaN if any coordinate is; one synchronisation)
    if not reach < float('inf'):
        raise ValueError('%s: the coordinates must be finite (NaN or inf found)' % what)
    if not reach < SV_REACH:
        raise ValueError('%s: a coordinate of magnitude %g does not fit the integer costs (limit %g)'
                         % (what, reach, SV_REACH))


def _batch(frames):                        # laid end to end: (all rows, ptr host i64 [n + 1], where each frame starts)
    ptr = np.concatenate([[0], np.cumsum([x.shape[0] for x in frames])]).astype(np.int64)
    return (frames[0] if len(frames) == 1 else torch.cat(frames)), ptr


def _scan_batch(points, what, check):
    """One scan [P, 3] or a list of scans -> (frames f32 contiguous, xyz f32 [sum P, 3], ptr host i64 [n + 1], single).
    Refused before require_gpu and before any launch: no scans, a scan that is not [P, 3], what check(frames) raises."""
    single = torch.is_tensor(points)
    frames = [points] if single else list(points)
    if not frames:
        raise ValueError('%s: no scans' % what)
    for x in frames:
        if not torch.is_tensor(x) or x.ndim != 2 or x.shape[1] != 3:
            raise ValueError('%s: points must be [P, 3], not %s' % (what, tuple(getattr(x, 'shape', ())),))
    check(frames)
    B.require_gpu(*frames)
    frames = [x.float().contiguous() for x in frames]
    xyz, ptr = _batch(frames)
    return frames, xyz, ptr, single


def _sv_ptr(sizes, dev):                   # a frame's supervoxel sizes (host) -> sv_ptr i64 [S + 1] on the device
    return torch.from_numpy(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)).to(dev)


def supervoxel_costs(xyz, centers):
    """The integer arc costs of the definition: xyz f32 [P,3] and centers f64 [K,3] on the GPU -> int32 [P,K],
    rint(1000 * distance) with the distance in f64 as numpy rounds it."""
    B.require_gpu(xyz, centers)
    xyz = xyz.float().contiguous()
    centers = centers.double().contiguous()
    if xyz.ndim != 2 or xyz.shape[1] != 3 or centers.ndim != 2 or centers.shape[1] != 3:
        raise ValueError('supervoxel_costs: xyz [P, 3] and centers [K, 3]')
    p, k = xyz.shape[0], centers.shape[0]
    if not 1 <= k <= SV_KMAX:
        raise ValueError('supervoxel_costs: %d centres (1..%d)' % (k, SV_KMAX))
    _finite_points(xyz, 'supervoxel_costs')
    _finite_points(centers, 'supervoxel_costs')
    cost = torch.empty((p, k), dtype=torch.int32, device=xyz.device)
    B.check(B.lib().lidal_supervoxel_costs(B.ptr(xyz), p, B.ptr(centers), k, B.ptr(cost), B.stream()),
            'supervoxel_costs')
    return cost


def balanced_assign(cost, size_min, size_max):
    """The exact least-cost assignment of P points to K <= 64 clusters with every cluster size in
    [size_min, size_max]: cost int32 [P,K] on the GPU (or a list of such frames, with one bound each or one pair for
    all) -> (labels i64 [P] on the GPU, objective) per frame.  Ties: DESIGN.md section 11.  Infeasible bounds raise
    ValueError before anything is launched; an error word of the kernel raises RuntimeError."""
    single = torch.is_tensor(cost)
    frames = [cost] if single else list(cost)
    n = len(frames)
    lo = [int(v) for v in (size_min if isinstance(size_min, (list, tuple)) else [size_min] * n)]
    hi = [int(v) for v in (size_max if isinstance(size_max, (list, tuple)) else [size_max] * n)]
    if n == 0 or len(lo) != n or len(hi) != n:
        raise ValueError('balanced_assign: %d frames, %d / %d bounds' % (n, len(lo), len(hi)))
    k = frames[0].shape[1] if frames[0].ndim == 2 else 0
    for c, l, h in zip(frames, lo, hi):
        if c.dtype != torch.int32 or c.ndim != 2 or c.shape[1] != k:
            raise TypeError('balanced_assign: cost must be int32 [P, K] with one K for all frames')
        _check_bounds(c.shape[0], k, l, h, 'balanced_assign')
    B.require_gpu(*frames)
    dev = frames[0].device
    cost_all, ptr = _batch([c.contiguous() for c in frames])
    p_total = int(ptr[-1])
    ptr_dev = torch.from_numpy(ptr).to(dev)
    lo_dev = torch.tensor(lo, dtype=torch.int32, device=dev)
    hi_dev = torch.tensor(hi, dtype=torch.int32, device=dev)
    labels = torch.empty(p_total, dtype=torch.int32, device=dev)
    objective = torch.empty(n, dtype=torch.int64, device=dev)
    status = torch.empty((n, 2), dtype=torch.int32, device=dev)
    nbytes = B.lib().lidal_balanced_assign_workspace_bytes(p_total, n, k)
    ws = B.workspace(nbytes, dev)
    B.check(B.lib().lidal_balanced_assign(B.ptr(cost_all), B.ptr(ptr_dev), n, p_total, k, B.ptr(lo_dev), B.ptr(hi_dev),
                                          B.ptr(labels), None, B.ptr(objective), B.ptr(status), B.ptr(ws), nbytes,
                                          B.stream()), 'balanced_assign')
    _raise_flow_errors(status.cpu().numpy(), 'balanced_assign')
    obj = objective.cpu().numpy()
    out = [(labels[ptr[f]:ptr[f + 1]].long(), int(obj[f])) for f in range(n)]
    return out[0] if single else out


def kmeans_supervoxels(points, n_clusters=20, slack=0.05, random_state=0, details=False):
    """Size-constrained k-means supervoxels of raw scans on the GPU, in place of prepare_supervoxel_kmeans_sk.py:17-18
    (KMeansConstrained(n_clusters, size_min, size_max, n_init=1, max_iter=1, random_state).fit_predict) as this project
    defines it: greedy k-means++ seeds, integer costs rint(1000 * distance), an exact
    size-constrained assignment, one centre update, and the assignment again.

    points: f32 [P,3] on the GPU, or a list of such scans (one batch of launches).  Returns per scan
    (labels i64 [P], sv_ptr i64 [S+1], sv_idx i64 [P]) on the GPU: the labels, and the supervoxel CSR in the form of
    score.interframe.sv_csr (supervoxels in label order, empty clusters dropped, point ids ascending), which
    score_frame, region_scores, segment_entropy and train_labels take as it is.  details=True appends a dict with
    seeds, labels_first, centers, counts, objective (first, second), augmentations (first, second), size_min, size_max.
    Raises ValueError, before any launch, for n_clusters outside 1..64, fewer points than clusters, size bounds no
    assignment can meet (21 points in 20 clusters: size_max is 1) and coordinates that are not finite."""
    from .score.redal import kmeans_draws
    k = int(n_clusters)
    lo, hi = [], []

    def check(frames):
        for x in frames:
            l, h = supervoxel_bounds(x.shape[0], k, slack) if 1 <= k <= SV_KMAX else (0, 0)
            _check_bounds(x.shape[0], k, l, h, 'kmeans_supervoxels')
            lo.append(l), hi.append(h)
    frames, xyz, ptr, single = _scan_batch(points, 'kmeans_supervoxels', check)
    _finite_points(xyz, 'kmeans_supervoxels')
    n, dev = len(frames), xyz.device
    seed = int(np.random.RandomState(random_state).randint(2 ** 31 - 1, size=1)[0])
    draws = [kmeans_draws(x.shape[0], k, seed) for x in frames]
    trials = draws[0][2]
    first = np.array([d[0] for d in draws], dtype=np.int64)
    u = np.concatenate([d[1].reshape(-1) for d in draws] + [np.zeros(1)])
    u_dev = torch.from_numpy(u).to(dev)
    p_total, p_max = int(ptr[-1]), int(max(x.shape[0] for x in frames))
    lo_h, hi_h = np.array(lo, dtype=np.int32), np.array(hi, dtype=np.int32)
    seeds = torch.empty((n, k), dtype=torch.int32, device=dev)
    labels_first = torch.empty(p_total, dtype=torch.int32, device=dev)
    centers = torch.empty((n, k, 3), dtype=torch.float64, device=dev)
    labels = torch.empty(p_total, dtype=torch.int32, device=dev)
    order = torch.empty(p_total, dtype=torch.int32, device=dev)
    counts = torch.empty((n, k), dtype=torch.int32, device=dev)
    objective = torch.empty((2, n), dtype=torch.int64, device=dev)
    status = torch.empty((2, n, 2), dtype=torch.int32, device=dev)
    nbytes = B.lib().lidal_supervoxel_kmeans_workspace_bytes(p_total, p_max, n, k, trials)
    ws = B.workspace(nbytes, dev)
    B.check(B.lib().lidal_supervoxel_kmeans(B.ptr(xyz), ptr.ctypes.data, n, k, lo_h.ctypes.data, hi_h.ctypes.data,
                                            first.ctypes.data, B.ptr(u_dev), trials, B.ptr(seeds), B.ptr(labels_first),
                                            B.ptr(centers), B.ptr(labels), B.ptr(order), B.ptr(counts),
                                            B.ptr(objective), B.ptr(status), B.ptr(ws), nbytes, B.stream()),
            'supervoxel_kmeans')
    host = torch.cat([status.reshape(-1), counts.reshape(-1)]).cpu().numpy()        # the one read-back
    status_h, counts_h = host[:4 * n].reshape(2, n, 2), host[4 * n:].reshape(n, k)
    _raise_flow_errors(status_h, 'kmeans_supervoxels')
    objective_h = objective.cpu().numpy() if details else None
    out = []
    for f in range(n):
        a, b = int(ptr[f]), int(ptr[f + 1])
        item = (labels[a:b].long(), _sv_ptr(counts_h[f][counts_h[f] > 0], dev), order[a:b].long())
        if details:
            item += (dict(seeds=seeds[f], labels_first=labels_first[a:b].long(), centers=centers[f], counts=counts[f],
                          objective=(int(objective_h[0, f]), int(objective_h[1, f])),
                          augmentations=(int(status_h[0, f, 1]), int(status_h[1, f, 1])),
                          size_min=lo[f], size_max=hi[f]),)
        out.append(item)
    return out[0] if single else out


# ---- VCCS supervoxels (dataset/prepare_supervoxel_VCCS_sk.py) --------------------------------
_VCCS_ERRORS = {1: 'a cell does not fit 21 bits per axis', 2: 'an occupied cell was not found among the voxels',
                3: 'a seed cell has no voxel'}


def vccs_parameters(voxel_resolution=0.5, seed_resolution=10.0):
    """(min_seed, rounds) of the definition, in Python floats: the least number of voxels within half a seed resolution
    a seed candidate must exceed (15.7 at the defaults), and the number of synchronous rounds (35)."""
    rv, rs = float(voxel_resolution), float(seed_resolution)
    return 0.05 * (0.5 * rs) ** 2 * math.pi / rv ** 2, int(1.8 * rs / rv) - 1


def _check_vccs(frames, rv, rs, w_s, w_n):
    if not (rv > 0 and math.isfinite(rv) and math.isfinite(rs)):
        raise ValueError('vccs_supervoxels: voxel_resolution=%r must be positive and finite' % rv)
    if rs < 2 * rv:
        raise ValueError('vccs_supervoxels: seed_resolution=%r is below two voxels of %r' % (rs, rv))
    if SV_REACH / rv >= 2 ** 20:
        raise ValueError('vccs_supervoxels: cells of %r m do not fit 21 bits per axis over +-%g m' % (rv, SV_REACH))
    if not (w_s >= 0 and w_n >= 0 and math.isfinite(w_s) and math.isfinite(w_n)):
        raise ValueError('vccs_supervoxels: the importances must not be negative')
    for x in frames:
        if x.shape[0] == 0:
            raise ValueError('vccs_supervoxels: a scan without points')
        if x.shape[0] >= 2 ** 24:
            raise ValueError('vccs_supervoxels: %d points in one scan (at most 2^24 - 1)' % x.shape[0])
    if sum(x.shape[0] for x in frames) >= 2 ** 31 // 27:
        raise ValueError('vccs_supervoxels: %d points in one batch (fewer than %d)'
                         % (sum(x.shape[0] for x in frames), 2 ** 31 // 27))
    for x in frames:
        _finite_points(x, 'vccs_supervoxels')


def vccs_supervoxels(points, voxel_resolution=0.5, seed_resolution=10.0, spatial_importance=0.4, normal_importance=1.0,
                     min_points=100, details=False):
    """VCCS supervoxels of raw scans on the GPU, in place of prepare_supervoxel_VCCS_sk.py:17-28 (every scan piped
    through pcl::SupervoxelClustering<PointXYZ>(0.5, 10.0) with spatial importance 0.4 and normal importance 1.0) as
    this project defines them.  The PCL library's labels are not reproduced.

    points: f32 [P,3] on the GPU, or a list of such scans (one batch of launches).  Returns per scan
    (labels i64 [P], sv_ptr i64 [S+1], sv_idx i64) on the GPU: label 0 is "no supervoxel"; the CSR holds the labels
    != 0 with strictly more than min_points points, in label order with ascending point ids
    (prepare_supervoxel_VCCS_sk.py:72-77), in the form score_frame, region_scores, segment_entropy and train_labels
    take.  details=True appends a dict with cells, centroids, normals, point_voxel, qs, n, seed_voxels, owners, counts,
    rounds, min_seed.  Raises ValueError before any launch for what the definition refuses."""
    rv, rs = float(voxel_resolution), float(seed_resolution)
    w_s, w_n = float(spatial_importance), float(normal_importance)
    frames, xyz, ptr, single = _scan_batch(points, 'vccs_supervoxels', lambda fr: _check_vccs(fr, rv, rs, w_s, w_n))
    min_seed, rounds = vccs_parameters(rv, rs)
    n, dev = len(frames), xyz.device
    p = int(ptr[-1])
    i32 = dict(dtype=torch.int32, device=dev)
    labels = torch.empty(p, dtype=torch.int64, device=dev)
    point_voxel, cells, nv = torch.empty(p, **i32), torch.empty((p, 3), **i32), torch.empty(p, **i32)
    qs = torch.empty((p, 3), dtype=torch.int64, device=dev)
    cen = torch.empty((p, 3), dtype=torch.float64, device=dev)
    nrm = torch.empty((p, 3), dtype=torch.float64, device=dev)
    seed_voxels, owners, order, counts = (torch.empty(p, **i32) for _ in range(4))
    status = torch.empty(4 + 2 * (n + 1), dtype=torch.int64, device=dev)
    nbytes = B.lib().lidal_vccs_workspace_bytes(p, n)
    ws = B.workspace(nbytes, dev)
    B.check(B.lib().lidal_vccs(B.ptr(xyz), ptr.ctypes.data, n, rv, rs, w_s, w_n, min_seed, rounds, B.ptr(labels),
                               B.ptr(point_voxel), B.ptr(cells), B.ptr(qs), B.ptr(nv), B.ptr(cen), B.ptr(nrm),
                               B.ptr(seed_voxels), B.ptr(owners), B.ptr(order), B.ptr(counts), B.ptr(status), B.ptr(ws),
                               nbytes, B.stream()), 'vccs')
    host = torch.cat([status, counts.long()]).cpu().numpy()                    # the one read-back
    st, counts_h = host[:status.numel()], host[status.numel():]
    if st[0] != 0:
        raise RuntimeError('vccs_supervoxels: %s (error word %d)' % (_VCCS_ERRORS.get(int(st[0]), '?'), int(st[0])))
    vptr, sptr = st[4:4 + n + 1], st[4 + n + 1:4 + 2 * (n + 1)]
    out = []
    for f in range(n):
        a, b = int(ptr[f]), int(ptr[f + 1])
        v0, v1, s0, s1 = int(vptr[f]), int(vptr[f + 1]), int(sptr[f]), int(sptr[f + 1])
        sizes = counts_h[s0:s1]
        keep = sizes > min_points
        starts = (b - a) - int(sizes.sum()) + np.concatenate([[0], np.cumsum(sizes)[:-1]]) if s1 > s0 else sizes
        local = order[a:b].long() - a                          # the scan's points by (label, point); label 0 first
        parts = [local[int(t):int(t) + int(c)] for t, c in zip(starts[keep], sizes[keep])]
        sv_idx = torch.cat(parts) if parts else torch.empty(0, dtype=torch.int64, device=dev)
        item = (labels[a:b], _sv_ptr(sizes[keep], dev), sv_idx)
        if details:
            item += (dict(cells=cells[v0:v1], centroids=cen[v0:v1], normals=nrm[v0:v1], qs=qs[v0:v1], n=nv[v0:v1],
                          point_voxel=point_voxel[a:b].long() - v0, seed_voxels=seed_voxels[s0:s1].long() - v0,
                          owners=owners[v0:v1].long(), counts=counts[s0:s1], rounds=rounds, min_seed=min_seed),)
        out.append(item)
    return out[0] if single else out


MAX_CLUSTER_SCANS = 32
MAX_CLUSTER_POINTS = 2 ** 30 - 1
N_CLUSTER_CLASSES = 64
_CLUSTER_ERRORS = {1: 'a live point lies outside the 21 bits per axis of the cell key',
                   2: 'a union-find walk ran out of its step bound'}


class Instances:
    """The instances of one euclidean_clusters call.  On the device: inst i32 [P] (-1: no instance), cls i32 [K],
    member_ptr i64 [K+1], members i32 (point rows of the batch, ascending within an instance), bbox f32 [K,6] (min x,
    y, z, max x, y, z) and sizes i64 [K].  On the host: inst_ptr i64 [S+1] (scan s owns the ids inst_ptr[s] ..
    inst_ptr[s+1]), point_ptr i64 [S+1] of the input and member_start i64 [S+1] = member_ptr[inst_ptr]."""
    __slots__ = ('inst', 'inst_ptr', 'cls', 'member_ptr', 'members', 'bbox', 'sizes', 'point_ptr', 'member_start')

    def __init__(self, **kw):
        for k in Instances.__slots__:
            setattr(self, k, kw[k])

    def __len__(self):
        return int(self.inst_ptr[-1])

    def as_csr(self, scan):
        """(ptr i64 [n+1], members i64) of scan `scan`'s n instances with scan-local rows: the sv_csr of train_labels."""
        k0, k1 = int(self.inst_ptr[scan]), int(self.inst_ptr[scan + 1])
        m0, m1 = int(self.member_start[scan]), int(self.member_start[scan + 1])
        return self.member_ptr[k0:k1 + 1] - m0, self.members[m0:m1].long() - int(self.point_ptr[scan])


def _tolerance_table(tolerance, what):
    tol = np.zeros(N_CLUSTER_CLASSES, dtype=np.float32)
    items = tolerance.items() if isinstance(tolerance, dict) else [(c, tolerance) for c in range(N_CLUSTER_CLASSES)]
    for c, t in items:
        if not 0 <= int(c) < N_CLUSTER_CLASSES or int(c) != c:
            raise ValueError('%s: class id %r is outside 0..63' % (what, c))
        t32 = np.float32(t)
        if not (t32 >= 0):
            raise ValueError('%s: the tolerance %r of class %d is negative or NaN' % (what, t, c))
        if t32 > 0 and not 2.0 ** -10 <= t32 <= 2.0 ** 10:
            raise ValueError('%s: the tolerance %r of class %d is outside [2^-10, 2^10] m' % (what, t, c))
        tol[int(c)] = t32
    return tol


def euclidean_clusters(points, labels=None, tolerance=0.5, min_points=1, max_points=None):
    """Instance ids by Euclidean clustering on the GPU (what PCL calls EuclideanClusterExtraction,
    in this project's own definition -- PCL's cluster order is not reproduced, the partition is the same): the connected
    components of the graph that joins two points of one scan and one class c whose f32 distance is below tolerance[c].

      points      f32 [P,3] on the GPU, or a list of 1..32 such scans (one call), as vccs_supervoxels takes them
      labels      i64 [P] (or a list): the labels_p of train_labels, or predictions; None: every point has class 0.
                  A point with a label outside 0..63, a class without a tolerance or a coordinate that is not finite has
                  no instance and joins nothing.
      tolerance   metres, one float for every class or {class: metres}; 0 = the class is not clustered
      min_points, max_points   the sizes kept (max_points=None: any)
    Returns an Instances record; the ids run scan after scan, in ascending order of an instance's smallest row.  One
    read-back (the instance counts).  ValueError, before the device is touched, for what the definition refuses, and
    after the call for a live point too far out for the cell key."""
    what = 'euclidean_clusters'
    tol = _tolerance_table(tolerance, what)
    if int(min_points) != min_points or min_points < 1:
        raise ValueError('%s: min_points=%r must be an integer >= 1' % (what, min_points))
    if max_points is not None and (int(max_points) != max_points or max_points < min_points):
        raise ValueError('%s: max_points=%r is below min_points=%r' % (what, max_points, min_points))

    def check(frames):
        if len(frames) > MAX_CLUSTER_SCANS:
            raise ValueError('%s: %d scans in one call (at most %d)' % (what, len(frames), MAX_CLUSTER_SCANS))
        if sum(x.shape[0] for x in frames) > MAX_CLUSTER_POINTS:
            raise ValueError('%s: %d points in one batch (fewer than 2^30)' % (what, sum(x.shape[0] for x in frames)))
        if labels is not None:
            labs = [labels] if torch.is_tensor(labels) else list(labels)
            if len(labs) != len(frames) or any(not torch.is_tensor(l) or l.numel() != x.shape[0]
                                               for l, x in zip(labs, frames)):
                raise ValueError('%s: the labels must match the points, scan by scan' % what)

    frames, xyz, ptr, _ = _scan_batch(points, what, check)
    n, dev, p = len(frames), xyz.device, int(ptr[-1])
    lab_all = None
    if labels is not None:
        labs = [labels] if torch.is_tensor(labels) else list(labels)
        B.require_gpu(*labs)
        labs = [l.to(torch.int64).contiguous().reshape(-1) for l in labs]
        lab_all = labs[0] if len(labs) == 1 else torch.cat(labs)
    max_points = max(p, int(min_points)) if max_points is None else int(max_points)
    i32 = dict(dtype=torch.int32, device=dev)
    inst = torch.full((p,), -1, **i32)
    if p == 0 or not (tol > 0).any():                                          # no instance: nothing to launch
        zero = np.zeros(n + 1, dtype=np.int64)
        return Instances(inst=inst, inst_ptr=zero, cls=torch.empty(0, **i32),
                         member_ptr=torch.zeros(1, dtype=torch.int64, device=dev), members=torch.empty(0, **i32),
                         bbox=torch.empty((0, 6), dtype=torch.float32, device=dev),
                         sizes=torch.empty(0, dtype=torch.int64, device=dev), point_ptr=ptr, member_start=zero.copy())
    cls, members = B.empty(p, torch.int32, dev), B.empty(p, torch.int32, dev)
    member_ptr = B.empty(p + 1, torch.int64, dev)
    bbox = B.empty((p, 6), torch.float32, dev)
    status = torch.empty(1 + 2 * (n + 1), dtype=torch.int64, device=dev)
    nbytes = B.lib().lidal_euclidean_clusters_workspace_bytes(p, n)
    ws = B.workspace(nbytes, dev)
    B.check(B.lib().lidal_euclidean_clusters(B.ptr(xyz), B.ptr(lab_all), p, ptr.ctypes.data, n, tol.ctypes.data,
                                             int(min_points), max_points, B.ptr(inst), B.ptr(cls), B.ptr(member_ptr),
                                             B.ptr(members), B.ptr(bbox), B.ptr(status), B.ptr(ws), nbytes, B.stream()),
            'euclidean_clusters')
    host = status.cpu().numpy()                                                # the one read-back
    if host[0] == 1:
        raise ValueError('%s: %s' % (what, _CLUSTER_ERRORS[1]))
    if host[0] != 0:
        raise RuntimeError('%s: %s (error word %d)' % (what, _CLUSTER_ERRORS.get(int(host[0]), '?'), int(host[0])))
    inst_ptr, member_start = host[1:n + 2].copy(), host[n + 2:2 * n + 3].copy()
    k, m = int(inst_ptr[-1]), int(member_start[-1])
    member_ptr = member_ptr[:k + 1]
    return Instances(inst=inst, inst_ptr=inst_ptr, cls=cls[:k], member_ptr=member_ptr, members=members[:m], bbox=bbox[:k],
                     sizes=member_ptr[1:] - member_ptr[:-1], point_ptr=ptr, member_start=member_start)


def draw_instance_paste(instances, scan, rng=np.random, classes=(), n_inst=1):
    """A paste mask for mix_scans(paste_masks=...): bool [P_scan] on the device, set on the rows of the chosen instances
    of scan `scan`.  The candidates are the scan's instances whose class is in `classes`, in id order; ONE
    rng.choice(len(candidates), size=min(n_inst, len(candidates)), replace=False) picks among them.  Without candidates
    (or with n_inst = 0) nothing is drawn and the mask is empty.  The classes are read back (one small copy)."""
    k0, k1 = int(instances.inst_ptr[scan]), int(instances.inst_ptr[scan + 1])
    a, b = int(instances.point_ptr[scan]), int(instances.point_ptr[scan + 1])
    wanted = sorted(set(int(c) for c in classes))
    cls = instances.cls[k0:k1].cpu().numpy() if k1 > k0 else np.zeros(0, dtype=np.int32)
    cand = k0 + np.nonzero(np.isin(cls, wanted))[0]
    local = instances.inst[a:b]
    take = min(int(n_inst), len(cand))
    if take <= 0:
        return torch.zeros(b - a, dtype=torch.bool, device=local.device)
    chosen = cand[np.asarray(rng.choice(len(cand), size=take, replace=False)).reshape(-1)]
    return torch.isin(local, torch.from_numpy(chosen.astype(np.int32)).to(local.device))


def supervoxel_tables(labels_per_frame, frame_names, ignore_label=None, min_points=0):
    """prepare_supervoxel_kmeans_sk.py:54-80 on host arrays: the per-frame supervoxel labels (arrays or tensors, in
    the order of the sorted label files) and their (sequence, frame name) pairs -> (tables, id2sv): per frame
    (sv_id i64 [S], sv2point list of i64 arrays) as io.save_supervoxels writes them -- supervoxels in np.unique(labels)
    order with ascending point ids, a cluster without points dropped, sv_id running across the frames -- and the
    id2sv list of (sequence, frame name, supervoxel of the frame) that io.save_id2sv writes.

    ignore_label=0, min_points=100 gives prepare_supervoxel_VCCS_sk.py:58-92: label 0 ("no supervoxel") is dropped and
    so is every supervoxel of min_points points or fewer; the supervoxels that stay are numbered 0.. inside the frame
    in label order.  The defaults drop nothing."""
    if len(labels_per_frame) != len(frame_names):
        raise ValueError('%d label arrays for %d frame names' % (len(labels_per_frame), len(frame_names)))
    tables, id2sv, next_id = [], [], 0
    for lab, (seq, name) in zip(labels_per_frame, frame_names):
        lab = lab.detach().cpu().numpy() if torch.is_tensor(lab) else np.asarray(lab)
        lab = lab.reshape(-1)
        order = np.argsort(lab, kind='stable')                    # by (label, point)
        values, starts = np.unique(lab[order], return_index=True)
        sv2point = [part.astype(np.int64) for part in np.split(order, starts[1:])] if len(values) else []
        if ignore_label is not None or min_points > 0:
            sv2point = [part for value, part in zip(values, sv2point)
                        if (ignore_label is None or value != ignore_label) and len(part) > min_points]
        sv_id = np.arange(len(sv2point), dtype=np.int64) + next_id
        next_id += len(sv2point)
        tables.append((sv_id, sv2point))
        id2sv.extend((seq, name, local) for local in np.arange(len(sv2point)))
    return tables, id2sv
