"""Validation mIoU on the GPU: counterpart of /root/reference/evaluate.py:95-124 and
utils/iou_sk.py:14-52.  The reference copies the logits to the host, gathers
voxel -> point, arg-maxes and bincounts in numpy per batch, then all-reduces the 19x19 int32 matrix;
here one kernel per batch accumulates the matrix on the device and the same all-reduce follows.

Panoptic quality beside it (csrc/panoptic.hip): predicted instances -- the model's argmax run
through data.euclidean_clusters, the baseline of the SemanticKITTI panoptic benchmark -- scored against the annotated
ones, the per-class sums accumulated on the device in the same way."""
import numpy as np
import torch
import torch.distributed as dist

from . import SparseTensor
from . import backend as B

__all__ = ['confusion_accumulate', 'evaluate_batches', 'iou_from_confusion', 'PanopticStats', 'panoptic_accumulate',
           'panoptic_quality', 'evaluate_panoptic_batches']


def confusion_accumulate(conf, logits_v_b, inverse_indices_b, labels_p_b):
    """conf i32 [C, C] (device, updated in place) += confusion of this batch
    (rows = prediction, columns = ground truth, labels >= 100 ignored: iou_sk.py:17)."""
    B.require_gpu(conf, logits_v_b, inverse_indices_b, labels_p_b)
    logits = logits_v_b.contiguous().float()
    inv = inverse_indices_b.contiguous().long()
    lab = labels_p_b.contiguous().long()
    assert conf.dtype == torch.int32 and conf.is_contiguous() and inv.shape == lab.shape
    c = logits.shape[1]
    B.check(B.lib().lidal_confusion_accumulate(B.ptr(logits), B.ptr(inv), B.ptr(lab), inv.numel(), c,
                                               B.ptr(conf), B.stream()), 'confusion_accumulate')
    return conf


def iou_from_confusion(confusion):
    """utils/iou_sk.py:21-52 without the printing: (per-class IoU list, mean IoU)."""
    confusion = np.asarray(confusion)
    n = confusion.shape[0]
    ious = []
    for i in range(n):
        tp = np.int32(confusion[i, i])
        fp = np.int32(confusion[i, :].sum()) - tp
        fn = np.int32(confusion[:, i].sum()) - tp
        denom = tp + fp + fn
        ious.append(float('nan') if denom == 0 else float(tp) / denom)
    return ious, sum(ious) / n


@torch.no_grad()
def evaluate_batches(model, batches, n_classes=19, group=None):
    """batches: iterable of dicts with coords_v_b, feats_v_b, inverse_indices_b, labels_p_b on the
    GPU (the reference's val collate).  Returns (confusion i32 [C,C] numpy, per-class IoU, mIoU)."""
    model.eval()
    # on the model's device from the start: a rank without batches still joins the all-reduce
    conf = torch.zeros((n_classes, n_classes), dtype=torch.int32, device=next(model.parameters()).device)
    for b in batches:
        logits, _ = model(SparseTensor(b['feats_v_b'], b['coords_v_b']))
        confusion_accumulate(conf, logits, b['inverse_indices_b'], b['labels_p_b'])
    if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
        dist.all_reduce(conf, op=dist.ReduceOp.SUM, group=group)          # evaluate.py:117-119
    conf = conf.cpu().numpy()
    ious, miou = iou_from_confusion(conf)
    return conf, ious, miou


# ---- panoptic quality ---------------------------------------------------------------------------
MAX_PANOPTIC_CLASSES = 64     # csrc/panoptic.hip: 6 class bits in a segment key, one bit per class in `things`
MAX_PANOPTIC_SCANS = 32
MAX_PANOPTIC_POINTS = 2 ** 30 - 1
_PANOPTIC_ERRORS = {1: 'an instance value of a thing class outside [-1, 2^30 - 2]'}
_PQ_EPS = 1e-15


class PanopticStats:
    """The accumulators of panoptic_accumulate, zeroed: tp, fp, fn i64 [C], iou f64 [C] and the status word i64 [1], on
    `device` (a GPU for panoptic_accumulate; 'cpu' holds a read-back copy)."""
    __slots__ = ('n_classes', 'tp', 'fp', 'fn', 'iou', 'status')

    def __init__(self, n_classes, device):
        if int(n_classes) != n_classes or not 1 <= n_classes <= MAX_PANOPTIC_CLASSES:
            raise ValueError('PanopticStats: n_classes=%r is outside 1..%d' % (n_classes, MAX_PANOPTIC_CLASSES))
        self.n_classes = int(n_classes)
        self.tp, self.fp, self.fn = (torch.zeros(self.n_classes, dtype=torch.int64, device=device) for _ in range(3))
        self.iou = torch.zeros(self.n_classes, dtype=torch.float64, device=device)
        self.status = torch.zeros(1, dtype=torch.int64, device=device)

    def tensors(self):
        return self.tp, self.fp, self.fn, self.iou, self.status

    def cpu(self):
        """A copy on the host (one synchronisation)."""
        out = PanopticStats(self.n_classes, 'cpu')
        for name in ('tp', 'fp', 'fn', 'iou', 'status'):
            setattr(out, name, getattr(self, name).cpu())
        return out


def _things_mask(things, n_classes, what):
    mask = 0
    for c in things:
        if int(c) != c or not 0 <= int(c) < n_classes:
            raise ValueError('%s: thing class %r is outside 0..%d' % (what, c, n_classes - 1))
        mask |= 1 << int(c)
    return mask


def panoptic_accumulate(stats, pred_sem, pred_inst, gt_sem, gt_inst, things, min_points=50):
    """stats (a PanopticStats on the GPU, updated in place) += the panoptic sums of this batch: one library call, nothing
    read back (lidal_panoptic_accumulate; include/lidal_amd.h carries the definition).

      pred_sem, gt_sem    integer class per point: a tensor [P], or a list of 1..32 per-scan tensors as euclidean_clusters
                          takes them.  A point whose gt_sem is outside [0, C) (the ignore label 255) is void and counts
                          nowhere; a pred_sem outside [0, C) is no prediction.
      pred_inst, gt_inst  integer instance per point, the same layout: Instances.inst (-1: no instance) resp.
                          data.instance_ids.  Ids are per scan; the columns of stuff rows are not looked at.
      things              the class ids that have instances (data.SK_THINGS); every other class is stuff
      min_points          an unmatched segment smaller than this is neither a false positive nor a false negative
    ValueError before the device is touched for mismatched lengths, more than 64 classes or 32 scans, a thing id
    outside [0, C) or min_points < 1.  An instance value out of range sets the status word: panoptic_quality raises."""
    what = 'panoptic_accumulate'
    if not isinstance(stats, PanopticStats):
        raise ValueError('%s: stats must be a PanopticStats' % what)
    c = stats.n_classes
    if not 1 <= c <= MAX_PANOPTIC_CLASSES:
        raise ValueError('%s: %d classes (at most %d)' % (what, c, MAX_PANOPTIC_CLASSES))
    mask = _things_mask(things, c, what)
    if int(min_points) != min_points or min_points < 1:
        raise ValueError('%s: min_points=%r must be an integer >= 1' % (what, min_points))
    cols = []
    for name, col in (('pred_sem', pred_sem), ('pred_inst', pred_inst), ('gt_sem', gt_sem), ('gt_inst', gt_inst)):
        col = [col] if torch.is_tensor(col) else list(col)
        if not col or any(not torch.is_tensor(t) or t.is_floating_point() for t in col):
            raise ValueError('%s: %s must be an integer tensor or a list of them' % (what, name))
        cols.append(col)
    sizes = [t.numel() for t in cols[0]]
    if any([t.numel() for t in col] != sizes for col in cols[1:]):
        raise ValueError('%s: the four columns must have the same lengths, scan by scan' % what)
    if len(sizes) > MAX_PANOPTIC_SCANS:
        raise ValueError('%s: %d scans in one call (at most %d)' % (what, len(sizes), MAX_PANOPTIC_SCANS))
    if sum(sizes) > MAX_PANOPTIC_POINTS:
        raise ValueError('%s: %d points in one batch (fewer than 2^30)' % (what, sum(sizes)))
    B.require_gpu(*stats.tensors(), *[t for col in cols for t in col])
    dev = stats.tp.device
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n, p = len(sizes), int(ptr[-1])
    if p == 0:
        return stats

    def flat(col, dtype):
        col = [t.to(dtype).contiguous().reshape(-1) for t in col]
        return col[0] if len(col) == 1 else torch.cat(col)

    ps, gs = flat(cols[0], torch.int64), flat(cols[2], torch.int64)
    pi, gi = flat(cols[1], torch.int32), flat(cols[3], torch.int32)
    nbytes = B.lib().lidal_panoptic_accumulate_workspace_bytes(p, n)
    ws = B.workspace(nbytes, dev)
    B.check(B.lib().lidal_panoptic_accumulate(B.ptr(ps), B.ptr(pi), B.ptr(gs), B.ptr(gi), p, ptr.ctypes.data, n, c, mask,
                                              int(min_points), B.ptr(stats.tp), B.ptr(stats.fp), B.ptr(stats.fn),
                                              B.ptr(stats.iou), B.ptr(stats.status), B.ptr(ws), nbytes, B.stream()),
            'panoptic_accumulate')
    return stats


def panoptic_quality(stats, things):
    """The accumulators read back once -> a dict of f64 numpy arrays [C] and floats:
        sq = iou / max(tp, eps), rq = tp / max(tp + 0.5 fp + 0.5 fn, eps), pq = sq * rq        (eps = 1e-15)
        PQ, SQ, RQ           the means over all C classes (the benchmark's: an absent class counts as 0)
        PQ_th, SQ_th, RQ_th  over the thing classes;  PQ_st, SQ_st, RQ_st over the stuff classes (nan if there is none)
        present              bool [C]: tp + fp + fn > 0
    ValueError if the status word is set (an instance value was out of range in some call)."""
    what = 'panoptic_quality'
    c = stats.n_classes
    mask = _things_mask(things, c, what)
    tp, fp, fn, iou, status = (t.cpu().numpy() for t in stats.tensors())
    if int(status[0]) != 0:
        raise ValueError('%s: %s (error word %d)' % (what, _PANOPTIC_ERRORS.get(int(status[0]), '?'), int(status[0])))
    tp, fp, fn = (a.astype(np.float64) for a in (tp, fp, fn))
    sq = iou.astype(np.float64) / np.maximum(tp, _PQ_EPS)
    rq = tp / np.maximum(tp + 0.5 * fp + 0.5 * fn, _PQ_EPS)
    pq = sq * rq
    is_thing = np.array([(mask >> k) & 1 == 1 for k in range(c)], dtype=bool)
    out = {'pq': pq, 'sq': sq, 'rq': rq, 'present': (tp + fp + fn) > 0}

    def mean(a, sel):
        return float(a[sel].mean()) if sel.any() else float('nan')

    for name, a in (('PQ', pq), ('SQ', sq), ('RQ', rq)):
        out[name] = float(a.mean())
        out[name + '_th'] = mean(a, is_thing)
        out[name + '_st'] = mean(a, ~is_thing)
    return out


@torch.no_grad()
def evaluate_panoptic_batches(model, batches, things, tolerance, min_points=50, cluster_min_points=1, n_classes=19,
                              group=None):
    """From a model and raw scans to PQ: per batch of data.val_batch(..., with_instances=True) -- the val collate plus
    the per-scan `points` and `gt_inst` -- the logits give the per-point argmax through inverse_indices_b,
    data.euclidean_clusters(points, argmax, tolerance, min_points=cluster_min_points) gives the predicted instances, and
    panoptic_accumulate adds the batch to the sums; the semantic confusion is accumulated beside it by
    confusion_accumulate.  `tolerance` is euclidean_clusters': metres, or {class: metres} -- name the thing classes only,
    a stuff class needs no clusters.  With a process group up the sums are all-reduced as evaluate_batches' are; with
    more than two ranks the f64 IoU sums are then added in the collective's order, not a fixed one.
    Returns (PanopticStats on the host, panoptic_quality's dict, confusion i32 [C,C] numpy, mIoU)."""
    from . import data
    things = tuple(things)
    model.eval()
    dev = next(model.parameters()).device
    stats = PanopticStats(n_classes, dev)
    conf = torch.zeros((n_classes, n_classes), dtype=torch.int32, device=dev)
    for b in batches:
        logits, _ = model(SparseTensor(b['feats_v_b'], b['coords_v_b']))
        confusion_accumulate(conf, logits, b['inverse_indices_b'], b['labels_p_b'])
        pred = logits.argmax(1)[b['inverse_indices_b'].long()]
        sizes = [x.shape[0] for x in b['points']]
        pred_scans = list(torch.split(pred, sizes))
        inst = data.euclidean_clusters(b['points'], pred_scans, tolerance=tolerance, min_points=cluster_min_points)
        panoptic_accumulate(stats, pred_scans, list(torch.split(inst.inst, sizes)),
                            list(torch.split(b['labels_p_b'], sizes)), list(b['gt_inst']), things, min_points)
    if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
        for t in (conf,) + stats.tensors()[:4]:
            dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
        dist.all_reduce(stats.status, op=dist.ReduceOp.MAX, group=group)
    host = stats.cpu()
    conf = conf.cpu().numpy()
    _, miou = iou_from_confusion(conf)
    return host, panoptic_quality(host, things), conf, miou
