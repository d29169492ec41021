"""Frame-level selection on the GPU: the baselines the reference ships in score/frame_level/.

  frame_uncertainty   softmax_entropy.py / margin_sampling.py / least_confidence_sampling.py worker_func for one frame:
                      the means of the per-point entropy, margin (top1 - top2) and confidence (top1), one pass over
                      prob (lidal_frame_uncertainty)
  segment_entropy     segment_entropy.py worker_func: the size-weighted log2 entropy of each supervoxel's predicted-class
                      histogram, summed over the frame (lidal_segment_entropy)
  frame_feature       core_set.py:66, outfeat.mean(0) (lidal_frame_feature)
  coreset             core_set.py:74-92, the greedy k-center over all frames' features (lidal_coreset)
  select_frames       the 1 % top-k of ENT / MAR / CONF / SEGENT (see reference_zero_half below)
  random_frames       frame_level/RAND.py's draw
  VIEWD / VIEWE / VOTE  beyond the reference: how much the augmented views of a frame disagreed (view_level.py)
  BALD / MCENT          MC-dropout: the frame means of the mutual information and of the passes' mean entropy
                        (mc_dropout.py); VOTE beside them is the variation ratio of the passes
  frame_sequence      infer_frame per frame, then only the requested scores (scalars, or a [96] vector for CSET)
  FrameBoard          all sequences' frames in train_split order (the reference's seq_offsets), the per-sequence flags

The reference writes prob (and outfeat for CSET) of every frame to disk and reads it back in a CPU pool; here every
score is a reduction of tensors infer_frame already holds on the device, and only a few numbers per frame stay
resident.  Orders and bars: DESIGN.md section 9.
"""
import numpy as np
import torch

from .. import backend as B
from .. import io

__all__ = ['frame_uncertainty', 'segment_entropy', 'frame_feature', 'coreset', 'num_to_add', 'select_frames',
           'random_frames', 'frame_sequence', 'FrameBoard', 'METRICS', 'SK_TRAIN_SPLIT']

METRICS = ('ENT', 'MAR', 'CONF', 'SEGENT', 'CSET', 'VIEWD', 'VIEWE', 'VOTE', 'BALD', 'MCENT')
LARGEST = {'ENT': True, 'MAR': True, 'CONF': False, 'SEGENT': True,       # MAR: "largest", as the reference (sic)
           'VIEWD': True, 'VIEWE': True, 'VOTE': True, 'BALD': True, 'MCENT': True}
VIEW_METRICS = ('VIEWD', 'VIEWE', 'VOTE')
MC_METRICS = ('BALD', 'MCENT')
SK_TRAIN_SPLIT = ['00', '01', '02', '03', '04', '05', '06', '07', '09', '10']
MAX_CLASSES = 32
MAX_FEAT_DIM = 128


def _device_f32(x, what):
    if not torch.is_tensor(x):
        x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()
    B.require_gpu(x)
    x = x.float().contiguous()
    if not bool(torch.isfinite(x).all()):
        raise ValueError('%s: the input must be finite (NaN or inf found)' % what)
    return x


def frame_uncertainty(prob):
    """np.mean(entropy(prob, axis=1)), np.mean(top1 - top2) and np.mean(top1) of one frame's prob f32 [P, C]
    (2 <= C <= 32) as three f32 0-d device tensors (ent, mar, conf)."""
    prob = _device_f32(prob, 'frame_uncertainty')
    if prob.ndim != 2:
        raise ValueError('frame_uncertainty: prob must be [P, C], got %s' % (tuple(prob.shape),))
    p, c = prob.shape
    if not 2 <= c <= MAX_CLASSES:
        raise ValueError('frame_uncertainty: C=%d classes; 2..%d are supported (the margin needs two)' %
                         (c, MAX_CLASSES))
    out = torch.empty(3, dtype=torch.float32, device=prob.device)
    nbytes = B.lib().lidal_frame_uncertainty_workspace_bytes(p)
    ws = B.workspace(nbytes, prob.device)
    B.check(B.lib().lidal_frame_uncertainty(B.ptr(prob), p, c, B.ptr(out), B.ptr(ws), nbytes, B.stream()),
            'frame_uncertainty')
    return out[0], out[1], out[2]


def segment_entropy(pred, sv_ptr, sv_idx, class_num):
    """segment_entropy.py::worker_func for one frame on device tensors: pred i64 [P], the supervoxel CSR of
    interframe.sv_csr.  f64 0-d device tensor; NaN if a supervoxel is empty (the reference's 0 / 0)."""
    B.require_gpu(pred, sv_ptr, sv_idx)
    pred = pred.to(torch.int64).contiguous()
    sv_ptr = sv_ptr.to(torch.int64).contiguous()
    sv_idx = sv_idx.to(torch.int64).contiguous()
    p = pred.numel()
    s = sv_ptr.numel() - 1
    if class_num < 1:
        raise ValueError('segment_entropy: class_num must be positive')
    if sv_idx.numel() and (int(sv_idx.min()) < 0 or int(sv_idx.max()) >= p):
        raise ValueError('segment_entropy: supervoxel point ids outside [0, %d)' % p)
    out = torch.empty((), dtype=torch.float64, device=pred.device)
    nbytes = B.lib().lidal_segment_entropy_workspace_bytes(s)
    ws = B.workspace(nbytes, pred.device)
    B.check(B.lib().lidal_segment_entropy(B.ptr(pred), p, B.ptr(sv_ptr), B.ptr(sv_idx), s, int(class_num), B.ptr(out),
                                          B.ptr(ws), nbytes, B.stream()), 'segment_entropy')
    return out


def frame_feature(feat):
    """core_set.py:66, outfeat.mean(0) of feat f32 [P, D]: f32 [D] device tensor, bit for bit."""
    feat = _device_f32(feat, 'frame_feature')
    if feat.ndim != 2:
        raise ValueError('frame_feature: feat must be [P, D], got %s' % (tuple(feat.shape),))
    p, d = feat.shape
    out = torch.empty(d, dtype=torch.float32, device=feat.device)
    nbytes = B.lib().lidal_frame_feature_workspace_bytes(p)
    ws = B.workspace(nbytes, feat.device)
    B.check(B.lib().lidal_frame_feature(B.ptr(feat), p, d, B.ptr(out), B.ptr(ws), nbytes, B.stream()), 'frame_feature')
    return out


def num_to_add(n_frames):
    """round(0.01 * N): the reference's per-round budget (Python's round, halves to even)."""
    return int(round(0.01 * n_frames))


def _host_bool(flags):
    flags = flags.detach().cpu().numpy() if torch.is_tensor(flags) else np.asarray(flags)
    return flags.astype(bool).reshape(-1)


def coreset(feats, labeled, num_add=None, return_min_dist=False):
    """core_set.py:74-92: the greedy k-center over feats f32 [N, D] (D <= 128; one frame_feature per frame) from the
    labeled frames (bool [N]).  num_add defaults to round(0.01 N).  Returns (picks i64 [num_add] device tensor in pick
    order, new flags bool [N] numpy), and the final min_dist f32 [N] device tensor with return_min_dist.  Raises
    ValueError where the reference fails: no labeled frame, or a pick that is selected already (all remaining
    distances 0)."""
    feats = _device_f32(feats, 'coreset')
    if feats.ndim != 2:
        raise ValueError('coreset: feats must be [N, D], got %s' % (tuple(feats.shape),))
    n, d = feats.shape
    if not 1 <= d <= MAX_FEAT_DIM:
        raise ValueError('coreset: the feature width must be in 1..%d' % MAX_FEAT_DIM)
    flags = _host_bool(labeled)
    if flags.shape[0] != n:
        raise ValueError('coreset: %d flags for %d frames' % (flags.shape[0], n))
    lab = np.where(flags)[0]
    if lab.size == 0:
        raise ValueError('coreset: no labeled frame (the reference fails on np.min over an empty axis)')
    num_add = num_to_add(n) if num_add is None else int(num_add)
    if not 0 <= num_add <= n - lab.size:
        raise ValueError('coreset: num_add=%d must be in 0..%d, the unlabeled count' % (num_add, n - lab.size))
    dev = feats.device
    lab_dev = torch.from_numpy(lab.astype(np.int64)).to(dev)
    picks = torch.empty(num_add, dtype=torch.int64, device=dev)
    min_dist = torch.empty(n, dtype=torch.float32, device=dev)
    status = torch.empty(2, dtype=torch.int32, device=dev)
    nbytes = B.lib().lidal_coreset_workspace_bytes(n, num_add)
    ws = B.workspace(nbytes, dev)
    B.check(B.lib().lidal_coreset(B.ptr(feats), n, d, B.ptr(lab_dev), lab.size, num_add, B.ptr(picks), B.ptr(min_dist),
                                  B.ptr(status), B.ptr(ws), nbytes, B.stream()), 'coreset')
    st = status.cpu().numpy()
    if st[1] != 0 or st[0] < 0:
        raise RuntimeError('coreset: inconsistent device status %s' % st.tolist())
    if st[0] > 0:
        raise ValueError('coreset: pick %d is a frame selected already (every remaining distance is 0; the reference '
                         'asserts here)' % int(st[0]))
    out = flags.copy()
    out[picks.cpu().numpy()] = True
    return (picks, out, min_dist) if return_min_dist else (picks, out)


def select_frames(flags, scores, largest=True, reference_zero_half=False):
    """The 1 % selection of ENT / MAR / CONF / SEGENT over all frames (flags bool [N], scores [N], the frames in
    FrameBoard order): new flags bool [N].  CONF takes largest=False.

    Default: the round(0.01 N) unlabeled frames of largest (smallest) f32 score, ties at the k-th place to the lower
    frame index, NaN ordered as numpy sorts it (above every number).
    reference_zero_half=True: the reference's expression itself.  Its __main__ blocks start the score array from
    np.zeros_like(all_frame_flag) and append the real scores behind it, so unlabeled_ids index the zero half and the
    flags are whatever np.argpartition returns on N equal keys, which depends on the host CPU's numpy dispatch."""
    flags = _host_bool(flags)
    scores = np.asarray(scores.detach().cpu().numpy() if torch.is_tensor(scores) else scores, dtype=np.float32)
    scores = scores.reshape(-1)
    if scores.shape[0] != flags.shape[0]:
        raise ValueError('select_frames: %d scores for %d frames' % (scores.shape[0], flags.shape[0]))
    num_add = num_to_add(flags.shape[0])
    out = flags.copy()
    if reference_zero_half:
        all_scores = np.append(np.zeros_like(flags, dtype=np.float32), scores)
        unlabeled_ids = np.where(flags == False)[0]         # noqa: E712  (the reference's expression)
        unlabeled_scores = all_scores[unlabeled_ids]
        if largest:
            selected_ids = np.argpartition(unlabeled_scores, -num_add)[-num_add:]
        else:
            selected_ids = np.argpartition(unlabeled_scores, num_add)[:num_add]
        out[unlabeled_ids[selected_ids]] = True
        return out
    unl = np.where(~flags)[0]
    s = scores[unl]
    nan = np.isnan(s)
    s0 = np.where(nan, np.float32(0), s)
    order = np.lexsort((unl, -s0, ~nan)) if largest else np.lexsort((unl, s0, nan))
    out[unl[order[:num_add]]] = True
    return out


def random_frames(flags, rng=None):
    """frame_level/RAND.py: round(0.01 N) draws WITH replacement from the unlabeled frames (rng.choice; the numpy
    global generator, as the reference, when rng is None).  New flags bool [N]."""
    flags = _host_bool(flags)
    rng = np.random if rng is None else rng
    frame_flag_all = flags.astype(np.float64)            # the reference appends into np.array([]): float
    unlabeled = np.where(frame_flag_all == False)[0]     # noqa: E712
    selected = rng.choice(unlabeled, int(np.round(0.01 * len(frame_flag_all))))
    out = flags.copy()
    out[selected] = True
    return out


def frame_sequence(model, frames, metrics=('ENT', 'MAR', 'CONF'), inf_reps=8, autocast=False, class_num=None):
    """The scoring pass of the frame-level metrics over one sequence on one GPU: per frame infer_frame (with the [P, 96]
    feature only when CSET is asked), then only the requested values.  Frame dicts are score_sequence's (coords, feats,
    inverse; sv_ptr / sv_idx for SEGENT).  class_num (SEGENT) defaults to the model's class count.  Returns
    {metric: [per frame: f32 0-d (ENT / MAR / CONF / VIEWD / VIEWE / VOTE), f64 0-d (SEGENT) or f32 [D] (CSET) device
    tensor]}.  VIEWD / VIEWE / VOTE come out of the same inference (view_level.frame_view_scores).  BALD / MCENT (f32
    0-d) put the model under nn.mc_dropout for the whole pass (ValueError for a model without counter dropout): the
    `inf_reps` rows of a point are then MC-dropout passes, every other metric asked for in the same call is taken of those
    passes too, and VOTE is their variation ratio (mc_dropout.frame_mc_scores)."""
    import contextlib
    from ..nn import mc_dropout
    from .mc_dropout import frame_mc_scores
    from .prob_inference import infer_frame
    from .view_level import frame_view_scores
    metrics = tuple(metrics)
    bad = [m for m in metrics if m not in METRICS]
    if bad:
        raise ValueError('frame_sequence: unknown metrics %s (known: %s)' % (bad, METRICS))
    want_feat = 'CSET' in metrics
    want_mc = any(m in metrics for m in MC_METRICS)
    want_views = any(m in metrics for m in (VIEW_METRICS[:2] if want_mc else VIEW_METRICS))
    out = {m: [] for m in metrics}
    with (mc_dropout(model) if want_mc else contextlib.nullcontext()):
        for d in frames:
            r = infer_frame(model, d['coords'], d['feats'], d['inverse'], inf_reps, autocast=autocast,
                            return_feat=want_feat, return_view_scores=want_views, return_mc_scores=want_mc)
            prob, pred = r[0], r[1]
            if any(m in metrics for m in ('ENT', 'MAR', 'CONF')):
                ent, mar, conf = frame_uncertainty(prob)
                for m, v in (('ENT', ent), ('MAR', mar), ('CONF', conf)):
                    if m in out:
                        out[m].append(v)
            if 'SEGENT' in out:
                out['SEGENT'].append(segment_entropy(pred, d['sv_ptr'], d['sv_idx'],
                                                     prob.shape[1] if class_num is None else class_num))
            if want_feat:
                out['CSET'].append(frame_feature(r[2]))
            if want_views:
                for m, v in zip(VIEW_METRICS, frame_view_scores(*r[-2 if want_mc else -1], inf_reps)):
                    if m in out:
                        out[m].append(v)
            if want_mc:             # (VOTE: the same agree either way; taken here unless the view scores ran as well)
                for m, v in zip(MC_METRICS + ('VOTE',), frame_mc_scores(*r[-1], inf_reps)):
                    if m in out and not (m == 'VOTE' and want_views):
                        out[m].append(v)
    return out


def _host(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


class FrameBoard:
    """All frames of a split in train_split order (the reference's all_frame_flag and seq_offsets), the per-frame
    scores of one round and the selection.  flags: per sequence the bool flags of the previous round."""

    def __init__(self, flags, train_split=None):
        flags = [_host_bool(f) for f in flags]
        self.train_split = list(train_split) if train_split is not None else None
        self.seq_offsets = [0]
        for f in flags:
            self.seq_offsets.append(self.seq_offsets[-1] + f.shape[0])
        self.flags = np.concatenate(flags) if flags else np.zeros(0, bool)
        self.scores = {}
        self.feats = None

    @classmethod
    def load(cls, root, dataset_name, r_id, metric, model_name=None, train_split=SK_TRAIN_SPLIT):
        """The flags the reference's __main__ starts round r_id from (frame_flag/0r for r_id == 1)."""
        return cls([io.load_frame_flag(io.frame_flag_path(root, dataset_name, s, r_id - 1, metric, model_name))
                    for s in train_split], train_split)

    def __len__(self):
        return self.flags.shape[0]

    def add(self, seq_index, metric, values):
        """values: frame_sequence()[metric] of sequence number seq_index (or host values), one per frame."""
        b, e = self.seq_offsets[seq_index], self.seq_offsets[seq_index + 1]
        if len(values) != e - b:
            raise ValueError('FrameBoard.add: %d values for %d frames of sequence %d' % (len(values), e - b, seq_index))
        if metric == 'CSET':
            rows = np.stack([_host(v) for v in values]).astype(np.float32) if len(values) else None
            if self.feats is None:
                self.feats = np.zeros((len(self), rows.shape[1] if rows is not None else 0), np.float32)
            if rows is not None:
                self.feats[b:e] = rows
        else:
            if metric not in self.scores:
                self.scores[metric] = np.zeros(len(self), np.float32)
            self.scores[metric][b:e] = np.array([float(_host(v)) for v in values], dtype=np.float32)

    def select(self, metric, reference_zero_half=False, rng=None):
        """The new flags of all frames (bool [N]) for one metric; RAND draws from rng."""
        if metric == 'RAND':
            return random_frames(self.flags, rng)
        if metric == 'CSET':
            return coreset(self.feats, self.flags)[1]
        return select_frames(self.flags, self.scores[metric], LARGEST[metric], reference_zero_half)

    def split(self, flags):
        """flags of all frames -> per sequence, as the reference saves them."""
        return [flags[self.seq_offsets[i]:self.seq_offsets[i + 1]] for i in range(len(self.seq_offsets) - 1)]

    def save(self, root, dataset_name, r_id, metric, flags, model_name=None):
        for s, f in zip(self.train_split, self.split(flags)):
            io.save_frame_flag(io.frame_flag_path(root, dataset_name, s, r_id, metric, model_name), f)
