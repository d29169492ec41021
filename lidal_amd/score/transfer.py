"""Annotations and predictions carried across the registered frames of a sequence.

The scorer (interframe.py) finds, for every point of a frame, its nearest point in up to 24 registered neighbour frames.
Here that match table is a product of its own (`match_points`), and two things ride on it:

  * `transfer_labels`: a point nobody annotated takes the label its matched points in the neighbour frames agree on --
    the same surface, labelled once, trains in every frame that sees it;
  * `fuse_predictions`: the mean probability of a point over itself and its matches (the row whose entropy the scorer
    calls intere), its class and its confidence: a temporal ensemble, what `train_labels(pseudo=)` and
    `semi.pseudo_labels(labels=)` take.

One hop: a frame reads the labels it is GIVEN, never what a transfer produced.  Single process; everything stays on the
GPU, `stats` included, until the caller reads it.
"""
import ctypes

import torch

from .. import backend as B
from .interframe import _ptr_array, neighbour_ids

__all__ = ['match_points', 'transfer_labels', 'fuse_predictions', 'transfer_sequence', 'STATS']

MAX_NEI = 32
MAX_CLASSES = 32
# stats i64 [n_classes + 7]: the points given each class, then these
STATS = ('own', 'none', 'weak', 'gated', 'confirmed', 'contradicted', 'invalid')


def _frames(bank, i, frames, nei_num, what):
    if i not in bank.world:
        raise ValueError('%s: frame %r is not in the bank' % (what, i))
    if frames is None:
        frames = neighbour_ids(i, len(bank), nei_num)
    frames = [int(f) for f in frames]
    if len(frames) > MAX_NEI:
        raise ValueError('%s: %d neighbour frames, at most %d' % (what, len(frames), MAX_NEI))
    for f in frames:
        if f not in bank.world:
            raise ValueError('%s: neighbour frame %d is not in the bank' % (what, f))
    return frames


def _check_match(match, n, p, what):
    if not isinstance(match, torch.Tensor):
        raise TypeError('%s: match must be a tensor' % what)
    if match.dtype != torch.int32 or tuple(match.shape) != (n, p) or not match.is_contiguous():
        raise ValueError('%s: match must be a contiguous int32 [%d, %d] tensor (match_points of the same frames)'
                         % (what, n, p))


def _check_i64(t, p, what, name):
    if not isinstance(t, torch.Tensor):
        raise TypeError('%s: %s must be a tensor' % (what, name))
    if t.dtype != torch.int64 or tuple(t.shape) != (p,):
        raise ValueError('%s: %s must be an int64 [%d] tensor' % (what, name, p))


def match_points(bank, i, frames=None, nei_num=24):
    """match i32 [n, P]: match[k, q] = the nearest point of frame frames[k] to point q of frame i within the bank's
    dis_thresh (ties: the lowest index), or -1 -- stage 1 of score_points, kept.  frames: an explicit list of frame ids
    (at most 32), default neighbour_ids(i, len(bank), nei_num)."""
    frames = _frames(bank, i, frames, nei_num, 'match_points')
    q_pts = bank.world[i]
    B.require_gpu(q_pts)
    p, n = q_pts.shape[0], len(frames)
    match = torch.empty((n, p), dtype=torch.int32, device=q_pts.device)
    g_arr = _ptr_array(ctypes.c_void_p, [bank.grid(f) for f in frames])
    p_arr = _ptr_array(ctypes.c_void_p, [bank.world[f] for f in frames])
    n_arr = (ctypes.c_int64 * n)(*[bank.world[f].shape[0] for f in frames])
    B.check(B.lib().lidal_interframe_match(B.ptr(q_pts), p, g_arr, p_arr, n_arr, n, bank.dis_thresh, B.ptr(match),
                                           B.stream()), 'interframe_match')
    return match


def _label_arguments(bank, i, labels, n_classes, frames, nei_num, min_votes, min_agree, gate, match, what):
    """Everything transfer_labels refuses, before the device is touched.  Returns (frames, own labels or None)."""
    if not isinstance(n_classes, int) or isinstance(n_classes, bool):
        raise TypeError('%s: n_classes must be an int' % what)
    if not 1 <= n_classes <= MAX_CLASSES:
        raise ValueError('%s: n_classes must be in 1..%d, got %d' % (what, MAX_CLASSES, n_classes))
    if not isinstance(min_votes, int) or isinstance(min_votes, bool):
        raise TypeError('%s: min_votes must be an int' % what)
    if min_votes < 1:
        raise ValueError('%s: min_votes must be at least 1, got %d' % (what, min_votes))
    if isinstance(min_agree, bool) or not isinstance(min_agree, (int, float)):
        raise TypeError('%s: min_agree must be a number' % what)
    if not 0.0 < float(min_agree) <= 1.0:
        raise ValueError('%s: min_agree must be in (0, 1], got %r' % (what, min_agree))
    if not hasattr(labels, 'get'):
        raise TypeError('%s: labels must map a frame id to its int64 [P] tensor' % what)
    frames = _frames(bank, i, frames, nei_num, what)
    p = bank.world[i].shape[0]
    for f in set(frames + [i]):
        if labels.get(f) is not None:
            _check_i64(labels[f], bank.world[f].shape[0], what, 'labels[%d]' % f)
    if gate is not None:
        _check_i64(gate, p, what, 'gate')
    if match is not None:
        _check_match(match, len(frames), p, what)
    return frames, labels.get(i)


def transfer_labels(bank, i, labels, n_classes, frames=None, nei_num=24, min_votes=1, min_agree=1.0, gate=None,
                    ignore_index=255, match=None, return_votes=False):
    """Labels of frame i with the annotations of its neighbour frames carried over.  labels: {frame id: i64 [P_f]}, a
    frame without an entry votes nothing, labels[i] (if any) are the point's own and win.  A point without a label of
    its own takes the class most of its matched, labelled points have (the lowest class on a tie) when at least
    min_votes of them voted, the winner holds at least min_agree of the votes, and gate (i64 [P], the model's own
    prediction -- the one defence against moving objects), if given, names the same class; otherwise ignore_index.
    Returns (labels_p i64 [P], stats i64 [n_classes + 7] on the GPU: per class, then STATS); with return_votes also
    (votes i32 [P], agree i32 [P]).  match: match_points of the same frames, to share it with fuse_predictions."""
    what = 'transfer_labels'
    frames, own = _label_arguments(bank, i, labels, n_classes, frames, nei_num, min_votes, min_agree, gate, match, what)
    nei_labels = [labels.get(f) for f in frames]
    B.require_gpu(bank.world[i], own, gate, match, *nei_labels)
    if match is None:
        match = match_points(bank, i, frames)
    p, n = bank.world[i].shape[0], len(frames)
    dev = bank.world[i].device
    out = torch.empty(p, dtype=torch.int64, device=dev)
    votes = torch.empty(p, dtype=torch.int32, device=dev)
    agree = torch.empty(p, dtype=torch.int32, device=dev)
    stats = torch.empty(n_classes + len(STATS), dtype=torch.int64, device=dev)
    nei_labels = [t.contiguous() if t is not None else None for t in nei_labels]
    l_arr = (ctypes.c_void_p * n)(*[B.ptr(t) for t in nei_labels])
    n_arr = (ctypes.c_int64 * n)(*[bank.world[f].shape[0] for f in frames])
    own = own.contiguous() if own is not None else None
    gate = gate.contiguous() if gate is not None else None
    B.check(B.lib().lidal_interframe_transfer(B.ptr(match), p, n_classes, n, n_arr, l_arr, B.ptr(own), B.ptr(gate),
                                              int(ignore_index), min_votes, float(min_agree), B.ptr(out), B.ptr(votes),
                                              B.ptr(agree), B.ptr(stats), None, None, None, None, None, None,
                                              B.stream()), 'interframe_transfer')
    return (out, stats, votes, agree) if return_votes else (out, stats)


def fuse_predictions(bank, i, frames=None, nei_num=24, match=None):
    """(prob f32 [P,C], pred i64 [P], conf f32 [P], count i32 [P]) of frame i: the mean probability row of a point over
    itself and its matched points (the scorer's sums: its entropy is intere of score_points), the first maximum of the
    row, that entry, and the number of matches."""
    what = 'fuse_predictions'
    frames = _frames(bank, i, frames, nei_num, what)
    for f in [i] + frames:
        if bank.prob[f] is None:
            raise ValueError('%s: frame %d was added without probabilities (FrameBank.add(world, prob))' % (what, f))
    q_prob = bank.prob[i]
    p, c = q_prob.shape
    if not 1 <= c <= MAX_CLASSES:
        raise ValueError('%s: classes must be in 1..%d, got %d' % (what, MAX_CLASSES, c))
    for f in frames:
        if bank.prob[f].shape[1] != c:
            raise ValueError('%s: frame %d has %d classes, frame %d has %d' % (what, f, bank.prob[f].shape[1], i, c))
    if match is not None:
        _check_match(match, len(frames), p, what)
    B.require_gpu(q_prob, match)
    if match is None:
        match = match_points(bank, i, frames)
    n, dev = len(frames), q_prob.device
    prob = torch.empty((p, c), dtype=torch.float32, device=dev)
    pred = torch.empty(p, dtype=torch.int64, device=dev)
    conf = torch.empty(p, dtype=torch.float32, device=dev)
    count = torch.empty(p, dtype=torch.int32, device=dev)
    f_arr = _ptr_array(ctypes.c_void_p, [bank.prob[f] for f in frames])
    n_arr = (ctypes.c_int64 * n)(*[bank.world[f].shape[0] for f in frames])
    B.check(B.lib().lidal_interframe_transfer(B.ptr(match), p, c, n, n_arr, None, None, None, 255, 1, 1.0, None, None,
                                              None, None, B.ptr(q_prob), f_arr, B.ptr(prob), B.ptr(pred), B.ptr(conf),
                                              B.ptr(count), B.stream()), 'interframe_transfer')
    return prob, pred, conf, count


def transfer_sequence(bank, labels, n_classes, order=None, nei_num=24, min_votes=1, min_agree=1.0, gates=None,
                      ignore_index=255, summary=False):
    """transfer_labels for every frame of the bank (or the frame ids in `order`), each reading the labels it was GIVEN
    and never an output: one hop, so the result does not depend on the order of the frames.  gates: {frame id: i64
    [P_f]} or None.  Returns ({frame id: labels_p}, stats i64 [n_classes + 7] summed over the frames, on the GPU); with
    summary=True the second value is a dict of Python ints instead -- {'classes': [...], 'own': ..., ...} -- at the
    price of the one read-back."""
    what = 'transfer_sequence'
    order = sorted(bank.world) if order is None else [int(f) for f in order]
    if gates is not None and not hasattr(gates, 'get'):
        raise TypeError('%s: gates must map a frame id to its int64 [P] tensor' % what)
    plans = [_label_arguments(bank, i, labels, n_classes, None, nei_num, min_votes, min_agree,
                              gates.get(i) if gates is not None else None, None, what)[0] for i in order]
    out, total = {}, None
    for i, frames in zip(order, plans):
        out[i], stats = transfer_labels(bank, i, labels, n_classes, frames=frames, min_votes=min_votes,
                                        min_agree=min_agree, gate=gates.get(i) if gates is not None else None,
                                        ignore_index=ignore_index)
        total = stats if total is None else total + stats
    if total is None:
        total = torch.zeros(n_classes + len(STATS), dtype=torch.int64)
    if not summary:
        return out, total
    host = total.tolist()
    report = {'classes': host[:n_classes]}
    report.update(zip(STATS, host[n_classes:]))
    return out, report
