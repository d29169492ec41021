"""The mean-teacher step of semi-supervised training (csrc/semi.hip), what LaserMix and PolarMix were invented for: a
TEACHER that is an exponential moving average of the student labels the points nobody annotated, those pseudo labels
travel through the mix (data.mix_scans), and the student trains on the mixed batch with a CONSISTENCY term against the
teacher.  All opt-in: train_step, train_batch and mixed_train_batch do exactly what they did.

    teacher = EmaTeacher(student)                                   # a clean copy: eval mode, no gradients
    ...
    logits = teacher.model(SparseTensor(b['feats_v_b'], b['coords_v_b']))[0]        # b = data.val_batch(...), no_grad
    labels_p, stats = pseudo_labels(logits, 0.9, inverse=b['inverse_indices_b'], labels=b['labels_p_b'])
    mixed = data.mix_scans(points, intensity, [..., labels_p, ...], mixes)
    batch = data.voxelize_batch(...)
    loss, logits, cons = semi_train_step(student, teacher, opt, feats, coords, labels)

EmaTeacher.update is ONE launch over every parameter and buffer (lidal_ema_step), pseudo_labels one launch,
consistency_loss two forward launches and one backward launch; none of them synchronises or reads anything back.
The definitions are this project's own; tests/semi_ref.py restates them in numpy."""
import copy

import numpy as np
import torch
from torch.autograd import Function

from . import backend as B
from .flat import place_on_axis

__all__ = ['EmaTeacher', 'pseudo_labels', 'consistency_loss', 'consistency_forward', 'semi_train_step', 'ema_alpha',
           'MAX_CLASSES']

MAX_CLASSES = 32
_KINDS = {'mse': 0, 'kl': 1}


def ema_alpha(alpha, updates, warmup=True):
    """The alpha of update number `updates` (0-based): min(alpha, 1 - 1 / (updates + 1)) with warm-up -- the first update
    copies the student, the second averages the two, ... -- else alpha."""
    return min(float(alpha), 1.0 - 1.0 / (updates + 1)) if warmup else float(alpha)


def _strip(module):
    """Take the caches this package hangs on modules (launch programs, map traces) out of `module`'s tree; returns what
    was taken so that it can be put back."""
    taken = []
    for m in module.modules():
        for k in [k for k in m.__dict__ if k.startswith('_lidal_')]:
            taken.append((m, k, m.__dict__.pop(k)))
    return taken


def _clean_copy(student):
    """copy.deepcopy of the student that shares no cached plan, weight image or map trace with it: the module caches
    are taken off the student for the time of the copy (a copied launch program would still hold the student's
    addresses), and Parameter.__deepcopy__ clones the data alone, so no `_lidal_images` travels with a parameter."""
    taken = _strip(student)
    try:
        twin = copy.deepcopy(student)
    finally:
        for m, k, v in taken:
            m.__dict__[k] = v
    for t in list(twin.parameters()) + list(twin.buffers()):
        for k in [k for k in getattr(t, '__dict__', {}) if k.startswith('_lidal_')]:
            delattr(t, k)
    return twin


class EmaTeacher:
    """teacher = alpha_eff * teacher + (1 - alpha_eff) * student over every parameter (and, with buffers='ema', every
    float buffer) in ONE launch; integer buffers (num_batches_tracked) and, with buffers='copy', the float buffers
    (BatchNorm's running statistics) are copied by the same launch.

      student   the module being trained
      alpha     the decay, 0 <= alpha <= 1 (1: the teacher never moves; 0: every update is a copy)
      warmup    alpha_eff = min(alpha, 1 - 1 / (updates + 1)) (ema_alpha): the teacher starts as the running mean
      buffers   'copy' or 'ema'
      model     the teacher module to use instead of a clean deep copy of the student

    `.model` is in eval() and none of its parameters asks for a gradient.  Per f32 element t = t + (s - t) * oma with
    oma = (float)(1.0 - alpha_eff) formed in double on the host, the two operations rounded separately, subnormals kept,
    NaN and Inf as IEEE has them (the form of Adam's first moment, csrc/optim.hip); alpha_eff == 0 copies, since
    t + (s - t) is not s in floating point.  Copies move 32-bit words that no arithmetic touches.

    Parameters and buffers pair by name.  ValueError, naming the first offender, for a name missing on either side, a
    shape or dtype mismatch, a parameter (or averaged buffer) that is not float32, a tensor that is not contiguous or
    whose element size is not a multiple of four bytes, and tensors on more than one device.

    The device table (one record per tensor: teacher address, student address, first word on the virtual axis, words,
    kind) is uploaded when an address in it changed -- ordinarily once; `table_uploads` and `launches` count as
    optim.Adam's do.  Every update() and copy_from() ends with backend._bump_epoch(): the writes go through raw
    pointers, no version counter moves, and the teacher's cached weight images and folded BatchNorm maps would otherwise
    serve the previous weights.

    Under data parallelism every rank updates its own teacher from the student weights the ranks share after the
    optimizer step: identical inputs, identical arithmetic, no collective."""

    def __init__(self, student, alpha=0.999, warmup=True, buffers='copy', model=None):
        if not isinstance(student, torch.nn.Module):
            raise ValueError('EmaTeacher: student must be a torch.nn.Module, got %s' % type(student).__name__)
        if not 0.0 <= float(alpha) <= 1.0:
            raise ValueError('EmaTeacher: alpha must be in [0, 1], got %r' % (alpha,))
        if buffers not in ('copy', 'ema'):
            raise ValueError("EmaTeacher: buffers must be 'copy' or 'ema', got %r" % (buffers,))
        self.alpha = float(alpha)
        self.warmup = bool(warmup)
        self.buffers = buffers
        self.updates = 0
        self.launches = 0               # kernel launches so far
        self.table_uploads = 0          # host-to-device copies of the table so far
        self._table = None
        self._addrs = None
        self._v_end = 0
        self._n_recs = 0
        if model is None:
            model = _clean_copy(student)
        elif not isinstance(model, torch.nn.Module):
            raise ValueError('EmaTeacher: model must be a torch.nn.Module, got %s' % type(model).__name__)
        self._pairs = self._pair(model, student)    # (refuses before the teacher is touched)
        self._student = student
        self.model = model
        model.eval()
        for p in model.parameters():
            p.requires_grad_(False)

    # ---- pairing -----------------------------------------------------------------------------------------------
    def _pair(self, teacher, student):
        """[(name, teacher tensor, student tensor, kind)] in the teacher's order; kind 0 lerp, 1 copy."""
        pairs = []
        devices = set()
        for what, get in (('parameter', lambda m: m.named_parameters()), ('buffer', lambda m: m.named_buffers())):
            mine, theirs = dict(get(teacher)), dict(get(student))
            for name in theirs:
                if name not in mine:
                    raise ValueError('EmaTeacher: %s %r of the student is missing in the teacher' % (what, name))
            for name, t in mine.items():
                s = theirs.get(name)
                if s is None:
                    raise ValueError('EmaTeacher: %s %r of the teacher is missing in the student' % (what, name))
                if t.shape != s.shape:
                    raise ValueError('EmaTeacher: %s %r has shape %s in the teacher and %s in the student'
                                     % (what, name, tuple(t.shape), tuple(s.shape)))
                if t.dtype != s.dtype:
                    raise ValueError('EmaTeacher: %s %r is %s in the teacher and %s in the student'
                                     % (what, name, t.dtype, s.dtype))
                lerp = what == 'parameter' or (self.buffers == 'ema' and t.dtype.is_floating_point)
                if lerp and t.dtype != torch.float32:
                    raise ValueError('EmaTeacher: %s %r must be float32 to be averaged, got %s' % (what, name, t.dtype))
                if t.element_size() % 4 != 0:
                    raise ValueError('EmaTeacher: %s %r has %d-byte elements (%s): the kernel moves 32-bit words'
                                     % (what, name, t.element_size(), t.dtype))
                for side, x in (('teacher', t), ('student', s)):
                    if not x.is_contiguous():
                        raise ValueError("EmaTeacher: the %s's %s %r is not contiguous (shape %s, strides %s)"
                                         % (side, what, name, tuple(x.shape), x.stride()))
                    devices.add(x.device)
                if len(devices) > 1:
                    raise ValueError('EmaTeacher: tensors on more than one device (%s), first at %s %r'
                                     % (', '.join(sorted(str(d) for d in devices)), what, name))
                if t is s or (t.numel() and t.data_ptr() == s.data_ptr()):
                    raise ValueError('EmaTeacher: %s %r is the same memory in teacher and student' % (what, name))
                pairs.append((name, t, s, 0 if lerp else 1))
        # Module order (the state_dict's): the small tensors of a BatchNorm then lie between the convolutions' weights
        # on the virtual axis.  With the 156 small buffers of SPVCNN together behind its 161 parameters a few workgroups
        # walked them one load latency after the other: 0.149 ms per update instead of 0.055.
        order = {k: i for i, k in enumerate(teacher.state_dict().keys())}
        pairs.sort(key=lambda r: order.get(r[0], len(order)))
        return pairs

    def _build_table(self, pairs, addrs, device):
        live = [(at, as_, t.numel() * (t.element_size() // 4), kind)
                for (name, t, s, kind), (at, as_) in zip(pairs, addrs) if t.numel()]    # zero-element tensors are skipped
        # the teacher's phase in a 128-byte line fixes the axis
        starts, self._v_end = place_on_axis([r[0] for r in live], [r[2] for r in live])
        recs = [(at, as_, v, n, kind) for (at, as_, n, kind), v in zip(live, starts)]
        self._n_recs = len(recs)
        self._table = torch.from_numpy(np.array(recs, dtype=np.int64).reshape(-1, 5)).to(device) if recs else None
        self.table_uploads += 1
        self._addrs = addrs

    def _launch(self, student, oma, all_copy):
        if student is None:
            student = self._student
        if student is not self._student or self._pairs is None:
            self._pairs = self._pair(self.model, student)
            self._student = student
            self._addrs = None
        pairs = self._pairs
        addrs = [(t.data_ptr(), s.data_ptr()) for _, t, s, _ in pairs]
        if addrs != self._addrs:
            tensors = [x for _, t, s, _ in pairs for x in (t, s)]
            B.require_gpu(*tensors)
            for (name, t, s, _), (at, as_) in zip(pairs, addrs):        # (a parameter may have been replaced: re-check)
                if not (t.is_contiguous() and s.is_contiguous()) or t.shape != s.shape or t.dtype != s.dtype:
                    self._pairs = None
                    raise ValueError('EmaTeacher: %r changed its shape, dtype or layout since it was paired' % name)
                if (at % 4 or as_ % 4) and t.numel():
                    raise ValueError('EmaTeacher: %r is not aligned to four bytes' % name)
            self._build_table(pairs, addrs, pairs[0][1].device if pairs else torch.device('cuda'))
        if self._n_recs:
            B.check(B.lib().lidal_ema_step(self._table.data_ptr(), self._n_recs, self._v_end, oma, 1 if all_copy else 0,
                                           B.stream()), 'ema_step')
            self.launches += 1
        B._bump_epoch()

    # ---- the methods -------------------------------------------------------------------------------------------
    def alpha_eff(self):
        """The alpha the next update() uses."""
        return ema_alpha(self.alpha, self.updates, self.warmup)

    @torch.no_grad()
    def update(self, student=None):
        """One launch: the teacher moves towards `student` (default: the student of construction or of the last call)."""
        a = self.alpha_eff()
        self._launch(student, 1.0 - a, a == 0.0)
        self.updates += 1

    @torch.no_grad()
    def copy_from(self, student):
        """One launch with every record of the copy kind: the teacher's tensors become the student's, bit for bit."""
        self._launch(student, 1.0, True)

    def rebind(self, student=None):
        """Pair the tensors again.  Pairing happens at construction and when update() is handed another module; a
        tensor whose storage moved is noticed by its address, but a Parameter OBJECT that was replaced inside the same
        module is not: call this after such surgery."""
        student = self._student if student is None else student
        self._pairs = self._pair(self.model, student)
        self._student = student
        self._addrs = None

    def state_dict(self):
        return {'model': self.model.state_dict(), 'updates': self.updates, 'alpha': self.alpha}

    def load_state_dict(self, state):
        self.model.load_state_dict(state['model'])
        self.updates = int(state['updates'])
        self.alpha = float(state['alpha'])
        B._bump_epoch()


# ---------------------------------------------------------------------------------------------------- pseudo labels
def _check_scores(x, what, dtypes=(torch.float32, torch.bfloat16)):
    if not torch.is_tensor(x) or x.dim() != 2:
        raise ValueError('%s must be a [n, c] tensor, got %s' % (what, tuple(getattr(x, 'shape', ()))))
    if x.dtype not in dtypes:
        raise ValueError('%s must be %s, got %s' % (what, ' or '.join(str(d) for d in dtypes), x.dtype))
    if not 1 <= x.shape[1] <= MAX_CLASSES:
        raise ValueError('%s: classes must be in 1..%d, got %d' % (what, MAX_CLASSES, x.shape[1]))


def _check_index(x, what, p=None):
    if not torch.is_tensor(x) or x.dim() != 1 or x.dtype != torch.int64:
        raise ValueError('%s must be an int64 [p] tensor, got %s %s'
                         % (what, getattr(x, 'dtype', type(x).__name__), tuple(getattr(x, 'shape', ()))))
    if p is not None and x.shape[0] != p:
        raise ValueError('%s has %d entries for %d points' % (what, x.shape[0], p))


def pseudo_labels(logits, thresholds, inverse=None, labels=None, ignore_index=255, return_conf=False):
    """The teacher's confident predictions as labels, one launch (lidal_pseudo_labels), nothing read back.

      logits       f32 or bf16 [nv, c], c in 1..32: the teacher's rows
      thresholds   a number, or f32 [c] on the device: the confidence a prediction of class k needs
      inverse      i64 [p]: the row of every point (val_batch / score_sample give it); None: point i is row i
      labels       i64 [p]: human labels, which win wherever they are not ignore_index

    Per point: arg = the first maximum of its row, conf = the f32 softmax there (expf(x - mx), running f32 sum in class
    order, f32 divide); out = the human label, else arg where conf >= thresholds[arg], else ignore_index.  A row with a
    NaN is never accepted.  An inverse entry outside [0, nv) gives ignore_index, is counted, and is never read through.
    Returns (out i64 [p], stats i64 [c + 2] = rows accepted per class, rows rejected, bad indices -- human-labelled
    points are in none of them) and, with return_conf, conf f32 [p] (0 at a bad index)."""
    what = 'pseudo_labels'
    _check_scores(logits, what + ': logits')
    nv, c = logits.shape
    p = nv
    if inverse is not None:
        _check_index(inverse, what + ': inverse')
        p = inverse.shape[0]
    if labels is not None:
        _check_index(labels, what + ': labels', p)
    thr_t, thr = None, 0.0
    if torch.is_tensor(thresholds):
        if thresholds.dtype != torch.float32 or tuple(thresholds.shape) != (c,):
            raise ValueError('%s: thresholds must be a number or float32 [%d], got %s %s'
                             % (what, c, thresholds.dtype, tuple(thresholds.shape)))
        thr_t = thresholds
    else:
        try:
            thr = float(thresholds)
        except (TypeError, ValueError):
            raise ValueError('%s: thresholds must be a number or float32 [%d], got %r' % (what, c, thresholds)) from None
    if not -2 ** 63 <= int(ignore_index) < 2 ** 63:
        raise ValueError('%s: ignore_index %r does not fit int64' % (what, ignore_index))
    B.require_gpu(logits, inverse, labels, thr_t)
    logits = logits.contiguous()
    inverse = inverse.contiguous() if inverse is not None else None
    labels = labels.contiguous() if labels is not None else None
    thr_t = thr_t.contiguous() if thr_t is not None else None
    dev = logits.device
    out = torch.empty(p, dtype=torch.int64, device=dev)
    stats = torch.empty(c + 2, dtype=torch.int64, device=dev)
    conf = torch.empty(p, dtype=torch.float32, device=dev) if return_conf else None
    B.check(B.lib().lidal_pseudo_labels(B.ptr(logits), B.dtype_code(logits.dtype), nv, c, B.ptr(thr_t), thr,
                                        B.ptr(inverse), B.ptr(labels), int(ignore_index), p, B.ptr(out), B.ptr(stats),
                                        B.ptr(conf), B.stream()), 'pseudo_labels')
    return (out, stats, conf) if return_conf else (out, stats)


# ---------------------------------------------------------------------------------------------------- consistency
def _consistency_operands(student, teacher, kind, min_conf, probs):
    what = 'consistency_loss'
    if kind not in _KINDS:
        raise ValueError("%s: kind must be 'mse' or 'kl', got %r" % (what, kind))
    if probs and kind != 'mse':
        raise ValueError("%s: probs=True takes kind='mse' only" % what)
    dtypes = (torch.float32,) if probs else (torch.float32, torch.bfloat16)
    _check_scores(student, what + ': student ' + ('probabilities' if probs else 'logits'), dtypes)
    _check_scores(teacher, what + ': teacher ' + ('probabilities' if probs else 'logits'), dtypes)
    if student.shape != teacher.shape:
        raise ValueError('%s: student rows %s and teacher rows %s do not correspond'
                         % (what, tuple(student.shape), tuple(teacher.shape)))
    n, c = student.shape
    if n * c >= 1 << 30:
        raise ValueError('%s: %d rows x %d classes reach 2^30 entries' % (what, n, c))
    try:
        mc = float(min_conf)
    except (TypeError, ValueError):
        raise ValueError('%s: min_conf must be a number, got %r' % (what, min_conf)) from None
    if mc != mc:
        raise ValueError('%s: min_conf is NaN' % what)
    B.require_gpu(student, teacher)
    return student.contiguous(), teacher.detach().contiguous(), _KINDS[kind], mc


def consistency_forward(student, teacher, kind='mse', min_conf=0.0, probs=False, per_row=False):
    """The forward launches alone: (out2 f64 [2] = {loss, sum of the masked row terms}, per_row f32 [n] or None).  What
    consistency_loss and the tests build on; n == 0 gives zeros without a launch."""
    return _consistency_launch(*_consistency_operands(student, teacher, kind, min_conf, probs), probs, per_row)


def _consistency_launch(zs, zt, k, mc, probs, per_row):
    n, c = zs.shape
    dev = zs.device
    if n == 0:
        return (torch.zeros(2, dtype=torch.float64, device=dev),
                torch.zeros(0, dtype=torch.float32, device=dev) if per_row else None)
    L = B.lib()
    out2 = torch.empty(2, dtype=torch.float64, device=dev)
    rows = torch.empty(n, dtype=torch.float32, device=dev) if per_row else None
    nbytes = L.lidal_consistency_workspace_bytes(n)
    ws = B.workspace(nbytes, dev)
    B.check(L.lidal_consistency_fwd(B.ptr(zs), B.dtype_code(zs.dtype), B.ptr(zt), B.dtype_code(zt.dtype), n, c, k,
                                    1 if probs else 0, mc, B.ptr(out2), B.ptr(rows), B.ptr(ws), nbytes, B.stream()),
            'consistency_fwd')
    return out2, rows


class _Consistency(Function):
    @staticmethod
    def forward(ctx, student, teacher, kind, min_conf, probs, per_row):
        zs, zt, k, mc = _consistency_operands(student, teacher, kind, min_conf, probs)
        out2, rows = _consistency_launch(zs, zt, k, mc, probs, per_row)
        ctx.save_for_backward(zs, zt)
        ctx.args = (k, mc, 1 if probs else 0)
        loss = out2[0].to(torch.float32)
        if per_row:
            ctx.mark_non_differentiable(rows)
            return loss, rows
        return loss

    @staticmethod
    def backward(ctx, g, *_):
        zs, zt = ctx.saved_tensors
        k, mc, probs = ctx.args
        n, c = zs.shape
        dz = torch.empty_like(zs)
        if n:
            gs = g.reshape(1).float().contiguous()
            B.check(B.lib().lidal_consistency_bwd(B.ptr(zs), B.dtype_code(zs.dtype), B.ptr(zt), B.dtype_code(zt.dtype),
                                                  n, c, k, probs, mc, B.ptr(gs), B.ptr(dz), B.stream()),
                    'consistency_bwd')
        return dz, None, None, None, None, None


def consistency_loss(student_logits, teacher_logits, kind='mse', min_conf=0.0, probs=False, per_row=False):
    """The consistency term between a student's and a teacher's rows of the SAME voxel batch, differentiable with
    respect to the student only (lidal_consistency_fwd / _bwd: two forward launches, one backward launch).

      student_logits / teacher_logits   [n, c], each f32 or bf16, c in 1..32, n * c < 2^30
      kind      'mse': mean over rows and classes of (softmax(zs) - softmax(zt))^2 = F.mse_loss of the two softmaxes, the
                       mean teacher's and LaserMix's term;
                'kl' : F.kl_div(log_softmax(zs), softmax(zt), reduction='batchmean'), distillation
      min_conf  rows whose teacher confidence (its largest probability) is below it are left out; the denominator
                stays n whatever is masked
      probs     'mse' only: the operands are f32 probabilities, and the gradient is the one with respect to them
      per_row   also return r f32 [n], the rows' terms, already masked

    Both softmaxes are the f32 row softmax of pseudo_labels; the rows' terms are summed in f32 in numpy's order
    (csrc/npsum.h np_sum_f32) and over the rows in f64 in a fixed order, so two calls give the same bits.  The incoming
    gradient is read on the device: no synchronisation.  n == 0 gives 0 without a launch."""
    _consistency_operands(student_logits, teacher_logits, kind, min_conf, probs)       # refuse before autograd sees it
    return _Consistency.apply(student_logits, teacher_logits, kind, min_conf, bool(probs), bool(per_row))


# ---------------------------------------------------------------------------------------------------- the step
def semi_train_step(student, teacher, optimizer, feats_v_b, coords_v_b, labels_v_b, cons_weight=1.0, kind='mse',
                    min_conf=0.0, criterion=None, autocast=False):
    """One mean-teacher iteration: zero_grad, the teacher's forward pass under no_grad, the student's on the SAME
    SparseTensor (the coordinate tables and kernel maps are built once: for SPVCNN / MinkUNet as one network.Geometry
    with the backward's lists, which both the inference plan and the training plan admit), loss = criterion(logits,
    labels) + cons_weight * consistency_loss(logits, teacher logits), backward, optimizer.step(),
    teacher.update(student).  Returns (loss, logits, consistency), detached.

    cons_weight == 0 skips the teacher's pass and the consistency term (returned as 0): the student's update is
    train_step's, and the teacher still follows it."""
    from . import SparseTensor
    from .nn.functional.fused import cross_entropy
    from .train_step import forward_backward
    if not isinstance(teacher, EmaTeacher):
        raise ValueError('semi_train_step: teacher must be an EmaTeacher, got %s' % type(teacher).__name__)
    if kind not in _KINDS:
        raise ValueError("semi_train_step: kind must be 'mse' or 'kl', got %r" % (kind,))
    optimizer.zero_grad()
    if cons_weight == 0:
        loss, logits = forward_backward(student, feats_v_b, coords_v_b, labels_v_b, autocast, None, criterion)
        cons = torch.zeros((), dtype=torch.float32, device=logits.device)
    else:
        from .network import MinkUNet, SPVCNN
        from .network.geometry import Geometry
        x = SparseTensor(feats_v_b, coords_v_b)
        if (isinstance(student, (SPVCNN, MinkUNet)) and type(teacher.model) is type(student) and student.training
                and torch.is_grad_enabled()):
            x.geometry = Geometry.build(student, coords_v_b, True)
        with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16, enabled=autocast):
            t_logits, _ = teacher.model(x)
        with torch.autocast('cuda', dtype=torch.bfloat16, enabled=autocast):
            logits, _ = student(x)
        sup = cross_entropy(logits, labels_v_b, ignore_index=255) if criterion is None else criterion(logits, labels_v_b)
        cons = consistency_loss(logits, t_logits, kind=kind, min_conf=min_conf)
        loss = sup + cons_weight * cons
        loss.backward()
    optimizer.step()
    teacher.update(student)
    return loss.detach(), logits.detach(), cons.detach()
