"""`optimizer.step()` of the training step (train.py:56,140) as ONE kernel launch over every parameter tensor of a group
at once (csrc/optim.hip), opt-in beside torch.optim:

    opt = lidal_amd.optim.Adam(model.parameters())          # the reference's defaults: lr 1e-3, betas (0.9, 0.999), eps 1e-8
    opt = lidal_amd.optim.AdamW(model.parameters(), lr=2e-3, weight_decay=0.01, clip_grad_norm=10)
    opt = lidal_amd.optim.SGD(model.parameters(), lr=0.24, momentum=0.9, nesterov=True, weight_decay=1e-4)

The arithmetic is torch's single-tensor Adam / AdamW / SGD with every operation rounded separately in f32
(tests/adam_ref.py and tests/optim_ref.py restate it in numpy; the kernels equal them bit for bit).  What makes one
launch possible:

  * state: ONE flat f32 buffer per state array and parameter group (`exp_avg` and `exp_avg_sq`; SGD's `momentum_buffer`,
    none at all with momentum 0); `state[p][...]` are views of them and Adam's `state[p]['step']` a view of one host
    tensor per group, so `state_dict()` has the format of the torch optimizer of the same name, loads into it and the
    other way round;
  * a device table with one record per parameter (address, where its gradient is, where its state is, how many
    elements), uploaded when an address in it changed -- ordinarily once: after the planned step (network/plan.py) the
    gradients are views of one flat buffer with a fixed layout (flat.BackToBack, the test DataParallel uses), and the
    table then names them RELATIVE to that buffer, which is a fresh allocation every step; any other gradients are named
    by absolute address;
  * the launch covers a run of consecutive records that share their step count and hyperparameters: one launch per group
    and step, more only where a parameter skipped steps (`.grad is None`) or is missing inside a group.

`clip_grad_norm=max_norm` (every optimizer here; an attribute, so it can change between steps) is
torch.nn.utils.clip_grad_norm_(all parameters, max_norm) folded into the step with nothing read back: one launch writes f64
partial sums of g * g in an order fixed by (record, element index) alone, one workgroup forms `total` and
`coef = min(max_norm / (total + 1e-6), 1)` on the device, and the update launches use `grad * coef` (also when coef is 1,
as torch multiplies unconditionally).  The clipped gradient is NOT written back: `.grad` keeps what backward() produced.
`optimizer.grad_norm` is the total norm as a 0-d f32 device tensor, refreshed by every clipped step (None before the
first): logging it costs no synchronisation.  The norm runs over all groups; a non-finite norm is not treated specially
(coef is 0 or NaN, as in torch).

After a step `backend._bump_epoch()` tells the cached weight operands (LDS images, folded BatchNorm maps) that the
parameters moved: writes through raw pointers move no version counter."""
import math

import numpy as np
import torch

from . import backend as B
from .flat import LINE, BackToBack, place_on_axis

__all__ = ['Adam', 'AdamW', 'SGD']


class _Group:
    """What one parameter group keeps beside its dict (which state_dict() serialises)."""
    __slots__ = ('params', 'numels', 'offs', 'size', 'bufs', 'steps', 'steps_t', 'uniform', 'rec0', 'vbase', 'inserted',
                 'device')


class _OneLaunch(torch.optim.Optimizer):
    """The table, the address check, the runs, the flat state, the gradient norm and the counters: what Adam, AdamW and
    SGD share.  A subclass names its state arrays (_STATE), says whether state[p] holds 'step' (_HAS_STEP), what a group
    may not ask for (_REFUSED), and launches one run (_launch)."""
    _NAME = None
    _REFUSED = ()
    _STATE = ()
    _HAS_STEP = False

    def _setup(self, clip_grad_norm):
        self._rt = []                   # _Group per parameter group
        self._params = None             # the parameters of every group in record order
        self._table = None              # device table: int64 [records, 5], then the [records + 1] slot starts of the norm
        self._n_rec = 0
        self._n_slots = 0               # f64 partial sums of the gradient norm: sum(ceil(n_r / block))
        self._addr_p = None             # per record: the parameter's address in the table
        self._addr_g = None             # per record: the gradient's address minus the base the table is relative to
        self._flat_form = False         # the table's gradient words are relative to a flat buffer
        self._b2b = BackToBack()
        self._norm = None               # device f32 [2]: total norm, clip coefficient
        self.grad_norm = None           # 0-d view of the total norm, refreshed by every clipped step
        self.launches = 0               # kernel launches so far
        self.table_uploads = 0          # host-to-device copies of the table so far
        self.clip_grad_norm = clip_grad_norm
        self._check_clip()

    # ---- what it refuses -----------------------------------------------------------------------------------------
    def _check_clip(self):
        c = self.clip_grad_norm
        if c is None:
            return None
        if isinstance(c, (torch.Tensor, bool)) or not isinstance(c, (int, float)) or not c > 0:
            raise ValueError('lidal_amd.optim.%s: clip_grad_norm must be a positive Python number or None (got %r)'
                             % (self._NAME, c))
        return float(c)

    @classmethod
    def _check_group(cls, group):
        for key in cls._REFUSED:
            if group.get(key):
                hint = '; lidal_amd.optim.AdamW is the decoupled form' if key == 'decoupled_weight_decay' else ''
                raise ValueError('lidal_amd.optim.%s does not implement %s=%r (torch.optim.%s does%s)'
                                 % (cls._NAME, key, group[key], cls._NAME, hint))
        if isinstance(group['lr'], torch.Tensor):
            raise ValueError('lidal_amd.optim.%s: lr must be a Python number, not a tensor' % cls._NAME)

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        group = self.param_groups[-1]
        try:
            self._check_group(group)
            devices = set()
            for g in self.param_groups:
                for p in g['params']:
                    devices.add(p.device)
            for p in group['params']:
                if p.dtype != torch.float32:
                    raise ValueError('lidal_amd.optim.%s: parameters must be float32 (got %s of shape %s)'
                                     % (self._NAME, p.dtype, tuple(p.shape)))
                if not p.is_contiguous():
                    raise ValueError('lidal_amd.optim.%s: parameters must be contiguous (shape %s, strides %s)'
                                     % (self._NAME, tuple(p.shape), p.stride()))
            if len(devices) > 1:
                raise ValueError('lidal_amd.optim.%s: parameters on more than one device (%s)'
                                 % (self._NAME, ', '.join(sorted(str(d) for d in devices))))
        except ValueError:
            self.param_groups.pop()
            raise
        self._table = None

    # ---- state ---------------------------------------------------------------------------------------------------
    def _groups(self):
        """What every group keeps beside its dict; the flat state is allocated at first use (a step or load_state_dict)."""
        rt = self._rt
        while len(rt) < len(self.param_groups):
            group = self.param_groups[len(rt)]
            g = _Group()
            g.params = list(group['params'])
            g.numels = [p.numel() for p in g.params]
            # the state offset takes the parameter's phase in a 128-byte line
            g.offs, g.size = place_on_axis([p.data_ptr() for p in g.params], g.numels)
            g.device = g.params[0].device if g.params else torch.device('cpu')
            g.bufs = None
            g.steps = [0] * len(g.params)
            g.steps_t = torch.zeros(len(g.params), dtype=torch.float32) if self._HAS_STEP else None
            g.uniform = 0
            g.inserted = False
            rt.append(g)
            self._table = None
            self._params = None
        return rt

    def _state_bufs(self, g):
        if g.bufs is None:
            g.bufs = [torch.zeros(max(g.size, 1), dtype=torch.float32, device=g.device) for _ in self._STATE]
        return g.bufs

    def _insert_state(self, g, indices):
        bufs = self._state_bufs(g)
        for i in indices:
            p = g.params[i]
            if p not in self.state:
                o, n = g.offs[i], g.numels[i]
                st = {'step': g.steps_t[i]} if self._HAS_STEP else {}
                for key, buf in zip(self._STATE, bufs):
                    st[key] = buf[o:o + n].view(p.shape)
                self.state[p] = st

    def _loaded_step(self, entry):
        """The step count of a loaded state entry that holds every state array."""
        raise NotImplementedError

    def load_state_dict(self, state_dict):
        """Accepts this optimizer's dict or that of the torch optimizer of the same name: the loaded state arrays are copied
        INTO the flat buffers (the base class would put the loaded tensors in the views' place).  As in torch, state_dict()
        hands out the live tensors: copy.deepcopy it before loading it into an optimizer that goes on stepping beside this
        one."""
        super().load_state_dict(state_dict)
        for group in self.param_groups:
            for key in ('foreach', 'fused'):        # how torch implements its step: nothing this optimizer does
                group.pop(key, None)
            self._check_group(group)
        self._rt = []
        self._table = None
        self._params = None
        loaded = self.state
        self.state = type(loaded)(dict)
        for k, v in loaded.items():
            if not isinstance(k, torch.Tensor):
                self.state[k] = v
        for g in self._groups():
            have = [i for i, p in enumerate(g.params)           # (SGD: no entry, or None for the buffer, is "first step")
                    if p in loaded and all(isinstance(loaded[p].get(key), torch.Tensor) for key in self._STATE)]
            if not have:
                continue
            steps = [self._loaded_step(loaded[g.params[i]]) for i in have]
            if any(isinstance(s, torch.Tensor) and s.is_cuda for s in steps):
                steps = torch.stack([torch.as_tensor(s).float().reshape(()).to(steps[0].device) for s in steps]).tolist()
            bufs = self._state_bufs(g)
            for i, s in zip(have, steps):
                p = g.params[i]
                o, n = g.offs[i], g.numels[i]
                for key, buf in zip(self._STATE, bufs):
                    buf[o:o + n].copy_(loaded[p][key].reshape(-1))
                g.steps[i] = int(round(float(s)))
            if self._HAS_STEP:
                g.steps_t.copy_(torch.tensor(g.steps, dtype=torch.float32))
            g.uniform = g.steps[0] if len(set(g.steps)) == 1 else None
            self._insert_state(g, have)
            g.inserted = len(have) == len(g.params)

    # ---- the table -----------------------------------------------------------------------------------------------
    def _build_table(self, rt, grads, addr_p, addr_g, device):
        """One record per parameter of every group, group after group.  `grads`: per record the gradient or None.  Behind
        the records: where each record's partial sums of the gradient norm start (one slot per block of its elements)."""
        n_rec = len(addr_p)
        present = [g for g in grads if g is not None and g.numel()]
        base = 0
        self._flat_form = False
        if present and all(g is not None for g in grads) and self._b2b.flat(present) is not None:
            base = present[self._b2b.layout[1]].data_ptr()
            self._flat_form = True
        gword = [(a - base) if a is not None else None for a in addr_g]
        offs, vstart, numels = [], [], []
        r = 0
        v = 0
        for g in rt:
            g.rec0 = r
            v += -v % LINE
            g.vbase = v                         # virtual index = vbase + state offset
            offs += g.offs
            vstart += [v + o for o in g.offs]
            numels += g.numels
            r += len(g.params)
            v += g.size
        block = int(B.lib_handle().lidal_grad_norm_block_elems())
        slots = np.zeros(n_rec + 1, dtype=np.int64)
        np.cumsum([-(-n // block) for n in numels], out=slots[1:])
        words = np.array([addr_p, [w or 0 for w in gword], offs, vstart, numels], dtype=np.int64).T.reshape(-1)
        self._table = torch.from_numpy(np.concatenate([words, slots])).to(device)
        self._n_rec = n_rec
        self._n_slots = int(slots[-1])
        self.table_uploads += 1
        self._addr_p = list(addr_p)
        self._addr_g = gword

    # ---- the gradient norm ---------------------------------------------------------------------------------------
    def _clip_coef(self, max_norm, grads, base, device):
        """Launches the norm of `grads` (per record the gradient or None) and returns the device address of the clip
        coefficient: a launch per run of consecutive records that all have, or all lack, a gradient, and the finish."""
        L = B.lib()
        stream = B.stream()
        if self._norm is None:
            self._norm = torch.zeros(2, dtype=torch.float32, device=device)
            self.grad_norm = self._norm[0]
        table = self._table.data_ptr()
        slots = table + self._n_rec * 40
        n_slots = self._n_slots
        partials = B.workspace(8 * n_slots, device).data_ptr() if n_slots else None
        if n_slots:
            r0 = 0
            n_rec = self._n_rec
            while r0 < n_rec:
                missing = grads[r0] is None
                r1 = r0 + 1
                while r1 < n_rec and (grads[r1] is None) == missing:
                    r1 += 1
                B.check(L.lidal_grad_norm_partials(table, slots, r0, r1, base or None, partials, n_slots,
                                                   1 if missing else 0, stream), 'grad_norm_partials')
                self.launches += 1
                r0 = r1
        B.check(L.lidal_grad_norm_finish(partials, n_slots, max_norm, self._norm.data_ptr(), stream), 'grad_norm_finish')
        self.launches += 1
        return self._norm.data_ptr() + 4

    # ---- the step ------------------------------------------------------------------------------------------------
    def _advances(self, group):
        """Does a step of this group move its parameters' step counts?"""
        return True

    def _run_key(self, group, done):
        """What the records of one launch must share, given the steps a parameter has done."""
        return done

    def _count_after(self, done):
        """A parameter's step count after one more step."""
        return done + 1

    def _launch(self, L, group, g, table, r0, r1, v0, v1, base, key, coef, stream):
        raise NotImplementedError

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        name = self._NAME
        max_norm = self._check_clip()
        rt = self._groups()
        grads, addr_g = [], []
        complete = []                   # per group: every parameter has a gradient
        for group, g in zip(self.param_groups, rt):
            if len(group['params']) != len(g.params):
                raise ValueError('lidal_amd.optim.%s: the parameters of a group changed after the first step' % name)
            self._check_group(group)
            whole = True
            for p in g.params:
                gr = p.grad
                if gr is None:
                    whole = False
                    grads.append(None)
                    addr_g.append(None)
                    continue
                if gr.layout is not torch.strided:
                    raise ValueError('lidal_amd.optim.%s does not take sparse gradients%s'
                                     % (name, ' (torch.optim.SparseAdam does)' if self._HAS_STEP else ''))
                if gr.dtype is not torch.float32:
                    raise ValueError('lidal_amd.optim.%s: gradients must be float32 (got %s for a parameter of '
                                     'shape %s)' % (name, gr.dtype, tuple(p.shape)))
                if not gr.is_contiguous():
                    gr = gr.contiguous()
                grads.append(gr)
                addr_g.append(gr.data_ptr() if gr.numel() else None)        # (an empty tensor has no address: it reads 0)
            complete.append(whole)
        present = grads if all(complete) else [gr for gr in grads if gr is not None]
        if not present:
            return loss
        params = self._params
        if params is None:
            params = self._params = [p for g in rt for p in g.params]
        addr_p = [p.data_ptr() for p in params]
        # is the table still right?  every parameter where it was, every gradient at ONE common distance from its word
        base = None
        ok = self._table is not None and addr_p == self._addr_p
        if ok:
            for a, w in zip(addr_g, self._addr_g):
                if a is None:
                    continue
                if w is None or (base is not None and a - w != base):
                    ok = False
                    break
                base = a - w
            ok = ok and (base == 0 or self._flat_form)
        if not ok:
            B.require_gpu(*params)
            B.require_gpu(*present)
            self._build_table(rt, grads, addr_p, addr_g, params[0].device)
            base = next((a - w for a, w in zip(addr_g, self._addr_g) if a is not None), 0)
        L = B.lib()
        stream = B.stream()
        table = self._table.data_ptr()
        coef = None if max_norm is None else self._clip_coef(max_norm, grads, base, params[0].device)
        for group, g, whole in zip(self.param_groups, rt, complete):
            n = len(g.params)
            mine = grads[g.rec0:g.rec0 + n]
            advance = self._advances(group)
            if g.uniform is not None and whole:       # (never `None in mine`: that compares tensors with ==)
                runs = [(0, n, self._run_key(group, g.uniform))]
                if advance:
                    g.uniform = self._count_after(g.uniform)      # (g.steps is brought up to date when the group stops being uniform)
                    if n and self._HAS_STEP:
                        g.steps_t += 1
                    if not g.inserted:
                        self._insert_state(g, range(n))
                        g.inserted = True
            else:
                # runs of consecutive records that have a gradient and share their step count
                if g.uniform is not None:
                    g.steps = [g.uniform] * n
                runs = []
                for i, gr in enumerate(mine):
                    if gr is None or g.numels[i] == 0:
                        continue
                    key = self._run_key(group, g.steps[i])
                    if runs and runs[-1][1] == i and runs[-1][2] == key:
                        runs[-1] = (runs[-1][0], i + 1, key)
                    else:
                        runs.append((i, i + 1, key))
                if advance:
                    idx = [i for i, gr in enumerate(mine) if gr is not None]
                    for i in idx:
                        g.steps[i] = self._count_after(g.steps[i])
                    if self._HAS_STEP:
                        g.steps_t[torch.tensor(idx, dtype=torch.int64)] += 1
                    self._insert_state(g, idx)
                g.uniform = g.steps[0] if len(set(g.steps)) == 1 else None
            for i0, i1, key in runs:
                v0 = (g.vbase + g.offs[i0]) & -LINE
                v1 = g.vbase + g.offs[i1 - 1] + g.numels[i1 - 1]
                if v1 <= v0:
                    continue
                self._launch(L, group, g, table, g.rec0 + i0, g.rec0 + i1, v0, v1, base or None, key, coef, stream)
                self.launches += 1
        B._bump_epoch()
        return loss


def _check_adam_args(name, lr, betas, eps, weight_decay):
    if isinstance(lr, torch.Tensor):
        raise ValueError('lidal_amd.optim.%s: lr must be a Python number, not a tensor' % name)
    if not 0.0 <= lr:
        raise ValueError('Invalid learning rate: %r' % (lr,))
    if not 0.0 <= eps:
        raise ValueError('Invalid epsilon value: %r' % (eps,))
    if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
        raise ValueError('Invalid beta parameters: %r' % (betas,))
    if not 0.0 <= weight_decay:
        raise ValueError('Invalid weight_decay value: %r' % (weight_decay,))


class Adam(_OneLaunch):
    """torch.optim.Adam (coupled weight decay).  Without clip_grad_norm a step is lidal_adam_step alone."""
    _NAME = 'Adam'
    _REFUSED = ('amsgrad', 'maximize', 'capturable', 'differentiable', 'decoupled_weight_decay')
    _STATE = ('exp_avg', 'exp_avg_sq')
    _HAS_STEP = True
    _DECOUPLED = False

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, maximize=False,
                 capturable=False, differentiable=False, clip_grad_norm=None):
        _check_adam_args(self._NAME, lr, betas, eps, weight_decay)
        self._setup(clip_grad_norm)
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize,
                        capturable=capturable, differentiable=differentiable)
        if self._DECOUPLED:
            defaults['decoupled_weight_decay'] = True
        super().__init__(params, defaults)

    def _loaded_step(self, entry):
        return entry['step']

    def _launch(self, L, group, g, table, r0, r1, v0, v1, base, done, coef, stream):
        lr, (beta1, beta2), eps, wd = group['lr'], group['betas'], group['eps'], group['weight_decay']
        t = done + 1
        m, v = g.bufs
        scalars = (1 - beta1, beta2, 1 - beta2, math.sqrt(1 - beta2 ** t), eps, -(lr / (1 - beta1 ** t)), wd)
        if coef is None and not self._DECOUPLED:
            B.check(L.lidal_adam_step(table, r0, r1, v0, v1, base, m.data_ptr(), v.data_ptr(), g.size, *scalars, stream),
                    'adam_step')
        else:
            B.check(L.lidal_adam_step_ex(table, r0, r1, v0, v1, base, m.data_ptr(), v.data_ptr(), g.size, *scalars,
                                         1 if self._DECOUPLED else 0, 1 - lr * wd, coef, stream),
                    'adamw_step' if self._DECOUPLED else 'adam_step_clipped')


class AdamW(Adam):
    """torch.optim.AdamW: p = p * (1 - lr * weight_decay) first, then Adam's five lines on the plain gradient.  Its
    param_groups carry decoupled_weight_decay=True, as torch's do, and its state_dict loads into torch.optim.AdamW."""
    _NAME = 'AdamW'
    _REFUSED = ('amsgrad', 'maximize', 'capturable', 'differentiable')
    _DECOUPLED = True

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, maximize=False,
                 capturable=False, differentiable=False, clip_grad_norm=None):
        super().__init__(params, lr, betas, eps, weight_decay, amsgrad, maximize=maximize, capturable=capturable,
                         differentiable=differentiable, clip_grad_norm=clip_grad_norm)

    @classmethod
    def _check_group(cls, group):
        super()._check_group(group)
        if not group.get('decoupled_weight_decay', True):
            raise ValueError('lidal_amd.optim.AdamW does not implement decoupled_weight_decay=False '
                             '(lidal_amd.optim.Adam is the coupled form)')
        group['decoupled_weight_decay'] = True


class SGD(_OneLaunch):
    """torch.optim.SGD.  One flat `momentum_buffer` per group, allocated by the first step with momentum != 0; with momentum
    0 there is no state at all, as in torch.  torch's SGD keeps no step count in its state, so the counts live on the
    host: a parameter's first step with momentum writes buf = g, and a loaded dict without a buffer for a parameter means
    'first step' for it."""
    _NAME = 'SGD'
    _REFUSED = ('maximize', 'differentiable')
    _STATE = ('momentum_buffer',)
    _HAS_STEP = False

    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, *, maximize=False,
                 differentiable=False, clip_grad_norm=None):
        if isinstance(lr, torch.Tensor):
            raise ValueError('lidal_amd.optim.SGD: lr must be a Python number, not a tensor')
        if lr < 0.0:
            raise ValueError('Invalid learning rate: %r' % (lr,))
        if momentum < 0.0:
            raise ValueError('Invalid momentum value: %r' % (momentum,))
        if weight_decay < 0.0:
            raise ValueError('Invalid weight_decay value: %r' % (weight_decay,))
        self._setup(clip_grad_norm)
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov,
                        maximize=maximize, differentiable=differentiable)
        super().__init__(params, defaults)

    @classmethod
    def _check_group(cls, group):
        super()._check_group(group)
        if group['nesterov'] and (group['momentum'] <= 0 or group['dampening'] != 0):
            raise ValueError('Nesterov momentum requires a momentum and zero dampening')

    def _loaded_step(self, entry):
        return 1                        # a buffer: this parameter has stepped

    def _advances(self, group):
        return group['momentum'] != 0

    def _run_key(self, group, done):
        return group['momentum'] != 0 and done == 0         # the launch writes buf = g

    def _count_after(self, done):
        return 1                        # all that counts: a parameter that lagged is level again once it has its buffer

    def _launch(self, L, group, g, table, r0, r1, v0, v1, base, first, coef, stream):
        mom = group['momentum']
        buf = self._state_bufs(g)[0].data_ptr() if mom != 0 else None
        B.check(L.lidal_sgd_step(table, r0, r1, v0, v1, base, buf, g.size, mom, 1 - group['dampening'], -group['lr'],
                                 group['weight_decay'], 1 if group['nesterov'] else 0, 1 if first else 0, coef, stream),
                'sgd_step')
