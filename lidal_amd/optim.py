"""`optimizer.step()` of the training step (train.py:56,140) as ONE kernel launch: Adam over every parameter tensor of a
group at once (csrc/optim.hip, lidal_adam_step), opt-in beside torch.optim.Adam.

    opt = lidal_amd.optim.Adam(model.parameters())          # the reference's defaults: lr 1e-3, betas (0.9, 0.999), eps 1e-8

The arithmetic is torch's single-tensor Adam with every operation rounded separately in f32 (tests/adam_ref.py restates
it in numpy; the kernel equals it bit for bit).  What makes one launch possible:

  * state: ONE flat f32 `exp_avg` buffer and ONE flat `exp_avg_sq` buffer per parameter group; `state[p]['exp_avg']` /
    `['exp_avg_sq']` are views of them and `state[p]['step']` a view of one host tensor per group, so `state_dict()` has
    torch.optim.Adam's format, loads into it and the other way round;
  * a device table with one record per parameter (address, where its gradient is, where its state is, how many
    elements), uploaded when an address in it changed -- ordinarily once: after the planned step (network/plan.py) the
    gradients are views of one flat buffer with a fixed layout (flat.BackToBack, the test DataParallel uses), and the
    table then names them RELATIVE to that buffer, which is a fresh allocation every step; any other gradients are named
    by absolute address;
  * the launch covers a run of consecutive records that share their step count and hyperparameters: one launch per group
    and step, more only where a parameter skipped steps (`.grad is None`) or is missing inside a group.

After a step `backend._bump_epoch()` tells the cached weight operands (LDS images, folded BatchNorm maps) that the
parameters moved: writes through raw pointers move no version counter."""
import math

import numpy as np
import torch

from . import backend as B
from .flat import BackToBack

__all__ = ['Adam']

_REFUSED = ('amsgrad', 'maximize', 'capturable', 'differentiable', 'decoupled_weight_decay')
_LINE = 32              # elements of a 128-byte line: the virtual axis keeps every tensor's phase in it


class _Group:
    """What one parameter group keeps beside its dict (which state_dict() serialises)."""
    __slots__ = ('params', 'numels', 'offs', 'size', 'm', 'v', 'steps', 'steps_t', 'uniform', 'rec0', 'vbase', 'inserted')


class Adam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, maximize=False,
                 capturable=False, differentiable=False):
        if isinstance(lr, torch.Tensor):
            raise ValueError('lidal_amd.optim.Adam: lr must be a Python number, not a tensor')
        if not 0.0 <= lr:
            raise ValueError('Invalid learning rate: %r' % (lr,))
        if not 0.0 <= eps:
            raise ValueError('Invalid epsilon value: %r' % (eps,))
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError('Invalid beta parameters: %r' % (betas,))
        if not 0.0 <= weight_decay:
            raise ValueError('Invalid weight_decay value: %r' % (weight_decay,))
        self._rt = []                   # _Group per parameter group
        self._params = None             # the parameters of every group in record order
        self._table = None              # device table int64 [records, 5]
        self._addr_p = None             # per record: the parameter's address in the table
        self._addr_g = None             # per record: the gradient's address minus the base the table is relative to
        self._flat_form = False         # the table's gradient words are relative to a flat buffer
        self._b2b = BackToBack()
        self.launches = 0               # kernel launches so far
        self.table_uploads = 0          # host-to-device copies of the table so far
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize,
                        capturable=capturable, differentiable=differentiable)
        super().__init__(params, defaults)

    # ---- what it refuses -----------------------------------------------------------------------------------------
    @staticmethod
    def _check_group(group):
        for key in _REFUSED:
            if group.get(key):
                raise ValueError('lidal_amd.optim.Adam does not implement %s=%r (torch.optim.Adam does)' % (key, group[key]))
        if isinstance(group['lr'], torch.Tensor):
            raise ValueError('lidal_amd.optim.Adam: lr must be a Python number, not a tensor')

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
                    raise ValueError('lidal_amd.optim.Adam: parameters must be float32 (got %s of shape %s)'
                                     % (p.dtype, tuple(p.shape)))
                if not p.is_contiguous():
                    raise ValueError('lidal_amd.optim.Adam: parameters must be contiguous (shape %s, strides %s)'
                                     % (tuple(p.shape), p.stride()))
            if len(devices) > 1:
                raise ValueError('lidal_amd.optim.Adam: parameters on more than one device (%s)'
                                 % ', '.join(sorted(str(d) for d in devices)))
        except ValueError:
            self.param_groups.pop()
            raise
        self._table = None

    # ---- state ---------------------------------------------------------------------------------------------------
    def _groups(self):
        """The flat state of every group, allocated at first use (a step or load_state_dict)."""
        rt = self._rt
        while len(rt) < len(self.param_groups):
            group = self.param_groups[len(rt)]
            g = _Group()
            g.params = list(group['params'])
            g.numels = [p.numel() for p in g.params]
            g.offs = []
            off = 0
            for p, n in zip(g.params, g.numels):        # the state offset takes the parameter's phase in a 128-byte line
                off += (p.data_ptr() // 4 - off) % _LINE
                g.offs.append(off)
                off += n
            g.size = off
            dev = g.params[0].device if g.params else torch.device('cpu')
            g.m = torch.zeros(max(off, 1), dtype=torch.float32, device=dev)
            g.v = torch.zeros(max(off, 1), dtype=torch.float32, device=dev)
            g.steps = [0] * len(g.params)
            g.steps_t = torch.zeros(len(g.params), dtype=torch.float32)
            g.uniform = 0
            g.inserted = False
            rt.append(g)
            self._table = None
            self._params = None
        return rt

    def _insert_state(self, g, indices):
        for i in indices:
            p = g.params[i]
            if p not in self.state:
                o, n = g.offs[i], g.numels[i]
                self.state[p] = {'step': g.steps_t[i], 'exp_avg': g.m[o:o + n].view(p.shape),
                                 'exp_avg_sq': g.v[o:o + n].view(p.shape)}

    def load_state_dict(self, state_dict):
        """Accepts this optimizer's dict or torch.optim.Adam's: the loaded moments are copied INTO the flat buffers (the
        base class would put the loaded tensors in the views' place).  As in torch, state_dict() hands out the live tensors:
        copy.deepcopy it before loading it into an optimizer that goes on stepping beside this one."""
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
            have = [i for i, p in enumerate(g.params) if p in loaded and len(loaded[p])]
            if not have:
                continue
            steps = [loaded[g.params[i]]['step'] for i in have]
            if any(isinstance(s, torch.Tensor) and s.is_cuda for s in steps):
                steps = torch.stack([torch.as_tensor(s).float().reshape(()).to(steps[0].device) for s in steps]).tolist()
            for i, s in zip(have, steps):
                p = g.params[i]
                o, n = g.offs[i], g.numels[i]
                g.m[o:o + n].copy_(loaded[p]['exp_avg'].reshape(-1))
                g.v[o:o + n].copy_(loaded[p]['exp_avg_sq'].reshape(-1))
                g.steps[i] = int(round(float(s)))
            g.steps_t.copy_(torch.tensor(g.steps, dtype=torch.float32))
            g.uniform = g.steps[0] if len(set(g.steps)) == 1 else None
            self._insert_state(g, have)
            g.inserted = len(have) == len(g.params)

    # ---- the table -----------------------------------------------------------------------------------------------
    def _build_table(self, rt, grads, addr_p, addr_g, device):
        """One record per parameter of every group, group after group.  `grads`: per record the gradient or None."""
        n_rec = len(addr_p)
        present = [g for g in grads if g is not None]
        base = 0
        self._flat_form = False
        if len(present) == n_rec and self._b2b.flat(present) is not None:
            base = present[self._b2b.layout[1]].data_ptr()
            self._flat_form = True
        gword = [(a - base) if a is not None else None for a in addr_g]
        offs, vstart, numels = [], [], []
        r = 0
        v = 0
        for g in rt:
            g.rec0 = r
            v += -v % _LINE
            g.vbase = v                         # virtual index = vbase + state offset
            offs += g.offs
            vstart += [v + o for o in g.offs]
            numels += g.numels
            r += len(g.params)
            v += g.size
        words = np.array([addr_p, [w or 0 for w in gword], offs, vstart, numels], dtype=np.int64).T.copy()
        self._table = torch.from_numpy(words).to(device)
        self.table_uploads += 1
        self._addr_p = list(addr_p)
        self._addr_g = gword

    # ---- the step ------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        rt = self._groups()
        grads, addr_g = [], []
        complete = []                   # per group: every parameter has a gradient
        for group, g in zip(self.param_groups, rt):
            if len(group['params']) != len(g.params):
                raise ValueError('lidal_amd.optim.Adam: the parameters of a group changed after the first step')
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
                    raise ValueError('lidal_amd.optim.Adam does not take sparse gradients (torch.optim.SparseAdam does)')
                if gr.dtype is not torch.float32:
                    raise ValueError('lidal_amd.optim.Adam: gradients must be float32 (got %s for a parameter of '
                                     'shape %s)' % (gr.dtype, tuple(p.shape)))
                if not gr.is_contiguous():
                    gr = gr.contiguous()
                grads.append(gr)
                addr_g.append(gr.data_ptr())
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
            base = next(a - w for a, w in zip(addr_g, self._addr_g) if a is not None)
        L = B.lib()
        stream = B.stream()
        table = self._table.data_ptr()
        for group, g, whole in zip(self.param_groups, rt, complete):
            n = len(g.params)
            mine = grads[g.rec0:g.rec0 + n]
            if g.uniform is not None and whole:       # (never `None in mine`: that compares tensors with ==)
                runs = [(0, n, g.uniform)]
                g.uniform += 1                  # (g.steps is brought up to date when the group stops being uniform)
                if n:
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
                    if runs and runs[-1][1] == i and runs[-1][2] == g.steps[i]:
                        runs[-1] = (runs[-1][0], i + 1, g.steps[i])
                    else:
                        runs.append((i, i + 1, g.steps[i]))
                idx = [i for i, gr in enumerate(mine) if gr is not None]
                for i in idx:
                    g.steps[i] += 1
                g.steps_t[torch.tensor(idx, dtype=torch.int64)] += 1
                g.uniform = g.steps[0] if len(set(g.steps)) == 1 else None
                self._insert_state(g, idx)
            if not runs:
                continue
            lr, (beta1, beta2), eps, wd = group['lr'], group['betas'], group['eps'], group['weight_decay']
            for i0, i1, done in runs:
                t = done + 1
                v0 = (g.vbase + g.offs[i0]) & -_LINE
                v1 = g.vbase + g.offs[i1 - 1] + g.numels[i1 - 1]
                if v1 <= v0:
                    continue
                B.check(L.lidal_adam_step(table, g.rec0 + i0, g.rec0 + i1, v0, v1, base or None, g.m.data_ptr(),
                                          g.v.data_ptr(), g.size, 1 - beta1, beta2, 1 - beta2,
                                          math.sqrt(1 - beta2 ** t), eps, -(lr / (1 - beta1 ** t)), wd, stream),
                        'adam_step')
                self.launches += 1
        B._bump_epoch()
        return loss
