"""Side-stream forks of a launch plan that ride on the producing launch (csrc/plan.hip run_ops, launch_tail in
csrc/common.h): the side stream waits for the completion event of the launch in front of the fork, and the main
stream carries no marker.  Every case compares bytes against the same operations queued on the main stream alone, with
the producers' outputs poisoned before each run (a consumer that started early reads the poison), and reads the
library's counters (forks attached to a launch, forks that fell back to a marker): a silent fallback passes no case."""
import array
import copy
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'

OP_BN_BWD, OP_COLSUM, OP_TRANSPOSE_F32, OP_FORK, OP_JOIN = 7, 11, 23, 26, 27
F32, BF16 = 0, 1
SHAPES = [(n, c, dt) for n in (129, 1000) for c in (32, 96) for dt in (torch.bfloat16, torch.float32)]
IDS = ['%dx%d-%s' % (n, c, 'bf16' if dt == torch.bfloat16 else 'f32') for n, c, dt in SHAPES]


def _lib():
    from lidal_amd import backend as B
    return B.lib_handle()


def _counts(reset=False):
    from lidal_amd import backend as B
    return B.plan_fork_counts(reset=reset)


class _Streams:
    """A main stream of its own (not the default stream) and the library's side streams 1 and 2."""

    def __init__(self):
        from lidal_amd import backend as B
        dev = torch.device('cuda', torch.cuda.current_device())
        self.main = torch.cuda.Stream()
        self.raw = [self.main.cuda_stream, B.side_stream(dev, 1).cuda_stream, B.side_stream(dev, 2).cuda_stream]

    def run(self, ops):
        """ops: (kind, side stream, [argument words]); -> the library's return code, after the device has drained."""
        words = []
        for kind, side, args in ops:
            words.append(kind | (side << 16))
            words += [int(a) for a in args]
        arr = array.array('q', words)
        streams = (ctypes.c_void_p * 3)(*self.raw)
        torch.cuda.synchronize()
        rc = _lib().lidal_plan_run_streams(arr.buffer_info()[0], len(words), len(ops), streams, 3)
        torch.cuda.synchronize()
        return rc


class _Bn:
    """One BatchNorm backward (x, dy -> dx, grad_gamma, grad_beta) and the words of its plan operation."""

    def __init__(self, n, c, dtype, seed):
        g = torch.Generator(device=DEV).manual_seed(seed)
        self.n, self.c, self.code = n, c, BF16 if dtype == torch.bfloat16 else F32
        self.x = torch.randn(n, c, device=DEV, generator=g).to(dtype)
        self.dy = torch.randn(n, c, device=DEV, generator=g).to(dtype)
        self.gamma = torch.rand(c, device=DEV, generator=g) + 0.5
        self.beta = torch.randn(c, device=DEV, generator=g) * 0.1
        xf = self.x.float()
        self.mean = xf.mean(0)
        self.invstd = (xf.var(0, unbiased=False) + 1e-5).rsqrt()
        self.dx = torch.empty_like(self.x)
        self.gg = torch.empty(c, device=DEV)
        self.gb = torch.empty(c, device=DEV)
        self.ws_bytes = int(_lib().lidal_bn_workspace_bytes(n, c))
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=DEV)

    def op(self, side=0, code=None):
        p = lambda t: t.data_ptr()
        return (OP_BN_BWD, side, [p(self.x), p(self.dy), self.c, self.code if code is None else code, self.n, self.c,
                                  p(self.gamma), p(self.beta), 1, p(self.mean), p(self.invstd), p(self.dx), p(self.gg),
                                  p(self.gb), p(self.ws), self.ws_bytes])

    def outputs(self):
        return [self.dx, self.gg, self.gb]


class _Colsum:
    """Column sums of a [n, c] matrix into `out`, with a workspace of its own."""

    def __init__(self, src, n, c, code):
        self.src, self.n, self.c, self.code = src, n, c, code
        self.out = torch.empty(c, device=DEV)
        self.ws_bytes = int(_lib().lidal_bn_workspace_bytes(n, c)) + 3 * c * 4
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=DEV)

    def op(self, side=0):
        return (OP_COLSUM, side, [self.src.data_ptr(), self.code, self.n, self.c, self.out.data_ptr(), self.ws.data_ptr(),
                                  self.ws_bytes])


def _poison(tensors):
    for t in tensors:
        t.view(torch.uint8).fill_(0x7F)


def _bytes(tensors):
    return [t.contiguous().view(torch.uint8).clone() for t in tensors]


def _compare(streams, outputs, plain, forked, counts):
    """Run `plain` (main stream only), then `forked`: the same bytes in `outputs`, and the counters read `counts`."""
    _poison(outputs)
    assert streams.run(plain) == 0, _lib().lidal_last_error()
    want = _bytes(outputs)
    _poison(outputs)
    _counts(reset=True)
    assert streams.run(forked) == 0, _lib().lidal_last_error()
    assert _counts() == counts
    for i, (a, b) in enumerate(zip(want, _bytes(outputs))):
        assert torch.equal(a, b), i


@pytest.mark.parametrize('n,c,dtype', SHAPES, ids=IDS)
def test_one_fork_rides_on_the_batchnorm_launch(n, c, dtype):
    s = _Streams()
    bn = _Bn(n, c, dtype, 1)
    cs = _Colsum(bn.dx, n, c, bn.code)
    _compare(s, bn.outputs() + [cs.out], [bn.op(), cs.op()],
             [bn.op(), (OP_FORK, 1, []), cs.op(1), (OP_JOIN, 1, [])], (1, 0))


@pytest.mark.parametrize('n,c,dtype', SHAPES, ids=IDS)
def test_two_forks_share_one_launch(n, c, dtype):
    s = _Streams()
    bn = _Bn(n, c, dtype, 2)
    a, b = _Colsum(bn.dx, n, c, bn.code), _Colsum(bn.dx, n, c, bn.code)
    _compare(s, bn.outputs() + [a.out, b.out], [bn.op(), a.op(), b.op()],
             [bn.op(), (OP_FORK, 1, []), (OP_FORK, 2, []), a.op(1), b.op(2), (OP_JOIN, 1, []), (OP_JOIN, 2, [])], (2, 0))


@pytest.mark.parametrize('n,c', [(129, 32), (129, 96), (1000, 32), (1000, 96)])
def test_producer_without_a_tail_launch_falls_back_to_a_marker(n, c):
    """lidal_transpose_f32 does not carry the event: the fork records its marker, the consumer still sees the result."""
    s = _Streams()
    src = torch.randn(c, n, device=DEV)
    dst = torch.empty(n, c, device=DEV)
    cs = _Colsum(dst, n, c, F32)
    tr = (OP_TRANSPOSE_F32, 0, [src.data_ptr(), n, dst.data_ptr(), c, n])
    _compare(s, [dst, cs.out], [tr, cs.op()], [tr, (OP_FORK, 1, []), cs.op(1), (OP_JOIN, 1, [])], (0, 1))
    assert torch.equal(dst, src.t())


@pytest.mark.parametrize('n,c,dtype', SHAPES, ids=IDS)
def test_fork_with_nothing_to_attach_to(n, c, dtype):
    s = _Streams()
    bn = _Bn(n, c, dtype, 4)
    # the fork opens the plan (what it orders against was queued by an earlier call)
    first = _Colsum(bn.x, n, c, bn.code)
    _compare(s, [first.out], [first.op()], [(OP_FORK, 1, []), first.op(1), (OP_JOIN, 1, [])], (0, 1))
    # the second fork follows an operation that ran on side stream 1: only the first one attaches
    a, b = _Colsum(bn.dx, n, c, bn.code), _Colsum(bn.dx, n, c, bn.code)
    _compare(s, bn.outputs() + [a.out, b.out], [bn.op(), a.op(), b.op()],
             [bn.op(), (OP_FORK, 1, []), a.op(1), (OP_FORK, 2, []), b.op(2), (OP_JOIN, 1, []), (OP_JOIN, 2, [])], (1, 1))


@pytest.mark.parametrize('n,c,dtype', SHAPES, ids=IDS)
def test_host_side_error_between_dispatch_and_fork(n, c, dtype):
    s = _Streams()
    bn = _Bn(n, c, dtype, 5)
    cs = _Colsum(bn.dx, n, c, bn.code)
    tail = [(OP_FORK, 1, []), cs.op(1), (OP_JOIN, 1, [])]
    # an unknown operation kind where the fork should be, and a producer refused (bad dtype) while its fork's event
    # is pending: both are host-side checks, nothing is launched for them
    for bad in ([bn.op(), (999, 0, [])] + tail, [bn.op(code=7)] + tail):
        _counts(reset=True)
        assert s.run(bad) != 0
        assert b'plan_run: op' in _lib().lidal_last_error()
        assert _counts() == (0, 0)
        # the next plan of this thread runs, attaches, and computes the same bytes
        _compare(s, bn.outputs() + [cs.out], [bn.op(), cs.op()], [bn.op()] + tail, (1, 0))


@pytest.mark.parametrize('n,c,dtype', SHAPES, ids=IDS)
def test_forty_edges_reuse_one_side_stream(n, c, dtype):
    """One event per side stream, re-bound by every producing launch: each wait means the launch it follows."""
    s = _Streams()
    bns = [_Bn(n, c, dtype, 100 + k) for k in range(40)]
    for b in bns[1:]:                       # (main-stream operations are ordered among themselves: one workspace)
        b.ws = bns[0].ws
    sums = [_Colsum(b.dx, n, c, b.code) for b in bns]
    for q in sums[1:]:                      # (so are the consumers on side stream 1)
        q.ws = sums[0].ws
    plain, forked = [], []
    for b, q in zip(bns, sums):
        plain += [b.op(), q.op()]
        forked += [b.op(), (OP_FORK, 1, []), q.op(1)]
    forked.append((OP_JOIN, 1, []))
    outputs = [t for b in bns for t in b.outputs()] + [q.out for q in sums]
    _compare(s, outputs, plain, forked, (40, 0))


def _step(model, batch, planned):
    from lidal_amd.network import plan
    from lidal_amd.train_step import forward_backward
    saved = plan.ENABLED
    plan.ENABLED = planned
    try:
        torch.manual_seed(11)               # SPVCNN's dropout masks
        loss, logits = forward_backward(model, *batch, autocast=True)
        torch.cuda.synchronize()
        return loss.detach().clone(), logits.detach().clone(), [p.grad.clone() for p in model.parameters()]
    finally:
        plan.ENABLED = saved


@pytest.mark.parametrize('name', ['spvcnn', 'minkunet'])
def test_whole_planned_step_attaches_its_forks(name):
    from lidal_amd import synth
    from lidal_amd.network import SPVCNN, MinkUNet
    torch.manual_seed(0)
    a = {'spvcnn': SPVCNN, 'minkunet': MinkUNet}[name](19).to(DEV).train()
    b = copy.deepcopy(a)
    d = synth.make_train_batch(n_frames=1, n_points=10000, seed=77)
    batch = tuple(torch.from_numpy(d[k]).to(DEV) for k in ('feats_v_b', 'coords_v_b', 'labels_v_b'))
    la, ya, ga = _step(a, batch, planned=False)
    _counts(reset=True)
    lb, yb, gb = _step(b, batch, planned=True)
    attached, marker = _counts()
    assert torch.equal(la, lb) and torch.equal(ya, yb)
    for (k, _), p, q in zip(a.named_parameters(), ga, gb):
        assert torch.equal(p.view(torch.uint8), q.view(torch.uint8)), k
    print('%s: %d forks attached to a launch, %d behind a marker' % (name, attached, marker))
    assert attached + marker >= 40, (attached, marker)
    assert attached >= 0.9 * (attached + marker), (attached, marker)
