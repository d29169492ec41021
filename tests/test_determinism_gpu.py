"""Run-to-run bit-equality of whole training runs: the planned step with EVERY
side stream on (weight gradients, shortcut branches, the point branch, the next step's tables) repeated from one state
must give the same losses, logits, gradients and parameters bit for bit.  scripts/exp/determinism_steps.py is the
exploratory form of this file (which gradients differ, by how much); profiles/README.md has the history: the ONE pair
that was ever seen to differ -- the fused f64 block tail of the f32 mode while f32 weight gradients ran beside it on their
side stream, one run in ~20 -- is off by default and cannot be put together by the environment knobs any more
(network/plan.py side()); round 6 met the same signature at 100 % with the split-form weight gradients beside the BatchNorm
backward of the f32 mode, which now runs single-stream (plan.SIDE_F32)."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _batches(n, points):
    from lidal_amd import synth
    out = []
    for i in range(n):
        b = synth.make_train_batch(n_frames=2, n_points=points + 7000 * i, seed=100 + i)
        out.append(tuple(torch.from_numpy(b[k]).to(DEV) for k in ('feats_v_b', 'coords_v_b', 'labels_v_b')))
    return out


def _run(base, batches, steps, autocast, prefetch):
    from lidal_amd.network import GeometryPrefetcher
    from lidal_amd.train_step import train_step
    model = copy.deepcopy(base)
    opt = torch.optim.Adam(model.parameters(), fused=True)
    torch.manual_seed(1)                 # (dropout masks: the same draws in every repetition)
    pf = GeometryPrefetcher(model, device=torch.device(DEV)) if prefetch else None
    g = pf.submit(batches[0][1]) if pf else None
    hist = []
    for s in range(steps):
        f, c, lab = batches[s % len(batches)]
        loss, logits = train_step(model, opt, f, c, lab, autocast=autocast, geometry=g)
        if pf:
            g = pf.submit(batches[(s + 1) % len(batches)][1])
        hist.append((loss.detach().clone(), logits.detach().float().sum().clone()))
    if pf:
        pf.drain()
    torch.cuda.synchronize()
    return hist, [p.detach().clone() for p in model.parameters()], [p.grad.detach().clone() for p in model.parameters()]


def _same(a, b):
    (ha, pa, ga), (hb, pb, gb) = a, b
    first = next((i for i, (u, v) in enumerate(zip(ha, hb)) if not (torch.equal(u[0], v[0]) and torch.equal(u[1], v[1]))), None)
    assert first is None, 'losses / logits differ from step %d on' % first
    bad = [i for i, (u, v) in enumerate(zip(ga, gb)) if not torch.equal(u, v)]
    assert not bad, 'gradients of %d parameters differ in the last step' % len(bad)
    assert all(torch.equal(u, v) for u, v in zip(pa, pb))


@pytest.mark.parametrize('name', ['spvcnn', 'minkunet'])
def test_fifty_bf16_steps_twice_are_bit_equal_with_every_side_stream_on(name):
    from lidal_amd.network import SPVCNN, MinkUNet, plan
    assert plan.ENABLED and plan.SIDE_ROWS and plan.BRANCH_ROWS and plan.POINT_SIDE      # the shipped concurrency
    torch.manual_seed(0)
    base = (SPVCNN if name == 'spvcnn' else MinkUNet)(19).to(DEV).train()
    batches = _batches(3, 60000)         # 90-107 k voxels: level 0 is above BRANCH_ROWS, every level's weight gradients on the side stream
    a = _run(base, batches, 50, True, True)
    b = _run(base, batches, 50, True, True)
    _same(a, b)
    assert all(torch.isfinite(l[0]) for l in a[0])


@pytest.mark.parametrize('side', [False, True])
def test_f32_steps_are_bit_equal_run_to_run(side):
    """The f32 parity mode, eight repetitions of six steps.  side=False: as shipped (round 6: every kernel of the f32 step on
    one stream).  side=True: the weight gradients -- in the split form -- beside the data gradients with the main stream
    joining before every BatchNorm backward (plan.F32_BN_ALONE): the other configuration found clean.  (With the weight
    gradients beside the BatchNorm backward too, EVERY run of this test differed: profiles/README.md, round 6.)"""
    from lidal_amd.network import SPVCNN, plan
    from lidal_amd.nn.functional import norm
    assert norm.TAIL_SUMS_ROWS == 0 and plan.F32_BN_ALONE and not plan.SIDE_F32
    torch.manual_seed(0)
    base = SPVCNN(19).to(DEV).train()
    batches = _batches(3, 60000)
    saved = plan.SIDE_F32
    plan.SIDE_F32 = side
    try:
        first = _run(base, batches, 6, False, False)
        for _ in range(7):
            _same(first, _run(base, batches, 6, False, False))
    finally:
        plan.SIDE_F32 = saved
