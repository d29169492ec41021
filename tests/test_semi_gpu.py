"""lidal_amd.semi on the GPU (csrc/semi.hip) against the numpy restatement tests/semi_ref.py: the
one-launch EMA bit for bit at every edge of its chunks and phases and on a real network, the pseudo labels exactly under
thresholds no confidence is near, the consistency term and its gradient within 8 x the f32 restatement's own distance
from the all-f64 reference, its exact properties, and the mean-teacher step end to end."""
import math

import numpy as np
import pytest
import torch

import semi_ref as R
from guarded_ws import Guarded

pytestmark = pytest.mark.gpu
DEV = 'cuda'
PATTERN = -1515870811                   # 0xA5A5A5A5 as int32: the bytes around every view


def _g(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_f32(got, want):
    """Equal as raw bits; where the restatement has a NaN the kernel must have a NaN (IEEE 754 leaves a NaN's sign and
    payload to the implementation, and the restatement runs on another one)."""
    got, want = np.asarray(got, np.float32).reshape(-1), np.asarray(want, np.float32).reshape(-1)
    nan = np.isnan(want)
    return np.array_equal(nan, np.isnan(got)) and np.array_equal(_bits(got)[~nan], _bits(want)[~nan])


# ==================================================================================================== the EMA
def _chunk():
    from lidal_amd import backend as B
    return int(B.lib().lidal_ema_chunk_elems())


def _values(rng, n):
    v = (rng.normal(size=n) * 10.0 ** rng.integers(-3, 3, n)).astype(np.float32)
    tiny = np.finfo(np.float32).tiny
    special = np.array([np.nan, np.inf, -np.inf, tiny / 4, -tiny / 8, 1e-45, 0.0, -0.0], np.float32)
    spots = set(range(min(n, 6))) | {n // 2 + k for k in range(6) if n // 2 + k < n} | {n - 1 - k for k in range(min(n, 6))}
    for k, i in enumerate(sorted(spots)):               # at the head, in the middle and at the tail
        v[i] = special[k % len(special)]
    return v


class _Views(torch.nn.Module):
    """Parameters, float buffers and int64 buffers that are views into ONE int32 arena filled with a pattern: tensor k
    starts `offs[k]` elements behind a 16-byte boundary, eight pattern words lie between neighbours."""

    def __init__(self, sizes, offs, seed, int_words=True):
        super().__init__()
        rng = np.random.default_rng(seed)
        self.spans = []                                 # (name, kind, first word, words)
        at = 0
        plan = []
        for k, (n, o) in enumerate(zip(sizes, offs)):
            for kind in ('p', 'f', 'i'):
                words = 2 * n if kind == 'i' else n
                oo = (o & 2) if kind == 'i' else o          # (an int64 starts on 8 bytes)
                at = (at + 8 + 3) // 4 * 4 + oo
                plan.append(('%s%d' % (kind, k), kind, at, words))
                at += words
        self.arena = torch.full((at + 16,), PATTERN, dtype=torch.int32, device=DEV)
        for name, kind, a0, words in plan:
            view = self.arena[a0:a0 + words]
            if kind == 'i':
                w = rng.integers(0, 2 ** 32, words, dtype=np.uint64).astype(np.uint32)
                w[::3] = 0x7FC00001                     # words that are NaN patterns when read as f32
                w[1::5] = 0xFF800001
                view.copy_(_g(w.view(np.int32)))
                t = view.view(torch.int64) if words else torch.zeros(0, dtype=torch.int64, device=DEV)
                self.register_buffer(name, t)
            else:
                view.copy_(_g(_values(rng, words).view(np.int32)))
                t = view.view(torch.float32)
                if kind == 'p':
                    self.register_parameter(name, torch.nn.Parameter(t))
                else:
                    self.register_buffer(name, t)
            self.spans.append((name, kind, a0, words))

    def tensors(self):
        return {**dict(self.named_parameters()), **dict(self.named_buffers())}

    def words(self):
        return self.arena.cpu().numpy().copy()


def _expected_arena(teacher_words, student_views, spans, alpha, buffers):
    want = teacher_words.copy()
    for name, kind, a0, n in spans:
        t = want[a0:a0 + n].view(np.float32)
        s = student_views[name]
        if kind == 'i' or (kind == 'f' and buffers == 'copy') or alpha == 0.0:
            want[a0:a0 + n] = s
        else:
            want[a0:a0 + n] = R.ema_update(t, s.view(np.float32), alpha).view(np.int32)
    return want


def _arena_matches(got, want, spans, alpha, buffers):
    inside = np.zeros(len(want), bool)
    for name, kind, a0, n in spans:
        inside[a0:a0 + n] = True
        lerp = kind == 'p' or (kind == 'f' and buffers == 'ema')
        if lerp and alpha != 0.0:
            assert _same_f32(got[a0:a0 + n].view(np.float32), want[a0:a0 + n].view(np.float32)), name
        else:
            assert np.array_equal(got[a0:a0 + n], want[a0:a0 + n]), name          # copies: no bit may move
    assert np.array_equal(got[~inside], want[~inside]), 'a byte outside the views was written'
    assert (want[~inside] == PATTERN).all()


@pytest.mark.parametrize('phase', ['same_phase', 'other_phase'])
@pytest.mark.parametrize('alpha,buffers', [(0.0, 'copy'), (0.5, 'ema'), (0.999, 'copy'), (1.0, 'ema')])
def test_ema_equals_the_restatement_at_every_edge(alpha, buffers, phase):
    """Sizes 0, 1, 3, 4, 5 and around one and two chunks, each tensor 0..3 elements behind a 16-byte boundary, student
    at the teacher's phase (16-byte path with heads and tails) or one element off (4-byte path); subnormals, infinities
    and NaNs among the values, NaN patterns in the int64 words.  Three updates: every tensor equals the restatement bit
    for bit (a NaN for a NaN), no byte outside the views moves, one launch each, one table upload; a reallocated
    student tensor costs one more upload."""
    from lidal_amd import semi
    ch = _chunk()
    sizes = [0, 1, 3, 4, 5, ch - 1, ch, ch + 1, 2 * ch + 5]
    offs_t = [k % 4 for k in range(len(sizes))]
    offs_s = offs_t if phase == 'same_phase' else [(o + 1) % 4 for o in offs_t]
    teacher, student = _Views(sizes, offs_t, 1), _Views(sizes, offs_s, 2)
    for (name, kind, a0, n), (_, _, b0, _) in zip(teacher.spans, student.spans):
        if n and kind != 'i':
            assert ((a0 - b0) % 4 == 0) == (phase == 'same_phase')
    ema = semi.EmaTeacher(student, alpha=alpha, warmup=False, buffers=buffers, model=teacher)
    assert ema.model is teacher
    student_before = student.words()
    for step in range(3):
        sv = {name: student_before[a0:a0 + n] for name, _, a0, n in student.spans}
        want = _expected_arena(teacher.words(), sv, teacher.spans, alpha, buffers)
        ema.update()
        assert ema.launches == step + 1 and ema.updates == step + 1
        _arena_matches(teacher.words(), want, teacher.spans, alpha, buffers)
        assert np.array_equal(student.words(), student_before)
    assert ema.table_uploads == 1
    fresh = torch.full((sizes[6] + 7,), PATTERN, dtype=torch.int32, device=DEV)
    new = fresh[3:3 + sizes[6]].view(torch.float32)
    new.copy_(student.p6.detach() * 2)
    student.p6.data = new                               # reallocated: its address changed
    sv = {name: student_before[b0:b0 + n] for name, _, b0, n in student.spans}
    sv['p6'] = new.cpu().numpy().view(np.int32)
    t_words = teacher.words()
    want = _expected_arena(t_words, sv, teacher.spans, alpha, buffers)
    ema.update()
    assert ema.table_uploads == 2 and ema.launches == 4
    _arena_matches(teacher.words(), want, teacher.spans, alpha, buffers)
    assert (fresh[:3] == PATTERN).all() and (fresh[3 + sizes[6]:] == PATTERN).all()
    # copy_from: every record of the copy kind, whatever alpha says
    ema.copy_from(student)
    for name, t in teacher.tensors().items():
        s = student.tensors()[name]
        assert np.array_equal(t.detach().cpu().numpy().view(np.uint8), s.detach().cpu().numpy().view(np.uint8)), name
    assert ema.launches == 5 and ema.updates == 4


def test_warm_up_walks_its_schedule_on_the_device():
    """alpha = 0.999 with warm-up: update k uses min(alpha, 1 - 1 / (k + 1)) -- a copy, then the mean of two, ..."""
    from lidal_amd import semi
    rng = np.random.default_rng(3)
    s = torch.nn.Linear(37, 11).to(DEV)
    ema = semi.EmaTeacher(s)
    t = {k: v.detach().cpu().numpy().copy() for k, v in ema.model.named_parameters()}
    for k in range(4):
        with torch.no_grad():
            for p in s.parameters():
                p.copy_(_g(rng.normal(size=tuple(p.shape)).astype(np.float32)))
        ema.update(s)
        a = R.ema_alpha(0.999, k)
        for name, p in s.named_parameters():
            t[name] = R.ema_update(t[name], p.detach().cpu().numpy(), a)
            assert _same_f32(dict(ema.model.named_parameters())[name].cpu().numpy(), t[name]), (k, name)


def _batch(seed, n_points=6000):
    from lidal_amd import synth
    b = synth.make_train_batch(n_frames=1, n_points=n_points, seed=seed)
    return (torch.from_numpy(b['coords_v_b']).to(DEV), torch.from_numpy(b['feats_v_b']).to(DEV),
            torch.from_numpy(b['labels_v_b']).to(DEV))


def _eval_logits(model, f, c):
    import lidal_amd
    was = model.training
    model.eval()
    with torch.no_grad():
        out = model(lidal_amd.SparseTensor(f, c))[0].float().clone()
    model.train(was)
    return out


def test_teacher_of_a_real_network_follows_the_student_through_the_caches():
    """MinkUNet(19) that has trained a step (so it carries a launch program and map traces): the teacher's eval-mode
    logits equal the student's byte for byte after construction; after the student's weights moved and update() ran at
    alpha = 0 -- NO backward pass in between, so only the epoch bump can tell the teacher's cached weight images and
    folded BatchNorm maps -- they are equal again; after an update at alpha = 0.99 every parameter equals the
    restatement and every buffer the student's; a state_dict round trip keeps `updates`."""
    from lidal_amd import semi
    from lidal_amd.network import MinkUNet
    from lidal_amd.train_step import train_step
    c, f, lab = _batch(5)
    torch.manual_seed(2)
    student = MinkUNet(19).to(DEV).train()
    opt = torch.optim.Adam(student.parameters(), lr=1e-2)
    train_step(student, opt, f, c, lab)
    ema = semi.EmaTeacher(student, alpha=0.0, warmup=False)
    teacher = ema.model
    for m in teacher.modules():
        assert not [k for k in m.__dict__ if k.startswith('_lidal_')]
    assert not teacher.training and not any(p.requires_grad for p in teacher.parameters())
    first = _eval_logits(teacher, f, c)                 # fills the teacher's inference caches
    assert torch.equal(first, _eval_logits(student, f, c))
    with torch.no_grad():
        for p in student.parameters():
            p.mul_(1.0 + 0.05 * torch.randn_like(p))
    moved = _eval_logits(student, f, c)
    assert not torch.equal(moved, first)
    ema.update(student)                                 # alpha = 0: a copy through raw pointers
    assert torch.equal(_eval_logits(teacher, f, c), moved)
    assert ema.launches == 1 and ema.table_uploads == 1
    # alpha = 0.99 against the restatement
    ema.alpha = 0.99
    before = {k: v.detach().cpu().numpy().copy() for k, v in teacher.state_dict().items()}
    with torch.no_grad():
        for p in student.parameters():
            p.add_(0.01 * torch.randn_like(p))
        for b in student.buffers():
            if b.dtype == torch.int64:
                b.add_(7)
            else:
                b.mul_(1.5)
    ema.update()
    names = {k for k, _ in student.named_parameters()}
    for k, v in student.state_dict().items():
        got = teacher.state_dict()[k].cpu().numpy()
        if k in names:
            assert _same_f32(got, R.ema_update(before[k], v.detach().cpu().numpy(), 0.99)), k
        else:
            assert np.array_equal(got, v.cpu().numpy()), k
    assert ema.table_uploads == 1 and ema.launches == 2 and ema.updates == 2
    sd = ema.state_dict()
    other = semi.EmaTeacher(student, alpha=0.5)
    other.load_state_dict(sd)
    assert other.updates == 2 and other.alpha == 0.99
    assert all(torch.equal(a, b) for a, b in zip(other.model.state_dict().values(), teacher.state_dict().values()))


def test_an_update_moves_the_weight_epoch_and_no_version_counter():
    from lidal_amd import backend as B
    from lidal_amd import semi
    s = torch.nn.Linear(5, 3).to(DEV)
    ema = semi.EmaTeacher(s, alpha=0.5, warmup=False)
    with torch.no_grad():
        s.weight.add_(1.0)
    w = ema.model.weight
    version, epoch, hits = w._version, B.WEIGHT_EPOCH[0], B.HITS.get('ema_step', 0)
    ema.update()
    assert B.WEIGHT_EPOCH[0] == epoch + 1 and B.HITS.get('ema_step', 0) == hits + 1 and w._version == version
    ema.copy_from(s)
    assert B.WEIGHT_EPOCH[0] == epoch + 2 and torch.equal(w, s.weight.detach())


# ==================================================================================================== pseudo labels
def _pl_case(p, c, dtype, with_inverse, seed):
    rng = np.random.default_rng(seed)
    nv = max(1, p // 2 + 3) if with_inverse else p
    x = R.logits_grid(nv, c, seed, dtype)
    if nv >= 8:
        x[4, c // 3] = np.nan                           # a NaN row: never accepted
    inverse = None
    if with_inverse:
        inverse = rng.integers(0, nv, p).astype(np.int64)
        if p >= 4:
            inverse[1], inverse[p - 1] = -1, nv         # outside: ignore_index, counted, never read through
            inverse[2] = -2 ** 40
    human = np.where(rng.random(p) < 0.25, rng.integers(0, max(c, 2), p), 255).astype(np.int64)
    return x, nv, inverse, human


def _class_thresholds(x, c):
    """Per class the midpoint of the widest gap between the sorted f64 confidences of its rows inside [0.3, 0.99]."""
    arg, conf = R.confidence(x, np.float64)
    thr = np.zeros(c, np.float32)
    for k in range(c):
        t, gap = R.gap_threshold(conf[arg == k])
        assert gap > 2e-5
        thr[k] = t
    return thr


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
@pytest.mark.parametrize('c', [1, 16, 19, 32])
@pytest.mark.parametrize('p', [1, 255, 257])
def test_pseudo_labels_equal_the_f64_reference(p, c, dtype):
    """With and without an inverse map, with and without human labels.  The labels are compared EXACTLY with the all-f64
    reference on the condition -- asserted -- that no row's f64 confidence lies within 1e-5 of its threshold (the f32
    softmax of at most 32 classes is within (32 + 4) * 2^-24 = 2.2e-6 of the f64 one; the f32 numpy form shows at most
    3.7e-7 over this grid); the confidences are held within the same 1e-5, the counts equal the reference's, human
    labels pass through, and a second call on a side stream gives the same bytes."""
    from lidal_amd import semi
    side = torch.cuda.Stream()
    for with_inverse in (False, True):
        x, nv, inverse, human = _pl_case(p, c, dtype, with_inverse, 100 * p + c)
        thr = _class_thresholds(x, c)
        arg64, conf64 = R.confidence(x, np.float64)
        with np.errstate(invalid='ignore'):
            assert int((np.abs(conf64 - thr.astype(np.float64)[arg64]) <= 1e-5).sum()) == 0
        xg = _g(x).to(torch.bfloat16) if dtype == 'bf16' else _g(x)
        if dtype == 'bf16':
            assert np.array_equal(_bits(xg.float().cpu().numpy()), _bits(x))
        for with_labels in (False, True):
            lab = human if with_labels else None
            want, wstats, wconf = R.pseudo_labels(x, thr, inverse, lab, 255, np.float64)
            args = (xg, _g(thr))
            kw = dict(inverse=None if inverse is None else _g(inverse), labels=None if lab is None else _g(lab),
                      return_conf=True)
            out, stats, conf = semi.pseudo_labels(*args, **kw)
            assert out.dtype == torch.int64 and stats.dtype == torch.int64 and conf.dtype == torch.float32
            assert np.array_equal(out.cpu().numpy(), want)
            assert np.array_equal(stats.cpu().numpy(), wstats)
            got = conf.cpu().numpy().astype(np.float64)
            assert np.array_equal(np.isnan(got), np.isnan(wconf))
            ok = ~np.isnan(wconf)
            assert ok.sum() == 0 or np.abs(got[ok] - wconf[ok]).max() <= 1e-5
            if with_labels:
                assert np.array_equal(out.cpu().numpy()[lab != 255], lab[lab != 255])
                assert int(stats.sum()) == int((lab == 255).sum())
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                out2, stats2, conf2 = semi.pseudo_labels(*args, **kw)
            side.synchronize()
            assert torch.equal(out, out2) and torch.equal(stats, stats2)
            assert np.array_equal(_bits(conf.cpu().numpy()), _bits(conf2.cpu().numpy()))
            plain = semi.pseudo_labels(*args, inverse=kw['inverse'], labels=kw['labels'])
            assert len(plain) == 2 and torch.equal(plain[0], out)


def test_pseudo_labels_take_one_number_for_every_class():
    from lidal_amd import semi
    x = R.logits_grid(257, 19, 7)
    _, conf64 = R.confidence(x, np.float64)
    thr, gap = R.gap_threshold(conf64)
    assert gap > 2e-5
    want, wstats, _ = R.pseudo_labels(x, thr, None, None, 255, np.float64)
    out, stats = semi.pseudo_labels(_g(x), thr)
    assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(stats.cpu().numpy(), wstats)
    assert 0 < wstats[:19].sum() < 257
    out, stats = semi.pseudo_labels(_g(x), thr, ignore_index=-1)
    assert np.array_equal(out.cpu().numpy(), np.where(want == 255, -1, want))
    empty, stats = semi.pseudo_labels(torch.zeros((0, 19), device=DEV), 0.5)
    assert empty.shape == (0,) and not stats.any()


# ==================================================================================================== consistency
# The f32 numpy restatement against the all-f64 reference over the whole grid below (semi_ref.consistency /
# consistency_grad, measured on the CPU; the bf16 student's gradient is rounded to bf16 in both):
CPU_LOSS = {'f32': 1.67e-7, 'bf16': 3.03e-7}
CPU_DZ = {'f32': 1.28e-6, 'bf16': 3.02e-3}
SLACK = 8           # the device's expf / logf may differ from numpy's by a couple of ulp per call


def consistency_case(n, c, dtype, seed=0):
    zs = R.logits_grid(n, c, 1000 + seed + 7 * n + c, dtype)
    zt = R.logits_grid(n, c, 2000 + seed + 7 * n + c, 'f32')
    return zs, zt


def masking_conf(zt):
    _, conf64 = R.confidence(zt, np.float64)
    thr, gap = R.gap_threshold(conf64)
    assert gap > 2e-5
    assert int((np.abs(conf64 - float(np.float32(thr))) <= 1e-5).sum()) == 0
    return thr


def restated(zs, zt, kind, mc, dtype, ft):
    """(loss, dz) in `ft`; the bf16 student's gradient as the bf16 it is returned in."""
    loss, _, mask = R.consistency(zs, zt, kind, mc, False, ft)
    dz = R.consistency_grad(zs, zt, 1.5, kind, mc, False, ft)
    if dtype == 'bf16' and ft is np.float32:
        dz = R.bf16_round(dz)
    return loss, dz.astype(np.float64), mask


def _run_consistency(zs, zt, kind, mc, dtype, g=1.5, **kw):
    from lidal_amd import semi
    s = _g(zs)
    if dtype == 'bf16':
        s = s.to(torch.bfloat16)
    s.requires_grad_(True)
    out = semi.consistency_loss(s, _g(zt), kind=kind, min_conf=mc, **kw)
    loss = out[0] if isinstance(out, tuple) else out
    (loss * g).backward()
    return out, s.grad


@pytest.mark.parametrize('c', [1, 16, 19, 32])
@pytest.mark.parametrize('n', [1, 255, 257, 4099])
def test_consistency_within_eight_times_the_f32_restatement(n, c):
    """f32 and bf16 student logits, both kinds, min_conf 0 and one value that masks some rows (the midpoint of the widest
    gap of the f64 teacher confidences, no confidence within 1e-5 of it).  Loss and dz against the all-f64 reference,
    relative to max|ref|; the bar is 8 x the largest deviation of the f32 numpy restatement from that reference over
    this same grid, measured on the CPU:
        loss  f32 student  CPU 1.67e-7   GPU observed 1.90e-7
        loss  bf16 student CPU 3.03e-7   GPU observed 2.75e-7
        dz    f32 student  CPU 1.28e-6   GPU observed 1.27e-6
        dz    bf16 student CPU 3.02e-3   GPU observed 3.01e-3   (the rounding of dz to bf16 included)
    Beside it, exactly: masked rows have dz == 0 and a zero per_row; the bf16 gradient is the f32 kernel's gradient on
    the same values rounded once; the total is within n * 2^-53 * sum|r| of math.fsum of the f32 per_row values; two
    calls give the same bytes."""
    from lidal_amd import semi
    for dtype in ('f32', 'bf16'):
        zs, zt = consistency_case(n, c, dtype)
        for kind in R.KINDS:
            for mc in (0.0, masking_conf(zt)):
                ref_loss, ref_dz, mask = restated(zs, zt, kind, mc, dtype, np.float64)
                (loss, rows), dz = _run_consistency(zs, zt, kind, mc, dtype, per_row=True)
                assert loss.dtype == torch.float32 and dz.dtype == (torch.bfloat16 if dtype == 'bf16' else torch.float32)
                got_dz = dz.float().cpu().numpy().astype(np.float64)
                scale_l, scale_d = abs(ref_loss), np.abs(ref_dz).max()
                out2, _ = semi.consistency_forward(_g(zs).to(dz.dtype), _g(zt), kind, mc)
                e_loss = abs(float(out2[0]) - ref_loss) / scale_l if scale_l else abs(float(out2[0]))
                e_dz = np.abs(got_dz - ref_dz).max() / scale_d if scale_d else np.abs(got_dz).max()
                print('consistency n=%d c=%d %s %s min_conf=%.4f: loss %.3e dz %.3e' % (n, c, dtype, kind, mc, e_loss, e_dz))
                assert e_loss <= SLACK * CPU_LOSS[dtype], (dtype, kind, mc, e_loss)
                assert e_dz <= SLACK * CPU_DZ[dtype], (dtype, kind, mc, e_dz)
                assert abs(float(loss.detach()) - float(out2[0])) <= 2.0 ** -23 * abs(float(out2[0]))     # the f32 the caller gets
                r = rows.cpu().numpy()
                assert not got_dz[~mask].any() and not r[~mask].any()
                total = math.fsum(float(v) for v in r)
                assert abs(float(out2[1]) - total) <= n * 2.0 ** -53 * math.fsum(abs(float(v)) for v in r)
                if dtype == 'bf16':
                    _, dz32 = _run_consistency(zs, zt, kind, mc, 'f32')
                    assert np.array_equal(_bits(R.bf16_round(dz32.cpu().numpy())), _bits(dz.float().cpu().numpy()))
                (loss_b, rows_b), dz_b = _run_consistency(zs, zt, kind, mc, dtype, per_row=True)
                assert torch.equal(loss, loss_b) and torch.equal(rows, rows_b)
                assert np.array_equal(dz.view(torch.int16 if dtype == 'bf16' else torch.int32).cpu().numpy(),
                                      dz_b.view(torch.int16 if dtype == 'bf16' else torch.int32).cpu().numpy())


@pytest.mark.parametrize('kind', R.KINDS)
@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_identical_rows_cost_nothing(kind, dtype):
    for n, c in ((1, 1), (257, 19), (4099, 32)):
        z = R.logits_grid(n, c, n + c, dtype)
        (loss, rows), dz = _run_consistency(z, z, kind, 0.0, dtype, per_row=True)
        assert float(loss.detach()) == 0.0 and not rows.any() and not dz.any()


def test_a_bf16_teacher_is_its_f32_values():
    from lidal_amd import semi
    zs, zt = consistency_case(257, 19, 'f32')
    zt = R.bf16_round(zt)
    for kind in R.KINDS:
        a, _ = semi.consistency_forward(_g(zs), _g(zt), kind)
        b, _ = semi.consistency_forward(_g(zs), _g(zt).to(torch.bfloat16), kind)
        c, _ = semi.consistency_forward(_g(R.bf16_round(zs)).to(torch.bfloat16), _g(zt).to(torch.bfloat16), kind)
        d, _ = semi.consistency_forward(_g(R.bf16_round(zs)), _g(zt), kind)
        assert torch.equal(a, b) and torch.equal(c, d)


@pytest.mark.parametrize('c', [1, 16, 19, 32])
@pytest.mark.parametrize('n', [1, 255, 257, 4099])
def test_on_probabilities_everything_equals_the_restatement_bit_for_bit(n, c):
    """probs=True has no expf in it: per_row and the gradient with respect to the student's probabilities equal
    semi_ref bit for bit, masked and not, and the f64 total is within n * 2^-53 * sum|r| of math.fsum(per_row)."""
    from lidal_amd import semi
    rng = np.random.default_rng(n * 40 + c)
    ps = rng.dirichlet(np.ones(c) * 0.3, n).astype(np.float32)
    pt = rng.dirichlet(np.ones(c) * 0.3, n).astype(np.float32)
    if n > 3:
        pt[3] = 0.0                                     # a row whose confidence is 0
    for mc in (0.0, 0.7 if c > 1 else 1.0):
        loss_w, r_w, mask = R.consistency(ps, pt, 'mse', mc, True, np.float32)
        dz_w = R.consistency_grad(ps, pt, 0.37, 'mse', mc, True, np.float32)
        s = _g(ps).requires_grad_(True)
        loss, rows = semi.consistency_loss(s, _g(pt), min_conf=mc, probs=True, per_row=True)
        (loss * 0.37).backward()
        assert np.array_equal(_bits(rows.cpu().numpy()), _bits(r_w))
        assert np.array_equal(_bits(s.grad.cpu().numpy()), _bits(dz_w))
        if c > 1 and n > 3:
            assert not mask.all() or mc == 0.0
        out2, _ = semi.consistency_forward(_g(ps), _g(pt), 'mse', mc, probs=True)
        bound = n * 2.0 ** -53 * math.fsum(abs(float(v)) for v in r_w)
        assert abs(float(out2[1]) - math.fsum(float(v) for v in r_w)) <= bound
        assert abs(float(out2[0]) - loss_w) <= bound / (n * c) + 2.0 ** -52 * abs(loss_w)
        assert float(loss) == float(np.float32(float(out2[0])))


@pytest.mark.parametrize('c', [1, 2, 19, 32])
def test_one_softmax_across_the_units(c):
    """csrc/rows.h holds the one row softmax: P = view_mean_softmax of one view through the identity (score.hip) is the
    softmax pseudo_labels and the consistency term (semi.hip) take of the same logits.  So conf is P.max(1) bit for bit
    and the accepted labels are pred; and the 'mse' term on logits equals the one on P(zs), P(zt) bit for bit in out2 and
    per_row, unmasked and under a min_conf that masks some rows."""
    from lidal_amd import semi
    from lidal_amd.score.prob_inference import view_mean_softmax
    n = 257
    zs, zt = (_g(z) for z in consistency_case(n, c, 'f32'))
    ident = torch.arange(n, device=DEV)
    (ps, _), (pt, pred) = view_mean_softmax(zs, ident, 1), view_mean_softmax(zt, ident, 1)
    top = pt.max(1).values
    thr = float(top.median()) if c > 1 else 1.0
    labels, stats, conf = semi.pseudo_labels(zt, thr, return_conf=True)
    assert torch.equal(conf.view(torch.int32), top.view(torch.int32))
    took = labels != 255
    assert int(took.sum()) == int(stats[:c].sum()) > 0 and torch.equal(labels[took], pred[took])
    if c > 1:
        assert int(stats[c]) > 0                        # and some were rejected
    for mc in (0.0, thr if c > 1 else 2.0):
        a2, a_rows = semi.consistency_forward(zs, zt, 'mse', mc, probs=False, per_row=True)
        b2, b_rows = semi.consistency_forward(ps, pt, 'mse', mc, probs=True, per_row=True)
        assert torch.equal(a2.view(torch.int64), b2.view(torch.int64))
        assert torch.equal(a_rows.view(torch.int32), b_rows.view(torch.int32))
        assert mc == 0.0 or int((top < mc).sum()) > 0


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_consistency_operands_off_the_16_byte_grid_give_the_same_bits(dtype):
    """`x[1:]` of a [258, 19] matrix starts 76 (f32) or 38 (bf16) bytes into its allocation.  The consistency kernels
    move their rows by elements wherever they start: forward and backward equal those on aligned copies bit for bit,
    both kinds, and the row in front of each view is not touched (tests/test_loss_gpu.py holds the losses to the same)."""
    from lidal_amd import semi
    n, c = 257, 19
    wholes = []
    for z in consistency_case(n, c, 'f32'):
        whole = torch.full((n + 1, c), 7.0, device=DEV).to(dtype)
        whole[1:] = _g(z).to(dtype)
        wholes.append(whole)

    def run(s, t, kind):
        s = s.detach().requires_grad_(True)             # (a leaf on the same storage)
        loss, rows = semi.consistency_loss(s, t, kind=kind, per_row=True)
        (loss * 1.5).backward()
        out2, _ = semi.consistency_forward(s.detach(), t, kind)
        return out2, loss.detach(), rows, s.grad

    for kind in R.KINDS:
        views = [w[1:].detach() for w in wholes]
        assert all(v.data_ptr() % 16 != 0 and v.is_contiguous() for v in views)
        got = run(views[0], views[1], kind)
        want = run(views[0].clone(), views[1].clone(), kind)
        for a, b in zip(got, want):
            assert torch.equal(a, b)
        assert float(want[0][1]) != 0.0 and bool(want[3].any())
    assert all(bool((w[0] == 7.0).all()) for w in wholes)


def test_forward_scratch_is_exactly_what_the_library_says(monkeypatch):
    from lidal_amd import backend as B
    from lidal_amd import semi
    for n, c in ((1, 1), (257, 19), (4099, 32)):
        zs, zt = consistency_case(n, c, 'f32')
        want, _ = semi.consistency_forward(_g(zs), _g(zt), 'kl')
        g = Guarded()
        with monkeypatch.context() as mp:
            mp.setattr(B, 'workspace', g)
            got, _ = semi.consistency_forward(_g(zs), _g(zt), 'kl')
        g.check()
        assert [nb for _, nb in g.bufs] == [B.lib().lidal_consistency_workspace_bytes(n)]
        assert torch.equal(got, want)


def test_no_rows_no_launch():
    from lidal_amd import backend as B
    from lidal_amd import semi
    hits = dict(B.HITS)
    s = torch.zeros((0, 19), device=DEV, requires_grad=True)
    loss = semi.consistency_loss(s, torch.zeros((0, 19), device=DEV))
    loss.backward()
    assert float(loss) == 0.0 and s.grad.shape == (0, 19)
    assert B.HITS.get('consistency_fwd', 0) == hits.get('consistency_fwd', 0)
    assert B.HITS.get('consistency_bwd', 0) == hits.get('consistency_bwd', 0)


# ==================================================================================================== end to end
def _twin_models():
    from lidal_amd.network import MinkUNet
    torch.manual_seed(4)
    a = MinkUNet(19).to(DEV).train()
    b = MinkUNet(19).to(DEV).train()
    b.load_state_dict(a.state_dict())
    return a, b


def test_without_consistency_the_student_trains_as_train_step_does():
    """semi_train_step(cons_weight=0): the student's parameters are torch.equal to a twin's trained by train_step, over
    two steps, and the teacher is the restated EMA of the new weights."""
    from lidal_amd import semi
    from lidal_amd.optim import Adam
    from lidal_amd.train_step import train_step
    c, f, lab = _batch(11)
    student, twin = _twin_models()
    opt_s, opt_t = Adam(student.parameters(), lr=1e-2), Adam(twin.parameters(), lr=1e-2)
    ema = semi.EmaTeacher(student, alpha=0.9, warmup=False)
    for step in range(2):
        before = {k: v.detach().cpu().numpy().copy() for k, v in ema.model.named_parameters()}
        loss_t, logits_t = train_step(twin, opt_t, f, c, lab)
        loss_s, logits_s, cons = semi.semi_train_step(student, ema, opt_s, f, c, lab, cons_weight=0)
        assert torch.equal(loss_s, loss_t) and torch.equal(logits_s, logits_t) and float(cons) == 0.0
        for (k, p), q in zip(student.named_parameters(), twin.parameters()):
            assert torch.equal(p, q), (step, k)
            assert _same_f32(dict(ema.model.named_parameters())[k].cpu().numpy(),
                             R.ema_update(before[k], p.detach().cpu().numpy(), 0.9)), (step, k)
        for (k, b), q in zip(student.named_buffers(), twin.buffers()):
            assert torch.equal(b, q) and torch.equal(dict(ema.model.named_buffers())[k], b), (step, k)
    assert ema.launches == 2 and ema.table_uploads == 1


@pytest.mark.parametrize('kind', R.KINDS)
def test_the_mean_teacher_step_trains_and_a_fresh_teacher_agrees_exactly(kind):
    """cons_weight = 1: teacher and student run on the same SparseTensor, the loss is finite, the parameters move and the
    teacher follows.  A freshly copied teacher and the student in eval-mode BatchNorm give the same logits byte for byte,
    so their consistency is exactly 0 -- both kinds."""
    import lidal_amd
    from lidal_amd import semi
    c, f, lab = _batch(12)
    student, _ = _twin_models()
    opt = torch.optim.Adam(student.parameters(), lr=1e-3)
    ema = semi.EmaTeacher(student, alpha=0.99)
    student.eval()
    with torch.no_grad():
        x = lidal_amd.SparseTensor(f, c)
        zs, zt = student(x)[0], ema.model(x)[0]
    assert torch.equal(zs, zt)
    assert float(semi.consistency_loss(zs, zt, kind=kind)) == 0.0
    student.train()
    w0 = student.classifier[0].weight.detach().clone()
    for step in range(2):
        loss, logits, cons = semi.semi_train_step(student, ema, opt, f, c, lab, cons_weight=1.0, kind=kind)
        assert math.isfinite(float(loss)) and math.isfinite(float(cons)) and float(cons) >= 0.0
        assert logits.shape == (c.shape[0], 19) and not logits.requires_grad
    assert float(cons) > 0.0                            # batch statistics against running ones, and a teacher one step behind
    assert not torch.equal(student.classifier[0].weight, w0) and ema.updates == 2
    assert torch.isfinite(ema.model.classifier[0].weight).all()


def test_pseudo_labels_travel_through_the_mix():
    """pseudo_labels(labels=human) fed into mix_scans(labels=...): every mixed row carries labels[src]."""
    from lidal_amd import data, semi
    rng = np.random.default_rng(8)
    pts, inten, labs = [], [], []
    for n in (3000, 2500):
        xyz = (rng.normal(size=(n, 3)) * [20.0, 20.0, 2.0]).astype(np.float32)
        logits = R.logits_grid(n, 19, n)
        human = np.where(rng.random(n) < 0.05, rng.integers(0, 19, n), 255).astype(np.int64)
        out, stats = semi.pseudo_labels(_g(logits), 0.9, labels=_g(human))
        assert int(stats[:19].sum()) > 0 and int(stats[19]) > 0
        pts.append(_g(xyz)); inten.append(_g(rng.uniform(0, 1, n).astype(np.float32))); labs.append(out)
    mixes = list(data.draw_lasermix(0, 1, np.random.RandomState(0))) + list(data.draw_polarmix(0, 1, np.random.RandomState(1)))
    mixed = data.mix_scans(pts, inten, labs, mixes)
    assert mixed['labels'].shape[0] == 2 * 5500
    assert torch.equal(mixed['labels'], torch.cat(labs)[mixed['src']])
