"""data.mix_scans (lidal_mix_scans: mixed LaserMix / PolarMix style samples in three launches) bit for
bit against the numpy restatement tests/mix_ref.py -- at the block edges, for 1, 2 and 32 mixes, at the ends of every
descriptor field and on coordinates that are zero, negative zero, subnormal when squared, NaN and infinite -- twice with
equal results, in exactly-sized scratch between guards, and composed into mixed_train_batch: equal to train_batch under
identity mixes, and feeding train_step."""
import math

import numpy as np
import pytest
import torch

import mix_ref as R
from guarded_ws import Guarded

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SIZES = (0, 1, 255, 256, 257, 1000)              # around one block of 256 slots, and several blocks
ALL = 2 ** 64 - 1


def _g(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _scans(sizes, seed):
    """Random scans with labels drawn from both sides of every bound of the paste: (xyz, intensity, labels) per scan."""
    rng = np.random.default_rng(seed)
    out = []
    for n in sizes:
        xyz = (rng.normal(size=(n, 3)) * [20.0, 20.0, 2.0]).astype(np.float32)
        lab = rng.choice([-1, 0, 1, 5, 63, 64, 100, 255], n).astype(np.int64)
        out.append((xyz, rng.uniform(0, 1, n).astype(np.float32), lab))
    return out


def _run(scans, mixes, labels=True):
    from lidal_amd import data
    return data.mix_scans([_g(s[0]) for s in scans], [_g(s[1]) for s in scans],
                          [_g(s[2]) for s in scans] if labels else None, mixes)


def _ref(scans, mixes, labels=True):
    ptr = np.concatenate([[0], np.cumsum([len(s[0]) for s in scans])]).astype(np.int64)
    return R.mix_scans(np.concatenate([s[0] for s in scans]), np.concatenate([s[1] for s in scans]),
                       np.concatenate([s[2] for s in scans]) if labels else None, ptr, mixes)


def _same(got, want):
    """Every output, the floats as raw bits."""
    assert got['point_ptr'].dtype == np.int64 and np.array_equal(got['point_ptr'], want['point_ptr'])
    assert got['parts'].dtype == np.int64 and np.array_equal(got['parts'], want['parts'])
    n = int(want['point_ptr'][-1])
    assert got['points'].shape == (n, 3) and got['points'].dtype == torch.float32
    assert np.array_equal(got['points'].cpu().numpy().view(np.uint32), want['points'].view(np.uint32))
    assert np.array_equal(got['intensity'].cpu().numpy().view(np.uint32), want['intensity'].view(np.uint32))
    assert got['src'].dtype == torch.int64 and np.array_equal(got['src'].cpu().numpy(), want['src'])
    if want['labels'] is None:
        assert got['labels'] is None
    else:
        assert got['labels'].dtype == torch.int64 and np.array_equal(got['labels'].cpu().numpy(), want['labels'])


def _equal(a, b):
    for k in ('points', 'intensity', 'labels', 'src'):
        assert torch.equal(a[k].view(torch.int32) if a[k].dtype == torch.float32 else a[k],
                           b[k].view(torch.int32) if b[k].dtype == torch.float32 else b[k]), k
    assert np.array_equal(a['point_ptr'], b['point_ptr']) and np.array_equal(a['parts'], b['parts'])


def _rot(*angles):
    return np.array([[math.cos(a), math.sin(a)] for a in angles]).astype(np.float32)


def _catalogue():
    """32 mixes over the scans of SIZES: the ends of every field of the descriptor."""
    from lidal_amd.data import Mix, identity_mix, wedge_vectors, class_mask, draw_lasermix, draw_polarmix
    t31 = np.tan(np.deg2rad(np.linspace(-60.0, 60.0, 31))).astype(np.float32)
    half = wedge_vectors(0.7, math.pi)
    mixes = [identity_mix(j) for j in range(len(SIZES))]
    mixes += [
        Mix(5, 5, wedge=half, take_a=0b01, take_b=0b10),                                  # A equal to B, a sector of exactly pi
        Mix(5, 4),                                                                        # masks all zero: no rows
        Mix(3, 5, t31, wedge_vectors(5.0, 2.0), ALL, ALL, class_mask((1, 5, 63)), _rot(0.1, 1.7, 3.0, 4.4)),   # 64 cells, 4 pastes
        Mix(2, 3, [0.0], None, 0b11, 0b11, class_mask((40,)), _rot(1.0)),                 # a paste mask that selects nothing
        Mix(0, 5, take_a=1, take_b=1, paste_classes=ALL, paste_rot=_rot(0.5, 2.5, 3.5, 5.5)),   # every class 0..63, no other label
        Mix(1, 0, take_a=1, take_b=1, paste_classes=ALL, paste_rot=_rot(0.3)),            # one row and none
        Mix(0, 1, take_a=1, take_b=1, paste_classes=ALL, paste_rot=_rot(0.3, 0.6)),
        Mix(4, 2, t31, None, 0x55555555, 0xAAAAAAAA),                                     # 31 boundaries without a sector
        Mix(4, 5, [-0.05], wedge_vectors(3.0, 0.5), 0b0110, 0b1001),
        Mix(5, 3, [-0.1, -0.1, 0.2], None, 0b1010, 0b0101, class_mask((0,)), _rot(2.0)),  # two equal boundaries: area 1 is empty
        Mix(2, 4, (), None, 0, 1, class_mask((5, 63)), _rot(0.0, math.pi)),               # nothing of A
        Mix(3, 2, [0.0], half, 0, 0, class_mask((1,)), _rot(4.0)),                        # pastes alone
    ]
    rs = np.random.RandomState(17)
    while len(mixes) < 32:
        a, b = rs.randint(2, 6), rs.randint(2, 6)
        mixes += draw_lasermix(a, b, rs) if len(mixes) % 4 < 2 else draw_polarmix(a, b, rs, (0, 5), n_rot=1 + len(mixes) % 4)
    return mixes[:32]


@pytest.fixture(scope='module')
def scans():
    return _scans(SIZES, 1)


# ---- 1. bit for bit against the restatement ---------------------------------------------------------------------------
def test_thirty_two_mixes_at_the_block_edges(scans):
    from lidal_amd import backend as B
    mixes = _catalogue()
    assert len(mixes) == 32
    before = B.HITS.get('mix_scans', 0)
    got = _run(scans, mixes)
    assert B.HITS['mix_scans'] == before + 1                              # one library call
    want = _ref(scans, mixes)
    _same(got, want)
    parts = want['parts']
    assert list(parts[:6, 0]) == list(SIZES) and not parts[7].any()       # identities; the mix without rows
    assert parts[8, 2] > 0 and (parts[8, 2:] == parts[8, 2]).all()        # four pastes of the same rows
    assert parts[9, 2] == 0 and parts[16, 0] == 0 and parts[17, :2].sum() == 0 and parts[17, 2] > 0
    lab = np.concatenate([s[2] for s in scans])
    at = int(want['point_ptr'][10] + parts[10, :2].sum())
    pasted = lab[want['src'][at:int(want['point_ptr'][11])]]
    assert len(pasted) and set(pasted) == {0, 1, 5, 63}                   # -1, 64, 100 and 255 are never pasted


@pytest.mark.parametrize('case', ['one', 'two', 'one_empty', 'no_rows', 'no_labels'])
def test_one_and_two_mixes(scans, case):
    from lidal_amd import data
    cat = _catalogue()
    labels = True
    if case == 'one':
        mixes = [cat[8]]
    elif case == 'two':
        mixes = list(data.draw_lasermix(4, 5, np.random.RandomState(2)))
    elif case == 'one_empty':
        mixes = [cat[7]]                                                  # blocks, but nothing kept
    elif case == 'no_rows':
        scans, mixes = scans[:1], [data.identity_mix(0), data.Mix(0, 0, take_a=1, take_b=1)]       # no block at all
    else:
        labels, mixes = False, [cat[6], cat[13], cat[14]]
    got = _run(scans, mixes, labels)
    want = _ref(scans, mixes, labels)
    _same(got, want)
    if case in ('one_empty', 'no_rows'):
        assert got['points'].shape[0] == 0 and not got['parts'].any()


def test_edge_values_in_one_scan():
    """The origin, negative zeros, a point on the z axis, NaN, infinities and coordinates whose squares are subnormal take
    the cells IEEE arithmetic gives them.  The non-finite rows carry label 255: rotating them makes NaNs, whose sign and
    payload the definition leaves open."""
    from lidal_amd.data import Mix, wedge_vectors
    nan, inf, z = float('nan'), float('inf'), -0.0
    rows = [(0, 0, 0), (z, z, z), (z, 0, 1), (0, z, -1), (0, 0, 5), (0, 0, -5), (1e-20, 1e-20, 1e-20), (-1e-20, 1e-20, 0),
            (1e-20, z, -1e-21), (3e-23, 0, 1e-23), (1, 0, 0), (0, 1, 0), (-1, 0, z), (0, -1, 0), (1, 1, 1), (-2, 3, -1),
            (nan, 1, 1), (1, nan, 0), (1, 1, nan), (inf, 1, 1), (-inf, 0, 0), (1, 1, inf), (0, 0, -inf), (inf, inf, inf)]
    xyz = np.array(rows, dtype=np.float32)
    lab = np.array([3] * 16 + [255] * 8, dtype=np.int64)
    scan = [(xyz, np.arange(len(rows), dtype=np.float32), lab)]
    tans = np.array([-0.5, 0.0, 0.5], dtype=np.float32)
    axes = np.array([1.0, 0.0, -1.0, 0.0], dtype=np.float32)              # the half plane y >= 0 (and y > 0 by the second test)
    mixes = [Mix(0, 0, tans, axes, 1 << c, ALL & ~(1 << c) & 0xFF) for c in range(8)]
    mixes += [Mix(0, 0, tans, wedge_vectors(0.3, 1.0), 0xFF, 0, 1 << 3, _rot(0.0, 1.0, math.pi / 2, 4.0)),
              Mix(0, 0, tans, None, 0b0101, 0b1010), Mix(0, 0, take_a=1)]
    got = _run(scan, mixes)
    want = _ref(scan, mixes)
    _same(got, want)
    assert (want['parts'][:8, :2].sum(axis=1) == len(rows)).all()         # every row is in exactly one cell
    assert (want['parts'][:8, 0] > 0).sum() >= 4                          # ... and the cells differ
    assert list(want['parts'][8]) == [24, 0, 16, 16, 16, 16]


# ---- 2. determinism, exact scratch ---------------------------------------------------------------------------------------
def test_two_calls_give_equal_outputs(scans):
    mixes = _catalogue()
    a = _run(scans, mixes)
    b = _run(scans, mixes)
    _equal(a, b)


def test_exact_scratch_between_guards(scans, monkeypatch):
    from lidal_amd import backend as B, data
    mixes = _catalogue()
    want = _run(scans, mixes)
    torch.cuda.synchronize()
    g = Guarded()
    monkeypatch.setattr(B, 'workspace', g)
    got = _run(scans, mixes)
    g.check()
    slots = data._mix_arguments([len(s[0]) for s in scans], mixes, True)[1]
    assert [n for _, n in g.bufs] == [B.lib().lidal_mix_scans_workspace_bytes(slots, len(mixes))]
    _equal(got, want)


def test_scratch_one_byte_short_is_refused(scans, monkeypatch):
    from lidal_amd import backend as B
    handle = B.lib_handle()

    class Short:
        def __getattr__(self, name):
            fn = getattr(handle, name)
            return (lambda *a: fn(*a) - 1) if name == 'lidal_mix_scans_workspace_bytes' else fn
    g = Guarded()
    monkeypatch.setattr(B, 'workspace', g)
    monkeypatch.setattr(B, 'lib', lambda: Short())
    with pytest.raises(RuntimeError, match='too small'):
        _run(scans, _catalogue()[:2])
    g.check()


# ---- 3. in front of voxelize_batch ---------------------------------------------------------------------------------------
def _label_inputs(points, seed):
    """Raw SemanticKITTI words, four angular supervoxels with flags 1 / 2 / 0 and pseudo-labels per scan."""
    from lidal_amd import data, synth
    from lidal_amd.score.interframe import sv_csr
    table = data.sk_label_map()
    ids = np.nonzero(table != 255)[0]
    rng = np.random.default_rng(seed)
    raws, csrs, flags, pseudos = [], [], [], []
    for k, pts in enumerate(points):
        p = pts.shape[0]
        raw = (rng.choice(ids, p) | (rng.integers(1, 65536, p) << 16)).astype(np.uint32)
        raws.append(_g(raw.view(np.int32)))
        csrs.append(sv_csr(synth.angular_supervoxels(pts, 4), DEV)[:2])
        flags.append(np.array([[1, 2, 0, 1], [0, 1, 2, 2], [1, 1, 2, 0]][k % 3]))
        pseudos.append(_g(rng.integers(0, 19, p)))
    return table, raws, csrs, flags, pseudos


def _raycast(n_points, seeds):
    from lidal_amd import synth
    world = synth.make_world(5)
    return [synth.raycast_scan(world, (18.0 + 3 * i, 0.0), np.random.default_rng([23, s]), n_beams=16, n_az=128,
                               n_points=n) for i, (n, s) in enumerate(zip(n_points, seeds))]


def test_identity_mixes_give_train_batch():
    from lidal_amd import data
    host = _raycast([500, 700], [0, 1])
    assert [len(h[0]) for h in host] == [500, 700]
    pairs = [(_g(p), _g(w)) for p, w in host]
    table, raws, csrs, flags, pseudos = _label_inputs([h[0] for h in host], 24)
    want = data.train_batch(pairs, raws, table, csrs, flags, pseudos, rng=np.random.RandomState(9))
    got = data.mixed_train_batch(pairs, raws, table, [data.identity_mix(j) for j in range(2)], csrs, flags, pseudos,
                                 rng=np.random.RandomState(9))
    for k in ('coords_v_b', 'feats_v_b', 'labels_v_b', 'inverse_indices_b'):
        assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), k
    assert torch.equal(got['src_p_b'], torch.arange(1200, device=DEV)) and torch.equal(got['src_b'], want['unique_idxs_b'])
    assert len(torch.unique(got['labels_v_b'])) > 2 and bool((got['labels_v_b'] == 255).any())


def test_mixed_batch_feeds_train_step():
    from lidal_amd import data
    from lidal_amd.network import MinkUNet
    from lidal_amd.nn import functional as F
    from lidal_amd.train_step import train_step
    host = _raycast([1500, 1200], [2, 3])
    pairs = [(_g(p), _g(w)) for p, w in host]
    table, raws, csrs, flags, pseudos = _label_inputs([h[0] for h in host], 25)
    rs = np.random.RandomState(4)
    mixes = list(data.draw_lasermix(0, 1, rs)) + list(data.draw_polarmix(0, 1, rs, paste_classes=(1, 6, 7, 17), n_rot=3))
    batch = data.mixed_train_batch(pairs, raws, table, mixes, csrs, flags, pseudos, rng=rs)
    labels_p = [data.train_labels(raws[k], table, csrs[k], flags[k], pseudos[k])[0].cpu().numpy() for k in range(2)]
    ref = R.mix_scans(np.concatenate([h[0] for h in host]), np.concatenate([h[1] for h in host]),
                      np.concatenate(labels_p), np.array([0, 1500, 2700]), mixes)
    assert ref['parts'][2:, 2:5].all() and not ref['parts'][:, 5].any()             # three pastes in each PolarMix twin
    uniq = batch['unique_idxs_b'].cpu().numpy()
    assert np.array_equal(batch['point_ptr'], ref['point_ptr']) and np.array_equal(batch['parts'], ref['parts'])
    assert np.array_equal(batch['labels_v_b'].cpu().numpy(), ref['labels'][uniq])
    assert np.array_equal(batch['src_b'].cpu().numpy(), ref['src'][uniq])
    assert np.array_equal(batch['labels_v_b'].cpu().numpy(), np.concatenate(labels_p)[batch['src_b'].cpu().numpy()])
    assert batch['coords_v_b'].shape[0] == len(uniq) and int(batch['coords_v_b'][:, 3].max()) == 3
    torch.manual_seed(3)
    model = MinkUNet(19).to(DEV).train()
    opt = torch.optim.Adam(model.parameters())
    loss, logits = train_step(model, opt, batch['feats_v_b'], batch['coords_v_b'], batch['labels_v_b'],
                              criterion=F.combined_loss)
    assert logits.shape == (len(uniq), 19) and math.isfinite(loss.item())
