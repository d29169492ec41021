"""Mixed samples without a GPU: the properties of the numpy restatement tests/mix_ref.py, what its
predicates mean against f64 angles, the host checks of data.mix_scans -- which run before anything touches the device
-- and the order in which the draw functions consume their generator."""
import math

import numpy as np
import pytest
import torch

import mix_ref as R


@pytest.fixture(scope='module')
def scan():
    """A 16-beam x 128-azimuth raycast scan (about 2 000 points)."""
    from lidal_amd import synth
    pts, inten = synth.raycast_scan(synth.make_world(3), (20.0, 0.0), np.random.default_rng(3), n_beams=16, n_az=128)
    assert 1500 <= len(pts) <= 2048
    return pts, inten


@pytest.fixture(scope='module')
def pair(scan):
    """Two scans laid end to end, with labels: (xyz, intensity, labels, point_ptr)."""
    from lidal_amd import synth
    pts_b, inten_b = synth.raycast_scan(synth.make_world(3), (31.0, 1.0), np.random.default_rng(4), n_beams=16, n_az=96)
    xyz = np.concatenate([scan[0], pts_b])
    labels = np.random.default_rng(5).choice([0, 3, 7, 18, 255], len(xyz)).astype(np.int64)
    return xyz, np.concatenate([scan[1], inten_b]), labels, np.array([0, len(scan[0]), len(xyz)], dtype=np.int64)


def _rows_once(outs, n):
    src = np.concatenate([o['src'] for o in outs])
    return len(src) == n and np.array_equal(np.sort(src), np.arange(n))


def _ascending_inside_parts(out):
    for m in range(len(out['parts'])):
        at = int(out['point_ptr'][m])
        for c in out['parts'][m]:
            if (np.diff(out['src'][at:at + c]) <= 0).any():
                return False
            at += int(c)
        if at != out['point_ptr'][m + 1]:
            return False
    return True


# ---- 1. the restatement's properties ------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed', [0, 1, 2, 3])
def test_lasermix_twins_hold_every_row_once(pair, seed):
    from lidal_amd import data
    twins = data.draw_lasermix(0, 1, np.random.RandomState(seed))
    out = R.mix_scans(*pair, twins)
    assert _rows_once([out], len(pair[0])) and _ascending_inside_parts(out)
    assert (out['parts'][:, :2] > 0).all() and (out['parts'][:, 2:] == 0).all()       # both scans in both twins
    assert np.array_equal(out['points'], pair[0][out['src']]) and np.array_equal(out['labels'], pair[2][out['src']])
    assert np.array_equal(out['intensity'], pair[1][out['src']])


@pytest.mark.parametrize('seed', [0, 1, 2, 3])
def test_polarmix_twins_without_paste_hold_every_row_once(pair, seed):
    from lidal_amd import data
    twins = data.draw_polarmix(0, 1, np.random.RandomState(seed))
    out = R.mix_scans(*pair, twins)
    assert _rows_once([out], len(pair[0])) and _ascending_inside_parts(out)
    assert (out['parts'][:, :2] > 0).all() and (out['parts'][:, 2:] == 0).all()
    assert np.array_equal(out['points'], pair[0][out['src']])


def test_polarmix_paste_adds_rotated_rows_of_the_chosen_classes(pair):
    from lidal_amd import data
    xyz, _, labels, ptr = pair
    m1, m2 = data.draw_polarmix(0, 1, np.random.RandomState(7), paste_classes=(3, 18), n_rot=3)
    out = R.mix_scans(*pair, [m1, m2])
    assert _ascending_inside_parts(out)
    for m, mix in enumerate((m1, m2)):
        rows = np.arange(ptr[mix.b], ptr[mix.b + 1])
        want = rows[np.isin(labels[rows], (3, 18))]
        at = int(out['point_ptr'][m] + out['parts'][m, :2].sum())
        assert list(out['parts'][m, 2:]) == [len(want)] * 3 + [0] and len(want) > 0
        for k in range(3):
            sl = slice(at + k * len(want), at + (k + 1) * len(want))
            assert np.array_equal(out['src'][sl], want) and np.array_equal(out['labels'][sl], labels[want])
            p, q = xyz[want].astype(np.float64), out['points'][sl].astype(np.float64)
            ang = np.arctan2(q[:, 1], q[:, 0]) - np.arctan2(p[:, 1], p[:, 0])
            c, s = mix.paste_rot[k].astype(np.float64)
            assert np.allclose(np.mod(ang - math.atan2(s, c) + math.pi, 2 * math.pi) - math.pi, 0.0, atol=1e-5)
            assert np.array_equal(q[:, 2], p[:, 2]) and np.allclose(np.hypot(q[:, 0], q[:, 1]), np.hypot(p[:, 0], p[:, 1]), rtol=1e-6)


def test_identity_mix_returns_the_scan_unchanged(pair):
    from lidal_amd import data
    xyz, inten, labels, ptr = pair
    out = R.mix_scans(xyz, inten, labels, ptr, [data.identity_mix(1), data.identity_mix(0)])
    n0, n1 = int(ptr[1]), int(ptr[2] - ptr[1])
    assert list(out['point_ptr']) == [0, n1, n1 + n0]
    assert np.array_equal(out['src'], np.concatenate([np.arange(n0, n0 + n1), np.arange(n0)]))
    assert np.array_equal(out['points'].view(np.uint32), xyz[out['src']].view(np.uint32))
    assert np.array_equal(out['labels'], labels[out['src']])
    assert np.array_equal(out['parts'], [[n1, 0, 0, 0, 0, 0], [n0, 0, 0, 0, 0, 0]])


# ---- 2. the predicates mean what they say ---------------------------------------------------------------------------------
@pytest.mark.parametrize('n_bounds', [1, 3, 5, 6, 31])
def test_band_equals_the_f64_pitch_band(scan, n_bounds):
    from lidal_amd import data
    pts = scan[0]
    mix = data.draw_lasermix(0, 0, np.random.RandomState(0), areas=(n_bounds + 1,))[0]
    assert len(mix.tans) == n_bounds and mix.tans.dtype == np.float32
    bounds = np.deg2rad(-25.0 + 28.0 * np.arange(1, n_bounds + 1, dtype=np.float64) / (n_bounds + 1))
    p = pts.astype(np.float64)
    pitch = np.arctan2(p[:, 2], np.hypot(p[:, 0], p[:, 1]))
    near = (np.abs(pitch[:, None] - bounds[None, :]) < 1e-6).any(axis=1)
    print('boundaries %d: %d of %d points within 1e-6 rad of one' % (n_bounds, near.sum(), len(pts)))
    assert near.sum() <= 0.01 * len(pts)
    want = (pitch[:, None] >= bounds[None, :]).sum(axis=1)
    band = R.cells(pts, mix.tans, None)[0]
    assert np.array_equal(band[~near], want[~near])
    assert band.min() == 0 and band.max() >= n_bounds - 1                # the beams reach the lowest and the highest areas


@pytest.mark.parametrize('alpha,width', [(0.3, math.pi), (2.0, 1.0), (5.5, 2.5)])
def test_sector_equals_the_f64_azimuth_test(scan, alpha, width):
    from lidal_amd import data
    pts = scan[0]
    p = pts.astype(np.float64)
    rel = np.mod(np.arctan2(p[:, 1], p[:, 0]) - alpha, 2 * math.pi)            # in [0, 2 pi)
    near = (np.minimum(rel, 2 * math.pi - rel) < 1e-5) | (np.abs(rel - width) < 1e-5)
    print('sector (%g, %g): %d of %d points within 1e-5 rad of an edge' % (alpha, width, near.sum(), len(pts)))
    assert near.sum() <= 0.01 * len(pts)
    inw = R.cells(pts, (), data.wedge_vectors(alpha, width))[1]
    assert np.array_equal(inw[~near], (rel < width)[~near])
    assert 0 < inw.sum() < len(pts)


def test_cells_combine_band_and_sector(scan):
    from lidal_amd import data
    tans = data.draw_lasermix(0, 0, np.random.RandomState(0), areas=(4,))[0].tans
    band, inw, cell = R.cells(scan[0], tans, data.wedge_vectors(1.0, 2.0))
    assert np.array_equal(cell, band + 4 * inw) and cell.max() == 7 and cell.min() == 0


# ---- 3. every refusal is raised with no device present ----------------------------------------------------------------------
def test_new_names_are_exported():
    from lidal_amd import data
    for name in ('Mix', 'identity_mix', 'draw_lasermix', 'draw_polarmix', 'mix_scans', 'mixed_train_batch'):
        assert name in data.__all__ and callable(getattr(data, name)), name


def test_mix_scans_checks_its_arguments_before_the_device():
    """CPU tensors throughout: every refusal below is a ValueError, raised before require_gpu could object."""
    from lidal_amd import data
    Mix = data.Mix
    pts, inten, lab = torch.zeros(5, 3), torch.zeros(5), torch.zeros(5, dtype=torch.int64)
    big, big_i = torch.zeros(1, 3).expand(2 ** 28, 3), torch.zeros(1).expand(2 ** 28)
    rot = [(1.0, 0.0)]
    cases = {
        'no mixes': [],
        'too many': [data.identity_mix(0)] * 33,
        'scan a': [Mix(2, 0, take_a=1)],
        'scan b': [Mix(0, -1, take_a=1)],
        '32 tangents': [Mix(0, 1, tans=np.arange(32))],
        'descending': [Mix(0, 1, tans=[0.1, 0.0])],
        'nan tangent': [Mix(0, 1, tans=[0.0, float('nan')])],
        'inf tangent': [Mix(0, 1, tans=[0.0, float('inf')])],
        'nan wedge': [Mix(0, 1, wedge=(1.0, 0.0, float('nan'), 0.0))],
        'inf wedge': [Mix(0, 1, wedge=(float('inf'), 0.0, -1.0, 0.0))],
        'short wedge': [Mix(0, 1, wedge=(1.0, 0.0))],
        'bit above one cell': [Mix(0, 1, take_a=0b10)],
        'bit above four cells': [Mix(0, 1, tans=[0.0], wedge=(1.0, 0.0, -1.0, 0.0), take_b=1 << 4)],
        'negative mask': [Mix(0, 1, take_a=-1)],
        'five rotations': [Mix(0, 1, take_a=1, paste_classes=1, paste_rot=rot * 5)],
    }
    for name, mixes in cases.items():
        with pytest.raises(ValueError, match='mix_scans'):
            data.mix_scans([pts, pts], [inten, inten], [lab, lab], mixes)
    with pytest.raises(ValueError, match='paste needs labels'):
        data.mix_scans([pts, pts], [inten, inten], None, [Mix(0, 1, take_a=1, paste_classes=1, paste_rot=rot)])
    with pytest.raises(ValueError, match='slots'):                        # 2 * 2^28 * (1 + 1): 2^30 slots
        data.mix_scans([big, big], [big_i, big_i], None, [Mix(0, 1, take_a=1), Mix(1, 0, take_a=1)])
    with pytest.raises(ValueError, match='mix_scans'):
        data.mix_scans([pts, pts], [inten], None, [data.identity_mix(0)])
    with pytest.raises(ValueError, match='mix_scans'):
        data.mix_scans([torch.zeros(5, 4)], [inten], None, [data.identity_mix(0)])
    with pytest.raises(ValueError, match='mix_scans'):
        data.mix_scans([pts], [inten], [torch.zeros(4, dtype=torch.int64)], [data.identity_mix(0)])
    ok = [Mix(0, 1, tans=np.linspace(-0.4, 0.05, 31), wedge=(1.0, 0.0, -1.0, 0.0), take_a=2 ** 64 - 1, take_b=1 << 63,
              paste_classes=2 ** 64 - 1, paste_rot=rot * 4)] * 32
    with pytest.raises(RuntimeError, match='GPU only'):                   # well-formed arguments reach the device check
        data.mix_scans([pts, pts], [inten, inten], [lab, lab], ok)
    with pytest.raises(ValueError, match='mix_scans'):                    # ... and mixed_train_batch refuses as early
        data.mixed_train_batch([(pts, inten)], [lab], data.sk_label_map(), [Mix(0, 1, take_a=1)])
    with pytest.raises(ValueError, match='mixed_train_batch'):
        data.mixed_train_batch([(pts, inten)], [lab, lab], data.sk_label_map(), [data.identity_mix(0)])


def test_descriptor_matches_the_header():
    """The packed record is the header's lidal_mix_desc: 256 bytes, fields in the header's order."""
    import os
    import re
    from lidal_amd import data
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'include', 'lidal_amd.h')).read()
    body = re.search(r'typedef struct lidal_mix_desc \{(.*?)\} lidal_mix_desc;', header, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    names = [n for decl in body.split(';') for n in re.findall(r'(\w+)(?:\[[^\]]*\])?\s*(?:,|$)', decl.strip())]
    assert names == list(data._MIX_DESC.names) and data._MIX_DESC.itemsize == 256
    assert (data.MAX_MIXES, data.MAX_MIX_TANS, data.MAX_MIX_ROT) == tuple(
        int(re.search(r'#define %s (\d+)' % k, header).group(1)) for k in ('LIDAL_MIX_MAX', 'LIDAL_MIX_MAX_TANS', 'LIDAL_MIX_MAX_ROT'))
    desc, slots, ptr = data._mix_arguments([5, 7], [data.Mix(1, 0, tans=[0.5], take_a=3, take_b=1, paste_classes=8,
                                                             paste_rot=[(0.0, 1.0), (1.0, 0.0)])], True)
    d = desc[0]
    assert (d['a0'], d['na'], d['b0'], d['nb'], d['n_tans'], d['has_wedge'], d['n_rot']) == (5, 7, 0, 5, 1, 0, 2)
    assert slots == 7 + 5 * 3 and list(ptr) == [0, 5, 12] and list(d['rot'][:4]) == [0.0, 1.0, 1.0, 0.0]


# ---- 4. the draws ---------------------------------------------------------------------------------------------------------
class _Recorder:
    """A RandomState that notes which of its methods were called, in order."""

    def __init__(self, seed):
        self.rs, self.calls = np.random.RandomState(seed), []

    def randint(self, *a, **k):
        self.calls.append('randint')
        return self.rs.randint(*a, **k)

    def rand(self, *a, **k):
        self.calls.append('rand')
        return self.rs.rand(*a, **k)


def test_draws_consume_the_generator_in_the_documented_order():
    from lidal_amd import data
    rec = _Recorder(11)
    m1, m2 = data.draw_lasermix(0, 1, rec)
    assert rec.calls == ['randint']
    n = (3, 4, 5, 6)[np.random.RandomState(11).randint(4)]
    assert len(m1.tans) == n - 1 and np.array_equal(m1.tans, m2.tans)
    want = np.tan(np.deg2rad(-25.0 + 28.0 * np.arange(1, n) / n)).astype(np.float32)
    assert np.array_equal(m1.tans, want) and (np.diff(m1.tans) > 0).all()
    assert (m1.a, m1.b, m2.a, m2.b) == (0, 1, 0, 1)
    assert m1.take_a == m2.take_b == sum(1 << c for c in range(0, n, 2))
    assert m1.take_b == m2.take_a == sum(1 << c for c in range(1, n, 2))
    assert m1.take_a ^ m1.take_b == 2 ** n - 1 and m1.wedge is None and len(m1.paste_rot) == 0

    rec = _Recorder(12)
    p1, p2 = data.draw_polarmix(0, 1, rec)
    assert rec.calls == ['rand']
    alpha = 2.0 * math.pi * np.random.RandomState(12).rand()
    assert np.array_equal(p1.wedge, data.wedge_vectors(alpha, math.pi)) and np.array_equal(p1.wedge, p2.wedge)
    assert (p1.a, p1.b, p2.a, p2.b) == (0, 1, 1, 0) and (p1.take_a, p1.take_b) == (p2.take_a, p2.take_b) == (1, 2)
    assert p1.paste_classes == 0 and len(p1.paste_rot) == 0

    rec = _Recorder(12)
    q1, q2 = data.draw_polarmix(0, 1, rec, paste_classes=(1, 6, 7), n_rot=3)
    assert rec.calls == ['rand'] * 4
    rs = np.random.RandomState(12)
    u = [rs.rand() for _ in range(4)]
    assert np.array_equal(q1.wedge, p1.wedge) and q1.paste_classes == q2.paste_classes == 0b11000010
    ang = [(k + u[1 + k]) * 2.0 * math.pi / 3 for k in range(3)]
    assert np.array_equal(q1.paste_rot, np.array([[math.cos(a), math.sin(a)] for a in ang]).astype(np.float32))
    assert np.array_equal(q1.paste_rot, q2.paste_rot) and (q2.a, q2.b) == (1, 0)

    # the same seed, the same mixes; the numpy module serves as the generator too
    assert data.draw_lasermix(0, 1, np.random.RandomState(5)) == data.draw_lasermix(0, 1, np.random.RandomState(5))
    assert data.draw_polarmix(2, 3, np.random.RandomState(5), (4,)) == data.draw_polarmix(2, 3, np.random.RandomState(5), (4,))
    assert data.draw_polarmix(2, 3, np.random.RandomState(5), (4,)) != data.draw_polarmix(2, 3, np.random.RandomState(6), (4,))
    np.random.seed(5)
    assert data.draw_lasermix(0, 1) == data.draw_lasermix(0, 1, np.random.RandomState(5))
