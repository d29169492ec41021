"""Training labels on the GPU (lidal_train_labels): bit-equal to what the REFERENCE's SK_Dataset /
NU_Dataset return (tests/golden/labels_small.npz) through the GPU voxeliser's own unique_idxs, equal to
tests/labels_ref.py at full size and at the edges, input validation without a fault, run-to-run identity, and the
closed loop select -> flags -> train_sample -> collate -> train_step."""
import os

import numpy as np
import pytest
import torch

import labels_ref

pytestmark = pytest.mark.gpu
DEV = 'cuda'
MODES = ('train', 'train_sv', 'train_sv_pseudo')


def _dev(a):
    a = np.asarray(a)
    if a.dtype == np.uint32:                     # the u32 words of a .label file travel as int32 bits
        a = a.view(np.int32)
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _csr(lists):
    from lidal_amd.score.interframe import sv_csr
    return sv_csr(lists, DEV)[:2]


def _run(raw, table, lists=None, flags=None, pseudo=None, unique=None):
    """data.train_labels on host inputs -> numpy outputs."""
    from lidal_amd import data
    lp, lv = data.train_labels(_dev(raw), table, _csr(lists) if lists is not None else None, flags,
                               _dev(pseudo) if pseudo is not None else None, _dev(unique) if unique is not None else None)
    assert lp.dtype == torch.int64 and (lv is None or lv.dtype == torch.int64)
    return lp.cpu().numpy(), None if lv is None else lv.cpu().numpy()


def _equal_ref(raw, table, lists=None, flags=None, pseudo=None, unique=None):
    got = _run(raw, table, lists, flags, pseudo, unique)
    ref = labels_ref.train_labels(raw, table, lists, flags, pseudo, unique)
    assert np.array_equal(got[0], ref[0])
    assert (got[1] is None and ref[1] is None) or np.array_equal(got[1], ref[1])
    return got


def _lists(g, i):
    ptr, idx = g['sv_ptr%d' % i], g['sv_idx%d' % i]
    return [idx[ptr[k]:ptr[k + 1]] for k in range(ptr.shape[0] - 1)]


@pytest.mark.parametrize('ds', ['sk', 'nu'])
def test_train_labels_match_the_reference_datasets(golden_dir, ds):
    """Every mode of SK_Dataset / NU_Dataset.__getitem__, through voxelize_scan's own unique_idxs with the fixture's
    augmentation, and collate_fn's labels_v_b."""
    from lidal_amd import backend as B, data
    g = np.load(os.path.join(golden_dir, 'labels_small.npz'))
    table = _dev(data.sk_label_map() if ds == 'sk' else data.nu_label_map())
    before = B.HITS.get('train_labels', 0)
    for mode in MODES:
        samples = []
        for i in range(2):
            cv, fv, ui, _ = data.voxelize_scan(_dev(g['points%d' % i]), _dev(g['intensity%d' % i]), g['trans_m%d' % i],
                                               g['rnd%d' % i])
            assert np.array_equal(ui.cpu().numpy(), g['unique%d' % i])
            sv = 'train_sv' in mode
            lp, lv = data.train_labels(_dev(g['%s_raw%d' % (ds, i)]), table, _csr(_lists(g, i)) if sv else None,
                                       g['sv_flag%d' % i] if sv else None,            # scan 1: a bool file of round 0
                                       _dev(g['%s_pseudo%d' % (ds, i)]) if 'pseudo' in mode else None, ui)
            assert np.array_equal(lv.cpu().numpy(), g['%s_%s_labels_v%d' % (ds, mode, i)]), (mode, i)
            if mode == 'train':
                assert np.array_equal(lp.cpu().numpy(), g['%s_val_labels_p%d' % (ds, i)])
            samples.append({'coords_v': cv, 'feats_v': fv, 'labels_v': lv})
        col = data.collate(samples)
        assert col['labels_v_b'].dtype == torch.int64 and col['labels_v_b'].shape[0] == col['coords_v_b'].shape[0]
        assert np.array_equal(col['labels_v_b'].cpu().numpy(), g['%s_%s_labels_v_b' % (ds, mode)]), mode
    assert B.HITS['train_labels'] == before + 6
    # 'val': per-point labels alone
    lp, lv = data.train_labels(_dev(g['%s_raw0' % ds]), table)
    assert lv is None and np.array_equal(lp.cpu().numpy(), g['%s_val_labels_p0' % ds])


def _full_scan(seed=0):
    from lidal_amd import data, synth
    rng = np.random.default_rng(seed)
    pts, inten = synth.raycast_scan(synth.make_world(3), (30.0, 0.0), rng)
    assert pts.shape[0] > 100000
    trans_m, rnd = data.draw_augmentation(np.random.RandomState(7))
    _, _, ui, _ = data.voxelize_scan(_dev(pts), _dev(inten), trans_m, rnd)
    return pts, rng, ui.cpu().numpy()


@pytest.mark.parametrize('n_sv', [20, 2000])
def test_full_size_scan_equals_the_restatement(n_sv):
    from lidal_amd import data, synth
    pts, rng, unique = _full_scan()
    p = pts.shape[0]
    lists = synth.angular_supervoxels(pts, n_sv)
    lists[1] = np.concatenate([lists[1], lists[2][: len(lists[2]) // 2]])          # overlap
    lists[0] = lists[0][:-11]                                                      # points in no list
    flags = rng.integers(0, 3, n_sv)
    flags[1], flags[2] = 1, 2
    sk_ids = np.nonzero(data.sk_label_map() != 0)[0]
    sk_raw = (rng.choice(sk_ids, p) | (rng.integers(0, 65536, p) << 16)).astype(np.uint32)
    nu_raw = rng.integers(0, 32, p).astype(np.uint8)
    for raw, table, c in ((sk_raw, data.sk_label_map(), 19), (nu_raw, data.nu_label_map(), 16)):
        pseudo = rng.integers(0, c, p)
        for l, f, ps in ((None, None, None), (lists, flags, None), (lists, flags, pseudo)):
            lp, lv = _equal_ref(raw, table, l, f, ps, unique)
            assert lv.shape == unique.shape
        assert (lp != 255).any() and (lp == 255).any()


def test_edges():
    from lidal_amd import data
    rng = np.random.default_rng(5)
    sk, nu = data.sk_label_map(), data.nu_label_map()
    # p == 0, with and without supervoxels
    for raw, table in ((np.zeros(0, np.uint32), sk), (np.zeros(0, np.uint8), nu)):
        lp, lv = _equal_ref(raw, table, unique=np.zeros(0, np.int64))
        assert lp.shape == (0,) and lv.shape == (0,)
        _equal_ref(raw, table, [np.zeros(0, np.int64)] * 3, np.array([1, 2, 0]), np.zeros(0, np.int64))
    # p not a multiple of the vector width (4 words / 16 bytes), and above 2^17; an unaligned raw stream
    for p in (1, 3, 5, 15, 16, 17, 63, 64, 65, 1023, 4099, (1 << 17) + 13):
        order = rng.permutation(p)
        lists = [np.sort(c) for c in np.array_split(order[: p - p // 7], 9)] + [np.zeros(0, np.int64)]   # one empty
        flags = np.array([1, 2, 0, 1, 2, 0, 1, 2, 0, 1])
        unique = np.sort(rng.choice(p, max(1, p // 2), replace=False))
        for raw, table in (((rng.integers(10, 12, p) | (rng.integers(0, 65536, p) << 16)).astype(np.uint32), sk),
                           (rng.integers(0, 32, p).astype(np.uint8), nu)):
            pseudo = rng.integers(0, 16, p)
            _equal_ref(raw, table, unique=unique)
            _equal_ref(raw, table, lists, flags, None, unique)
            lp, _ = _equal_ref(raw, table, lists, flags, pseudo, unique)
            assert (lp[order[p - p // 7:]] == 255).all()                            # in no list: always 255
            # s == 0 and flags all zero: every label 255
            assert (_equal_ref(raw, table, [], np.zeros(0, np.int64), pseudo, unique)[0] == 255).all()
            assert (_equal_ref(raw, table, lists, np.zeros(10, np.int64), pseudo, unique)[1] == 255).all()
            # bool flags (round-0 files), as a host array and as a GPU tensor
            b = flags == 1
            ref = labels_ref.train_labels(raw, table, lists, b, None, unique)
            assert np.array_equal(_run(raw, table, lists, b, None, unique)[1], ref[1])
            assert np.array_equal(_run(raw, table, lists, torch.from_numpy(b).to(DEV), None, unique)[1], ref[1])
            if p > 1:
                tail = _dev(raw)[1:]                                               # contiguous, not 16-byte aligned
                assert tail.data_ptr() % 16 != 0
                got = data.train_labels(tail, _dev(table))[0].cpu().numpy()
                assert np.array_equal(got, labels_ref.train_labels(raw[1:], table)[0])


def test_invalid_ids_raise_and_leave_no_sticky_error():
    """Input validation, not a fault: an id beyond the table (numpy's IndexError in the reference) and indices outside
    their arrays are counted on the device, the wrapper raises, and the next valid call succeeds."""
    from lidal_amd import backend as B, data
    rng = np.random.default_rng(6)
    p = 5000
    nu_raw = rng.integers(0, 32, p).astype(np.uint8)
    sk_raw = rng.integers(10, 12, p).astype(np.uint32) | np.uint32(7 << 16)
    lists = [np.arange(0, 2500), np.arange(2500, p)]
    flags = np.array([1, 2])
    bad_nu, bad_sk = nu_raw.copy(), sk_raw.copy()
    bad_nu[[3, 4000]] = [100, 255]                      # == and > the last entry of the [100] table
    bad_sk[[17]] = 260 | (9 << 16)
    for raw, good, table, n_bad in ((bad_nu, nu_raw, data.nu_label_map(), 2), (bad_sk, sk_raw, data.sk_label_map(), 1)):
        with pytest.raises(IndexError, match='%d raw label ids' % n_bad):
            _run(raw, table, lists, flags)
        lp, _, cnt = data.train_labels(_dev(raw), table, check=False)           # the lazy form: counted, 255, no raise
        assert int(cnt.item()) == n_bad and (lp.cpu().numpy()[(raw.astype(np.int64) & 0xFFFF) >= len(table)] == 255).all()
        with pytest.raises(IndexError):
            data.check_labels([cnt])
        _equal_ref(good, table, lists, flags, rng.integers(0, 16, p), np.arange(0, p, 3))
    # membership and voxel indices outside [0, p): counted and skipped, nothing written out of bounds
    with pytest.raises(IndexError):
        _run(nu_raw, data.nu_label_map(), [np.array([0, 1, p]), np.array([-1, 5])], flags, rng.integers(0, 16, p))
    with pytest.raises(IndexError):
        _run(nu_raw, data.nu_label_map(), unique=np.array([0, p + 3]))
    _equal_ref(nu_raw, data.nu_label_map(), lists, flags, rng.integers(0, 16, p), np.arange(0, p, 3))
    torch.cuda.synchronize()
    # host-side argument errors come back as the library's status, and do not stick either
    with pytest.raises(RuntimeError, match='label table'):
        data.train_labels(_dev(nu_raw), np.zeros(2000, np.int64))
    with pytest.raises(TypeError):
        data.train_labels(_dev(nu_raw.astype(np.int64)), data.nu_label_map())
    with pytest.raises(ValueError):
        data.train_labels(_dev(nu_raw), data.nu_label_map(), _csr(lists), np.array([1, 2, 0]))
    _equal_ref(nu_raw, data.nu_label_map())
    assert B.lib().lidal_last_error() is not None


def test_two_runs_are_bit_identical():
    from lidal_amd import data, synth
    pts, rng, unique = _full_scan(1)
    p = pts.shape[0]
    lists = synth.angular_supervoxels(pts, 200)
    for k in range(0, 198, 3):                                                     # heavy overlap: many ORs per word
        lists[k] = np.concatenate([lists[k], lists[k + 1], lists[k + 2][::2]])
    flags = rng.integers(0, 3, 200)
    raw = _dev(rng.integers(0, 32, p).astype(np.uint8))
    pseudo = _dev(rng.integers(0, 16, p))
    csr, ui, table = _csr(lists), _dev(unique), _dev(data.nu_label_map())
    runs = [data.train_labels(raw, table, csr, flags, pseudo, ui) for _ in range(3)]
    for lp, lv in runs[1:]:
        assert torch.equal(lp, runs[0][0]) and torch.equal(lv, runs[0][1])


def test_the_loop_closes_from_selection_to_a_training_step():
    """score.select's flags -> per-frame flag arrays -> train_sample -> collate -> one train_step on a MinkUNet."""
    from lidal_amd import data, synth
    from lidal_amd.network import MinkUNet
    from lidal_amd.score import select
    from lidal_amd.score.interframe import sv_csr
    from lidal_amd.train_step import train_step
    n_frames, n_sv, n_pts = 5, 20, 3000
    seq = synth.make_sequence(n_frames, n_points=n_pts, seed=4, n_sv=n_sv, n_beams=16, n_az=512)
    rng = np.random.default_rng(8)
    pnums = np.concatenate([[len(l) for l in fr['sv2point']] for fr in seq]).astype(np.int64)
    centers = np.concatenate([[fr['world'][l].mean(0) for l in fr['sv2point']] for fr in seq]).astype(np.float32)
    total = n_frames * n_sv
    flags_in = np.zeros(total, dtype=bool)
    flags_in[:n_sv] = True                                                         # round 0: frame 0 fully labeled
    flags = select(flags_in, rng.random(total).astype(np.float32), rng.random(total).astype(np.float32), pnums, centers,
                   100 * int(pnums.sum()) // 10)                                   # 10 % of the points per pass
    assert (flags == 1).sum() > n_sv and (flags == 2).sum() > 0
    per_frame = [flags[i * n_sv:(i + 1) * n_sv] for i in range(n_frames)]
    keep = data.labeled_frames(per_frame)
    assert 0 in keep and len(keep) >= 2
    table = _dev(data.sk_label_map())
    ids = np.nonzero((data.sk_label_map() != 255) & (data.sk_label_map() != 0))[0]          # annotated, kept classes

    def batch(frame_flags, seed):
        samples, expect = [], 0
        for i in keep:
            fr = seq[i]
            p = fr['points'].shape[0]
            r = np.random.default_rng([seed, i])
            raw = (r.choice(ids, p) | (r.integers(1, 65536, p) << 16)).astype(np.uint32)
            pseudo = r.integers(0, 19, p)
            s = data.train_sample(_dev(fr['points']), _dev(fr['intensity']), _dev(raw), table, sv_csr(fr['sv2point'], DEV),
                                  frame_flags[i], _dev(pseudo), rng=np.random.RandomState(1000 * seed + i))
            assert set(s) == {'coords_v', 'feats_v', 'labels_v'} and s['labels_v'].shape[0] == s['coords_v'].shape[0]
            # what the restatement predicts for these voxels: the same draws, the voxeliser's own unique_idxs
            trans_m, rnd = data.draw_augmentation(np.random.RandomState(1000 * seed + i))
            ui = data.voxelize_scan(_dev(fr['points']), _dev(fr['intensity']), trans_m, rnd)[2].cpu().numpy()
            ref_v = labels_ref.train_labels(raw, data.sk_label_map(), fr['sv2point'], frame_flags[i], pseudo, ui)[1]
            assert np.array_equal(s['labels_v'].cpu().numpy(), ref_v)
            expect += int((ref_v != 255).sum())
            samples.append(s)
        return data.collate(samples), expect

    col, expect = batch(per_frame, 31)
    assert int((col['labels_v_b'] != 255).sum()) == expect and expect > 0
    assert int(col['coords_v_b'][:, 3].max()) == len(keep) - 1
    torch.manual_seed(2)
    model = MinkUNet(19).to(DEV).train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    loss, logits = train_step(model, opt, col['feats_v_b'], col['coords_v_b'], col['labels_v_b'])
    torch.cuda.synchronize()
    assert np.isfinite(loss.item()) and logits.shape == (col['coords_v_b'].shape[0], 19)
    # a round with nothing selected: every label is 255
    col0, expect0 = batch([np.zeros(n_sv, dtype=np.int64)] * n_frames, 32)
    assert expect0 == 0 and col0['labels_v_b'].shape[0] > 0 and bool((col0['labels_v_b'] == 255).all())
