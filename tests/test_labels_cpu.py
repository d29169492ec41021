"""Host side of the training labels, no GPU: tests/labels_ref.py and the package's label tables
against the fixture the REFERENCE's SK_Dataset / NU_Dataset produced (tests/golden/labels_small.npz, written by
make_golden_labels.py), the frame filters of the loaders, the file readers, and the refusal of CPU tensors."""
import os

import numpy as np
import pytest
import torch

import labels_ref

MODES = ('train', 'train_sv', 'train_sv_pseudo')


def _lists(g, i):
    ptr, idx = g['sv_ptr%d' % i], g['sv_idx%d' % i]
    return [idx[ptr[k]:ptr[k + 1]] for k in range(ptr.shape[0] - 1)]


def ref_labels(g, ds, mode, i):
    """labels_ref on scan i of the fixture in one of the reference's modes."""
    sv = 'train_sv' in mode
    return labels_ref.train_labels(g['%s_raw%d' % (ds, i)], g['%s_label_map' % ds], _lists(g, i) if sv else None,
                                   g['sv_flag%d' % i] if sv else None,
                                   g['%s_pseudo%d' % (ds, i)] if 'pseudo' in mode else None, g['unique%d' % i])


def test_fixture_covers_what_it_claims(golden_dir):
    g = np.load(os.path.join(golden_dir, 'labels_small.npz'))
    assert g['sk_raw0'].dtype == np.uint32 and g['nu_raw0'].dtype == np.uint8
    assert (g['sk_raw0'] >> 16).min() > 0                                   # instance ids in the high half
    ids = set((g['sk_raw0'] & 0xFFFF).tolist())
    assert {2, 100} < ids and len(ids) == 36 and max(ids) < 260              # the 34 named ids + two absent ones
    assert set(g['nu_raw0'].tolist()) == set(range(32)) | {50}
    assert set(g['sv_flag0'].tolist()) == {0, 1, 2} and g['sv_flag1'].dtype == bool
    for i in range(2):
        lists = _lists(g, i)
        p = g['points%d' % i].shape[0]
        covered = np.zeros(p, int)
        for l in lists:
            covered[l] += 1
        assert (covered == 0).sum() == 7 and (covered == 2).sum() == 100 and len(lists[-1]) == 0
    assert g['sk_label_map'].dtype == np.float64 and g['sk_label_map'].shape == (260,)
    assert g['sk_label_map'][2] == 0 and g['sk_label_map'][252] == g['sk_label_map'][10] == 0


@pytest.mark.parametrize('ds', ['sk', 'nu'])
def test_labels_ref_equals_the_reference_datasets(golden_dir, ds):
    g = np.load(os.path.join(golden_dir, 'labels_small.npz'))
    for mode in MODES:
        per_scan = []
        for i in range(2):
            labels_p, labels_v = ref_labels(g, ds, mode, i)
            assert labels_v.dtype == np.int64
            assert np.array_equal(labels_v, g['%s_%s_labels_v%d' % (ds, mode, i)]), (ds, mode, i)
            if mode == 'train':
                assert np.array_equal(labels_p, g['%s_val_labels_p%d' % (ds, i)])
            per_scan.append(labels_v)
        assert np.array_equal(np.concatenate(per_scan), g['%s_%s_labels_v_b' % (ds, mode)])
    # the modes differ on this fixture: the mask removes labels, the pseudo labels bring some back
    kept = [int((g['%s_%s_labels_v_b' % (ds, m)] != 255).sum()) for m in MODES]
    assert kept[0] > kept[2] > kept[1] > 0


def test_label_maps_equal_the_reference_tables(golden_dir):
    from lidal_amd import data
    g = np.load(os.path.join(golden_dir, 'labels_small.npz'))
    sk, nu = data.sk_label_map(), data.nu_label_map()
    assert sk.dtype == np.int64 and sk.shape == (260,) and nu.dtype == np.int64 and nu.shape == (100,)
    assert np.array_equal(sk, g['sk_label_map']) and np.array_equal(nu, g['nu_label_map'])
    assert sk[2] == 0 and sk[0] == 255 and sorted(set(sk.tolist())) == list(range(19)) + [255]
    assert sorted(set(nu.tolist())) == list(range(16)) + [255]


def test_frame_filters():
    from lidal_amd import data
    flags = [np.zeros(4, dtype=bool), np.array([0, 1, 0]), np.array([0, 2, 0]), np.zeros(0, dtype=np.int64),
             np.ones(3, dtype=bool), np.array([0, 0])]
    kept = data.labeled_frames(flags)
    assert kept.dtype == np.int64 and kept.tolist() == [1, 2, 4]            # a flag-2-only frame counts
    assert data.labeled_frames([]).tolist() == []
    # sk_dataloader.py:160-172: per-sequence files appended (RAND.py's are float), then astype(bool)
    per_seq = [np.array([True, False, False]), np.array([0.0, 1.0]), np.zeros(0, dtype=bool), np.array([True])]
    assert data.frames_from_flag(per_seq).tolist() == [0, 4, 5]
    assert data.frames_from_flag(np.array([False, True, True])).tolist() == [1, 2]
    assert data.frames_from_flag(np.zeros(3, dtype=bool)).tolist() == []


def test_train_labels_has_no_cpu_fallback(golden_dir):
    from lidal_amd import data
    g = np.load(os.path.join(golden_dir, 'labels_small.npz'))
    raw = torch.from_numpy(g['nu_raw0'])
    with pytest.raises(RuntimeError, match='GPU only'):
        data.train_labels(raw, data.nu_label_map())
    with pytest.raises(RuntimeError, match='GPU only'):
        data.train_sample(torch.from_numpy(g['points0']), torch.from_numpy(g['intensity0']), raw, data.nu_label_map(),
                          rng=np.random.RandomState(0))


def test_readers_round_trip_what_the_reference_reads(tmp_path, golden_dir):
    """Files written the way the reference reads them (np.fromfile with its dtypes and widths, np.load)."""
    from lidal_amd import io as lio
    g = np.load(os.path.join(golden_dir, 'labels_small.npz'))
    pts, inten = g['points0'], g['intensity0']
    xyzi = np.concatenate([pts, inten[:, None]], 1).astype(np.float32)
    xyzi.tofile(tmp_path / 'sk.bin')
    np.concatenate([xyzi, np.full((xyzi.shape[0], 1), 7, np.float32)], 1).tofile(tmp_path / 'nu.pcd.bin')
    for name, ds in (('sk.bin', 'SK'), ('nu.pcd.bin', 'NU')):
        p, i = lio.load_scan(str(tmp_path / name), ds)
        assert p.dtype == torch.float32 and i.dtype == torch.float32 and p.is_contiguous()
        assert np.array_equal(p.numpy(), pts) and np.array_equal(i.numpy(), inten)
    g['sk_raw0'].tofile(tmp_path / 'sk.label')
    g['nu_raw0'].tofile(tmp_path / 'nu_lidarseg.bin')
    sk = lio.load_labels(str(tmp_path / 'sk.label'), 'SK')
    assert sk.dtype == torch.int32 and np.array_equal(sk.numpy().view(np.uint32), g['sk_raw0'])
    nu = lio.load_labels(str(tmp_path / 'nu_lidarseg.bin'), 'NU')
    assert nu.dtype == torch.uint8 and np.array_equal(nu.numpy(), g['nu_raw0'])
    with pytest.raises(ValueError, match='SK'):
        lio.load_labels(str(tmp_path / 'sk.label'), 'kitti360')
    lio.save_prob_pred(str(tmp_path / 'prob/0.npy'), str(tmp_path / 'pred/0.npy'), torch.rand(g['sk_pseudo0'].shape[0], 19),
                       torch.from_numpy(g['sk_pseudo0']))
    pred = lio.load_pred(str(tmp_path / 'pred/0.npy'))
    assert pred.dtype == torch.int64 and np.array_equal(pred.numpy(), g['sk_pseudo0'])
    assert np.array_equal(np.load(tmp_path / 'pred/0.npy'), g['sk_pseudo0'])        # as sk_dataset.py:119 reads it
