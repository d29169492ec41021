"""Frame-level selection, the host side: the numpy restatement of the kernels' orders (tests/frame_ref.py) against the
reference's own worker_func values and __main__ flags (tests/golden/make_golden_frame.py), the selection rules, the
flag files and the C-ABI surface."""
import os
import re

import numpy as np
import pytest

import frame_inputs as FI
import frame_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENT_ULPS = 1            # ENT rests on libm's log, SEGENT on numpy's log2: the steps not restated
SEGENT_ULPS = 64


def _fixture(golden_dir):
    return np.load(os.path.join(golden_dir, 'frame_small.npz'))


def ulps32(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def ulps64(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a.view(np.int64).astype(object) - b.view(np.int64).astype(object)).astype(np.float64)


def test_regenerated_inputs_match_fixture(golden_dir):
    g = _fixture(golden_dir)
    frames = [FI.worker_frame(k) for k in range(len(FI.WORKER_SIZES))] + [FI.empty_sv_frame()]
    assert FI.sha256(*[a for f in frames for a in (f['prob'], f['pred'])],
                     *[p for f in frames for p in f['sv2point']]) == str(g['worker_inputs_sha'])
    shas = []
    for s_i in range(len(FI.SEQS)):
        for i in range(FI.MAIN_FRAMES):
            f = FI.main_frame(s_i, i)
            shas += [f['prob'], f['pred']] + f['sv2point']
    assert FI.sha256(*shas) == str(g['main_inputs_sha'])
    assert np.array_equal(np.concatenate(FI.main_flags_in()), g['main_flags_in'])
    seed = int(g['cset_seed'])
    assert FI.sha256(FI.cset_feats(seed)) == str(g['cset_feats_sha'])
    assert np.array_equal(np.concatenate(FI.cset_flags_in(seed)), g['cset_flags_in'])


def test_restatement_equals_worker_func(golden_dir):
    """MAR and CONF bit for bit; ENT and SEGENT within the stated bars (here, on the generator's numpy, they are
    exact as well)."""
    g = _fixture(golden_dir)
    worst = [0, 0]
    for k in range(len(FI.WORKER_SIZES)):
        f = FI.worker_frame(k)
        e, ma, c = frame_ref.uncertainty(f['prob'])
        assert ma == g['worker_mar'][k] and c == g['worker_conf'][k], k
        worst[0] = max(worst[0], int(ulps32(e, g['worker_ent'][k])))
        s = frame_ref.segment_entropy(f['pred'], f['sv2point'], f['class_num'])
        worst[1] = max(worst[1], int(ulps64(s, g['worker_segent'][k])))
    print('restatement vs worker_func: ENT %d ulp, SEGENT %d ulp' % tuple(worst))
    assert worst[0] <= ENT_ULPS and worst[1] <= SEGENT_ULPS
    f = FI.empty_sv_frame()
    assert np.isnan(frame_ref.segment_entropy(f['pred'], f['sv2point'], f['class_num']))
    assert np.isnan(g['worker_segent_empty'])


def test_point_uncertainty_order_matches_numpy():
    """The written-out row sums and entr are numpy's and scipy's own, row by row."""
    scipy_stats = pytest.importorskip('scipy.stats')
    prob = FI.worker_frame(9)['prob']
    ent, mar, conf = frame_ref.point_uncertainty(prob)
    assert np.array_equal(ent, scipy_stats.entropy(prob, axis=1))
    srt = np.sort(prob, axis=-1)
    assert np.array_equal(mar, srt[:, -1] - srt[:, -2]) and np.array_equal(conf, srt[:, -1])
    assert np.array_equal(frame_ref.rows_pairwise_f32(prob), np.sum(prob, axis=1))
    feat = np.random.RandomState(0).normal(size=(20000, 96)).astype(np.float32)
    assert np.array_equal(frame_ref.frame_feature(feat), feat.mean(0))
    assert np.array_equal(frame_ref.frame_feature(feat[:, :1]), feat[:, :1].mean(0))


def _topk(flags, scores, largest):
    unl = [i for i in range(len(flags)) if not flags[i]]
    key = (lambda i: (-float(scores[i]), i)) if largest else (lambda i: (float(scores[i]), i))
    out = np.array(flags, bool)
    out[sorted(unl, key=key)[:int(round(0.01 * len(flags)))]] = True
    return out


def test_select_frames_is_the_top_k_of_the_scores(golden_dir):
    from lidal_amd.score.frame_level import LARGEST, select_frames
    g = _fixture(golden_dir)
    flags = g['main_flags_in']
    for m in ('ENT', 'MAR', 'CONF', 'SEGENT'):
        sc = g['main_scores_' + m]
        got = select_frames(flags, sc, LARGEST[m])
        assert np.array_equal(got, _topk(flags, sc, LARGEST[m])), m
        assert (got & ~flags).sum() == int(g['main_num_add'])
    # ties at the k-th place go to the lower frame index; NaN counts as the largest value (numpy's sort order)
    flags = np.zeros(300, bool)
    sc = np.zeros(300, np.float32)
    sc[[250, 40, 7]] = [5.0, 5.0, np.nan]
    assert np.where(select_frames(flags, sc, True))[0].tolist() == [7, 40, 250]
    assert np.where(select_frames(flags, sc, False))[0].tolist() == [0, 1, 2]
    sc[:] = 1.0
    assert np.where(select_frames(flags, sc, True))[0].tolist() == [0, 1, 2]
    with pytest.raises(ValueError):
        select_frames(flags, sc[:10])


def test_reference_zero_half_mode(golden_dir):
    """The reference's flags rest on np.argpartition over equal keys, which depends on the host's CPU dispatch: where
    this host's probe equals the generator's, the literal mode reproduces the recorded flags; elsewhere it equals the
    literal expression evaluated here."""
    from lidal_amd.score.frame_level import LARGEST, select_frames
    g = _fixture(golden_dir)
    flags = g['main_flags_in']
    num_add = int(g['main_num_add'])
    big, small = frame_ref.argpartition_probe(int((~flags).sum()), num_add)
    same_host = np.array_equal(big, g['main_probe_largest']) and np.array_equal(small, g['main_probe_smallest'])
    print('argpartition probe %s the generator\'s' % ('equals' if same_host else 'differs from'))
    unl = np.where(~flags)[0]
    for m in ('ENT', 'MAR', 'CONF', 'SEGENT'):
        got = select_frames(flags, g['main_scores_' + m], LARGEST[m], reference_zero_half=True)
        if same_host:
            assert np.array_equal(got, g['main_flags_' + m]), m
        else:
            want = flags.copy()
            want[unl[big if LARGEST[m] else small]] = True
            assert np.array_equal(got, want), m
        # the reference's flags do not depend on the scores
        assert np.array_equal(got, select_frames(flags, -g['main_scores_' + m], LARGEST[m], reference_zero_half=True))


def test_coreset_restatement_reproduces_reference_main(golden_dir):
    g = _fixture(golden_dir)
    seed = int(g['cset_seed'])
    flags = g['cset_flags_in']
    picks, _ = frame_ref.coreset(FI.cset_feats(seed), flags, int(round(0.01 * flags.size)))
    out = flags.copy()
    out[picks] = True
    assert np.array_equal(out, g['cset_flags_out'])
    assert picks.size == 20 and float(g['cset_min_gap']) > 1e-5


def test_random_frames_equals_rand_draw(golden_dir):
    from lidal_amd.score.frame_level import random_frames
    g = _fixture(golden_dir)
    got = random_frames(g['main_flags_in'], np.random.RandomState(int(g['main_rand_seed'])))
    assert np.array_equal(got, g['main_flags_RAND'])
    np.random.seed(int(g['main_rand_seed']))          # rng=None: numpy's global generator, as RAND.py
    assert np.array_equal(random_frames(g['main_flags_in']), g['main_flags_RAND'])


def test_frame_board_and_flag_files(tmp_path, golden_dir):
    from lidal_amd import io
    from lidal_amd.score.frame_level import FrameBoard, select_frames
    g = _fixture(golden_dir)
    root = str(tmp_path)
    for s, f in zip(FI.SEQS, FI.main_flags_in()):
        io.save_frame_flag(io.frame_flag_path(root, 'SK', s, 0), f)
    board = FrameBoard.load(root, 'SK', 1, 'ENT', 'SPVCNN')
    assert np.array_equal(board.flags, g['main_flags_in'])
    assert board.seq_offsets == list(range(0, 301, FI.MAIN_FRAMES))
    sc = g['main_scores_ENT']
    for i in range(len(FI.SEQS)):
        board.add(i, 'ENT', sc[board.seq_offsets[i]:board.seq_offsets[i + 1]])
    new = board.select('ENT')
    assert np.array_equal(new, select_frames(board.flags, sc, True))
    board.save(root, 'SK', 1, 'ENT', new, 'SPVCNN')
    back = [io.load_frame_flag(os.path.join(root, 'Processing_files/SK/frame_flag/SPVCNN/ENT/1r', s + '.npy'))
            for s in FI.SEQS]
    assert all(b.dtype == bool for b in back) and np.array_equal(np.concatenate(back), new)
    path = io.frame_flag_path(root, 'SK', '00', 2, 'RAND')
    assert path.endswith(os.path.join('frame_flag', 'RAND', '2r', '00.npy'))
    io.save_frame_flag(path, np.zeros(4, bool))
    np.save(path, np.array([0.0, 1.0, 0.0, 1.0]))            # RAND.py writes float flags
    assert io.load_frame_flag(path).tolist() == [False, True, False, True]


def test_frame_symbols_declared_and_exported():
    from lidal_amd import backend as B
    import lidal_amd.score as S
    header = open(os.path.join(ROOT, 'include', 'lidal_amd.h')).read()
    names = ['lidal_frame_uncertainty_workspace_bytes', 'lidal_frame_uncertainty', 'lidal_segment_entropy_workspace_bytes',
             'lidal_segment_entropy', 'lidal_frame_feature_workspace_bytes', 'lidal_frame_feature',
             'lidal_coreset_workspace_bytes', 'lidal_coreset']
    for n in names:
        assert re.search(r'\b%s\(' % n, header), n
        assert n in B.SIGNATURES, n
        assert getattr(B.lib_handle(), n) is not None
    assert B.lib().lidal_version() >= 163
    assert B.lib().lidal_coreset_workspace_bytes(19130, 191) >= 19130 * 4
    for n in ('frame_uncertainty', 'segment_entropy', 'frame_feature', 'coreset', 'select_frames', 'random_frames',
              'frame_sequence', 'FrameBoard'):
        assert n in S.__all__ and hasattr(S, n), n
