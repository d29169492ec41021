"""The counter-based dropout without a GPU: the generator of tests/dropout_ref.py against Random123's known answers, the
host's thr / scale, the refusals of lidal_dropout_apply (all before any launch), the new plan kind, and the state_dict
surface of SPVCNN(dropout_seed=...)."""
import array

import numpy as np
import pytest
import torch

import dropout_ref as D


def _hex(words):
    return ' '.join('%08x' % int(w[0]) for w in words)


def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32 with 10 rounds."""
    f = 0xffffffff
    assert _hex(D.philox4x32_10((0, 0, 0, 0), (0, 0))) == '6627e8d5 e169c58d bc57ac4c 9b00dbd8'
    assert _hex(D.philox4x32_10((f, f, f, f), (f, f))) == '408f276d 41c83b0e a20bc7c6 6d5451fd'
    assert _hex(D.philox4x32_10((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0))) == \
        'd16cfe09 94fdcceb 5001e420 24126ea1'


def test_words_follow_the_element_index_across_the_32_bit_group_boundary():
    """Element e uses word e & 3 of group e >> 2, whatever `first` is; the group index is 64 bits wide."""
    first = 2 ** 34 - 8
    w = D.words(16, 5, 9, first)
    for i in (0, 7, 8, 15):
        e = first + i
        g = e >> 2
        want = D.philox4x32_10((g & 0xffffffff, g >> 32, 9, 0), (5, 0))[e & 3][0]
        assert int(w[i]) == int(want), i
    assert np.array_equal(D.words(8, 5, 9, first + 8), w[8:])
    assert not np.array_equal(D.words(8, 5, 9, 0), D.words(8, 5, 9, 2 ** 34))       # (the high counter word counts)


@pytest.mark.parametrize('p,thr,scale', [(0.3, 3006477107, np.float32(1.0 / 0.7)), (0.5, 2 ** 31, np.float32(2.0)),
                                         (1e-12, 0xffffffff, np.float32(1.0)), (1 - 2.0 ** -33, 0, np.float32(2.0 ** 33))])
def test_threshold_and_scale_as_the_host_forms_them(p, thr, scale):
    from lidal_amd.nn.dropout import mask_constants
    got_thr, got_scale = mask_constants(p)
    assert got_thr == thr and isinstance(got_thr, int)
    assert np.float32(got_scale) == scale and float(np.float32(got_scale)) == got_scale        # an f32 value
    assert (got_thr, np.float32(got_scale)) == D.constants(p)
    assert mask_constants(1.0)[0] == 0 and mask_constants(0.0) == (0xffffffff, 1.0)
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError):
            mask_constants(bad)


def test_refusals_come_before_any_launch():
    """No GPU here: a call that got as far as a launch would fail with another message (or crash on the fake address)."""
    from lidal_amd import backend as B
    L = B.lib()
    ok = 0x10000
    cases = [((ok, 16, B.F32, 4, 1, 0, 100, 2.0), b'multiple of 8'),
             ((ok, 16, B.F32, -8, 1, 0, 100, 2.0), b'multiple of 8'),
             ((ok, 16, B.F32, 0, 1, 0, 2 ** 32, 2.0), b'thr'),
             ((ok, 16, B.F32, 0, 1, 0, -1, 2.0), b'thr'),
             ((ok, 16, 7, 0, 1, 0, 100, 2.0), b'bad dtype'),
             ((ok + 8, 16, B.BF16, 0, 1, 0, 100, 2.0), b'16-byte aligned'),
             ((ok, -1, B.F32, 0, 1, 0, 100, 2.0), b'negative')]
    for args, what in cases:
        assert L.lidal_dropout_apply(*args, None) != 0, args
        assert what in L.lidal_last_error(), (args, L.lidal_last_error())
    assert L.lidal_dropout_apply(ok, 0, B.F32, 0, 1, 0, 100, 2.0, None) == 0        # nothing to do, nothing launched


def test_the_plan_kind_is_known_and_refused_when_truncated():
    from lidal_amd import backend as B
    from lidal_amd.network import plan
    L = B.lib()
    assert plan.OP_DROPOUT_APPLY == 35 and L.lidal_plan_op_args(35) == 8
    assert plan._HIT_NAMES[35] == 'dropout_apply'
    short = array.array('q', [plan.OP_DROPOUT_APPLY, 0, 0, 0])
    assert L.lidal_plan_run(short.buffer_info()[0], 4, 1, None, None) != 0
    assert b'truncated' in L.lidal_last_error() and b'dropout_apply' in L.lidal_last_error()
    # a whole operation with a bad argument: the callee's refusal, with the operation's place in the plan
    bad = array.array('q', [plan.OP_DROPOUT_APPLY, 0x10000, 16, B.F32, 4, 1, 0, 100, plan._dbits(2.0)])
    assert L.lidal_plan_run(bad.buffer_info()[0], len(bad), 1, None, None) != 0
    assert b'op 0 (dropout_apply)' in L.lidal_last_error() and b'multiple of 8' in L.lidal_last_error()


def test_the_module_has_no_state_and_the_models_keys_are_unchanged():
    from torch import nn
    from lidal_amd import nn as spnn
    from lidal_amd.network import SPVCNN, MinkUNet
    a, b = SPVCNN(19), SPVCNN(19, dropout_seed=1)
    assert type(a.dropout) is nn.Dropout
    d = b.dropout
    assert isinstance(d, spnn.Dropout) and not isinstance(d, nn.Dropout)
    assert (d.p, d.inplace, d.seed, d.calls, d.mc) == (0.3, True, 1, 0, False)
    assert isinstance(d.seed, int) and isinstance(d.calls, int) and isinstance(d.mc, bool)
    assert list(d.parameters()) == [] and list(d.buffers()) == [] and d.state_dict() == {}
    assert list(a.state_dict()) == list(b.state_dict())
    b.load_state_dict(a.state_dict())
    a.load_state_dict(b.state_dict())
    d.set_rng_state((2 ** 64 - 1, 7))
    assert d.rng_state() == (2 ** 64 - 1, 7)
    with pytest.raises(ValueError):
        d.set_rng_state((2 ** 64, 0))
    with pytest.raises(RuntimeError, match='GPU only'):
        d(torch.zeros(8))
    # use_counter_dropout keeps p, inplace and the mode; mc_dropout sets and restores mc, also after an exception
    a.eval()
    new = spnn.use_counter_dropout(a, seed=3)
    assert a.dropout is new and (new.p, new.inplace, new.seed, new.training) == (0.3, True, 3, False)
    assert list(a.state_dict()) == list(b.state_dict())
    with spnn.mc_dropout(a):
        assert new.mc is True
    assert new.mc is False
    with pytest.raises(KeyError):
        with spnn.mc_dropout(a):
            raise KeyError('x')
    assert new.mc is False
    for m in (MinkUNet(19), SPVCNN(19)):
        with pytest.raises(ValueError, match='no lidal_amd.nn.Dropout'):
            with spnn.mc_dropout(m):
                pass
    with pytest.raises(ValueError):
        spnn.use_counter_dropout(MinkUNet(19))


def test_keep_fraction_of_the_restatement():
    """p = 0.3 over 4 736 elements (one row block of the coarsest level of a small scan): the kept fraction is within
    6 binomial standard deviations, 6 * sqrt(0.3 * 0.7 / 4736) = 0.040, of 0.7."""
    n = 4736
    frac = D.keep(n, 0.3, 0, 0).mean()
    print('kept fraction %.4f' % frac)
    assert 6 * np.sqrt(0.3 * 0.7 / n) < 0.0401
    assert abs(frac - 0.7) <= 0.040
    assert D.keep(64, 1.0, 0, 0).sum() == 0
    m = D.multiplier(n, 0.3, 0, 0)
    assert set(np.unique(m)) == {np.float32(0), np.float32(1.0 / 0.7)}
