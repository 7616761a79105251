"""Host: the routing plan of a mixed-modality batch (mec_fusion_mixed_plan, include/mec.h). The header states it
exactly -- compact order is ascending sample index; x_idx[b] counts the earlier samples that have modality x,
-1 when b lacks it; route by the number of bits (three bits: ATTENTION with a model, AVERAGE without); att lists
the ATTENTION samples ascending, then -1 up to B -- so the numpy mirror below reproduces it entry for entry.
No GPU: the plan is host code, and the argument errors of mec_fusion_fwd_mixed are raised before any device
call (a null handle is a valid argument there: no attention model)."""
import ctypes

import numpy as np
import pytest

from mec import _lib

IP = ctypes.POINTER(ctypes.c_int32)
UP = ctypes.POINTER(ctypes.c_uint8)
NONE, SINGLE, AVERAGE, ATTENTION = 0, 1, 2, 3


def _plan(present, have_model=1):
    p = np.ascontiguousarray(present, np.uint8)
    B = int(p.size)
    out = [np.full(B, -7, np.int32) for _ in range(5)]  # s_idx, t_idx, i_idx, route, att
    counts = np.full(3, -7, np.int32)
    n = _lib.load().mec_fusion_mixed_plan(p.ctypes.data_as(UP), B, have_model, *(a.ctypes.data_as(IP) for a in out),
                                          counts.ctypes.data_as(IP))
    return n, out, counts


def _mirror(present, have_model):
    """The plan as include/mec.h states it."""
    p = np.asarray(present, np.int64)
    has = np.stack([(p >> m) & 1 for m in range(3)])                       # [3,B]
    idx = np.where(has == 1, np.cumsum(has, 1) - has, -1).astype(np.int32)  # earlier samples with the modality
    bits = has.sum(0)
    route = np.where(bits == 3, ATTENTION if have_model else AVERAGE, bits).astype(np.int32)
    att = np.full(p.size, -1, np.int32)
    rows = np.flatnonzero(route == ATTENTION)
    att[:rows.size] = rows
    return rows.size, [idx[0], idx[1], idx[2], route, att], has.sum(1).astype(np.int32)


def _same(present, have_model):
    n, out, counts = _plan(present, have_model)
    mn, mout, mcounts = _mirror(present, have_model)
    assert n == mn
    for a, b in zip(out, mout):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(counts, mcounts)


def test_hand_checked_plan():
    n, (s, t, i, route, att), counts = _plan([7, 2, 0, 6, 7, 1, 5, 7], 1)
    assert n == 3
    assert s.tolist() == [0, -1, -1, -1, 1, 2, 3, 4]
    assert t.tolist() == [0, 1, -1, 2, 3, -1, -1, 4]
    assert i.tolist() == [0, -1, -1, 1, 2, -1, 3, 4]
    assert route.tolist() == [ATTENTION, SINGLE, NONE, AVERAGE, ATTENTION, SINGLE, AVERAGE, ATTENTION]
    assert att.tolist() == [0, 4, 7, -1, -1, -1, -1, -1]
    assert counts.tolist() == [5, 5, 5]


def test_hand_checked_plan_without_model():
    n, (s, t, i, route, att), counts = _plan([7, 2, 0, 6, 7, 1, 5, 7], 0)
    assert n == 0
    assert route.tolist() == [AVERAGE, SINGLE, NONE, AVERAGE, AVERAGE, SINGLE, AVERAGE, AVERAGE]
    assert att.tolist() == [-1] * 8
    assert s.tolist() == [0, -1, -1, -1, 1, 2, 3, 4] and counts.tolist() == [5, 5, 5]


@pytest.mark.parametrize('have_model', [0, 1])
def test_all_eight_patterns_equal_the_mirror(have_model):
    _same(np.arange(8), have_model)
    _same(np.arange(8)[::-1], have_model)
    for v in range(8):  # a batch of one pattern alone
        _same([v] * 3, have_model)


@pytest.mark.parametrize('have_model', [0, 1])
def test_random_batch_equals_the_mirror(have_model):
    present = np.random.default_rng(257 + have_model).integers(0, 8, 257)
    _same(present, have_model)
    n, (s, t, i, route, att), counts = _plan(present, have_model)
    for idx, c in zip((s, t, i), counts):  # each compact row used once, in sample order
        assert idx[idx >= 0].tolist() == list(range(c))
    assert n == (np.count_nonzero(present == 7) if have_model else 0)


def test_empty_batch_returns_zero():
    lib = _lib.load()
    assert lib.mec_fusion_mixed_plan(None, 0, 1, None, None, None, None, None, None) == 0
    n, _, counts = _plan(np.zeros(0, np.uint8))
    assert n == 0 and counts.tolist() == [0, 0, 0]


def test_plan_errors():
    lib = _lib.load()
    n, _, _ = _plan([1, 8, 2])
    assert n == -1 and b'0..7' in lib.mec_last_error()
    a, c = np.zeros(2, np.int32), np.zeros(3, np.int32)
    p, cp = a.ctypes.data_as(IP), c.ctypes.data_as(IP)
    pr = np.array([3, 7], np.uint8).ctypes.data_as(UP)
    good = [pr, 2, 1, p, p, p, p, p, cp]
    for k in (0, 3, 4, 5, 6, 7, 8):
        args = list(good)
        args[k] = None
        assert lib.mec_fusion_mixed_plan(*args) == -1
        assert b'null pointer' in lib.mec_last_error()
    assert lib.mec_fusion_mixed_plan(pr, -1, 1, p, p, p, p, p, cp) == -1
    assert b'B < 0' in lib.mec_last_error()


def _args(**kw):
    """A descriptor whose pointers are non-null dummies (never read: every case below is refused first)."""
    d = ctypes.c_void_p(64)
    base = dict(s_feat=d, t_feat=d, i_feat=d, s_pred=d, t_pred=d, i_pred=d, ns=2, nt=2, ni=2, s_idx=d, t_idx=d, i_idx=d,
                att=d, n_att=0, B=4, fused=d, logits=d, attn_w=d, dec_w=d)
    base.update(kw)
    return _lib.FusionMixedArgs(**base)


@pytest.mark.parametrize('kw,msg', [
    (dict(s_idx=None), b'null index array'), (dict(t_idx=None), b'null index array'), (dict(i_idx=None), b'null index array'),
    (dict(fused=None), b'null output'), (dict(logits=None), b'null output'), (dict(attn_w=None), b'null output'),
    (dict(dec_w=None), b'null output'),
    (dict(B=-1), b'negative count'), (dict(ns=-1), b'negative count'), (dict(nt=-2), b'negative count'),
    (dict(ni=-1), b'negative count'), (dict(n_att=-1), b'negative count'),
    (dict(n_att=1), b'needs the fusion model'),
    (dict(s_pred=None), b'null probs'), (dict(t_pred=None), b'null probs'), (dict(i_pred=None), b'null probs'),
])
def test_fwd_mixed_argument_errors_without_gpu(kw, msg):
    lib = _lib.load()
    assert lib.mec_fusion_fwd_mixed(None, ctypes.byref(_args(**kw)), None) == -1
    assert msg in lib.mec_last_error()


def test_fwd_mixed_null_descriptor_and_empty_batch_without_gpu():
    lib = _lib.load()
    assert lib.mec_fusion_fwd_mixed(None, None, None) == -1
    assert b'null descriptor' in lib.mec_last_error()
    # B == 0 returns 0 without a launch, whatever else the descriptor holds
    assert lib.mec_fusion_fwd_mixed(None, ctypes.byref(_lib.FusionMixedArgs()), None) == 0
