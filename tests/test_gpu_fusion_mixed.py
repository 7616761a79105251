"""GPU: the fusion step of a mixed-modality batch (mec_fusion_fwd_mixed through FusionHead.forward_mixed and
engine.fuse_mixed): every sample routed as MultimodalFusion.predict_multimodal routes one request.

The batch: B = 19, the 8 presence patterns twice plus three more all-three samples in a fixed shuffled order, so
n_att = 5 (at fusion_r = 4 one full group and a 1-row tail). That multiset gives every modality 11 rows, so
ns == nt == ni whatever the order; what makes a swapped index array show is that on every attention sample the
three compact indices are pairwise different (the order was chosen for that; asserted in the fixture), every
compact row being distinct. test_unequal_counts repeats the attention check on a batch whose three counts are
pairwise different.
Inputs at the scale of tests/golden/fusion.npz's rows (make_golden.py: uniform features, ReLU-like for speech
and image; probs the softmax of uniform logits). Every call goes through the C ABI on outputs pre-filled with NaN,
so an element the call leaves unwritten shows, and through the engine wrapper, which must return the same bits.
No test feeds out-of-range or inconsistent device indices: the clamp is a stated contract (include/mec.h)."""
import ctypes

import numpy as np
import pytest
import torch

from mec import _lib, engine, synthetic as syn
from oracle import fusion as o_f

pytestmark = pytest.mark.gpu

# the 8 patterns twice plus three more all-three samples, in a fixed shuffled order
PATTERNS = [6, 4, 0, 6, 7, 5, 2, 7, 7, 7, 1, 2, 3, 7, 1, 5, 4, 3, 0]
DIMS = (64, 768, 512)


def _inputs(present, seed):
    """Compact (feat, probs) per modality for the bitmask `present`, every row distinct."""
    present = np.asarray(present)
    out = []
    for m, (name, d) in enumerate(zip(('speech', 'text', 'image'), DIMS)):
        n = int(((present >> m) & 1).sum())
        f = syn.uniform(seed, f'mixed/{name}', (n, d), -1.0, 1.0)
        if name != 'text':
            f = np.maximum(f, 0) * 2.0  # ReLU features like the encoders'
        z = syn.uniform(seed + 1, f'mixed/pred/{name}', (n, 7), -3.0, 3.0)
        e = np.exp(z - z.max(-1, keepdims=True))
        out.append((f.astype(np.float32), (e / e.sum(-1, keepdims=True)).astype(np.float32)))
    return out


def _raw(handle, plan, dp, dev):
    """mec_fusion_fwd_mixed itself, on outputs pre-filled with NaN."""
    nan = lambda k, dt: torch.full((plan.B, k), float('nan'), dtype=dt, device=dev)  # noqa: E731
    fused, logits, aw, dw = nan(7, torch.float64), nan(7, torch.float32), nan(3, torch.float32), nan(3, torch.float32)
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    (sf, sp), (tf, tp), (imf, ip) = [(None, None) if x is None else x for x in dp]
    ns, nt, ni = plan.counts
    args = _lib.FusionMixedArgs(s_feat=p(sf), t_feat=p(tf), i_feat=p(imf), s_pred=p(sp), t_pred=p(tp), i_pred=p(ip),
                                ns=ns, nt=nt, ni=ni, s_idx=p(plan.dev[0]), t_idx=p(plan.dev[1]), i_idx=p(plan.dev[2]),
                                att=p(plan.dev[3]), n_att=plan.n_att, B=plan.B, fused=p(fused), logits=p(logits),
                                attn_w=p(aw), dec_w=p(dw))
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    assert _lib.load().mec_fusion_fwd_mixed(handle, ctypes.byref(args), stream) == 0, _lib.load().mec_last_error()
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in (fused, logits, aw, dw)]


def _run(head, plan, pairs, dev):
    dp = [None if p[0].shape[0] == 0 else tuple(engine.to_device(a, dev) for a in p) for p in pairs]
    raw = _raw(head.handle if head is not None else None, plan, dp, dev)
    for a in raw:
        assert not np.isnan(a).any()  # every element written
    if head is None:
        out = engine.fuse_mixed(plan, *(None if p is None else p[1] for p in dp))
    else:
        out = head.forward_mixed(plan, *dp)
    torch.cuda.synchronize()
    for a, t in zip(raw, out):
        np.testing.assert_array_equal(a, t.cpu().numpy())
    return raw


def _rows(plan, pairs, b):
    """Sample b's (feat, probs) per modality, None where absent."""
    return [None if idx[b] < 0 else (p[0][idx[b]], p[1][idx[b]]) for idx, p in zip((plan.s_idx, plan.t_idx, plan.i_idx), pairs)]


def _check_off_attention(plan, pairs, fused, logits, aw, dw):
    """AVERAGE, SINGLE and NONE rows, and the zeros of logits / attn_w / dec_w off the attention route."""
    assert fused.dtype == np.float64 and fused.shape == (plan.B, 7)
    seen = set()
    for b in range(plan.B):
        route = int(plan.route[b])
        seen.add(route)
        if route == _lib.ROUTE_ATTENTION:
            continue
        rows = _rows(plan, pairs, b)
        probs = [None if r is None else r[1].astype(np.float64) for r in rows]
        have = [p for p in probs if p is not None]
        if route == _lib.ROUTE_AVERAGE:
            assert len(have) >= 2
            np.testing.assert_array_equal(fused[b], o_f.fuse_predictions(*probs))  # float64, bit-exact with numpy
        elif route == _lib.ROUTE_SINGLE:
            assert len(have) == 1
            np.testing.assert_array_equal(fused[b], have[0])
        else:
            assert not have
            np.testing.assert_array_equal(fused[b], np.zeros(7))
        for a in (logits, aw, dw):
            np.testing.assert_array_equal(a[b], np.zeros(a.shape[1], np.float32))
    return seen


def _dense(plan, pairs):
    att = plan.att[:plan.n_att]
    return [np.ascontiguousarray(p[k][idx[att]]) for k in (0, 1) for idx, p in zip((plan.s_idx, plan.t_idx, plan.i_idx), pairs)]


def _check_attention_rows(head, plan, pairs, dev):
    """The attention rows against FusionHead.forward on the same rows gathered densely (same bits, for the
    handle's current fusion_r / fusion_split) -> (fused, logits, aw, dw) of the mixed call."""
    att = plan.att[:plan.n_att]
    fused, logits, aw, dw = _run(head, plan, pairs, dev)
    want = head.forward(*(engine.to_device(a, dev) for a in _dense(plan, pairs)))
    torch.cuda.synchronize()
    wl, wp, wa, wd = (t.cpu().numpy() for t in want)
    probs32 = fused[att].astype(np.float32)
    np.testing.assert_array_equal(probs32.astype(np.float64), fused[att])  # float32 probs, widened exactly
    for got, ref in ((logits[att], wl), (probs32, wp), (aw[att], wa), (dw[att], wd)):
        np.testing.assert_array_equal(got, ref)
    return fused, logits, aw, dw


@pytest.fixture(scope='module')
def head(dev):
    return engine.FusionHead(device=dev)


@pytest.fixture(scope='module')
def batch(dev):
    plan = engine.fusion_mixed_plan(PATTERNS, True, dev)
    assert plan.B == 19 and plan.n_att == 5 and plan.counts == (11, 11, 11)
    assert sorted(PATTERNS) == sorted(list(range(8)) * 2 + [7, 7, 7])
    trip = np.stack([plan.s_idx, plan.t_idx, plan.i_idx])[:, plan.att[:5]]
    # a swapped pair of index arrays moves every attention row
    for a, b in ((0, 1), (0, 2), (1, 2)):
        assert (trip[a] != trip[b]).all()
    pairs = _inputs(PATTERNS, 21)
    # oracle reference of the attention rows, computed once
    ref = o_f.forward(syn.weights('fusion'), *_dense(plan, pairs))
    return plan, pairs, ref


@pytest.mark.parametrize('split', [1, 0])
@pytest.mark.parametrize('r', [4, 2, 1])
def test_mixed_batch_routes_every_row(head, batch, dev, r, split):
    plan, pairs, ref = batch
    head.set_option('fusion_r', r)
    head.set_option('fusion_split', split)
    try:
        fused, logits, aw, dw = _check_attention_rows(head, plan, pairs, dev)
    finally:
        head.set_option('fusion_r', 4)
        head.set_option('fusion_split', 1)
    att = plan.att[:plan.n_att]
    rl, rp, ra, rd = ref  # the bars of test_gpu_parity.test_fusion_golden
    assert np.abs(logits[att] - rl).max() < 1e-4
    assert np.abs(fused[att] - rp).max() < 1e-5
    assert np.abs(aw[att] - ra).max() < 1e-5
    assert np.abs(dw[att] - rd).max() < 1e-5
    assert np.array_equal(fused[att].argmax(1), rp.argmax(1))
    seen = _check_off_attention(plan, pairs, fused, logits, aw, dw)
    assert seen == {_lib.ROUTE_NONE, _lib.ROUTE_SINGLE, _lib.ROUTE_AVERAGE, _lib.ROUTE_ATTENTION}


def test_unequal_counts(head, dev):
    """ns = 8, nt = 5, ni = 4: a swapped index array or count reads another row (or is clamped)."""
    present = [7, 1, 1, 3, 7, 1, 2, 7, 5]
    plan = engine.fusion_mixed_plan(present, True, dev)
    assert plan.counts == (8, 5, 4) and plan.n_att == 3
    pairs = _inputs(present, 33)
    out = _check_attention_rows(head, plan, pairs, dev)
    _check_off_attention(plan, pairs, *out)


def test_no_attention_rows(head, dev):
    present = [3, 1, 6, 4, 5, 2]
    plan = engine.fusion_mixed_plan(present, True, dev)
    assert plan.n_att == 0 and (plan.att == -1).all()
    pairs = _inputs(present, 41)
    out = _run(head, plan, pairs, dev)
    assert _check_off_attention(plan, pairs, *out) == {_lib.ROUTE_SINGLE, _lib.ROUTE_AVERAGE}


def test_one_attention_row(head, dev):
    plan = engine.fusion_mixed_plan([7], True, dev)
    assert plan.n_att == 1 and plan.B == 1
    pairs = _inputs([7], 43)
    fused, logits, aw, dw = _check_attention_rows(head, plan, pairs, dev)
    ref = o_f.forward(syn.weights('fusion'), *_dense(plan, pairs))
    assert np.abs(fused - ref[1]).max() < 1e-5 and np.abs(logits - ref[0]).max() < 1e-4


def test_fuse_mixed_without_model_averages_three_present(batch, dev):
    _, pairs, _ = batch
    plan = engine.fusion_mixed_plan(PATTERNS, False, dev)
    assert plan.n_att == 0 and (plan.route[np.asarray(PATTERNS) == 7] == _lib.ROUTE_AVERAGE).all()
    out = _run(None, plan, pairs, dev)
    assert _check_off_attention(plan, pairs, *out) == {_lib.ROUTE_NONE, _lib.ROUTE_SINGLE, _lib.ROUTE_AVERAGE}
    for a in out[1:]:
        assert not a.any()


def test_flags_form_of_present_and_empty_batch(head, dev):
    flags = np.array([[1, 1, 1], [0, 1, 0], [0, 0, 0], [0, 1, 1]], bool)
    plan = engine.fusion_mixed_plan(flags, True, dev)
    assert plan.present.tolist() == [7, 2, 0, 6] and plan.route.tolist() == [3, 1, 0, 2]
    plan = engine.fusion_mixed_plan(np.zeros((0, 3), bool), True, dev)
    fused, logits, aw, dw = head.forward_mixed(plan, None, None, None)
    assert fused.shape == (0, 7) and fused.dtype == torch.float64 and logits.shape == (0, 7) and aw.shape == (0, 3)
    fused = engine.fuse_mixed(engine.fusion_mixed_plan([], False, dev))[0]
    assert fused.shape == (0, 7)


def test_argument_errors_that_need_a_handle(head, batch, dev):
    plan, pairs, _ = batch
    dp = [tuple(engine.to_device(a, dev) for a in p) for p in pairs]
    with pytest.raises(ValueError):  # a plan without the model's route given to the model, and the reverse
        head.forward_mixed(engine.fusion_mixed_plan(PATTERNS, False, dev), *dp)
    with pytest.raises(ValueError):
        engine.fuse_mixed(plan, *(p[1] for p in dp))
    with pytest.raises(ValueError):
        head.forward_mixed(plan, dp[0], None, dp[2])
    with pytest.raises(ValueError):
        head.forward_mixed(plan, dp[0], (dp[1][0][:5], dp[1][1][:5]), dp[2])
    # C ABI: refused before any launch
    lib, d = _lib.load(), ctypes.c_void_p(dp[0][1].data_ptr())
    base = dict(s_feat=d, t_feat=d, i_feat=d, s_pred=d, t_pred=d, i_pred=d, ns=3, nt=2, ni=3, s_idx=d, t_idx=d, i_idx=d,
                att=d, n_att=3, B=4, fused=d, logits=d, attn_w=d, dec_w=d)
    assert lib.mec_fusion_fwd_mixed(head.handle, ctypes.byref(_lib.FusionMixedArgs(**base)), None) == -1
    assert b'min(ns, nt, ni)' in lib.mec_last_error()
    base.update(n_att=2, t_feat=None)
    assert lib.mec_fusion_fwd_mixed(head.handle, ctypes.byref(_lib.FusionMixedArgs(**base)), None) == -1
    assert b'null features' in lib.mec_last_error()
    speech = engine.SpeechEncoder(device=dev)
    base.update(t_feat=d)
    assert lib.mec_fusion_fwd_mixed(speech.handle, ctypes.byref(_lib.FusionMixedArgs(**base)), None) == -1
    assert b'wrong kind' in lib.mec_last_error()
