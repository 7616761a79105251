"""GPU: FusedPipeline.forward_mixed at precision='fp32' on a batch of 12 requests: the 7 non-empty presence
patterns, one empty request and four more multi-modality ones. Each encoder runs once over its compact rows and
the fusion routes every request as predict_multimodal would.

Bars: the project's existing ones on those compact inputs -- text / image probs within TOL['fp32'] = 1e-5 of
the oracle (tests/test_gpu_dropin.py), speech probs within 1e-5 (tests/test_gpu_parity.py test_speech_batches);
attention rows within 1e-5 of the oracle chain fed with the oracle's own encoder outputs
(tests/test_gpu_fp32.py test_fused_fp32_end_to_end); average rows bit-exact against fuse_predictions of the
pipeline's own returned per-modality probs."""
import numpy as np
import pytest
import torch

from mec import _lib, engine, synthetic as syn
from oracle import fusion as o_f, image as o_i, speech as o_s, text as o_t

pytestmark = pytest.mark.gpu
TOL = 1e-5
PRESENT = [7, 1, 6, 0, 2, 5, 7, 3, 4, 7, 3, 6]  # bit 0 speech, 1 text, 2 image


@pytest.fixture(scope='module')
def pipe(dev):
    return engine.FusedPipeline(device=dev, precision='fp32')


@pytest.fixture(scope='module')
def case():
    """Compact inputs and the oracle's outputs on them, computed once."""
    p = np.asarray(PRESENT)
    ns, nt, ni = (int(((p >> m) & 1).sum()) for m in range(3))
    assert (ns, nt, ni) == (7, 8, 7) and set(PRESENT) == set(range(8))
    x = syn.speech_inputs(ns, seed=71)
    ids, mask = syn.text_inputs(nt, 128, seed=72, ragged=True)
    gray = syn.image_inputs(ni, seed=73)
    ref = {'speech': o_s.forward(syn.weights('speech'), x), 'text': o_t.forward(syn.weights('text'), ids, mask),
           'image': o_i.forward(syn.weights('image'), gray)}
    return (x, ids, mask, gray), ref


def _host(out):
    torch.cuda.synchronize()
    return {k: [t.cpu().numpy() for t in v] for k, v in out.items() if k != 'plan'}


def _check(out, ref):
    plan, got = out['plan'], _host(out)
    for name in ('speech', 'text', 'image'):
        err = float(np.abs(got[name][2] - ref[name][2]).max())
        print(f'forward_mixed {name}: compact probs max|d| {err:.3g}')
        assert got[name][2].shape == ref[name][2].shape and err <= TOL, name
        assert np.array_equal(got[name][2].argmax(1), ref[name][2].argmax(1)), name
    fused, logits, aw, dw = got['fusion']
    assert fused.dtype == np.float64 and fused.shape == (plan.B, 7)
    idx = (plan.s_idx, plan.t_idx, plan.i_idx)
    att = plan.att[:plan.n_att]
    assert plan.n_att == 3
    rf = o_f.forward(syn.weights('fusion'), *(ref[m][k][ix[att]] for k in (0, 2)
                                              for m, ix in zip(('speech', 'text', 'image'), idx)))
    err = float(np.abs(fused[att] - rf[1]).max())
    print(f'forward_mixed attention rows: fused probs max|d| {err:.3g}')
    assert err <= TOL and np.abs(aw[att] - rf[2]).max() <= TOL and np.abs(dw[att] - rf[3]).max() <= TOL
    assert np.array_equal(fused[att].argmax(1), rf[1].argmax(1))
    for b in range(plan.B):
        route = int(plan.route[b])
        if route == _lib.ROUTE_ATTENTION:
            continue
        own = [None if ix[b] < 0 else got[m][2][ix[b]].astype(np.float64)
               for m, ix in zip(('speech', 'text', 'image'), idx)]
        have = [p for p in own if p is not None]
        if route == _lib.ROUTE_AVERAGE:
            np.testing.assert_array_equal(fused[b], o_f.fuse_predictions(*own))
        elif route == _lib.ROUTE_SINGLE:
            np.testing.assert_array_equal(fused[b], have[0])
        else:
            np.testing.assert_array_equal(fused[b], np.zeros(7))
        for a in (logits, aw, dw):
            assert not a[b].any()


def test_three_calls_serial_then_pipelined(pipe, case, dev):
    (x, ids, mask, gray), ref = case
    args = [engine.to_device(a, dev) for a in (x, ids, mask, gray)]
    for it in range(3):  # 1st call serial (autotune), then concurrent + pipelined
        out = pipe.forward_mixed(*args, PRESENT)
        pipe.wait()
        assert set(out) == {'speech', 'text', 'image', 'fusion', 'plan'}
        _check(out, ref)
    assert pipe.check() == []


def test_text_lens(pipe, case, dev):
    (x, ids, mask, gray), ref = case
    args = [engine.to_device(a, dev) for a in (x, ids, mask, gray)]
    pipe.text.packed_rows = 0
    for it in range(2):
        out = pipe.forward_mixed(*args, PRESENT, text_lens=mask.sum(1))
        pipe.wait()
        _check(out, ref)
    assert 1 <= pipe.text.packed_rows <= ids.shape[0]  # the packed text leg ran


def test_skipped_encoders_and_epilogue(pipe, case, dev):
    (x, ids, mask, gray), ref = case
    none = (torch.empty(0, 128, dtype=torch.int32, device=dev), torch.empty(0, 48, 48, dtype=torch.uint8, device=dev))
    out, extra = pipe.forward_mixed(engine.to_device(x[:2], dev), none[0], none[0], none[1], [1, 0, 1],
                                    epilogue=lambda o: o['fusion'][0].sum(1))
    pipe.wait()
    got = _host(out)
    assert got['text'][0].shape == (0, 768) and got['image'][0].shape == (0, 512) and got['text'][2].shape == (0, 7)
    np.testing.assert_array_equal(got['fusion'][0][[0, 2]], got['speech'][2].astype(np.float64))
    assert not got['fusion'][0][1].any()
    np.testing.assert_array_equal(extra.cpu().numpy(), got['fusion'][0].sum(1))
    with pytest.raises(ValueError):  # 3 speech rows for a `present` that has 2
        pipe.forward_mixed(engine.to_device(x[:3], dev), none[0], none[0], none[1], [1, 0, 1])


def test_all_present_equals_forward(pipe, dev):
    B = 4
    ids, mask = syn.text_inputs(B, 128, seed=75, ragged=True)
    args = [engine.to_device(a, dev) for a in (syn.speech_inputs(B, seed=74), ids, mask, syn.image_inputs(B, seed=76))]
    want = _host(pipe.forward(*args))
    pipe.wait()
    got = _host(pipe.forward_mixed(*args, [7] * B))
    for name in ('speech', 'text', 'image'):
        for a, b in zip(got[name], want[name]):
            np.testing.assert_array_equal(a, b)
    fused, logits, aw, dw = got['fusion']
    wl, wp, wa, wd = want['fusion']
    np.testing.assert_array_equal(fused, wp.astype(np.float64))
    for a, b in ((logits, wl), (aw, wa), (dw, wd)):
        np.testing.assert_array_equal(a, b)


def test_check_repairs_a_mixed_batch(case, dev):
    """An fp32x3 range trip of the image handle on a mixed batch (the scaled conv of tests/test_gpu_x3_robust.py):
    check() re-runs the compact image rows on the fp32 twin and the fusion through forward_mixed with the stored
    plan, in place; the second batch runs on the widened handle."""
    from test_gpu_x3_robust import _w256
    (x, ids, mask, gray), ref = case
    ref = dict(ref, image=o_i.forward(_w256(), gray))
    args = [engine.to_device(a, dev) for a in (x, ids, mask, gray)]
    pipe = engine.FusedPipeline(seed=1234, device=dev, weights={'image': _w256()}, precision='fp32x3')
    for rnd in range(2):
        out = pipe.forward_mixed(*args, PRESENT)
        redo = pipe.check()
        assert redo == (['image'] if rnd == 0 else []), (rnd, redo)
        _check(out, ref)
    assert pipe.image.x3_reruns == 1
