"""GPU: fp32x3 image plane exponents calibrated from an observed batch (include/mec.h mec_model_x3_observe,
mec_model_x3_observed, mec_create_x3_calibrated; engine.ImageEncoder.calibrate).

1. The reduction (mec_absmax_f32, csrc/absmax.hip) is exact: it equals np.abs(x).max() bit for bit at sizes on
   both sides of every path (scalar head, 16-byte groups, scalar tail, more than one workgroup, past 2^24), from
   an unaligned pointer, for signed zeros and denormals, and reads +inf for an inf or a NaN wherever it stands.
2. Observation changes no output bit, and a slot keeps the running maximum across forwards.
3. The network of test_gpu_x3_robust.py (one conv weight x 256, BN untouched), which trips the default handle,
   runs on a calibrated handle with no trip, no re-run and no added headroom, at the project's fp32 bars
   (probs 1e-5, feature 1e-4 relative, argmax exact) against the oracle; so do the weight x 2^-8 (whose exponent
   goes up instead of down), the unedited weights, a MobileNetV2 with a project conv x 256, and the fused pipeline.
4. x3_widen keeps the calibration: every exponent exactly 8 lower.
"""
import ctypes

import numpy as np
import pytest
import torch

from mec import _lib, engine, synthetic as syn
from oracle import image as o_i, image_mbv2 as o_mb

pytestmark = pytest.mark.gpu

PROB_TOL, FEAT_RTOL = 1e-5, 1e-4
SCALED = 'base.layer2.1.conv2.weight'  # test_gpu_x3_robust.py's edit; its output is report line layer2.1.conv2
# MobileNetV2: features[17]'s project conv, the one block that always runs layered (its GEMM epilogue writes the
# planes). Its BN estimate gives s = 7; the x 256 outputs reach |x| ~ 1800, 3.5 times the planes' range there.
MB_SCALED = 'base.features.17.conv.2.weight'


def _edit(kind, name, f):
    w = dict(syn.weights(kind))
    w[name] = (np.asarray(w[name], np.float32) * np.float32(f)).astype(np.float32)
    return w


def _exps(report):
    return {ln.split()[0]: int(ln.split()[1][2:]) for ln in report.splitlines()[1:]}


def _bars(name, ref, feat, probs):
    rf, _, rp = ref
    feat, probs = feat.cpu().numpy(), probs.cpu().numpy()
    err = float(np.abs(probs - rp).max())
    ferr = float(np.abs(feat - rf).max() / np.abs(rf).max())
    print(f'{name}: probs max|d| {err:.3g}, feat rel err {ferr:.3g}')
    assert err <= PROB_TOL and ferr <= FEAT_RTOL and (probs.argmax(1) == rp.argmax(1)).all(), name


# ------------------------------------------------------------------ the reduction
def _absmax(t, n, offset=0):
    out = ctypes.c_float(-1.0)
    ptr = ctypes.c_void_p(t.data_ptr() + 4 * offset)
    _lib.check(_lib.load().mec_absmax_f32(ptr, n, ctypes.byref(out), engine._stream(t.device)), 'mec_absmax_f32')
    return np.float32(out.value)


def _same_bits(a, b):
    return np.float32(a).tobytes() == np.float32(b).tobytes()


def test_absmax_equals_numpy_exactly(dev):
    rng = np.random.default_rng(91)
    big = (rng.standard_normal((1 << 24) + 4, dtype=np.float32) * np.float32(37.0))
    big_d = engine.to_device(big, dev)
    for n in (1, 3, 255, 257, 4099, (1 << 24) + 3):
        for offset in (0, 1):  # 1: the pointer starts one float into the allocation (3 head floats before a boundary)
            got, want = _absmax(big_d, n, offset), np.abs(big[offset:offset + n]).max()
            assert _same_bits(got, want), (n, offset, got, want)
    # the largest magnitude is negative
    x = rng.standard_normal(4099, dtype=np.float32)
    for at in (0, 2048, 4098):
        y = x.copy()
        y[at] = -1e6
        assert _same_bits(_absmax(engine.to_device(y, dev), 4099), np.float32(1e6)), at
    # -0.0 only: |x| = +0.0
    z = np.full(259, -0.0, np.float32)
    assert _same_bits(_absmax(engine.to_device(z, dev), 259), np.float32(0.0))
    # denormals only (the comparison is on the bit patterns: nothing is flushed)
    bits = rng.integers(1, 1 << 23, 1027, dtype=np.uint32) | (rng.integers(0, 2, 1027, dtype=np.uint32) << 31)
    d = bits.view(np.float32)
    want = (bits & np.uint32(0x7fffffff)).max().reshape(1).view(np.float32)[0]
    assert 0 < want < np.finfo(np.float32).tiny and _same_bits(want, np.abs(d).max())
    assert _same_bits(_absmax(engine.to_device(d, dev), 1027), want)


@pytest.mark.parametrize('bad', [np.nan, np.inf, -np.inf], ids=['nan', 'inf', '-inf'])
def test_absmax_reads_inf_for_a_non_finite_value(dev, bad):
    """n = 4099 from an aligned pointer: 1024 16-byte groups and a 3-float scalar tail; one float in: a 3-float
    head, 1024 groups, no tail (n = 4099) or a 1-float tail (n = 4100)."""
    x = np.random.default_rng(92).standard_normal(4101, dtype=np.float32)
    for offset, n in ((0, 4099), (1, 4099), (1, 4100)):
        for at in (0, n // 2, n - 2, n - 1):  # first (the head, when there is one), a group, the tail, last
            y = x.copy()
            y[offset + at] = bad
            got = _absmax(engine.to_device(y, dev), n, offset)
            assert np.isposinf(got), (offset, n, at, got)


# ------------------------------------------------------------------ observation
@pytest.fixture(scope='module')
def enc32(dev):
    return engine.ImageEncoder(device=dev, precision='fp32')


def _observe(enc, batches):
    """Arm, run the batches, read -> (float32 [n], the last forward's outputs on the host)."""
    lib = enc.lib
    n = lib.mec_model_x3_observe(enc.handle, 1)
    assert n == 37, lib.mec_last_error()
    for g in batches:
        out = [t.cpu() for t in enc.forward(g)]
    seen = np.zeros(n, np.float32)
    assert lib.mec_model_x3_observed(enc.handle, seen.ctypes.data_as(_lib.c_fp), n) == n, lib.mec_last_error()
    assert lib.mec_model_x3_observe(enc.handle, 0) == n
    return seen, out


def test_observation_changes_no_output_bit(dev, enc32):
    g = engine.to_device(syn.image_inputs(3, seed=93), dev)
    off = [t.cpu() for t in enc32.forward(g)]
    seen, on = _observe(enc32, [g])
    again = [t.cpu() for t in enc32.forward(g)]  # disarmed again
    enc32.check()
    for i, (a, b, c) in enumerate(zip(off, on, again)):
        assert torch.equal(a, b) and torch.equal(a, c), f'output {i}'
    assert np.isfinite(seen).all() and (seen > 0).all(), seen
    names = enc32.x3_names()
    assert len(names) == 37 and names[0] == 'stem' and names[1] == 'layer1.out' and names[2] == 'layer1.0.conv1'
    assert names[-1] == 'layer4.2.conv2' and 'layer2.1.conv2' in names


def test_slots_keep_the_running_maximum(dev, enc32):
    a = engine.to_device(syn.image_inputs(3, seed=94), dev)
    b = engine.to_device(syn.image_inputs(3, seed=95), dev)
    sa, _ = _observe(enc32, [a])
    sb, _ = _observe(enc32, [b])  # arming again zeroes the slots
    sab, _ = _observe(enc32, [a, b])
    assert not np.array_equal(sa, sb)
    assert np.array_equal(sab, np.maximum(sa, sb)), (sab, sa, sb)


def test_observation_needs_an_armed_fp32_image_handle(dev):
    lib = _lib.load()
    out = np.zeros(64, np.float32)
    fresh = engine.ImageEncoder(device=dev, precision='fp32')
    assert lib.mec_model_x3_observed(fresh.handle, out.ctypes.data_as(_lib.c_fp), 64) == -1
    assert b'never armed' in lib.mec_last_error()
    assert lib.mec_model_x3_observe(fresh.handle, 1) == 37
    assert lib.mec_model_x3_observed(fresh.handle, out.ctypes.data_as(_lib.c_fp), 36) == -1
    assert b'tensor count' in lib.mec_last_error()
    assert lib.mec_model_x3_observed(fresh.handle, out.ctypes.data_as(_lib.c_fp), 64) == 37 and not out.any()
    for other in (engine.ImageEncoder(device=dev), engine.SpeechEncoder(device=dev)):  # f16 image; not an image kind
        assert lib.mec_model_x3_observe(other.handle, 1) == -1
        assert b'MEC_PREC_FP32 handle of kind MEC_IMAGE or MEC_IMAGE_MBV2' in lib.mec_last_error()
    with pytest.raises(ValueError, match='fp32x3'):
        fresh.calibrate(engine.to_device(syn.image_inputs(2, seed=96), dev))


# ------------------------------------------------------------------ calibrated handles
def _calibrated_run(enc, oracle, w, dev, seeds=(101, 102)):
    """Calibrate on one batch of 8, run a different batch of 16 checked -> the calibration's result."""
    cal = enc.calibrate(engine.to_device(syn.image_inputs(8, seed=seeds[0]), dev))
    gray = syn.image_inputs(16, seed=seeds[1])
    feat, _, probs = enc.checked('forward', engine.to_device(gray, dev))
    enc.check()  # clean
    assert enc.x3_reruns == 0, 'the calibrated handle tripped'
    head = enc.x3_report().splitlines()[0]
    assert 'x3_headroom=0' in head and 'x3_calibrated=1' in head, head
    _bars(f'{enc.kind} calibrated', oracle.forward(w, gray), feat, probs)
    assert {k: s for k, (_, s) in cal.items()} == _exps(enc.x3_report())
    return cal


def test_calibration_prevents_the_overflow_resnet50(dev):
    """Fails without the feature: the default handle trips on this network (test_gpu_x3_robust.py)."""
    w = _edit('image', SCALED, 256.0)
    enc = engine.ImageEncoder(w, device=dev, precision='fp32x3')
    default = _exps(enc.x3_report())
    cal = _calibrated_run(enc, o_i, w, dev)
    assert len(cal) == 37
    seen, s = cal['layer2.1.conv2']
    print(f'layer2.1.conv2: observed {seen:.6g}, s {default["layer2.1.conv2"]} -> {s}')
    assert s < default['layer2.1.conv2']
    assert f'layer2.1.conv2 s={s} bound={seen:.6g}' in enc.x3_report()  # bound= shows the observed value


def test_calibration_raises_a_small_tensors_exponent(dev):
    """The weight x 2^-8: the tensor sits far below its estimate, and its exponent goes up."""
    w = _edit('image', SCALED, 2.0 ** -8)
    enc = engine.ImageEncoder(w, device=dev, precision='fp32x3')
    default = _exps(enc.x3_report())
    cal = _calibrated_run(enc, o_i, w, dev, seeds=(103, 104))
    assert cal['layer2.1.conv2'][1] > default['layer2.1.conv2']


def test_unedited_weights_and_widening_keep_the_calibration(dev):
    w = syn.weights('image')
    enc = engine.ImageEncoder(w, device=dev, precision='fp32x3')
    cal = _calibrated_run(enc, o_i, w, dev, seeds=(105, 106))
    before = _exps(enc.x3_report())
    enc.x3_widen()
    rep = enc.x3_report()
    head = rep.splitlines()[0]
    assert 'x3_headroom=8' in head and 'x3_calibrated=1' in head, head
    after = _exps(rep)
    assert after.keys() == before.keys() and all(after[k] == before[k] - 8 for k in before), (before, after)
    for k, (seen, _) in cal.items():  # still the observed bounds
        assert f'{k} s={after[k]} bound={seen:.6g}' in rep, k


def test_calibration_prevents_the_overflow_mobilenet_v2(dev):
    w = _edit('image_mbv2', MB_SCALED, 256.0)
    enc = engine.MobileNetImageEncoder(w, device=dev, precision='fp32x3')
    enc.forward(engine.to_device(syn.image_inputs(4, seed=107), dev))
    torch.cuda.synchronize()
    with pytest.raises(_lib.X3RangeError, match='f16 hi / lo range'):  # the premise: the default handle trips
        enc.check()
    default = _exps(enc.x3_report())
    cal = _calibrated_run(enc, o_mb, w, dev, seeds=(108, 109))
    assert list(cal) == ['features1-1.out', 'features2-3.out', 'features4-6.out', 'features7-10.out',
                         'features11-13.out', 'features14-16.out', 'features17-17.out']
    assert cal['features17-17.out'][1] < default['features17-17.out']


def test_fused_pipeline_calibrate_image(dev):
    """As test_gpu_x3_robust.py's pipeline test, but calibrated: nothing is re-run."""
    from oracle import fusion as o_f, speech as o_s, text as o_t
    B = 8
    x = syn.speech_inputs(B, seed=65)
    ids, mask = syn.text_inputs(B, 128, seed=66, ragged=True)
    gray = syn.image_inputs(B, seed=67)
    w = {k: syn.weights(k) for k in ('speech', 'text', 'fusion')}
    w['image'] = _edit('image', SCALED, 256.0)
    sf, _, sp = o_s.forward(w['speech'], x)
    tf, _, tp = o_t.forward(w['text'], ids, mask)
    imf, _, ip = o_i.forward(w['image'], gray)
    _, fp, _, _ = o_f.forward(w['fusion'], sf, tf, imf, sp, tp, ip)
    args = [engine.to_device(a, dev) for a in (x, ids, mask, gray)]
    pipe = engine.FusedPipeline(seed=1234, device=dev, weights={'image': w['image']}, precision='fp32x3')
    pipe.forward(*args)  # (on the default handle: trips, and is not asked about)
    pipe.wait()
    assert pipe._tuned == {B}
    cal = pipe.calibrate_image(engine.to_device(syn.image_inputs(B, seed=110), dev))
    assert len(cal) == 37 and pipe._tuned == set() and pipe._tuned_mixed == set()  # the next batch tunes serially
    out = pipe.forward(*args)
    assert pipe._tuned == {B}
    assert pipe.check() == []
    assert pipe.image.x3_reruns == 0 and pipe.image.x3_headroom == 0
    for name, got, ref in (('image', out['image'][2], ip), ('fusion', out['fusion'][1], fp)):
        err = float(np.abs(got.cpu().numpy() - ref).max())
        print(f'FusedPipeline calibrated {name}: probs max|d| {err:.3g}')
        assert err <= PROB_TOL
