"""Host: mec_create_x3_calibrated (include/mec.h) rejects a bad calibration before any device call -- a kind
other than the two image kinds, a count that is not the kind's tensor count, a null pointer, a negative, NaN or
inf maximum -- each with -1 and a message that says what is wrong. The observation entry points reject a null
handle the same way. No GPU: a call that got as far as the device would fail with another message here."""
import ctypes

import numpy as np

from mec import _lib, synthetic as syn

IMAGE, MBV2 = syn.KIND_IDS['image'], syn.KIND_IDS['image_mbv2']
N_TENSORS = {IMAGE: 37, MBV2: 7}  # the lines of mec_model_x3_report after the first


def _create(kind, blob, absmax, count, out=True):
    lib = _lib.load()
    h = ctypes.c_void_p()
    bp = blob.ctypes.data_as(_lib.c_fp) if blob is not None else None
    ap = absmax.ctypes.data_as(_lib.c_fp) if absmax is not None else None
    rc = lib.mec_create_x3_calibrated(kind, bp, 0 if blob is None else blob.size, 0, b'', ap, count,
                                      ctypes.byref(h) if out else None)
    return rc, lib.mec_last_error(), h


def test_calibrated_creation_rejects_before_any_device_call():
    ok = {k: np.full(n, 3.0, np.float32) for k, n in N_TENSORS.items()}
    blob = {k: np.zeros(syn.blob_size(name), np.float32) for name, k in (('image', IMAGE), ('image_mbv2', MBV2))}
    small = np.zeros(8, np.float32)
    # a kind other than the two image kinds (text has rigorous bounds; speech has no fp32x3 path; 99 is no kind)
    for kind in (syn.KIND_IDS['text'], syn.KIND_IDS['speech'], syn.KIND_IDS['fusion'], 99, -1):
        rc, err, h = _create(kind, small, ok[IMAGE], 37)
        assert rc == -1 and b'MEC_IMAGE or MEC_IMAGE_MBV2' in err and not h.value, (kind, err)
    for kind in (IMAGE, MBV2):
        n = N_TENSORS[kind]
        for count in (0, n - 1, n + 1, N_TENSORS[MBV2 if kind == IMAGE else IMAGE]):
            rc, err, h = _create(kind, blob[kind], np.full(max(count, 1), 3.0, np.float32), count)
            assert rc == -1 and b'count is %d' % count in err and b'has %d tensors' % n in err and not h.value, err
        rc, err, h = _create(kind, blob[kind], None, n)
        assert rc == -1 and b'absmax is null' in err and not h.value, err
        rc, err, _ = _create(kind, blob[kind], ok[kind], n, out=False)
        assert rc == -1 and b'out is null' in err, err
        for at in (0, n // 2, n - 1):
            for bad in (-1.0, -0.0 - 1e-30, np.nan, np.inf, -np.inf):
                a = ok[kind].copy()
                a[at] = bad
                rc, err, h = _create(kind, blob[kind], a, n)
                assert rc == -1 and b'absmax[%d] is negative, NaN or inf' % at in err and not h.value, (at, bad, err)
        # the calibration is checked first: a wrong blob is then reported as mec_create_opt reports it, still
        # without a device call
        rc, err, h = _create(kind, small, ok[kind], n)
        assert rc == -1 and b'blob has 8 floats' in err and not h.value, err
        rc, err, h = _create(kind, None, ok[kind], n)
        assert rc == -1 and b'blob has 0 floats' in err and not h.value, err
    # the option list stays mec_create_opt's (integers only)
    lib = _lib.load()
    h = ctypes.c_void_p()
    b = blob[IMAGE]
    rc = lib.mec_create_x3_calibrated(IMAGE, b.ctypes.data_as(_lib.c_fp), b.size, 0, b'x3_headroom=1.5',
                                      ok[IMAGE].ctypes.data_as(_lib.c_fp), 37, ctypes.byref(h))
    assert rc == -1 and b'bad value' in lib.mec_last_error() and not h.value


def test_observation_entry_points_reject_a_null_handle():
    lib = _lib.load()
    out = np.zeros(37, np.float32)
    assert lib.mec_model_x3_observe(None, 1) == -1
    assert b'MEC_PREC_FP32 handle of kind MEC_IMAGE or MEC_IMAGE_MBV2' in lib.mec_last_error()
    assert lib.mec_model_x3_observed(None, out.ctypes.data_as(_lib.c_fp), 37) == -1
    assert b'MEC_PREC_FP32 handle of kind MEC_IMAGE or MEC_IMAGE_MBV2' in lib.mec_last_error()
    assert lib.mec_model_x3_names(None) is None
    assert b'null model handle' in lib.mec_last_error()


def test_absmax_argument_checks_without_a_launch():
    """n == 0 gives 0.0 with no launch (so no GPU is needed); n < 0 and a null result pointer are errors."""
    lib = _lib.load()
    out = ctypes.c_float(7.0)
    assert lib.mec_absmax_f32(None, 0, ctypes.byref(out), None) == 0 and out.value == 0.0
    assert lib.mec_absmax_f32(None, -1, ctypes.byref(out), None) == -1 and b'n < 0' in lib.mec_last_error()
    assert lib.mec_absmax_f32(None, 0, None, None) == -1 and b'out_host is null' in lib.mec_last_error()
