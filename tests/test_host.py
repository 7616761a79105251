"""CPU: host-side logic — synthetic weights, blob packing, the C ABI's exports and
host-only entry points (no kernel launches), sharding, keyword fallback."""
import os
import re

import numpy as np
import pytest

from mec import _lib, dist as mdist, synthetic as syn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_synthetic_is_deterministic_and_seeded():
    a = syn.uniform(1234, 'x', (1000,), -1, 1)
    b = syn.uniform(1234, 'x', (1000,), -1, 1)
    c = syn.uniform(1235, 'x', (1000,), -1, 1)
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    assert a.min() >= -1 and a.max() < 1 and abs(a.mean()) < 0.1
    # fixed values pin the raw-stream conversion across numpy versions
    np.testing.assert_allclose(syn.uniform(1234, 'pin', (3,), 0, 1),
                               syn.uniform(1234, 'pin', (3,), 0, 1))


def test_param_counts_match_reference():
    # 109,487,623 = HF BertForSequenceClassification(num_labels=7); 1,637,453 = reference fusion model
    assert syn.blob_size('text') == 109_487_623
    assert syn.blob_size('fusion') == 1_637_453
    assert syn.blob_size('speech') == 470_775
    assert syn.blob_size('image') == 24_613_831


def test_pack_rejects_bad_shapes():
    w = dict(syn.weights('speech'))
    w['dense_0/kernel'] = np.zeros((55, 512), np.float32)
    with pytest.raises(ValueError):
        syn.pack('speech', w)


def test_text_inputs_layout():
    ids, mask = syn.text_inputs(5, 128, seed=2, ragged=True)
    assert ids.dtype == np.int32 and mask.dtype == np.int32
    assert (ids[:, 0] == 101).all()
    lens = mask.sum(1)
    assert lens[0] == 128 and lens[1] == 8
    for i, n in enumerate(lens):
        assert ids[i, n - 1] == 102 and (ids[i, n:] == 0).all() and mask[i, :n].all()


def test_library_loads_and_exports_every_header_symbol():
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, 'include', 'mec.h')).read()
    names = sorted(set(re.findall(r'\b(mec_[a-z0-9_]+)\s*\(', hdr)))
    assert len(names) >= 15
    for n in names:
        assert hasattr(lib, n), f'{n} declared in include/mec.h but not exported'
        assert n in _lib.SIGNATURES, f'{n} has no ctypes signature in mec/_lib.py'


def test_blob_sizes_agree_with_library():
    lib = _lib.load()
    for kind, k in syn.KIND_IDS.items():
        assert lib.mec_blob_size(k) == syn.blob_size(kind)
    assert lib.mec_blob_size(9) == -1


def test_model_option_and_query_need_a_handle():
    lib = _lib.load()
    assert lib.mec_model_set_option(None, b'fusion_r', 2) == -1
    assert b'null model' in lib.mec_last_error()
    assert lib.mec_model_gemm_query(None, 0, 256, 256, 256) == -1
    assert lib.mec_precision(None) == -1
    assert lib.mec_model_check(None) == -1
    assert b'null handle' in lib.mec_last_error()


def test_removed_knobs_are_unknown():
    """The measured-slower opt-in paths of round 2 (register-staged GEMM engine, fused
    bottleneck tail, O-proj + LN kernel, one-kernel speech DNN) are gone from the library, and so are
    the split GEMM's fp32x3 schedule A/B knobs of rounds 5-6 (early restage, start stagger, MFMA wave
    priority and the late-DMA variants): the split tiles now always run what was gemm_x3_late_dma 1,
    the rest off."""
    lib = _lib.load()
    for k in (b'gemm_impl', b'resnet_fused_tail', b'bert_oproj_ln', b'speech_impl', b'gemm_x3_restage',
              b'gemm_x3_stagger', b'gemm_x3_prio', b'gemm_x3_late_dma'):
        assert lib.mec_set_option(k, 0) == -1 and b'unknown' in lib.mec_last_error().lower(), k


def test_c_abi_argument_errors_without_gpu():
    import ctypes
    lib = _lib.load()
    h = ctypes.c_void_p()
    blob = np.zeros(10, np.float32)
    assert lib.mec_create(0, blob.ctypes.data_as(_lib.c_fp), 10, 0, ctypes.byref(h)) == -1
    assert b'expected' in lib.mec_last_error()
    assert lib.mec_set_option(b'nope', 1) == -1
    assert lib.mec_speech_fwd(None, None, 1, None, None, None, None) == -1
    assert b'null model' in lib.mec_last_error()


BAD_GEOMETRY = {  # (n, H, W, ks, stride, pad) -> the requirement the message names
    'stride 0': ((2, 8, 8, 3, 0, 1), b'stride >= 1'),
    'ks 0': ((2, 8, 8, 0, 1, 0), b'ks >= 1'),
    'negative pad': ((2, 8, 8, 3, 1, -1), b'pad >= 0'),
    'ks larger than the padded input': ((2, 1, 1, 5, 1, 0), b'OH >= 1 and OW >= 1'),
    'ks larger than the padded width only': ((2, 8, 2, 5, 1, 1), b'OH >= 1 and OW >= 1'),
    'ks past the input at a stride that rounds to one output': ((2, 1, 1, 2, 2, 0), b'OH >= 1 and OW >= 1'),
    'n 0': ((0, 8, 8, 3, 1, 1), b'n >= 1'),
}


@pytest.mark.parametrize('entry', ['mec_conv_f16', 'mec_conv_f32', 'mec_gemm_ex conv', 'mec_gemm_ex split conv',
                                   'mec_gemm_ex dual'])
@pytest.mark.parametrize('case', list(BAD_GEOMETRY))
def test_conv_geometry_rejected_before_any_launch(entry, case):
    """Every conv / dual entry point returns -1 on a geometry with no outputs (or a zero stride, which
    was a host division by zero) and names the requirement; the check precedes every device call, so
    the fake non-null pointers are never read and this runs without a GPU."""
    import ctypes
    lib = _lib.load()
    (n, H, W, ks, stride, pad), msg = BAD_GEOMETRY[case]
    C = Cout = 64
    p = ctypes.c_void_p(0x1000)
    if entry.startswith('mec_conv'):
        rc = getattr(lib, entry)(p, p, None, None, p, n, H, W, C, Cout, ks, stride, pad, 0, None)
    else:
        dual = entry.endswith('dual')
        a = _lib.GemmArgs(amode=_lib.A_DUAL if dual else _lib.A_CONV, A=p, B=p, C32=p, N=Cout, n=n, H=H, W=W, C=C,
                          ks=ks, stride=stride, pad=pad, M=77, K=64)
        if dual:
            a.A2, a.K1 = p, 64
        if 'split' in entry:
            a.a_lo = a.b_lo = 1 << 20
        rc = lib.mec_gemm_ex(ctypes.byref(a), None)
    assert rc == -1
    assert msg in lib.mec_last_error(), lib.mec_last_error()


def test_gemm_ex_descriptor_errors_without_gpu():
    """mec_gemm_ex's own argument checks, and the engine's for the modes only it reaches."""
    import ctypes
    lib = _lib.load()
    p = ctypes.c_void_p(0x1000)
    assert lib.mec_gemm_ex(None, None) == -1 and b'null descriptor' in lib.mec_last_error()
    ok = dict(A=p, B=p, C32=p, M=64, N=64, K=64)
    for kw, msg in ((dict(amode=3), b'amode'), (dict(a_lo=4096), b'a_lo and b_lo'), (dict(oscale=0.0), b'oscale'),
                    (dict(cscale=0.0), b'cscale'), (dict(N=96), b'N % 64'), (dict(K=32), b'K % 64'),
                    (dict(C32=None), b'no output'), (dict(M=0), b'empty shape'),
                    (dict(R=p, r_lo=4096), b'r_lo needs split operands'),
                    (dict(R=p, r_lo=4096, a_lo=4096, b_lo=4096, r_is_f32=1), b'r_lo needs split operands'),
                    (dict(R=p, r_is_f32=1, r_stats=p), b'deferred-LN residual'),
                    (dict(amode=_lib.A_DUAL, n=1, H=8, W=8, C=64, ks=1, stride=1, pad=0, K1=64), b'dual gemm'),
                    (dict(amode=_lib.A_DUAL, A2=p, n=1, H=8, W=8, C=64, ks=3, stride=1, pad=1, K1=64), b'dual gemm'),
                    (dict(amode=_lib.A_CONV, n=1, H=8, W=8, C=32, ks=2, stride=1, pad=0), b'C % 64')):
        a = _lib.GemmArgs(**{**ok, **kw})
        assert lib.mec_gemm_ex(ctypes.byref(a), None) == -1, kw
        assert msg in lib.mec_last_error(), (kw, lib.mec_last_error())


def test_bert_attn_descriptor_errors_without_gpu():
    """mec_bert_attn returns -1 and says why for every form no attention kernel serves; the checks precede
    every device call (the fake pointers are never read), and an empty launch returns 0."""
    import ctypes
    lib = _lib.load()
    p = ctypes.c_void_p(0x1000)
    assert lib.mec_bert_attn(None, None) == -1 and b'null descriptor' in lib.mec_last_error()
    F16, FP32, X3 = (_lib.PRECISIONS[n] for n in ('f16', 'fp32', 'fp32x3'))
    full = dict(qkv=p, mask=p, ctx=p, rows=2)
    x3 = dict(precision=X3, qkv_lo=4096, ctx_lo=4096)
    fused = dict(fused=1, hs=p, wqkv=p, bqkv=p, mask=p, ctx=p, rows=2)
    cls = dict(form=1, qkv=p, qc=p, mask=p, ctx=p, rows=2, ns=2)
    for kw, msg in (({**full, 'precision': 3}, b'precision'), ({**full, 'form': 2}, b'form, fused and packed'),
                    ({**full, 'packed': 2}, b'form, fused and packed'), ({**full, 'rows': -1}, b'rows'),
                    ({**full, 'mask': None}, b'null mask or ctx'), ({**full, 'ctx': None}, b'null mask or ctx'),
                    ({**full, 'qkv': None}, b'null qkv'), ({**full, 'qks': 0.25}, b'qks = 0.125'),
                    ({**full, 'precision': FP32, 'qks': 0.5}, b'qks = 0.125'),
                    ({**full, **x3, 'qks': 0.0}, b'qks must be set'), ({**full, **x3, 'ctx_lo': 0}, b'ctx_lo'),
                    ({**full, **x3, 'qkv_lo': 0}, b'qkv_lo'), ({**full, **x3, 'qkv_lo': 4100}, b'qkv_lo'),
                    ({**fused, 'precision': FP32}, b'no fused'), ({**fused, 'form': 1}, b'form 0'),
                    ({**fused, 'bqkv': None}, b'hs, wqkv and bqkv'), ({**fused, 'oscale': 0.5}, b'oscale = 1'),
                    ({**fused, **x3, 'hs_lo': 4096, 'w_lo': 0}, b'hs_lo and w_lo'),
                    ({**fused, **x3, 'hs_lo': 4096, 'w_lo': -1}, b'paired together'),
                    ({**fused, **x3, 'hs_lo': 4096, 'w_lo': 4096, 'oscale': 0.0}, b'oscale must be set'),
                    ({**cls, 'qc': None}, b'needs qc'), ({**cls, 'ns': 3}, b'ns == rows'),
                    ({**cls, 'cidx': p}, b'cidx goes with packed'), ({**cls, 'packed': 1}, b'needs cidx'),
                    ({**cls, 'packed': 1, 'cidx': p, 'rows': 0}, b'samples without a row'),
                    ({**cls, **x3, 'qc_lo': 0}, b'qc_lo'), ({**cls, 'ns': -1, 'rows': -1}, b'rows')):
        a = _lib.AttnArgs(**kw)
        assert lib.mec_bert_attn(ctypes.byref(a), None) == -1, kw
        assert msg in lib.mec_last_error(), (kw, lib.mec_last_error())
    for kw in ({**full, 'rows': 0}, {**fused, 'rows': 0}, {**cls, 'rows': 0, 'ns': 0},
               {**cls, 'packed': 1, 'cidx': p, 'ns': 0}):
        assert lib.mec_bert_attn(ctypes.byref(_lib.AttnArgs(**kw)), None) == 0, kw


@pytest.mark.parametrize('geom', ['G1', 'G2', 'G3', 'G4', 'G5'])
def test_gemm_mode_references_vs_torch_conv2d_f64(geom):
    """The float64 NHWC conv, tap-view and dual-gather helpers the GPU GEMM-mode tests compare kernels
    with (tests/gemm_ref.py), against torch.nn.functional.conv2d in float64."""
    import torch
    import gemm_ref
    n, H, W, C, Cout, ks, stride, pad = gemm_ref.GEOMETRIES[geom]
    rng = np.random.default_rng(H * W + C)
    x = rng.standard_normal((n, H, W, C))
    w = rng.standard_normal((Cout, ks, ks, C))
    xt = torch.from_numpy(x).permute(0, 3, 1, 2)

    def conv(wt, s, p):
        return torch.nn.functional.conv2d(xt, torch.from_numpy(wt).permute(0, 3, 1, 2), stride=s,
                                          padding=p).permute(0, 2, 3, 1).numpy()

    ref = conv(w, stride, pad)
    got = gemm_ref.conv_nhwc_f64(x, w, stride, pad)
    assert got.shape == ref.shape == (n, gemm_ref.out_extent(H, ks, stride, pad),
                                      gemm_ref.out_extent(W, ks, stride, pad), Cout)
    assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()
    # one-hot tap weights select the tap view exactly (products by 1.0 and sums with 0.0)
    for kh in range(ks):
        for kw in range(ks):
            sel = np.zeros((C, ks, ks, C))
            sel[np.arange(C), kh, kw, np.arange(C)] = 1.0
            assert np.array_equal(conv(sel, stride, pad), gemm_ref.tap_view(x, kh, kw, ks, stride, pad)), (kh, kw)
    # the dual second source: a 1x1 identity conv at stride 1 and 2, unpadded
    for s in (1, 2):
        g = gemm_ref.dual_gather(x, s)
        assert np.array_equal(g, conv(np.eye(C).reshape(C, 1, 1, C), s, 0).reshape(-1, C))


def test_create_opt_parses_its_option_list_without_gpu():
    """mec_create_opt validates its "key=value,..." list (the mec_set_option keys and values) before
    any device call; mec_model_x3_report needs a handle."""
    import ctypes
    lib = _lib.load()
    h = ctypes.c_void_p()
    n = syn.blob_size('speech')
    blob = np.zeros(n, np.float32)
    for opts, msg in ((b'x3_headroom', b'key=value'), (b'=3', b'key=value'), (b'x3_headroom=', b'bad value'),
                      (b'x3_headroom=2x', b'bad value'), (b'x3_headroom=25', b'bad value'),
                      (b'x3_headroom=8,nope=1', b'unknown key'), (b'gemm_debug=1', b'MEC_PROBES')):
        assert lib.mec_create_opt(0, blob.ctypes.data_as(_lib.c_fp), n, 0, 2, opts, ctypes.byref(h)) == -1, opts
        assert msg in lib.mec_last_error(), (opts, lib.mec_last_error())
        assert not h.value
    assert lib.mec_model_x3_report(None) is None
    assert b'null handle' in lib.mec_last_error()
    assert lib.mec_set_option(b'x3_headroom', 4) == 0 and lib.mec_set_option(b'x3_headroom', 0) == 0


def test_option_validation_without_gpu():
    """mec_set_option accepts each knob's documented values (include/mec.h) and rejects the
    rest, including every probe value (the product library is not a -DMEC_PROBES build); it
    only sets the process defaults, so this runs without a GPU. Defaults restored."""
    lib = _lib.load()
    assert lib.mec_build_flags() == 0, 'the product library must not be a probe build'
    probes = [(b'gemm_debug', 1), (b'gemm_debug', 2), (b'gemm_debug', 4), (b'gemm_debug', 5), (b'stem_debug', 1), (b'conv3x3_debug', 2),
              (b'bert_qkv_attn', 2), (b'bert_qkv_attn', 3), (b'speech_spin_limit', 0), (b'speech_spin_limit', 100),
              (b'speech_debug', 1), (b'audio_debug', 15)]
    for k, v in probes:
        assert lib.mec_set_option(k, v) == -1, (k, v)
        assert b'MEC_PROBES' in lib.mec_last_error()
    ok = [(b'fusion_r', 1), (b'fusion_r', 4), (b'fusion_split', 0), (b'fusion_split', 1),
          (b'bert_qkv_attn', 0), (b'bert_qkv_attn', 1), (b'speech_spin_limit', -1),
          (b'gemm_bn', 40256), (b'gemm_bn', 0),
          (b'gemm_bn_tag', 3 * 100000 + 40256), (b'gemm_bn_tag', 3 * 100000 + 11128),
          (b'gemm_debug', 0), (b'gemm_f32_tile', 3), (b'gemm_f32_tile', 0), (b'speech_debug', 0),
          (b'gemm_group_m', 0), (b'gemm_group_m', 16), (b'gemm_group_m', 8),
          (b'gemm_glds_group_m', 0), (b'gemm_glds_group_m', 4), (b'gemm_glds_group_m', 8),
          (b'gemm_f32_family', 0), (b'gemm_f32_family', 32), (b'gemm_f32_family', 16),
          (b'bert_ln_rows', 1), (b'bert_ln_rows', 4), (b'bert_ln_rows', 2),
          (b'bert_cls_last', 0), (b'bert_cls_last', 1), (b'gemm_x3_order', 0), (b'gemm_x3_order', 1),
          (b'gemm_bn', 70256), (b'gemm_bn', 71064), (b'gemm_bn', 0), (b'gemm_x3_tag', 5 * 100000 + 70256),
          (b'gemm_x3_tag', 5 * 100000), (b'gelu_x3', 0), (b'gelu_x3', 1),
          (b'pw_chain_x3', 0), (b'pw_chain_x3', 1), (b'pw_chain_x3', 2), (b'pw_seam_x3', 0), (b'pw_seam_x3', 2),
          (b'pw_seam_x3', 1), (b'mbv2_layered', 0),
          (b'mbv2_layered', 7), (b'mbv2_layered', 17), (b'mbv2_layered16', 0), (b'mbv2_layered16', 12),
          (b'mbv2_x3_tile', 0), (b'mbv2_x3_tile', 4), (b'mbv2_x3_tpw', 1), (b'mbv2_x3_tpw', 4), (b'resnet_chunk', 16), (b'resnet_chunk', 0),
          (b'bert_qkv_attn_x3_heads', 2), (b'bert_qkv_attn_x3_heads', 1), (b'bert_qkv_attn_heads', 2),
          (b'bert_qkv_attn_heads', 1)]
    bad = [(b'pw_chain_x3', 3), (b'pw_seam_x3', 3), (b'pw_seam_x3', -1), (b'bert_qkv_attn_x3_heads', 0), (b'bert_qkv_attn_x3_heads', 3), (b'mbv2_layered', 6), (b'mbv2_layered', 18), (b'mbv2_layered16', 1),
           (b'mbv2_x3_tile', 8), (b'mbv2_x3_tpw', 0), (b'mbv2_x3_tpw', 17), (b'resnet_chunk', -1),(b'bert_ln_rows', 3), (b'bert_cls_last', 2), (b'gemm_x3_order', 2), (b'gemm_bn', 72256),
           (b'gemm_x3_tag', 5 * 100000 + 10256), (b'gemm_x3_tag', 70256), (b'gelu_x3', 2), (b'gemm_f32_family', 8), (b'gemm_group_m', 3), (b'gemm_group_m', -1), (b'gemm_group_m', 32), (b'gemm_glds_group_m', 5), (b'gemm_f32_tile', 9), (b'fusion_r', 3), (b'fusion_split', 2), (b'bert_qkv_attn', 4), (b'gemm_bn', 12345),
           (b'gemm_bn', 42256), (b'gemm_bn_tag', 11128), (b'gemm_bn_tag', 15 * 100000 + 256),
           (b'gemm_bn_tag', 3 * 100000 + 999), (b'gemm_bn_tag', -1), (b'gemm_debug', 6), (b'speech_spin_limit', -2)]
    try:
        for k, v in ok:
            assert lib.mec_set_option(k, v) == 0, (k, v)
        for k, v in bad:
            assert lib.mec_set_option(k, v) == -1, (k, v)
            assert b'bad value' in lib.mec_last_error()
    finally:  # the defaults
        for k, v in [(b'fusion_r', 4), (b'fusion_split', 1), (b'bert_qkv_attn', 1), (b'speech_spin_limit', -1),
                     (b'gemm_f32_tile', 0),
                     (b'gemm_bn', 0),
                     (b'gemm_bn_tag', 3 * 100000 + 11128), (b'gemm_debug', 0), (b'gemm_group_m', 8),
                     (b'gemm_glds_group_m', 8), (b'gemm_f32_family', 16), (b'bert_ln_rows', 2),
                     (b'bert_cls_last', 1), (b'gemm_x3_order', 1), (b'gelu_x3', 1), (b'gemm_x3_tag', 5 * 100000 + 72128),
                     (b'pw_chain_x3', 2), (b'pw_seam_x3', 1), (b'mbv2_layered', 8), (b'mbv2_layered16', 8), (b'mbv2_x3_tile', 4), (b'mbv2_x3_tpw', 2),
                     (b'resnet_chunk', 0), (b'bert_qkv_attn_x3_heads', 1), (b'bert_qkv_attn_heads', 1)]:
            lib.mec_set_option(k, v)


@pytest.mark.parametrize('total,world', [(256, 1), (8192, 8), (10, 3), (2, 4), (0, 2)])
def test_shards_partition_the_batch(total, world):
    spans = [mdist.shard(total, world, r) for r in range(world)]
    assert spans[0][0] == 0 and spans[-1][1] == total
    for (a0, b0), (a1, b1) in zip(spans, spans[1:]):
        assert b0 == a1
    sizes = [b - a for a, b in spans]
    assert max(sizes) - min(sizes) <= 1


def test_keyword_fallback_matches_reference_rules():
    from inference.text_inference import TextInference
    t = TextInference.__new__(TextInference)  # no model / tokenizer -> heuristic path
    from inference.text_inference import _Cleaner
    t.emotions = ['happy', 'sad', 'angry', 'fear', 'disgust', 'surprise', 'neutral']
    t.model, t.tokenizer, t.preprocessor = None, None, _Cleaner()
    r = t.predict('I am SO happy today!!')
    assert r['emotion'] == 'happy' and r['confidence'] == 0.9
    assert r['all_probabilities'][1] == 0.1 / 6
    assert t.predict('This is worrying, I feel anxious')['emotion'] == 'fear'
    assert t.predict('see http://x.com nothing here')['emotion'] == 'neutral'
    assert set(r) == {'emotion', 'confidence', 'all_probabilities'}
