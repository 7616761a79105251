"""Paired fp32x3 planes (mec/x3pair.py, mec_gemm_f16x3_paired): a split tensor stored [rows][2K], each
32-element K chunk's hi halfs followed by its lo halfs, against the planar form on the same values.
Only addresses move, so every comparison is exact (torch.equal)."""
import ctypes

import pytest
import torch

from mec import _lib, x3pair

gpu = pytest.mark.gpu


# ------------------------------------------------------------------ host re-layout helper (no GPU)
def test_pair_round_trip_and_address_formula():
    rows, K = 5, 96
    g = torch.Generator().manual_seed(11)
    hi = torch.randn(rows, K, generator=g).half()
    lo = torch.randn(rows, K, generator=g).half()
    x = x3pair.pair(hi, lo)
    assert x.shape == (rows, 2 * K) and x.is_contiguous()
    flat = x.reshape(-1)
    seen = set()
    for r in range(rows):  # the address formula, element by element
        for k in range(K):
            for plane, src in ((0, hi), (1, lo)):
                i = r * 2 * K + (k // 32) * 64 + plane * 32 + (k % 32)
                assert x3pair.pair_index(r, k, K, plane) == i
                assert flat[i] == src[r, k]
                seen.add(i)
    assert len(seen) == rows * 2 * K  # a bijection onto the array
    h2, l2 = x3pair.unpair(x)
    assert torch.equal(h2, hi) and torch.equal(l2, lo)
    # one row's operands of one 32-deep K step: one aligned 128-byte line
    assert x3pair.pair_index(3, 64, K, 0) * 2 % 128 == 0
    assert x3pair.pair_index(3, 95, K, 1) - x3pair.pair_index(3, 64, K, 0) == 63
    with pytest.raises(ValueError):
        x3pair.pair(hi[:, :48], lo[:, :48])
    with pytest.raises(ValueError):
        x3pair.unpair(x[:, :96])


# ------------------------------------------------------------------ kernel level
def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _split(x):
    hi = x.half()
    return hi, (x - hi.float()).half()


M = 300  # a row tail on every tile (256- and 128-row tiles alike)
# every split tile the text path can launch: the pins (70256, 72128) and the autotuner's candidates
TILES = [70256, 70128, 71128, 71064, 70064, 72128]


@pytest.fixture(scope='module')
def operands(dev):
    """Planar and paired operands per (N, K), made once."""
    out = {}
    g = torch.Generator().manual_seed(29)
    for N in (256, 768):
        for K in (96, 768):
            a = torch.rand(M, K, generator=g) * 2 - 1
            b = (torch.rand(N, K, generator=g) * 2 - 1) * K ** -0.5
            (ah, al), (bh, bl) = _split(a), _split(b)
            out[N, K] = dict(
                A2=torch.stack((ah, al)).contiguous().to(dev), B2=torch.stack((bh, bl)).contiguous().to(dev),
                Ap=x3pair.pair(ah, al).to(dev), Bp=x3pair.pair(bh, bl).to(dev),
                bias=torch.randn(N, generator=g).to(dev), R=torch.randn(M, N, generator=g).to(dev))
    return out


@gpu
@pytest.mark.parametrize('K', [96, 768])
@pytest.mark.parametrize('N', [256, 768])
@pytest.mark.parametrize('tile', TILES)
def test_paired_gemm_same_bits_as_planar(dev, operands, tile, N, K):
    """mec_gemm_f16x3_paired against mec_gemm_f16x3 at one forced tile: bias + f32 residual -> f32 out;
    bias -> hi / lo out, paired (un-paired on the host) and planar."""
    lib = _lib.load()
    o = operands[N, K]
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    c32 = [torch.full((M, N), float('nan'), device=dev) for _ in range(2)]
    c16 = [torch.zeros(2, M, N, dtype=torch.float16, device=dev) for _ in range(2)]
    c16p = torch.zeros(M, 2 * N, dtype=torch.float16, device=dev)
    _lib.check(lib.mec_set_option(b'gemm_bn', tile), 'gemm_bn')
    try:
        _lib.check(lib.mec_gemm_f16x3(_p(o['A2']), M * K, _p(o['B2']), N * K, 0.5, _p(o['bias']), _p(o['R']), None, 0,
                                      _p(c32[0]), M, N, K, 0, st), 'planar f32')
        _lib.check(lib.mec_gemm_f16x3_paired(_p(o['Ap']), _p(o['Bp']), 0.5, _p(o['bias']), _p(o['R']), None, 0, 0,
                                             _p(c32[1]), M, N, K, 0, st), 'paired f32')
        _lib.check(lib.mec_gemm_f16x3(_p(o['A2']), M * K, _p(o['B2']), N * K, 1.0, _p(o['bias']), None, _p(c16[0]),
                                      M * N, None, M, N, K, 1, st), 'planar planes')
        _lib.check(lib.mec_gemm_f16x3_paired(_p(o['Ap']), _p(o['Bp']), 1.0, _p(o['bias']), None, _p(c16p), 1, 0,
                                             None, M, N, K, 1, st), 'paired planes')
        _lib.check(lib.mec_gemm_f16x3_paired(_p(o['Ap']), _p(o['Bp']), 1.0, _p(o['bias']), None, _p(c16[1]), 0, M * N,
                                             None, M, N, K, 1, st), 'paired operands, planar planes')
    finally:
        lib.mec_set_option(b'gemm_bn', 0)
    torch.cuda.synchronize()
    assert not torch.isnan(c32[0]).any()
    assert torch.equal(c32[0], c32[1])
    assert c16[0][1].abs().max() > 0  # the lo plane carries something
    hi, lo = x3pair.unpair(c16p)
    assert torch.equal(hi, c16[0][0]) and torch.equal(lo, c16[0][1])
    assert torch.equal(c16[1], c16[0])


@gpu
def test_paired_gemm_rejects_what_it_does_not_serve(dev):
    """The paired entry serves the K-interleaved term order only, and a planar C16 needs c_lo."""
    lib = _lib.load()
    x = torch.zeros(64, 128, dtype=torch.float16, device=dev)
    c = torch.zeros(2, 64, 64, dtype=torch.float16, device=dev)
    assert lib.mec_gemm_f16x3_paired(_p(x), _p(x), 1.0, None, None, _p(c), 0, 0, None, 64, 64, 64, 0, None) == -1
    assert b'c_lo' in lib.mec_last_error()
    _lib.check(lib.mec_set_option(b'gemm_x3_order', 0), 'gemm_x3_order')
    try:
        assert lib.mec_gemm_f16x3_paired(_p(x), _p(x), 1.0, None, None, _p(c), 1, 0, None, 64, 64, 64, 0, None) == -1
        assert b'K-interleaved' in lib.mec_last_error()
    finally:
        lib.mec_set_option(b'gemm_x3_order', 1)


# ------------------------------------------------------------------ text model
@pytest.fixture(scope='module')
def encoders(dev):
    """The fp32x3 text model from the same blob, planes planar (x3_layout 0) and paired (1)."""
    from mec import engine
    return {v: engine.TextEncoder(device=dev, precision='fp32x3', opts={'x3_layout': v}) for v in (0, 1)}


@gpu
@pytest.mark.parametrize('form', ['padded', 'packed'])
@pytest.mark.parametrize('B', [1, 3, 24])
def test_text_model_paired_same_bits_as_planar(dev, encoders, B, form):
    """feat, logits and probs of the two layouts, ragged masks (mid-batch short rows), padded and packed
    forwards, the full and the [CLS]-only last layer, one and two heads per fused QKV + attention workgroup."""
    from mec import engine, synthetic as syn
    ids, mask = syn.text_inputs(B, 128, seed=40 + B, ragged=True)
    args = (engine.to_device(ids, dev), engine.to_device(mask, dev))
    try:
        for cls_last in (0, 1):
            for heads in (1, 2):
                outs = {}
                for v, enc in encoders.items():
                    enc.set_option('bert_cls_last', cls_last)
                    enc.set_option('bert_qkv_attn_x3_heads', heads)
                    r = enc.forward(*args) if form == 'padded' else enc.forward_packed(*args)
                    outs[v] = [t.cpu() for t in r]
                    enc.check()
                for name, a, b in zip(('feat', 'logits', 'probs'), outs[0], outs[1]):
                    assert torch.isfinite(a).all()
                    assert torch.equal(a, b), f'{name} cls_last={cls_last} heads={heads}: max |d| {float((a - b).abs().max())}'
    finally:
        for enc in encoders.values():
            enc.set_option('bert_cls_last', 1)
            enc.set_option('bert_qkv_attn_x3_heads', 1)


@gpu
def test_text_model_paired_unfused_attention_same_bits(dev, encoders):
    """The split QKV GEMM + bert_attention_x3_kernel pair (bert_qkv_attn 0) reads and writes paired planes too."""
    from mec import engine, synthetic as syn
    ids, mask = syn.text_inputs(3, 128, seed=47, ragged=True)
    args = (engine.to_device(ids, dev), engine.to_device(mask, dev))
    outs = {}
    try:
        for v, enc in encoders.items():
            enc.set_option('bert_qkv_attn', 0)
            outs[v] = [t.cpu() for t in enc.forward(*args)]
            enc.check()
    finally:
        for enc in encoders.values():
            enc.set_option('bert_qkv_attn', 1)
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(a, b)


@gpu
def test_x3_layout_is_a_creation_time_option(dev, encoders):
    with pytest.raises(_lib.MecError, match='creation-time'):
        encoders[1].set_option('x3_layout', 0)
    with pytest.raises(_lib.MecError, match='paired'):
        encoders[1].set_option('gemm_x3_order', 0)  # the pass-major order reads planar planes only
    encoders[0].set_option('gemm_x3_order', 0)
    encoders[0].set_option('gemm_x3_order', 1)


@gpu
@pytest.mark.parametrize('layout', [0, 1])
def test_range_trip_raised_under_both_layouts(dev, layout):
    """An inf in FFN1's weight leaves the f16 range in the FFN1 epilogue's planes: check() raises, then clears."""
    import numpy as np
    from mec import engine, synthetic as syn
    w = dict(syn.weights('text'))
    a = np.array(w['bert.encoder.layer.0.intermediate.dense.weight'], np.float32)
    a.flat[0] = np.inf
    w['bert.encoder.layer.0.intermediate.dense.weight'] = a
    ids, mask = syn.text_inputs(4, 128, seed=3, ragged=True)
    enc = engine.TextEncoder(w, device=dev, precision='fp32x3', opts={'x3_layout': layout})
    enc.check()
    enc.forward(engine.to_device(ids, dev), engine.to_device(mask, dev))
    torch.cuda.synchronize()
    with pytest.raises(_lib.MecError, match='f16 hi / lo range'):
        enc.check()
    enc.check()
