"""gemm_x3_pp: tile 70256 on paired fp32x3 planes under the ping-pong schedule (gemm_pp_kernel SP = 3)
against the two-stage ring (gemm_x3_pp 0) on the same operands. The kernel-level tests set gemm_x3_pp 2,
which runs every launch on the new schedule (1, the default, leaves launches with an activation on the
ring); the model-level test compares 1 and 2 against 0. The schedule moves loads, barriers and
fragment reads, never a term of a sum, so every comparison is exact (torch.equal); outputs are pre-filled
with NaN and carry guard rows past M that must keep it.

Shapes (the smallest at which this pipeline can go wrong): K = 32 / 64 are one and two K tiles (the
prologue's branch and the issue guards decide everything), 96 / 128 the drains after three and four,
768 steady state; M = 1 a tile that is all tail, 127 / 300 a tail inside the first / second wave row,
256 exact, 513 three panels with one row in the last; N = 256 / 768 one and three column tiles."""
import ctypes

import pytest
import torch

from mec import _lib, x3pair

gpu = pytest.mark.gpu

TILE = 70256
PP_DEFAULT = 1  # csrc/mec_common.h Options::gemm_x3_pp
PP_ALL = 2      # every paired launch of the tile on the ping-pong schedule
KS, MS = (32, 64, 96, 128, 768), (1, 127, 256, 300, 513)
MMAX, NMAX, GUARD = 513, 768, 3
# (K, M, N) corners for the output forms b - d
CORNERS = [(32, 1, 256), (32, 513, 768), (64, 127, 256), (96, 300, 768), (128, 256, 256), (768, 513, 768),
           (768, 1, 256)]


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _split(x):
    hi = x.half()
    return hi, (x - hi.float()).half()


def _st(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


class _Knobs:
    """gemm_bn forced to the tile and gemm_x3_pp set, process-wide (the kernel-level entries carry no handle)."""

    def __init__(self, lib, pp):
        self.lib, self.pp = lib, pp

    def __enter__(self):
        _lib.check(self.lib.mec_set_option(b'gemm_bn', TILE), 'gemm_bn')
        _lib.check(self.lib.mec_set_option(b'gemm_x3_pp', self.pp), 'gemm_x3_pp')

    def __exit__(self, *exc):
        self.lib.mec_set_option(b'gemm_bn', 0)
        self.lib.mec_set_option(b'gemm_x3_pp', PP_DEFAULT)


@pytest.fixture(scope='module')
def operands(dev):
    """Per K: planar and paired operands for the largest M and N (a smaller case takes the leading rows of
    each, which both layouts keep contiguous), bias, residual, LayerNorm inputs. Made once, never written."""
    out = {}
    g = torch.Generator().manual_seed(61)
    for K in KS:
        a = torch.rand(MMAX, K, generator=g) * 2 - 1
        b = (torch.rand(NMAX, K, generator=g) * 2 - 1) * K ** -0.5
        (ah, al), (bh, bl) = _split(a), _split(b)
        R = torch.randn(MMAX, NMAX, generator=g)
        mean = R.double().mean(1)
        rstd = (R.double().var(1, unbiased=False) + 1e-12).rsqrt()
        out[K] = dict(
            ah=ah.to(dev), al=al.to(dev), bh=bh.to(dev), bl=bl.to(dev),
            Ap=x3pair.pair(ah, al).to(dev), Bp=x3pair.pair(bh, bl).to(dev),
            bias=torch.randn(NMAX, generator=g).to(dev), R=R.to(dev),
            stats=torch.stack((mean, rstd), 1).float().contiguous().to(dev),
            gamma=(torch.rand(NMAX, generator=g) + 0.5).to(dev), beta=torch.randn(NMAX, generator=g).to(dev))
    return out


def _case(o, M, N, dev):
    """The case's views / copies of the module operands: leading M rows of A, N rows of B, [M, N] residual."""
    K = o['ah'].shape[1]
    return dict(K=K, Ap=o['Ap'][:M], Bp=o['Bp'][:N], bias=o['bias'][:N], R=o['R'][:M, :N].contiguous(),
                stats=o['stats'][:M], gamma=o['gamma'][:N], beta=o['beta'][:N],
                A2=torch.stack((o['ah'][:M], o['al'][:M])).contiguous(),
                B2=torch.stack((o['bh'][:N], o['bl'][:N])).contiguous())


def _nan32(M, N, dev):
    return torch.full((M + GUARD, N), float('nan'), device=dev)


def _nan16(shape, dev):
    return torch.full(shape, float('nan'), dtype=torch.float16, device=dev)


def _written(t, M):
    """Rows < M hold no NaN, the guard rows all NaN (t: [..., M + GUARD, cols])."""
    return not torch.isnan(t[..., :M, :]).any() and bool(torch.isnan(t[..., M:, :]).all())


# ------------------------------------------------------------------ a. bias + f32 residual -> f32
@gpu
@pytest.mark.parametrize('M', MS)
@pytest.mark.parametrize('K', KS)
def test_pp_f32_residual_same_bits_as_ring(dev, operands, K, M):
    """The full K x M cross at N = 256, output form a."""
    _form_a(dev, operands, K, M, 256)


@gpu
@pytest.mark.parametrize('K,M', [(32, 513), (64, 300), (96, 127), (128, 1), (768, 300)])
def test_pp_f32_residual_three_column_tiles(dev, operands, K, M):
    _form_a(dev, operands, K, M, 768)


def _form_a(dev, operands, K, M, N):
    lib = _lib.load()
    c = _case(operands[K], M, N, dev)
    y = {}
    for pp in (0, PP_ALL):
        y[pp] = _nan32(M, N, dev)
        with _Knobs(lib, pp):
            _lib.check(lib.mec_gemm_f16x3_paired(_p(c['Ap']), _p(c['Bp']), 0.5, _p(c['bias']), _p(c['R']), None, 0, 0,
                                                 _p(y[pp]), M, N, K, 0, _st(dev)), f'gemm_x3_pp {pp}')
    torch.cuda.synchronize()
    assert _written(y[0], M) and _written(y[PP_ALL], M)
    assert torch.equal(y[PP_ALL][:M], y[0][:M])


# ------------------------------------------------------------------ b. bias + deferred-LN residual -> f32
@gpu
@pytest.mark.parametrize('K,M,N', CORNERS)
def test_pp_deferred_layernorm_residual(dev, operands, K, M, N):
    """mec_gemm_f16x3_paired_ln on the ping-pong schedule against itself under gemm_x3_pp 0 and against
    mec_gemm_ex on the planar planes (the ring): the O-projection / FFN2 epilogue."""
    lib = _lib.load()
    c = _case(operands[K], M, N, dev)
    y = {}
    for pp in (0, PP_ALL):
        y[pp] = _nan32(M, N, dev)
        with _Knobs(lib, pp):
            _lib.check(lib.mec_gemm_f16x3_paired_ln(
                _p(c['Ap']), _p(c['Bp']), 0.5, _p(c['bias']), _p(c['R']), _p(c['stats']), _p(c['gamma']), _p(c['beta']),
                None, 0, 0, 1.0, _p(y[pp]), M, N, K, 0, None, _st(dev)), f'paired_ln gemm_x3_pp {pp}')
    ref = _nan32(M, N, dev)
    with _Knobs(lib, PP_ALL):
        a = _lib.GemmArgs(A=c['A2'].data_ptr(), a_lo=M * K, B=c['B2'].data_ptr(), b_lo=N * K, oscale=0.5,
                          bias=c['bias'].data_ptr(), R=c['R'].data_ptr(), r_is_f32=1, r_stats=c['stats'].data_ptr(),
                          r_gamma=c['gamma'].data_ptr(), r_beta=c['beta'].data_ptr(), C32=ref.data_ptr(), M=M, N=N, K=K)
        _lib.check(lib.mec_gemm_ex(ctypes.byref(a), _st(dev)), 'planar deferred LN')
    torch.cuda.synchronize()
    assert _written(y[0], M) and _written(y[PP_ALL], M) and _written(ref, M)
    assert torch.equal(y[PP_ALL][:M], y[0][:M])
    assert torch.equal(y[PP_ALL][:M], ref[:M])


# ------------------------------------------------------------------ c, d. bias -> hi / lo planes
@gpu
@pytest.mark.parametrize('act,cscale', [(0, 1.0), (4, 1.0), (5, 1.0), (5, 4.0)])
@pytest.mark.parametrize('K,M,N', CORNERS)
def test_pp_plane_outputs(dev, operands, K, M, N, act, cscale):
    """c: paired planes (FFN1 / K|V form; act none, exact-erf GELU, branch-free-erf GELU; one cscale != 1),
    un-paired on the host, and d: planar planes from the paired operands, both against the planar planes
    that mec_gemm_ex writes from the planar operands."""
    lib = _lib.load()
    c = _case(operands[K], M, N, dev)
    L = (M + GUARD) * N  # lo plane offset of the planar outputs
    cp, cd = {}, {}
    for pp in (0, PP_ALL):
        cp[pp] = _nan16((M + GUARD, 2 * N), dev)
        cd[pp] = _nan16((2, M + GUARD, N), dev)
        with _Knobs(lib, pp):
            _lib.check(lib.mec_gemm_f16x3_paired_ln(
                _p(c['Ap']), _p(c['Bp']), 1.0, _p(c['bias']), None, None, None, None, _p(cp[pp]), 1, 0, cscale, None,
                M, N, K, act, None, _st(dev)), f'paired planes gemm_x3_pp {pp}')
            _lib.check(lib.mec_gemm_f16x3_paired_ln(
                _p(c['Ap']), _p(c['Bp']), 1.0, _p(c['bias']), None, None, None, None, _p(cd[pp]), 0, L, cscale, None,
                M, N, K, act, None, _st(dev)), f'planar planes gemm_x3_pp {pp}')
    ref = _nan16((2, M + GUARD, N), dev)
    with _Knobs(lib, PP_ALL):
        a = _lib.GemmArgs(A=c['A2'].data_ptr(), a_lo=M * K, B=c['B2'].data_ptr(), b_lo=N * K,
                          bias=c['bias'].data_ptr(), C16=ref.data_ptr(), c_lo=L, cscale=cscale, M=M, N=N, K=K, act=act)
        _lib.check(lib.mec_gemm_ex(ctypes.byref(a), _st(dev)), 'planar planes')
    torch.cuda.synchronize()
    assert _written(ref, M) and ref[1, :M].abs().max() > 0  # the lo plane carries something
    for pp in (0, PP_ALL):
        assert _written(cp[pp], M) and _written(cd[pp], M)
        hi, lo = x3pair.unpair(cp[pp][:M])
        assert torch.equal(hi, ref[0, :M]) and torch.equal(lo, ref[1, :M]), f'paired planes, gemm_x3_pp {pp}'
        assert torch.equal(cd[pp][:, :M], ref[:, :M]), f'planar planes, gemm_x3_pp {pp}'


# ------------------------------------------------------------------ determinism screen
@gpu
def test_pp_twenty_launches_agree(dev, operands):
    """A mis-placed read of a DMA-filled buffer passes single clean runs: 20 launches of one small case
    (output form c) into fresh NaN-filled buffers must all give the first one's bits."""
    lib = _lib.load()
    M, N, K = 300, 768, 96
    c = _case(operands[K], M, N, dev)
    outs = [_nan16((M + GUARD, 2 * N), dev) for _ in range(20)]
    with _Knobs(lib, PP_ALL):
        for o in outs:
            _lib.check(lib.mec_gemm_f16x3_paired_ln(
                _p(c['Ap']), _p(c['Bp']), 1.0, _p(c['bias']), None, None, None, None, _p(o), 1, 0, 1.0, None,
                M, N, K, 5, None, _st(dev)), 'paired planes')
    torch.cuda.synchronize()
    assert _written(outs[0], M)
    for i, o in enumerate(outs[1:], 1):
        assert torch.equal(o[:M], outs[0][:M]) and bool(torch.isnan(o[M:]).all()), f'launch {i}'


# ------------------------------------------------------------------ range flag
@gpu
def test_pp_range_flag_raised_by_the_plane_epilogue(dev, operands):
    """An FFN1-form launch (GELU, paired planes out) with its own flag word, so that only this launch's
    epilogue can raise it: in-range operands leave it 0; one A value of 60000 against one B value of 4 puts
    output (5, 7) at about 240000, past the f16 range, and the word reads 1, on the ping-pong schedule as on
    the ring, with the same plane bits (the hi plane holds inf there)."""
    lib = _lib.load()
    M, N, K = 300, 768, 96
    c = _case(operands[K], M, N, dev)
    Ab, Bb = c['Ap'].clone(), c['Bp'].clone()
    Ab[5, x3pair.pair_index(0, 3, K, 0)] = 60000.0  # hi plane, k = 3
    Bb[7, x3pair.pair_index(0, 3, K, 0)] = 4.0
    bad = {}
    for pp in (0, PP_ALL):
        flags = torch.zeros(2, dtype=torch.int32, device=dev)
        outs = []
        with _Knobs(lib, pp):
            for i, (A, B) in enumerate(((c['Ap'], c['Bp']), (Ab, Bb))):
                outs.append(_nan16((M + GUARD, 2 * N), dev))
                _lib.check(lib.mec_gemm_f16x3_paired_ln(
                    _p(A), _p(B), 1.0, _p(c['bias']), None, None, None, None, _p(outs[i]), 1, 0, 1.0, None, M, N, K, 5,
                    ctypes.c_void_p(flags[i:].data_ptr()), _st(dev)), f'gemm_x3_pp {pp}')
        torch.cuda.synchronize()
        assert flags.tolist() == [0, 1], f'gemm_x3_pp {pp}'
        assert _written(outs[0], M)
        hi, _ = x3pair.unpair(outs[1][:M])
        assert torch.isinf(hi[5, 7]) and int(torch.isinf(hi).sum()) == 1
        bad[pp] = outs[1][:M].view(torch.int16)
    assert torch.equal(bad[0], bad[PP_ALL])


# ------------------------------------------------------------------ text model
@pytest.fixture(scope='module')
def encoder(dev):
    """The paired fp32x3 text model with every split GEMM forced onto tile 70256, so that the N = 768 and
    [CLS]-row GEMMs run it at small B too (the pins would otherwise step aside)."""
    from mec import engine
    enc = engine.TextEncoder(device=dev, precision='fp32x3', opts={'x3_layout': 1})
    enc.set_option('gemm_bn', TILE)
    return enc


@gpu
@pytest.mark.parametrize('form', ['padded', 'packed'])
@pytest.mark.parametrize('B', [1, 3, 24])
def test_text_model_pp_same_bits_as_ring(dev, encoder, B, form):
    """feat, logits and probs under gemm_x3_pp 1 and 2 against 0, ragged masks, padded and packed forwards,
    the full and the [CLS]-only last layer; check() clean."""
    from mec import engine, synthetic as syn
    ids, mask = syn.text_inputs(B, 128, seed=60 + B, ragged=True)
    args = (engine.to_device(ids, dev), engine.to_device(mask, dev))
    try:
        for cls_last in (0, 1):
            encoder.set_option('bert_cls_last', cls_last)
            outs = {}
            for pp in (0, 1, PP_ALL):
                encoder.set_option('gemm_x3_pp', pp)
                r = encoder.forward(*args) if form == 'padded' else encoder.forward_packed(*args)
                outs[pp] = [t.cpu() for t in r]
                encoder.check()
            for pp in (1, PP_ALL):
                for name, a, b in zip(('feat', 'logits', 'probs'), outs[0], outs[pp]):
                    assert torch.isfinite(a).all()
                    assert torch.equal(a, b), (f'{name} cls_last={cls_last} gemm_x3_pp={pp}: '
                                               f'max |d| {float((a - b).abs().max())}')
    finally:
        encoder.set_option('bert_cls_last', 1)
        encoder.set_option('gemm_x3_pp', PP_DEFAULT)
