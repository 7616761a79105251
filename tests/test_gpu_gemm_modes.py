"""GPU: kernel-level parity of the GEMM engine's modes that the models launch but no other
kernel-level test reaches, through mec_gemm_ex (and mec_conv_f16 / mec_conv_f32): split-operand
(fp32x3) implicit-GEMM convs, the dual-source GEMM over K = [K1 | C] on f16 and split operands, the
split f16 residual and its prefetch variant, the deferred-LayerNorm residual, and plane output at a
plane scale. Exact cases (one nonzero product per term) are held to zero tolerance; dense cases to
the fp32 GEMM bar against float64 on the host (tests/gemm_ref.py, itself checked on the CPU) and to
1.5 x the exact-fp32 engine's own error on the same operands.

Split operands are laid out as the models lay them out: the lo plane of every activation buffer one
common stride L after its hi plane (A_DUAL reads both sources' lo planes at the same offset), at the
power-of-two plane scales the models' rule gives (test_gpu_fp32x3._act_exp; weights pre-scaled to
below 2^14), folded back by oscale. Device tensors stay in locals until the result has been copied
back (a temporary passed as a raw pointer would be freed and reused under the launch)."""
import contextlib
import ctypes
import functools

import numpy as np
import pytest
import torch

from gemm_ref import GEOMETRIES, conv_nhwc_f64, dual_gather, out_extent, tap_view
from mec import _lib
from test_gpu_fp32x3 import SPLIT_TILES, _act_exp, _split, x3_order
from test_gpu_kernels import TILE_IDS

pytestmark = pytest.mark.gpu

ENGINES = ['f16', 'x3 order 0', 'x3 order 1']
# A_DUAL shapes (n, H, W, C, K1, N, stride): a bottleneck's conv3 (K1 = width) + its downsample
# (C = cin) into N = 4 width outputs; D1 M = 120 (one partial tile), D3 M = 320 (partial last tile
# at BM = 128 and 256, rows of one tile from several images, OH = 8 from an odd H at stride 2)
DUAL_SHAPES = {'D1': (2, 10, 6, 128, 64, 256, 1), 'D3': (5, 15, 15, 128, 64, 256, 2)}


def _ptr(v):
    return v.data_ptr() if isinstance(v, torch.Tensor) else v


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _ex(lib, dev, what, **fields):
    """One mec_gemm_ex launch on the current stream; tensors among the fields pass their pointers
    (the caller keeps them alive)."""
    a = _lib.GemmArgs(**{k: _ptr(v) for k, v in fields.items()})
    _lib.check(lib.mec_gemm_ex(ctypes.byref(a), _stream(dev)), what)


def _order(engine):
    return x3_order(int(engine[-1])) if engine.startswith('x3') else contextlib.nullcontext()


def _put_planes(planes, L, dev):
    """[2, ...] f16 hi / lo planes in one device buffer, the lo plane L elements after the hi plane."""
    size = planes[0].size
    assert L >= size
    buf = torch.zeros(L + size, dtype=torch.float16)
    buf[:size] = torch.from_numpy(planes[0].ravel())
    buf[L:] = torch.from_numpy(planes[1].ravel())
    return buf.to(dev)


def _value(planes):
    return planes[0].astype(np.float32) + planes[1].astype(np.float32)


def _nan(shape, dev, dtype=torch.float32):
    return torch.full(shape, float('nan'), dtype=dtype, device=dev)


def _width(tile):
    return (256 if 40000 <= tile < 50000 else tile % 1000 if tile >= 70000 else
            tile % 10000 if tile % 10000 < 1000 else tile % 10000 - 1000)


class _tile:
    """gemm_bn forced for the block (0 = autotune), restored on exit."""

    def __init__(self, lib, tile):
        self.lib, self.tile = lib, tile

    def __enter__(self):
        _lib.check(self.lib.mec_set_option(b'gemm_bn', self.tile), f'gemm_bn {self.tile}')

    def __exit__(self, *exc):
        self.lib.mec_set_option(b'gemm_bn', 0)


# ------------------------------------------------------------------ (a) exact tap shifts
TAP_GEOMS = {'G1': GEOMETRIES['G1'], 'G2': GEOMETRIES['G2'], 'G5c': (1, 20, 20, 64, 64, 3, 1, 1)}


def _tap_weights(C, ks, kh, kw):
    w = np.zeros((C, ks, ks, C), np.float32)
    w[np.arange(C), kh, kw, np.arange(C)] = 1.0
    return w


@pytest.mark.parametrize('engine', ['f16', 'f32'] + ENGINES[1:])
@pytest.mark.parametrize('geom', list(TAP_GEOMS))
def test_conv_tap_shift_exact(dev, geom, engine):
    """Weights 1.0 at [co, kh, kw, c == co] only, no bias, no activation: the output is
    x[n, oh s - p + kh, ow s - p + kw, co] inside the image and 0 in the padding, exactly (one nonzero
    product per term), for every filter tap: tap addressing, padding, stride, H / W order and, on
    split operands, the lo plane at every tap (x = hi + lo of random planes, so every value carries
    lo bits; hi + lo is an fp32 value, so the fp32 sum lo + 0 + hi is exact in either term order)."""
    lib = _lib.load()
    n, H, W, C, Cout, ks, stride, pad = TAP_GEOMS[geom]
    assert C == Cout
    OH, OW = out_extent(H, ks, stride, pad), out_extent(W, ks, stride, pad)
    v = np.random.default_rng(H * W + C).standard_normal((n, H, W, C)).astype(np.float32)
    L = v.size + 192
    if engine == 'f16':
        x = v.astype(np.float16)
        xd = torch.from_numpy(x).to(dev)
    elif engine == 'f32':
        x = v
        xd = torch.from_numpy(x).to(dev)
    else:
        planes = _split(v)
        x = _value(planes)
        assert (planes[1] != 0).mean() > 0.9
        xd = _put_planes(planes, L, dev)
    with _order(engine):
        for kh in range(ks):
            for kw in range(ks):
                w = _tap_weights(C, ks, kh, kw)
                if engine == 'f16':
                    wd = torch.from_numpy(w.astype(np.float16)).to(dev)
                    y = _nan((n, OH, OW, Cout), dev, torch.float16)
                    _lib.check(lib.mec_conv_f16(_ptr(xd), _ptr(wd), None, None, _ptr(y), n, H, W, C, Cout, ks, stride,
                                                pad, 0, _stream(dev)), 'mec_conv_f16')
                elif engine == 'f32':
                    wd = torch.from_numpy(w).to(dev)
                    y = _nan((n, OH, OW, Cout), dev)
                    _lib.check(lib.mec_conv_f32(_ptr(xd), _ptr(wd), None, None, _ptr(y), n, H, W, C, Cout, ks, stride,
                                                pad, 0, _stream(dev)), 'mec_conv_f32')
                else:
                    wd = torch.from_numpy(_split(w)).to(dev)
                    y = _nan((n, OH, OW, Cout), dev)
                    _ex(lib, dev, 'split conv', amode=_lib.A_CONV, A=xd, a_lo=L, B=wd, b_lo=w.size, C32=y, N=Cout,
                        n=n, H=H, W=W, C=C, ks=ks, stride=stride, pad=pad)
                got = y.cpu()
                want = torch.from_numpy(np.ascontiguousarray(tap_view(x, kh, kw, ks, stride, pad)))
                assert torch.equal(got, want), f'tap ({kh}, {kw})'


# ------------------------------------------------------------------ (b) exact A_DUAL
@pytest.mark.parametrize('engine', ENGINES)
@pytest.mark.parametrize('stride', [1, 2])
@pytest.mark.parametrize('C', [64, 128])
def test_dual_exact(dev, C, stride, engine):
    """A_DUAL with N = K1 = C and a non-square second source (2 x 10 x 6 x C read at stride 1 / 2):
    B = [I | 0] returns A's rows, B = [0 | I] the strided view of A2, B = [I | I] (small-integer
    planes) their sum, all exactly: the source selection at the K1 boundary, the second source's
    stride addressing, and on split operands both sources' lo planes."""
    lib = _lib.load()
    n, H, W = 2, 10, 6
    OH, OW = out_extent(H, 1, stride, 0), out_extent(W, 1, stride, 0)
    M, K1, N = n * OH * OW, C, C
    L = max(M * K1, n * H * W * C) + 192
    rng = np.random.default_rng(C + stride)
    split = engine.startswith('x3')
    eye, zero = np.eye(C, dtype=np.float32), np.zeros((C, C), np.float32)
    with _order(engine):
        for name, B in (('[I | 0]', np.hstack([eye, zero])), ('[0 | I]', np.hstack([zero, eye])),
                        ('[I | I]', np.hstack([eye, eye]))):
            if name == '[I | I]':  # integers (+ multiples of 2^-6 as lo planes): every partial sum exact
                pa = np.stack([rng.integers(-32, 33, (M, K1)), rng.integers(-8, 9, (M, K1)) / 64]).astype(np.float16)
                pa2 = np.stack([rng.integers(-32, 33, (n, H, W, C)),
                                rng.integers(-8, 9, (n, H, W, C)) / 64]).astype(np.float16)
            else:
                pa = _split(rng.standard_normal((M, K1)).astype(np.float32))
                pa2 = _split(rng.standard_normal((n, H, W, C)).astype(np.float32))
            if split:
                a, a2 = _value(pa), _value(pa2)
                Ad, A2d, Bd = _put_planes(pa, L, dev), _put_planes(pa2, L, dev), torch.from_numpy(_split(B)).to(dev)
                lo = dict(a_lo=L, b_lo=B.size)
            else:
                a, a2 = pa[0].astype(np.float32), pa2[0].astype(np.float32)
                Ad, A2d = torch.from_numpy(pa[0]).to(dev), torch.from_numpy(pa2[0]).to(dev)
                Bd = torch.from_numpy(B.astype(np.float16)).to(dev)
                lo = {}
            y = _nan((M, N), dev)
            _ex(lib, dev, f'dual {name}', amode=_lib.A_DUAL, A=Ad, A2=A2d, K1=K1, B=Bd, C32=y, N=N, n=n, H=H, W=W,
                C=C, ks=1, stride=stride, pad=0, **lo)
            got = y.cpu()
            g2 = dual_gather(a2, stride)
            want = {'[I | 0]': a, '[0 | I]': g2, '[I | I]': a + g2}[name]
            assert torch.equal(got, torch.from_numpy(np.ascontiguousarray(want))), name


# ------------------------------------------------------------------ (c) dense random vs float64
def _weight_exp(w):
    return float(np.ceil(np.log2(16384 / np.abs(w).max())) - 1)


@functools.lru_cache(maxsize=None)
def _case(name):
    """fp32 operands of one conv (G*) or dual (D*) shape, with the float64 reference of the linear
    part, the fp32-GEMM-bar magnitude sum |x| |w| + |bias| + 1 and the plane exponents; computed
    once and shared (read-only) by the tests below."""
    rng = np.random.default_rng(sum(map(ord, name)))
    c = {'name': name}
    if name in GEOMETRIES:
        n, H, W, C, N, ks, stride, pad = GEOMETRIES[name]
        c['x'] = rng.standard_normal((n, H, W, C)).astype(np.float32)
        c['w'] = (rng.standard_normal((N, ks, ks, C)) * 0.03).astype(np.float32)
        lin = conv_nhwc_f64(c['x'], c['w'], stride, pad)
        mag = conv_nhwc_f64(np.abs(c['x']), np.abs(c['w']), stride, pad)
        c['geom'] = dict(n=n, H=H, W=W, C=C, ks=ks, stride=stride, pad=pad, N=N)
        c['residual'] = N == 4 * C
        amax = np.abs(c['x']).max()
    else:
        n, H, W, C, K1, N, stride = DUAL_SHAPES[name]
        M = n * out_extent(H, 1, stride, 0) * out_extent(W, 1, stride, 0)
        c['a'] = rng.standard_normal((M, K1)).astype(np.float32)
        c['a2'] = rng.standard_normal((n, H, W, C)).astype(np.float32)
        c['w'] = (rng.standard_normal((N, K1 + C)) * 0.03).astype(np.float32)
        c['cat'] = np.ascontiguousarray(np.hstack([c['a'], dual_gather(c['a2'], stride)]))  # [A | gathered A2]
        lin = c['cat'].astype(np.float64) @ c['w'].astype(np.float64).T
        mag = np.abs(c['cat']).astype(np.float64) @ np.abs(c['w']).astype(np.float64).T
        c['geom'] = dict(n=n, H=H, W=W, C=C, ks=1, stride=stride, pad=0, N=N, K1=K1)
        c['residual'] = N == 4 * K1
        amax = max(np.abs(c['a']).max(), np.abs(c['a2']).max())
    c['M'] = lin.size // N
    c['bias'] = rng.standard_normal(N).astype(np.float32)
    c['R'] = rng.standard_normal((c['M'], N)).astype(np.float32)
    c['lin'] = lin.reshape(c['M'], N) + c['bias']
    c['mag'] = mag.reshape(c['M'], N) + np.abs(c['bias']) + 1
    c['s_a'], c['e_w'] = _act_exp(float(amax)), _weight_exp(c['w'])
    return c


class _SplitOperands:
    """A case's split planes on the device and its mec_gemm_ex fields."""

    def __init__(self, c, dev):
        g = c['geom']
        sa, sw = 2.0 ** c['s_a'], 2.0 ** c['e_w']
        self.w = torch.from_numpy(_split(c['w'], sw)).to(dev)
        self.bias = torch.from_numpy(c['bias']).to(dev)
        self.fields = dict(B=self.w, b_lo=c['w'].size, oscale=2.0 ** (-c['s_a'] - c['e_w']), bias=self.bias, N=g['N'],
                           n=g['n'], H=g['H'], W=g['W'], C=g['C'], ks=g['ks'], stride=g['stride'], pad=g['pad'])
        if 'x' in c:
            L = c['x'].size + 192
            self.a = _put_planes(_split(c['x'], sa), L, dev)
            self.fields.update(amode=_lib.A_CONV, A=self.a, a_lo=L)
        else:
            L = max(c['a'].size, c['a2'].size) + 192
            self.a, self.a2 = _put_planes(_split(c['a'], sa), L, dev), _put_planes(_split(c['a2'], sa), L, dev)
            self.fields.update(amode=_lib.A_DUAL, A=self.a, A2=self.a2, K1=g['K1'], a_lo=L)
        self.r32 = torch.from_numpy(c['R']).to(dev)
        self.rlo = c['R'].size + 192
        self.rx3 = _put_planes(_split(c['R']), self.rlo, dev)

    def residual(self, rmode):
        return {'none': {}, 'f32': dict(R=self.r32, r_is_f32=1), 'split': dict(R=self.rx3, r_lo=self.rlo)}[rmode]


def _exact_engine(lib, dev, c, act, with_r):
    """The exact-fp32 MFMA engine on the case's fp32 operands: mec_conv_f32, or mec_gemm_f32 on the
    host-materialised [A | gathered A2]."""
    g = c['geom']
    wd, bd = torch.from_numpy(c['w']).to(dev), torch.from_numpy(c['bias']).to(dev)
    rd = torch.from_numpy(c['R']).to(dev) if with_r else None
    y = _nan((c['M'], g['N']), dev)
    if 'x' in c:
        xd = torch.from_numpy(c['x']).to(dev)
        _lib.check(lib.mec_conv_f32(_ptr(xd), _ptr(wd), _ptr(bd), _ptr(rd), _ptr(y), g['n'], g['H'], g['W'], g['C'],
                                    g['N'], g['ks'], g['stride'], g['pad'], act, _stream(dev)), 'mec_conv_f32')
    else:
        xd = torch.from_numpy(c['cat']).to(dev)
        _lib.check(lib.mec_gemm_f32(_ptr(xd), _ptr(wd), _ptr(bd), _ptr(rd), _ptr(y), c['M'], g['N'], c['cat'].shape[1],
                                    act, _stream(dev)), 'mec_gemm_f32')
    return y.cpu().numpy()


def _reference(c, act, with_r):
    ref = c['lin'] + (c['R'] if with_r else 0)
    bound = 2e-6 * (c['mag'] + (np.abs(c['R']) if with_r else 0))
    return (np.maximum(ref, 0) if act == 1 else ref), bound


@pytest.mark.parametrize('order', [0, 1])
@pytest.mark.parametrize('name', list(GEOMETRIES) + list(DUAL_SHAPES))
def test_split_conv_and_dual_vs_fp64(dev, name, order):
    """Split-operand conv (G1-G5) and dual GEMM (D1, D3) on dense random operands with a bias, with
    and without ReLU, and where N = 4 width also with an f32 residual and a split f16 residual
    (r_lo), read from C32. Two bars per variant: every element within the project's fp32 GEMM bar,
    |got - ref| <= 2e-6 (sum |x||w| + |bias| + |R| + 1), of the float64 reference; and the maximum
    error at most 1.5 x the exact-fp32 engine's on the same fp32 operands (a lost lo term can slip
    under the first bar at large K; it cannot under this one). Figures are printed per variant
    before the assertions."""
    lib = _lib.load()
    c = _case(name)
    ops = _SplitOperands(c, dev)
    failures = []
    with x3_order(order):
        for rmode in (['none', 'f32', 'split'] if c['residual'] else ['none']):
            for act in (0, 1):
                y = _nan((c['M'], c['geom']['N']), dev)
                _ex(lib, dev, f'split {name}', C32=y, act=act, **ops.fields, **ops.residual(rmode))
                got = y.cpu().numpy()
                e32 = _exact_engine(lib, dev, c, act, rmode != 'none')
                ref, bound = _reference(c, act, rmode != 'none')
                ex3, ee = np.abs(got - ref), np.abs(e32 - ref)
                print(f'MODES c {name} order {order} R {rmode} act {act}: max err/bound split {(ex3 / bound).max():.3g} '
                      f'exact {(ee / bound).max():.3g}; max err split {ex3.max():.3g} exact {ee.max():.3g} '
                      f'ratio {ex3.max() / ee.max():.3g}')
                if not ((ex3 <= bound).all() and (ee <= bound).all()):
                    failures.append(f'R {rmode} act {act}: outside the float64 bar')
                if not ex3.max() <= 1.5 * ee.max():
                    failures.append(f'R {rmode} act {act}: split max err {ex3.max():.3g} > 1.5 x exact {ee.max():.3g}')
    assert not failures, failures


# ------------------------------------------------------------------ (d) every tile, same bits
def _tiles(tiles, N):
    return [0] + [t for t in tiles if N % _width(t) == 0]


@pytest.mark.parametrize('order', [0, 1])
@pytest.mark.parametrize('name', ['G3', 'G5', 'D3'])
def test_split_conv_and_dual_every_tile_bit_identical(dev, name, order):
    """Per term order, every tile whose width divides N (pass-major: SPLIT_TILES[0] without the
    plain-A ping-pong tiles; K-interleaved: SPLIT_TILES[1]) and the autotuned launch write the same
    bits on split conv and split dual operands (bias, ReLU, C32 and plane output)."""
    lib = _lib.load()
    c = _case(name)
    ops = _SplitOperands(c, dev)
    M, N = c['M'], c['geom']['N']
    outs = {}
    with x3_order(order):
        for tile in _tiles([t for t in SPLIT_TILES[order] if t not in (40256, 41256)], N):
            y, pl = _nan((M, N), dev), _nan((2, M, N), dev, torch.float16)
            with _tile(lib, tile):
                _ex(lib, dev, f'split {name} tile {tile}', C32=y, C16=pl, c_lo=M * N, act=1, **ops.fields)
            outs[tile] = (y.cpu().numpy(), pl.cpu().numpy())
    ref, bound = _reference(c, 1, False)
    assert (np.abs(outs[0][0] - ref) <= bound).all()
    assert len(outs) >= (3 if N % 256 else 6)
    for tile, (y, pl) in outs.items():
        assert np.array_equal(y, outs[0][0]) and np.array_equal(pl, outs[0][1]), f'tile {tile} differs from the autotuned one'


def test_f16_dual_every_tile_bit_identical(dev):
    """The same for A_DUAL on f16 operands (D3) over TILE_IDS, against float64 of the f16 operands."""
    lib = _lib.load()
    c = _case('D3')
    g = c['geom']
    M, N = c['M'], g['N']
    a, a2, w = c['a'].astype(np.float16), c['a2'].astype(np.float16), c['w'].astype(np.float16)
    ad, a2d, wd = (torch.from_numpy(t).to(dev) for t in (a, a2, w))
    bd = torch.from_numpy(c['bias']).to(dev)
    outs = {}
    for tile in _tiles(TILE_IDS, N):
        y, y16 = _nan((M, N), dev), _nan((M, N), dev, torch.float16)
        with _tile(lib, tile):
            _ex(lib, dev, f'f16 dual tile {tile}', amode=_lib.A_DUAL, A=ad, A2=a2d, K1=g['K1'], B=wd, bias=bd, C32=y,
                C16=y16, act=1, N=N, n=g['n'], H=g['H'], W=g['W'], C=g['C'], ks=1, stride=g['stride'], pad=0)
        outs[tile] = (y.cpu().numpy(), y16.cpu().numpy())
    cat = np.hstack([a.astype(np.float64), dual_gather(a2, g['stride']).astype(np.float64)])
    ref = np.maximum(cat @ w.astype(np.float64).T + c['bias'], 0)
    bound = 2e-6 * (np.abs(cat) @ np.abs(w.astype(np.float64)).T + np.abs(c['bias']) + 1)
    assert (np.abs(outs[0][0] - ref) <= bound).all()
    assert np.array_equal(outs[0][1], outs[0][0].astype(np.float16))
    assert len(outs) == len(TILE_IDS) + 1
    for tile, (y, y16) in outs.items():
        assert np.array_equal(y, outs[0][0]) and np.array_equal(y16, outs[0][1]), f'tile {tile}'


# ------------------------------------------------------------------ (e) f16 conv: residual, no bias
def _rel_err(got, ref):
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-6))


def _conv_f16_case(dev, n, H, W, C, Cout, ks, stride, pad, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(n, H, W, C, generator=g).half()
    w = ((torch.rand(Cout, ks, ks, C, generator=g) * 2 - 1) * (C * ks * ks) ** -0.5).half()
    OH, OW = out_extent(H, ks, stride, pad), out_extent(W, ks, stride, pad)
    R = (torch.rand(n, OH, OW, Cout, generator=g) * 2 - 1).half()
    lin = torch.nn.functional.conv2d(x.permute(0, 3, 1, 2).float(), w.permute(0, 3, 1, 2).float(), stride=stride,
                                     padding=pad).permute(0, 2, 3, 1)
    return x.to(dev), w.to(dev), R.to(dev), lin, R.float()


@pytest.mark.parametrize('geom', ['G2', 'G3', 'G4'])
def test_conv_f16_residual_no_bias_no_act(dev, geom):
    """mec_conv_f16 with an f16 residual, no activation and bias = NULL on non-square / strided
    geometries, against the fp32 reference at the f16 output bar (2e-3 relative)."""
    lib = _lib.load()
    n, H, W, C, Cout, ks, stride, pad = GEOMETRIES[geom]
    xd, wd, Rd, lin, R = _conv_f16_case(dev, n, H, W, C, Cout, ks, stride, pad, H * W)
    y = _nan(tuple(lin.shape), dev, torch.float16)
    _lib.check(lib.mec_conv_f16(_ptr(xd), _ptr(wd), None, _ptr(Rd), _ptr(y), n, H, W, C, Cout, ks, stride, pad, 0,
                                _stream(dev)), 'mec_conv_f16')
    got = y.cpu().float()
    assert _rel_err(got, lin + R) < 2e-3


@pytest.mark.parametrize('variant', ['bias NULL', 'residual'])
@pytest.mark.parametrize('H,C,option', [(56, 64, b'conv3x3_direct'), (28, 128, b'conv3x3_halo'),
                                        (14, 256, b'conv3x3_halo')])
def test_conv_f16_halo_shapes_fall_through_to_gemm(dev, H, C, option, variant):
    """The three shapes launch_gemm routes to the halo-tile kernels (3x3 / 1, ReLU), with what those
    kernels do not take -- bias = NULL, or a residual: the call succeeds, matches the reference, and
    is the GEMM route (the same bits with the halo route's option off)."""
    lib = _lib.load()
    xd, wd, Rd, lin, R = _conv_f16_case(dev, 1, H, H, C, C, 3, 1, 1, H + C)
    bias = torch.rand(C, generator=torch.Generator().manual_seed(C)) - 0.5
    bd = bias.to(dev) if variant == 'residual' else None
    ref = torch.relu(lin + (R + bias if variant == 'residual' else 0))
    outs = []
    for on in (1, 0):
        y = _nan(tuple(lin.shape), dev, torch.float16)
        _lib.check(lib.mec_set_option(option, on), 'option')
        try:
            _lib.check(lib.mec_conv_f16(_ptr(xd), _ptr(wd), _ptr(bd), _ptr(Rd) if variant == 'residual' else None,
                                        _ptr(y), 1, H, H, C, C, 3, 1, 1, 1, _stream(dev)), f'mec_conv_f16 ({variant})')
        finally:
            lib.mec_set_option(option, 1)
        outs.append(y.cpu())
    assert _rel_err(outs[0].float(), ref) < 2e-3
    assert torch.equal(outs[0], outs[1])


# ------------------------------------------------------------------ (f) epilogue modes, plain split GEMM
PLAIN_SHAPES = [(300, 256, 128), (130, 768, 768)]


@functools.lru_cache(maxsize=None)
def _plain(M, N, K):
    rng = np.random.default_rng(M + N + K)
    c = dict(a=rng.standard_normal((M, K)).astype(np.float32), w=(rng.standard_normal((N, K)) * 0.03).astype(np.float32),
             bias=rng.standard_normal(N).astype(np.float32), R=(rng.standard_normal((M, N)) * 2 + 0.5).astype(np.float32),
             gamma=rng.standard_normal(N).astype(np.float32), beta=rng.standard_normal(N).astype(np.float32))
    c['s_a'], c['e_w'] = _act_exp(float(np.abs(c['a']).max())), _weight_exp(c['w'])
    mean = c['R'].astype(np.float64).mean(1)
    rstd = 1 / np.sqrt(c['R'].astype(np.float64).var(1) + 1e-12)
    c['stats'] = np.stack([mean, rstd], 1).astype(np.float32)  # the kernel's (mean, rstd), rounded to f32
    return c


def _plain_fields(c, dev, split=True):
    """(device tensors to keep alive, mec_gemm_ex fields) of a plain GEMM on c's operands."""
    M, K = c['a'].shape
    N = c['w'].shape[0]
    bd = torch.from_numpy(c['bias']).to(dev)
    if split:
        ad = torch.from_numpy(_split(c['a'], 2.0 ** c['s_a'])).to(dev)
        wd = torch.from_numpy(_split(c['w'], 2.0 ** c['e_w'])).to(dev)
        f = dict(A=ad, a_lo=M * K, B=wd, b_lo=N * K, oscale=2.0 ** (-c['s_a'] - c['e_w']))
    else:
        ad, wd = torch.from_numpy(c['a'].astype(np.float16)).to(dev), torch.from_numpy(c['w'].astype(np.float16)).to(dev)
        f = dict(A=ad, B=wd)
    return (ad, wd, bd), dict(bias=bd, M=M, N=N, K=K, **f)


@pytest.mark.parametrize('order', [0, 1])
@pytest.mark.parametrize('cscale', [2.0 ** -3, 2.0 ** 5])
@pytest.mark.parametrize('M,N,K', PLAIN_SHAPES)
def test_split_gemm_plane_output_at_plane_scale(dev, M, N, K, cscale, order):
    """Plane output at cscale != 1 (BERT FFN1's form): hi == f16(v cscale) and
    lo == f16(v cscale - hi) exactly, v the C32 result of the same launch without planes; C32
    written beside the planes still carries v."""
    lib = _lib.load()
    c = _plain(M, N, K)
    keep, f = _plain_fields(c, dev)
    with x3_order(order):
        v32, pl, v32b = _nan((M, N), dev), _nan((2, M, N), dev, torch.float16), _nan((M, N), dev)
        _ex(lib, dev, 'f32 out', C32=v32, act=4, **f)
        _ex(lib, dev, 'plane out', C16=pl, c_lo=M * N, cscale=cscale, C32=v32b, act=4, **f)
        v, hi, lo = v32.cpu().numpy(), pl[0].cpu().numpy(), pl[1].cpu().numpy()
        assert np.array_equal(v32b.cpu().numpy(), v)
    u = v * np.float32(cscale)
    assert np.array_equal(hi, u.astype(np.float16))
    assert np.array_equal(lo, (u - hi.astype(np.float32)).astype(np.float16))
    assert np.isfinite(hi).all() and (lo != 0).mean() > 0.9


@pytest.mark.parametrize('engine', ENGINES)
@pytest.mark.parametrize('M,N,K', PLAIN_SHAPES)
def test_gemm_deferred_layernorm_residual_vs_fp64(dev, M, N, K, engine):
    """The deferred-LayerNorm residual (r_stats): an f32 R enters as (R - mean) rstd gamma + beta with
    the row (mean, rstd) computed in float64 and rounded to f32; the float64 reference uses those
    rounded stats. Bar: the fp32 GEMM bar with |R| replaced by |R - mean| rstd |gamma| + |beta|. On
    split operands at both term orders and on f16 operands (bert.hip's form). The exact-fp32 engine
    has no deferred-LN mode (it rejects r_stats), so its figure, with the host-normalised residual
    rounded to f32 as a plain R, is printed and not asserted."""
    lib = _lib.load()
    c = _plain(M, N, K)
    split = engine.startswith('x3')
    keep, f = _plain_fields(c, dev, split)
    rd, sd = torch.from_numpy(c['R']).to(dev), torch.from_numpy(c['stats']).to(dev)
    gd, be = torch.from_numpy(c['gamma']).to(dev), torch.from_numpy(c['beta']).to(dev)
    a, w = (c['a'], c['w']) if split else (c['a'].astype(np.float16), c['w'].astype(np.float16))
    a, w = a.astype(np.float64), w.astype(np.float64)
    mean, rstd = c['stats'][:, :1].astype(np.float64), c['stats'][:, 1:].astype(np.float64)
    rn = (c['R'] - mean) * rstd * c['gamma'].astype(np.float64) + c['beta']
    ref = a @ w.T + c['bias'] + rn
    bound = 2e-6 * (np.abs(a) @ np.abs(w).T + np.abs(c['bias']) + np.abs(c['R'] - mean) * rstd * np.abs(c['gamma'])
                    + np.abs(c['beta']) + 1)
    with _order(engine):
        y = _nan((M, N), dev)
        _ex(lib, dev, 'deferred LN', R=rd, r_is_f32=1, r_stats=sd, r_gamma=gd, r_beta=be, C32=y, **f)
        err = np.abs(y.cpu().numpy() - ref)
    ad, wd, rnd, y32 = (torch.from_numpy(c['a']).to(dev), torch.from_numpy(c['w']).to(dev),
                        torch.from_numpy(rn.astype(np.float32)).to(dev), _nan((M, N), dev))
    _lib.check(lib.mec_gemm_f32(_ptr(ad), _ptr(wd), _ptr(keep[2]), _ptr(rnd), _ptr(y32), M, N, K, 0, _stream(dev)), 'f32')
    e32 = np.abs(y32.cpu().numpy() - (c['a'].astype(np.float64) @ c['w'].astype(np.float64).T + c['bias'] + rn))
    print(f'MODES f deferred-LN {M}x{N}x{K} {engine}: max err/bound {(err / bound).max():.3g}, max err {err.max():.3g} '
          f'(exact-fp32 engine on a host-normalised R {e32.max():.3g})')
    assert (err <= bound).all()


@pytest.mark.parametrize('order,tile', [(0, 1128), (0, 1064), (0, 11128), (0, 11064), (1, 71128), (1, 71064)])
def test_split_residual_prefetch_bit_identical(dev, order, tile):
    """The split f16 residual (r_lo) on the tiles of at most 128 x 128 at K <= 512, where
    gemm_prefetch_r 1 loads both residual planes before the K loop: the same bits as the
    epilogue-load form (gemm_prefetch_r 0), within the fp32 GEMM bar of float64 and 1.5 x the
    exact-fp32 engine's error. The residual is the fp32 value hi + lo of its planes (as in the models,
    where the planes are the tensor), so the split engine, the exact engine and the reference add the
    same fp32 residual: with a residual rounded to its 22-bit planes on the host instead, that
    rounding (2^-23 |R|, |R| up to 8 here) exceeds the fp32 accumulation error of a K = 128 product
    (measured 1.42e-6 against the exact engine's 7.6e-7) and the comparison prices the host split,
    not the kernel."""
    lib = _lib.load()
    M, N, K = PLAIN_SHAPES[0]
    c = dict(_plain(M, N, K))
    keep, f = _plain_fields(c, dev)
    rlo = M * N + 192
    rplanes = _split(c['R'])
    c['R'] = _value(rplanes)
    rx3 = _put_planes(rplanes, rlo, dev)
    outs = []
    with x3_order(order), _tile(lib, tile):
        for pre in (0, 1):
            _lib.check(lib.mec_set_option(b'gemm_prefetch_r', pre), 'gemm_prefetch_r')
            try:
                y = _nan((M, N), dev)
                _ex(lib, dev, f'r_lo prefetch {pre}', R=rx3, r_lo=rlo, C32=y, act=1, **f)
                outs.append(y.cpu().numpy())
            finally:
                lib.mec_set_option(b'gemm_prefetch_r', 1)
    ad, wd, rd, y32 = (torch.from_numpy(c['a']).to(dev), torch.from_numpy(c['w']).to(dev),
                       torch.from_numpy(c['R']).to(dev), _nan((M, N), dev))
    _lib.check(lib.mec_gemm_f32(_ptr(ad), _ptr(wd), _ptr(keep[2]), _ptr(rd), _ptr(y32), M, N, K, 1, _stream(dev)), 'f32')
    a, w = c['a'].astype(np.float64), c['w'].astype(np.float64)
    ref = np.maximum(a @ w.T + c['bias'] + c['R'], 0)
    bound = 2e-6 * (np.abs(a) @ np.abs(w).T + np.abs(c['bias']) + np.abs(c['R']) + 1)
    ex3, ee = np.abs(outs[1] - ref), np.abs(y32.cpu().numpy() - ref)
    print(f'MODES f r_lo order {order} tile {tile}: max err/bound split {(ex3 / bound).max():.3g} exact '
          f'{(ee / bound).max():.3g}; max err split {ex3.max():.3g} exact {ee.max():.3g}')
    assert np.array_equal(outs[0], outs[1])
    assert (ex3 <= bound).all() and (ee <= bound).all()
    assert ex3.max() <= 1.5 * ee.max()
