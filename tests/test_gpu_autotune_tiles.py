"""The autotuner only ever chooses a catalogued tile that is legal for N: on both GEMM engines, the first
eager launch of a shape leaves in the tune cache a tile of the engine's own candidates whose width
divides N, and the autotuned output is the forced-tile output bit for bit and meets float64.

The id lists and the width rule here are the test's own statement of the catalogue (csrc/gemm_tiles.h).
M = 300 (a ragged last M tile), K = 128; N = 192 leaves only the 64-wide tiles, N = 384 the 64- and
128-wide ones (no 256-wide tile, so no ping-pong tile). mec_gemm_query reports the f16 entry of a shape
before the pass-major split entry before the K-interleaved one, so each N runs the engines in the reverse
of that order, on shapes the process-wide cache has not seen (this module runs before the other kernel
tests; the fp32 entries are per MFMA family)."""
import ctypes

import numpy as np
import pytest
import torch

from mec import _lib
from test_gpu_fp32x3 import _split, x3_order
from test_gpu_kernels import _p, _rel_err, _s

pytestmark = pytest.mark.gpu

M, K = 300, 128
F16_CANDIDATES = [64, 128, 256, 1128, 1064, 10064, 10128, 10256, 11128, 11064, 20256, 30256, 20128, 40256, 41256,
                  50128, 60128, 50256]                # f16 operands and pass-major split operands
X3I_CANDIDATES = [70256, 70128, 71128, 71064, 70064]  # K-interleaved split operands; 72128 is pinned only
F32_WIDTH = {1: 128, 2: 128, 3: 64, 4: 256, 5: 128, 6: 128, 7: 64, 8: 256}
F32_FAMILY = {16: [5, 6, 7, 8], 0: [1, 2, 3, 4, 5, 6, 7, 8]}


def _width(tile):
    if 40000 <= tile < 50000:
        return 256
    if tile >= 70000:
        return tile % 1000
    return tile % 10000 if tile % 10000 < 1000 else tile % 10000 - 1000


def _legal(candidates, N):
    return {t for t in candidates if N % _width(t) == 0}


def test_the_legal_sets_of_n_192():
    assert _legal(F16_CANDIDATES, 192) == {64, 1064, 10064, 11064}
    assert _legal(X3I_CANDIDATES, 192) == {71064, 70064}
    assert [{t for t in F32_FAMILY[f] if 192 % F32_WIDTH[t] == 0} for f in (16, 0)] == [{7}, {3, 7}]


def _tuned_then_forced(lib, run, query, force_key, legal, what):
    """One eager autotuned call of a shape, the tile the cache then reports, and the same call with that
    tile forced."""
    auto = run()
    tile = query()
    print(f'{what}: autotuned tile {tile}, legal {sorted(legal)}')
    assert tile in legal, f'{what}: tile {tile} is not one of {sorted(legal)}'
    _lib.check(lib.mec_set_option(force_key, tile), force_key.decode())
    try:
        forced = run()
    finally:
        lib.mec_set_option(force_key, 0)
    assert torch.equal(auto, forced), f'{what}: autotuned output differs from forced tile {tile}'
    return auto.cpu().numpy().astype(np.float64)


@pytest.mark.parametrize('N', [192, 384])
def test_autotuner_chooses_a_catalogued_tile_legal_for_n(dev, N):
    lib = _lib.load()
    rng = np.random.default_rng(N)
    A = rng.standard_normal((M, K)).astype(np.float32)
    W = (rng.standard_normal((N, K)) * 0.03).astype(np.float32)
    bias = rng.standard_normal(N).astype(np.float32)
    absum = np.abs(A).astype(np.float64) @ np.abs(W).astype(np.float64).T + np.abs(bias) + 1
    ref = A.astype(np.float64) @ W.astype(np.float64).T + bias
    bd = torch.from_numpy(bias).to(dev)
    query = lambda: lib.mec_gemm_query(0, M, N, K)  # noqa: E731
    try:
        _lib.check(lib.mec_set_option(b'gemm_autotune', 1), 'gemm_autotune')
        _lib.check(lib.mec_set_option(b'gemm_bn', 0), 'gemm_bn')
        _lib.check(lib.mec_set_option(b'gemm_f32_tile', 0), 'gemm_f32_tile')

        # split operands (mec_gemm_f16x3; weights pre-scaled by 2^8, undone by oscale), K-interleaved then pass-major
        Ax, Wx = torch.from_numpy(_split(A)).to(dev), torch.from_numpy(_split(W, 256.0)).to(dev)

        def run_x3():
            C = torch.empty((M, N), device=dev)
            _lib.check(lib.mec_gemm_f16x3(_p(Ax), M * K, _p(Wx), N * K, ctypes.c_float(1 / 256), _p(bd), None, None, 0,
                                          _p(C), M, N, K, 0, _s()), 'mec_gemm_f16x3')
            torch.cuda.synchronize()
            return C

        for order, cands in ((1, X3I_CANDIDATES), (0, F16_CANDIDATES)):
            with x3_order(order):
                got = _tuned_then_forced(lib, run_x3, query, b'gemm_bn', _legal(cands, N), f'split order {order} N={N}')
            assert (np.abs(got - ref) <= 2e-6 * absum).all()  # test_gpu_fp32x3's bar

        # f16 operands (mec_gemm_f16)
        A16, W16 = torch.from_numpy(A).half().to(dev), torch.from_numpy(W).half().to(dev)
        ref16 = A16.cpu().double() @ W16.cpu().double().T + torch.from_numpy(bias).double()

        def run_f16():
            C = torch.empty((M, N), device=dev)
            _lib.check(lib.mec_gemm_f16(_p(A16), _p(W16), _p(bd), None, 0, None, _p(C), M, N, K, 0, _s()), 'mec_gemm_f16')
            torch.cuda.synchronize()
            return C

        got = _tuned_then_forced(lib, run_f16, query, b'gemm_bn', _legal(F16_CANDIDATES, N), f'f16 N={N}')
        assert _rel_err(torch.from_numpy(got), ref16) < 1e-5  # test_gpu_kernels' bar

        # fp32 operands (mec_gemm_f32), the autotune held to the 16x16x4 family and free
        A32, W32 = torch.from_numpy(A).to(dev), torch.from_numpy(W).to(dev)

        def run_f32():
            C = torch.empty((M, N), device=dev)
            _lib.check(lib.mec_gemm_f32(_p(A32), _p(W32), _p(bd), None, _p(C), M, N, K, 0, _s()), 'mec_gemm_f32')
            torch.cuda.synchronize()
            return C

        for family in (16, 0):
            _lib.check(lib.mec_set_option(b'gemm_f32_family', family), 'gemm_f32_family')
            legal = {t for t in F32_FAMILY[family] if N % F32_WIDTH[t] == 0}
            got = _tuned_then_forced(lib, run_f32, lambda: lib.mec_gemm_f32_query(0, M, N, K), b'gemm_f32_tile', legal,
                                     f'fp32 family {family} N={N}')
            assert (np.abs(got - ref) <= 2e-6 * absum).all()  # the fp32 GEMM bar (test_gpu_fp32, elementwise)
    finally:  # the defaults
        for k, v in ((b'gemm_autotune', 1), (b'gemm_bn', 0), (b'gemm_f32_tile', 0), (b'gemm_f32_family', 16),
                     (b'gemm_x3_order', 1)):
            lib.mec_set_option(k, v)
