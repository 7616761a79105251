"""gemm_x3_pp 0 (the two-stage ring) against 2 (the ping-pong schedule for every launch class) on the BERT
text path's paired split GEMMs at B = 256, tile 70256 forced, the two arms in alternating rounds of one
process on random data; one JSON line per shape.

    python tools/bench_x3_pp.py [--rounds 9] [--iters 20] [--shapes ffn1 ffn2 oproj kv] [--out FILE]

us / min / max: median and extremes of an arm's rounds. `gain_us` = ring median - ping-pong median; `clear`
is set when it exceeds the ring arm's full spread (max - min), tools/bench_x3_paired.py's rule. Every run
also checks that the two arms' outputs are the same bits. ffn2 and oproj run the deferred-LayerNorm
residual epilogue the model runs (mec_gemm_f16x3_paired_ln).
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'multimodal-emotion-classification_amd'))

import torch  # noqa: E402

from mec import _lib, x3pair  # noqa: E402

# name: (M, N, K, act, deferred-LN f32 residual + f32 out (else paired hi / lo planes out))
SHAPES = {
    'ffn1': (32768, 3072, 768, 5, False),
    'ffn2': (32768, 768, 3072, 0, True),
    'oproj': (32768, 768, 768, 0, True),
    'kv': (32768, 1536, 768, 0, False),
}
TILE = 70256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--shapes', nargs='+', default=list(SHAPES))
    ap.add_argument('--out', default=None, help='also append the JSON lines to this file')
    a = ap.parse_args()
    lib = _lib.load()
    dev = torch.device('cuda', 0)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    _lib.check(lib.mec_set_option(b'gemm_bn', TILE), 'gemm_bn')
    for name in a.shapes:
        M, N, K, act, res = SHAPES[name]
        ax = torch.randn(M, K, device=dev) * 0.5
        bx = torch.randn(N, K, device=dev) * K ** -0.5
        ah, bh = ax.half(), bx.half()
        Ap, Bp = x3pair.pair(ah, (ax - ah.float()).half()), x3pair.pair(bh, (bx - bh.float()).half())
        del ax, bx, ah, bh
        bias = torch.randn(N, device=dev)
        R = torch.randn(M, N, device=dev) if res else None
        stats = torch.stack((R.mean(1), R.var(1, unbiased=False).add(1e-12).rsqrt()), 1).contiguous() if res else None
        gamma = torch.rand(N, device=dev) + 0.5 if res else None
        beta = torch.randn(N, device=dev) if res else None
        out = [torch.empty(M, N, device=dev) if res else torch.empty(M, 2 * N, device=dev, dtype=torch.float16)
               for _ in range(2)]

        def run(pp):
            _lib.check(lib.mec_set_option(b'gemm_x3_pp', 2 * pp), 'gemm_x3_pp')
            o = out[pp]
            _lib.check(lib.mec_gemm_f16x3_paired_ln(p(Ap), p(Bp), 1.0, p(bias), p(R), p(stats), p(gamma), p(beta),
                                                    None if res else p(o), 1, 0, 1.0, p(o) if res else None, M, N, K,
                                                    act, None, st), name)
        for pp in (0, 1):  # warm
            run(pp)
        torch.cuda.synchronize()
        same = torch.equal(out[0], out[1])
        times = {0: [], 1: []}
        for _ in range(a.rounds):
            for pp in (0, 1):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                run(pp)
                e0.record()
                for _ in range(a.iters):
                    run(pp)
                e1.record()
                torch.cuda.synchronize()
                times[pp].append(e0.elapsed_time(e1) / a.iters * 1e3)
        r = {'shape': name, 'M': M, 'N': N, 'K': K, 'tile': TILE, 'grid': (M // 256) * (N // 256), 'same_bits': same}
        for pp, n in ((0, 'ring'), (1, 'pp')):
            t = sorted(times[pp])
            r[n] = {'us': round(t[len(t) // 2], 1), 'min': round(t[0], 1), 'max': round(t[-1], 1)}
        r['gain_us'] = round(r['ring']['us'] - r['pp']['us'], 1)
        r['gain_pct'] = round(100 * r['gain_us'] / r['ring']['us'], 2)
        r['clear'] = r['gain_us'] > r['ring']['max'] - r['ring']['min']
        line = json.dumps(r)
        print(line, flush=True)
        if a.out:
            with open(a.out, 'a') as fh:
                fh.write(line + '\n')
        del Ap, Bp, R, out
    lib.mec_set_option(b'gemm_bn', 0)
    lib.mec_set_option(b'gemm_x3_pp', 1)


if __name__ == '__main__':
    main()
