"""Planar against paired fp32x3 planes on the BERT text path's split GEMMs at B = 256 (mec_gemm_f16x3
against mec_gemm_f16x3_paired at one forced tile), the two arms in alternating rounds of one process
on random data; one JSON line per (shape, tile).

    python tools/bench_x3_paired.py [--rounds 9] [--iters 20] [--shapes ffn1 ffn2 oproj kv] [--out FILE]

us / min / max: median and extremes of an arm's rounds. `gain_us` = planar median - paired median;
`clear` is set when it exceeds the planar arm's full spread (max - min). Every run also checks that the
two arms' outputs are the same bits.
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

# name: (M, N, K, act, f32 residual + f32 out (else hi / lo planes out), tiles). FFN1 and FFN2 at their
# pins (FFN2: 72128 alone, 70256 inside the fused step); the O-projection and the last layer's K | V
# projection are autotuned in the model, so every candidate that divides N is timed
SHAPES = {
    'ffn1': (32768, 3072, 768, 5, False, [70256]),
    'ffn2': (32768, 768, 3072, 0, True, [72128, 70256]),
    'oproj': (32768, 768, 768, 0, True, [70256, 70128, 71128]),
    'kv': (32768, 1536, 768, 0, False, [70256, 70128, 71128]),
}


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
    for name in a.shapes:
        M, N, K, act, res, tiles = SHAPES[name]
        ax = torch.randn(M, K, device=dev) * 0.5
        bx = torch.randn(N, K, device=dev) * K ** -0.5
        ah, bh = ax.half(), bx.half()
        al, bl = (ax - ah.float()).half(), (bx - bh.float()).half()
        A2, B2 = torch.stack((ah, al)).contiguous(), torch.stack((bh, bl)).contiguous()
        Ap, Bp = x3pair.pair(ah, al), x3pair.pair(bh, bl)
        del ax, bx, ah, al, bh, bl
        bias = torch.randn(N, device=dev)
        R = torch.randn(M, N, device=dev) if res else None
        o16 = torch.empty(2, M, N, device=dev, dtype=torch.float16) if not res else None
        o16p = torch.empty(M, 2 * N, device=dev, dtype=torch.float16) if not res else None
        o32 = [torch.empty(M, N, device=dev) for _ in range(2)] if res else [None, None]

        def planar():
            _lib.check(lib.mec_gemm_f16x3(p(A2), M * K, p(B2), N * K, 1.0, p(bias), p(R), p(o16), M * N if not res else 0,
                                          p(o32[0]), M, N, K, act, st), name)

        def paired():
            _lib.check(lib.mec_gemm_f16x3_paired(p(Ap), p(Bp), 1.0, p(bias), p(R), p(o16p), 1, 0, p(o32[1]), M, N, K,
                                                 act, st), name)
        arms = (('planar', planar), ('paired', paired))
        for tile in tiles:
            _lib.check(lib.mec_set_option(b'gemm_bn', tile), 'gemm_bn')
            for _, f in arms:  # warm
                f()
            torch.cuda.synchronize()
            if res:
                same = torch.equal(o32[0], o32[1])
            else:
                hi, lo = x3pair.unpair(o16p)
                same = torch.equal(hi, o16[0]) and torch.equal(lo, o16[1])
                del hi, lo
            times = {n: [] for n, _ in arms}
            for _ in range(a.rounds):
                for n, f in arms:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.iters):
                        f()
                    e1.record()
                    torch.cuda.synchronize()
                    times[n].append(e0.elapsed_time(e1) / a.iters * 1e3)
            r = {'shape': name, 'M': M, 'N': N, 'K': K, 'tile': tile, 'same_bits': same}
            for n, _ in arms:
                t = sorted(times[n])
                r[n] = {'us': round(t[len(t) // 2], 1), 'min': round(t[0], 1), 'max': round(t[-1], 1)}
            r['gain_us'] = round(r['planar']['us'] - r['paired']['us'], 1)
            r['gain_pct'] = round(100 * r['gain_us'] / r['planar']['us'], 2)
            r['clear'] = r['gain_us'] > r['planar']['max'] - r['planar']['min']
            line = json.dumps(r)
            print(line, flush=True)
            if a.out:
                with open(a.out, 'a') as fh:
                    fh.write(line + '\n')
        lib.mec_set_option(b'gemm_bn', 0)


if __name__ == '__main__':
    main()
