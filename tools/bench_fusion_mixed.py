"""Mixed-modality batches on the GPU: what the routed fusion call and FusedPipeline.forward_mixed cost.

1. Fusion call: mec_fusion_fwd_mixed at B rows, all present, against mec_fusion_fwd on the same rows, both under
   the library's hipEvent hook (mec_prof_enable, TAG_FUSION), in alternating windows. --parent-lib names a
   build of another commit's library (the same ABI): its mec_fusion_fwd joins the alternation.
2. Pipeline: FusedPipeline.forward_mixed in requests/s, (a) all present against `forward`, (b) a seeded mix with
   each modality present with probability p against the one alternative without forward_mixed: one sub-batch
   per presence pattern (its encoders, then mec_fusion_fwd for the all-three pattern, mec_fuse_weighted for
   the two-modality ones), each sub-batch's inputs already split. Alternating windows, every shape warmed up
   (and autotuned) first; median window with min / max.
Prints one JSON line; --out also writes it to a file. Reads nothing outside the repository."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'multimodal-emotion-classification_amd'))

from mec import _lib, engine, synthetic as syn  # noqa: E402


def spread(v):
    return {'median': statistics.median(v), 'min': min(v), 'max': max(v)}


def load_other(path):
    """A library of another commit: the signatures of the entry points it has."""
    lib = ctypes.CDLL(os.path.abspath(path))
    for name, (res, args) in _lib.SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, args
    return lib


def fusion_call(B, iters, repeats, dev, parent_lib):
    rng = np.random.default_rng(5)
    feats = [engine.to_device(rng.random((B, d), np.float32), dev) for d in (64, 768, 512)]
    preds = [torch.softmax(engine.to_device(rng.standard_normal((B, 7)).astype(np.float32), dev), 1) for _ in range(3)]
    head = engine.FusionHead(device=dev)
    plan = engine.fusion_mixed_plan([7] * B, True, dev)
    pairs = list(zip(feats, preds))
    runs = {'mixed': (head, lambda: head.forward_mixed(plan, *pairs)), 'dense': (head, lambda: head.forward(*feats, *preds))}
    if parent_lib:
        load, engine._lib.load = engine._lib.load, (lambda lib=load_other(parent_lib): lib)
        try:
            old = engine.FusionHead(device=dev)
        finally:
            engine._lib.load = load
        runs['parent_dense'] = (old, lambda: old.forward(*feats, *preds))
    a, b = runs['mixed'][1](), runs['dense'][1]()
    torch.cuda.synchronize()
    same = bool(torch.equal(a[0].float(), b[1]) and torch.equal(a[1], b[0]) and torch.equal(a[2], b[2]))
    us = {k: [] for k in runs}
    for _ in range(repeats):
        for k, (m, fn) in runs.items():
            for _ in range(3):
                fn()
            m.prof_enable('fusion')
            for _ in range(iters):
                fn()
            torch.cuda.synchronize()
            ms, n = m.prof_read()
            m.prof_enable(0)
            us[k].append(1e3 * ms / max(n, 1))
    return {'B': B, 'iters': iters, 'mixed_equals_dense_bits': same, 'us_per_call': {k: spread(v) for k, v in us.items()}}


def window(fn, iters, pipe):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    pipe.wait()
    torch.cuda.synchronize()
    return iters / (time.perf_counter() - t0)


def pipeline(B, p, iters, repeats, dev, precision):
    pipe = engine.FusedPipeline(device=dev, precision=precision)
    ids, mask = syn.text_inputs(B, 128, seed=9, ragged=False)
    full = [engine.to_device(a, dev) for a in (syn.speech_inputs(B, seed=9), ids, mask, syn.image_inputs(B, seed=9))]
    flags = np.random.default_rng(11).random((B, 3)) < p
    bits = flags.astype(np.uint8) @ np.array([1, 2, 4], np.uint8)
    compact = [t[torch.from_numpy(np.flatnonzero(flags[:, m])).to(dev)].contiguous()
               for t, m in zip(full, (0, 1, 1, 2))]
    subs = []  # one sub-batch per non-empty pattern: its rows of each modality it has
    for pat in range(1, 8):
        rows = torch.from_numpy(np.flatnonzero(bits == pat)).to(dev)
        if len(rows):
            subs.append((pat, [t[rows].contiguous() for t in full]))

    def split():
        pipe.wait()  # the encoder handles are used on this stream below: the last all-three sub-batch must be done
        for pat, (x, i, m, g) in subs:
            if pat == 7:
                pipe.forward(x, i, m, g)
                continue
            s = pipe.speech.forward(x) if pat & 1 else None
            t = pipe.text.forward(i, m) if pat & 2 else None
            im = pipe.image.forward(g) if pat & 4 else None
            if sum(o is not None for o in (s, t, im)) > 1:
                engine.fuse_weighted(*(None if o is None else o[2] for o in (s, t, im)))

    runs = {'forward': lambda: pipe.forward(*full), 'mixed_all_present': lambda: pipe.forward_mixed(*full, [7] * B),
            'mixed_p': lambda: pipe.forward_mixed(*compact, bits), 'split_by_pattern_p': split}
    for fn in runs.values():  # serial autotune call, then a few concurrent ones
        for _ in range(3):
            fn()
    pipe.wait()
    torch.cuda.synchronize()
    rate = {k: [] for k in runs}
    for _ in range(repeats):
        for k, fn in runs.items():
            rate[k].append(B * window(fn, iters, pipe))
    pipe.check()
    return {'B': B, 'precision': precision, 'p': p, 'iters': iters,
            'counts': [int(flags[:, m].sum()) for m in range(3)], 'n_att': int((bits == 7).sum()),
            'sub_batches': {int(pat): int(len(a[0])) for pat, a in subs},
            'requests_per_s': {k: spread(v) for k, v in rate.items()}}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--p', type=float, default=0.6)
    ap.add_argument('--precision', default='fp32x3')
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--fusion-iters', type=int, default=200)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--parent-lib', default=None)
    ap.add_argument('--skip-pipeline', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = engine.require_gpu()
    res = {'fusion_call': fusion_call(a.batch, a.fusion_iters, a.repeats, dev, a.parent_lib)}
    if not a.skip_pipeline:
        res['pipeline'] = pipeline(a.batch, a.p, a.iters, a.repeats, dev, a.precision)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
