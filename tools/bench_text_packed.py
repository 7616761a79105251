#!/usr/bin/env python3
"""Times the packed BERT text path (TextEncoder.forward_packed) against the padded one at B = 256.

Per precision and per length set, on ONE handle and with hipEvents around windows of whole forwards:
  (a) forward on the padded batch [B,128];
  (b) forward_packed on the same batch (the host plan, its upload and the pack kernel included);
  (c) forward on Bp full rows (what the encoder alone costs at the packed size).
(b)/(a) is what packing buys; (b)/(c) is what it costs over the bare encoder at Bp rows: the plan and its
upload, the pack kernel, the segment compares and a [CLS] tail over B samples instead of Bp. The three are
timed in alternating windows (same clocks, same neighbours) after every shape was warmed up (and its GEMM
tiles autotuned); the median window is reported with min / max. Per-tag kernel times (mec_prof_enable) of
(b) and (c) follow in passes of their own, so a (b)/(c) above 10 % can be pinned on a launch class;
"untagged" is the rest of the forward (embedding, pack kernel, the [CLS]-only last layer, the heads).

Length sets: syn.text_inputs(256, ragged=True) (U[8,128]) and a seeded short set U[6,40].
Prints one JSON line; --out also writes it to a file (profiles/text_packed_b256.json).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'multimodal-emotion-classification_amd'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mec import engine, synthetic as syn  # noqa: E402

BERT_TAGS = ('bert_qkv', 'bert_attn', 'bert_oproj', 'bert_ffn1', 'bert_ffn2', 'bert_ln')


def length_sets(B):
    ids, mask = syn.text_inputs(B, 128, seed=0, ragged=True)
    yield 'ragged_u8_128', ids, mask
    lens = np.random.default_rng(20240).integers(6, 41, size=B)
    ids, _ = syn.text_inputs(B, 128, seed=1)
    mask = (np.arange(128)[None, :] < lens[:, None]).astype(np.int32)
    ids[np.arange(B), lens - 1] = 102
    ids[mask == 0] = 0
    yield 'short_u6_40', ids, mask


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def tag_ms(model, fn, iters, total):
    out = {}
    for tag in BERT_TAGS:
        model.prof_enable(tag)
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        out[tag] = model.prof_read()[0] / iters
    model.prof_enable(0)
    out['untagged'] = total - sum(out.values())
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--precisions', default='f16,fp32,fp32x3')
    ap.add_argument('--iters', type=int, default=10, help='forwards per timed window')
    ap.add_argument('--warmup', type=int, default=5, help='forwards of every shape before timing')
    ap.add_argument('--repeats', type=int, default=7, help='alternating windows per variant (median reported)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_text_packed: no GPU visible (nothing is measured on the CPU)')
    dev = torch.device('cuda', 0)
    B = a.batch
    res = {'device': torch.cuda.get_device_name(0), 'batch': B, 'iters': a.iters, 'warmup': a.warmup,
           'repeats': a.repeats, 'runs': []}
    for prec in a.precisions.split(','):
        m = engine.TextEncoder(device=dev, precision=prec)
        for name, ids, mask in length_sets(B):
            lens = mask.sum(1).astype(np.int32)
            bp = m.pack_plan(lens)[2]
            d_ids, d_mask = engine.to_device(ids, dev), engine.to_device(mask, dev)
            f_ids, f_mask = (engine.to_device(t, dev) for t in syn.text_inputs(bp, 128, seed=2))
            fns = {'a_padded': lambda: m.forward(d_ids, d_mask),
                   'b_packed': lambda: m.forward_packed(d_ids, lens=lens),
                   'c_full_bp_rows': lambda: m.forward(f_ids, f_mask)}
            for fn in fns.values():
                for _ in range(a.warmup):
                    fn()
            torch.cuda.synchronize()
            m.check()
            t = {k: [] for k in fns}
            for _ in range(a.repeats):
                for k, fn in fns.items():
                    t[k].append(timed(fn, a.iters))
            ms = {k: statistics.median(v) for k, v in t.items()}
            run = {'precision': prec, 'lengths': name, 'tokens': int(lens.sum()), 'Bp': bp,
                   'ms': ms, 'ms_min_max': {k: [min(v), max(v)] for k, v in t.items()},
                   'b_over_a': ms['b_packed'] / ms['a_padded'], 'b_over_c': ms['b_packed'] / ms['c_full_bp_rows'],
                   'rows_per_s': {k: B / v * 1e3 for k, v in ms.items() if k != 'c_full_bp_rows'},
                   'tag_ms_per_forward': {k: tag_ms(m, fns[k], a.iters, ms[k]) for k in ('b_packed', 'c_full_bp_rows')}}
            m.check()
            print(f"{prec:7s} {name:14s} Bp {bp:3d}  a {ms['a_padded']:.3f}  b {ms['b_packed']:.3f}  "
                  f"c {ms['c_full_bp_rows']:.3f} ms  b/a {run['b_over_a']:.3f}  b/c {run['b_over_c']:.3f}", file=sys.stderr)
            res['runs'].append(run)
        m.close()
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
