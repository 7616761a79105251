"""Time the BiLSTM text model (csrc/text_lstm.hip) against the HIP BERT text path, fp32, same batch.

    python3 tools/bench_text_lstm.py --batch 256 --out profiles/text_lstm_bench.json

Everything is measured on the GPU in one run: each model is warmed up (GEMM autotuning included),
then timed with device events around `iters` back-to-back forwards, `repeats` times, the two models
alternating; the medians are reported. Per-kernel times come from the library's hipEvent hook
(mec_prof_enable) in passes of their own, one launch class at a time: layer 1's recurrence (which
gathers the projected table itself), layer 2's input projection (fp32 GEMM), layer 2's recurrence,
the dense head. `--sweep` repeats the LSTM timing (whole forward and both recurrences) at every
"lstm_rows" tile. Prints one JSON line; --out also writes it to a file.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'multimodal-emotion-classification_amd'))

import torch  # noqa: E402

from mec import engine, synthetic as syn  # noqa: E402

LSTM_TAGS = ('lstm_rec1', 'lstm_proj', 'lstm_rec2', 'lstm_head')


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def kernel_ms(model, fn, iters):
    out = {}
    for tag in LSTM_TAGS:
        model.prof_enable(tag)
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        ms, n = model.prof_read()
        out[tag] = ms / max(n, 1)
    model.prof_enable(0)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--iters', type=int, default=50, help='LSTM forwards per timed window')
    ap.add_argument('--bert-iters', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--sweep', action='store_true', help='also time every lstm_rows tile')
    ap.add_argument('--no-bert', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_text_lstm: no GPU visible (nothing is measured on the CPU)')
    dev = torch.device('cuda', 0)
    B = a.batch
    lstm = engine.LstmTextEncoder(device=dev)
    ids = engine.to_device(syn.text_lstm_inputs(B, 128, seed=0, ragged=True), dev)
    f_lstm = lambda: lstm.forward(ids)  # noqa: E731
    res = {'device': torch.cuda.get_device_name(0), 'batch': B, 'iters': a.iters, 'repeats': a.repeats}
    bert = None
    if not a.no_bert:
        bert = engine.TextEncoder(device=dev, precision='fp32')
        bids, bmask = (engine.to_device(t, dev) for t in syn.text_inputs(B, 128, seed=0, ragged=True))
        f_bert = lambda: bert.forward(bids, bmask)  # noqa: E731
        for _ in range(max(2, a.warmup // 2)):
            f_bert()
    for _ in range(a.warmup):
        f_lstm()
    torch.cuda.synchronize()
    t_lstm, t_bert = [], []
    for _ in range(a.repeats):
        t_lstm.append(timed(f_lstm, a.iters))
        if bert is not None:
            t_bert.append(timed(f_bert, a.bert_iters))
    ms = statistics.median(t_lstm)
    res['lstm'] = {'lstm_rows': 'default', 'ms_per_forward': ms, 'ms_min_max': [min(t_lstm), max(t_lstm)],
                   'samples_per_s': B / ms * 1e3, 'kernel_ms': kernel_ms(lstm, f_lstm, a.iters)}
    if bert is not None:
        mb = statistics.median(t_bert)
        res['bert_fp32'] = {'ms_per_forward': mb, 'ms_min_max': [min(t_bert), max(t_bert)], 'samples_per_s': B / mb * 1e3}
        res['lstm_over_bert_speedup'] = mb / ms
    if a.sweep:
        res['sweep'] = []
        for rows in (1, 2, 4):
            lstm.set_option('lstm_rows', rows)
            for _ in range(a.warmup):
                f_lstm()
            torch.cuda.synchronize()
            t = [timed(f_lstm, a.iters) for _ in range(a.repeats)]
            k = kernel_ms(lstm, f_lstm, a.iters)
            res['sweep'].append({'lstm_rows': rows, 'ms_per_forward': statistics.median(t), 'ms_min_max': [min(t), max(t)],
                                 'rec1_ms': k['lstm_rec1'], 'rec2_ms': k['lstm_rec2']})
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
