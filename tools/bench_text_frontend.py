"""Time the text paths from strings to probabilities with tokenize='host' and tokenize='gpu'.

    python3 tools/bench_text_frontend.py --batch 256 --out profiles/text_frontend_bench.json

Everything is measured on the GPU host in one run. Seeded texts of U[6,40] words over a synthetic
vocabulary (no trained vocabulary exists offline: 30000 WordPiece entries for BERT, the 10000 most
frequent words for the Keras index, Zipf-distributed word choice, a share of texts made non-ASCII so that
the BERT path routes them to the host). For the BiLSTM class (FastTextEmotionPredictor) and for BERT f16
with pack=True (TextInference.predict_texts) the two settings alternate, after a warm-up, and a host
clock runs from the list of strings to the synchronized probabilities on the host; medians and min / max
over the repeats are reported, with the device-event time of mec_tok_encode alone and the share of rows
routed to the host. Prints one JSON line; --out also writes it to a file.

    python3 tools/bench_text_frontend.py --utf8-shares 0,0.02,0.3,1 --out profiles/text_frontend_utf8.json

measures, instead, BERT f16 pack=True with tokenize='host', 'gpu' and 'gpu_utf8' alternating, once per
share of non-ASCII texts (curly quotes, dashes, an ellipsis, accented vowels, emoji, no-break spaces put
into the same seeded texts), with the rows each GPU setting routes to the host and the device-event time
of mec_tok_encode for both WordPiece kinds on the same texts.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'multimodal-emotion-classification_amd'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mec import engine, tokenize as mtok  # noqa: E402


def make_words(n, rng):
    """n distinct pronounceable pseudo-words of 1..4 syllables, most frequent first."""
    cons, vow = 'bcdfghjklmnprstvwz', 'aeiou'
    seen, out = set(), []
    while len(out) < n:
        w = ''.join(cons[int(rng.integers(len(cons)))] + vow[int(rng.integers(len(vow)))]
                    + ('' if rng.random() < 0.6 else cons[int(rng.integers(len(cons)))])
                    for _ in range(int(rng.integers(1, 5))))
        if w not in seen:
            seen.add(w)
            out.append(w)
    return out


def make_texts(words, n_batches, B, rng, non_ascii):
    rank = np.arange(1, len(words) + 1, dtype=np.float64)
    p = (1 / rank) / (1 / rank).sum()
    suffix = ['s', 'ing', 'ed', 'ly', 'er']
    batches = []
    for _ in range(n_batches):
        texts = []
        for _ in range(B):
            ws = [words[int(i)] for i in rng.choice(len(words), int(rng.integers(6, 41)), p=p)]
            ws = [w + suffix[int(rng.integers(5))] if rng.random() < 0.1 else w for w in ws]
            t = ' '.join(ws).capitalize() + '.!?'[int(rng.integers(3))]
            if rng.random() < non_ascii:
                t += ' déjà vu'
            texts.append(t)
        batches.append(texts)
    return batches


ACCENTS = {'a': 'á', 'e': 'é', 'i': 'ï', 'o': 'ô', 'u': 'ü'}
RICH_VOCAB = ['—', '“', '”', '’', '…', '😀', '##😀']


def enrich(text, rng):
    """The text with what real input has: an accented vowel, a dash, curly quotes, an ellipsis, an emoji, a
    no-break space (one to three of these; always at least one non-ASCII character)."""
    ws = text.split(' ')
    for k in rng.choice(6, int(rng.integers(1, 4)), replace=False).tolist():
        i = int(rng.integers(len(ws)))
        if k == 0:
            hit = [j for j, c in enumerate(ws[i]) if c in ACCENTS]
            ws[i] = ws[i][:hit[0]] + ACCENTS[ws[i][hit[0]]] + ws[i][hit[0] + 1:] if hit else ws[i] + '’s'
        elif k == 1:
            ws[i] += ' —'
        elif k == 2:
            ws[i] = '“' + ws[i] + '”'
        elif k == 3:
            ws[-1] = ws[-1].rstrip('.!?') + '…'
        elif k == 4:
            ws[i] += ' 😀' if rng.random() < 0.5 else '😀'
        else:
            ws[i] += '\xa0' + ws[i]
    return ' '.join(ws)


def utf8_report(a, dev, words, vocab, res):
    """BERT f16 pack=True, three tokenize settings alternating, per share of non-ASCII texts."""
    from transformers import BertTokenizerFast
    from inference.text_inference import TextInference
    B = a.batch
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, 'vocab.txt'), 'w', encoding='utf-8') as f:
            f.write('\n'.join(vocab + RICH_VOCAB) + '\n')
        fast = BertTokenizerFast.from_pretrained(d)
    kinds = ('host', 'gpu', 'gpu_utf8')
    bert = {k: TextInference(seed=1234, device=dev, tokenizer=fast, precision='f16', tokenize=k) for k in kinds}
    fns = {k: (lambda texts, m=m: m.predict_texts(texts, pack=True)) for k, m in bert.items()}
    res['wordpiece_vocab'] = len(vocab + RICH_VOCAB)
    res['shares'] = {}
    for share in a.utf8_shares:
        rng = np.random.default_rng(0)
        batches = make_texts(words, a.batches, B, rng, 0.0)
        batches = [[enrich(t, rng) if rng.random() < share else t for t in b] for b in batches]
        assert bert['host'].predict_texts(batches[0], pack=True) == bert['gpu_utf8'].predict_texts(batches[0], pack=True)
        for k, fn in fns.items():
            for texts in batches:
                fn(texts)
            clocked(fn, batches, a.warmup, dev)
        ms = {k: [] for k in kinds}
        for r in range(a.repeats):
            for k, fn in fns.items():
                ms[k] += clocked(fn, [batches[r % len(batches)]], 1, dev)
        out = {'non_ascii_texts_share': float(np.mean([not t.isascii() for b in batches for t in b])),
               'mean_text_bytes': float(np.mean([len(t.encode()) for b in batches for t in b]))}
        for k in kinds:
            out[k] = summary(ms[k], B)
        for k in kinds[1:]:
            gt = bert[k].gpu_tokenizer
            routed = []
            for texts in batches:
                gt.encode(texts)
                routed.append(gt.host_rows / B)
            out[k]['rows_routed_to_host_share'] = float(np.mean(routed))
            out[k]['over_host_speedup'] = statistics.median(ms['host']) / statistics.median(ms[k])
            ev = [encode_event_ms(gt, batches[0], 50) for _ in range(a.event_repeats)]
            out[k]['tok_encode_event_ms'] = {'median': statistics.median(ev), 'min_max': [min(ev), max(ev)]}
            out[k]['tokenize_only'] = summary(clocked(gt.encode, batches, a.repeats, dev), B)
        out['host']['tokenize_only'] = summary(clocked(
            lambda texts: [engine.to_device(x, dev) for x in bert['host'].encode_batch(texts)], batches, a.repeats, dev), B)
        out['gpu_utf8_over_gpu_speedup'] = statistics.median(ms['gpu']) / statistics.median(ms['gpu_utf8'])
        res['shares'][str(share)] = out
    return res


def clocked(fn, batches, repeats, device):
    out = []
    for r in range(repeats):
        texts = batches[r % len(batches)]
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        fn(texts)
        torch.cuda.synchronize(device)
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def summary(ms, B):
    med = statistics.median(ms)
    return {'ms_per_batch': med, 'ms_min_max': [min(ms), max(ms)], 'texts_per_s': B / med * 1e3}


def encode_event_ms(gt, texts, iters):
    """Device-event time of mec_tok_encode alone: the bytes and offsets already on the device."""
    blob, off, _ = mtok.pack_texts(texts, gt._on_host)
    dev, B, L = gt.device, len(texts), gt.L
    text_d, off_d = engine.to_device(blob, dev), engine.to_device(off, dev)
    ids = torch.empty((B, L), dtype=torch.int32, device=dev)
    mask, n = torch.empty_like(ids), torch.empty((B,), dtype=torch.int32, device=dev)
    p = lambda t: engine._ptr(t)  # noqa: E731

    def run():
        rc = gt.lib.mec_tok_encode(gt.handle, p(text_d), p(off_d), B, L, p(ids), p(mask), p(n), engine._stream(dev))
        assert rc == 0
    for _ in range(5):
        run()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        run()
    e1.record()
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--repeats', type=int, default=51)
    ap.add_argument('--warmup', type=int, default=4)
    ap.add_argument('--batches', type=int, default=4, help='distinct text batches, cycled')
    ap.add_argument('--non-ascii', type=float, default=0.02, help='share of texts made non-ASCII')
    ap.add_argument('--vocab', type=int, default=30000)
    ap.add_argument('--utf8-shares', type=lambda v: [float(x) for x in v.split(',')], default=None,
                    help="comma-separated shares of non-ASCII texts: measure BERT with 'host', 'gpu' and 'gpu_utf8' at each")
    ap.add_argument('--event-repeats', type=int, default=11, help='--utf8-shares: event timings of mec_tok_encode')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_text_frontend: no GPU visible (nothing is measured on the CPU)')
    from transformers import BertTokenizerFast
    from inference.text_inference import TextInference
    from inference.text_lstm_inference import FastTextEmotionPredictor, KerasWordIndex
    dev = torch.device('cuda', 0)
    B = a.batch
    rng = np.random.default_rng(0)
    words = make_words(a.vocab - 100, rng)
    batches = make_texts(words, a.batches, B, rng, a.non_ascii)
    chars = [chr(c) for c in range(33, 127) if not chr(c).isupper()]
    vocab = (['[PAD]', '[UNK]', '[CLS]', '[SEP]', '[MASK]'] + chars + ['##' + c for c in chars if c.isalnum()]
             + ['##s', '##ing', '##ed', '##ly', '##er'] + words)
    vocab = list(dict.fromkeys(vocab))
    res = {'device': torch.cuda.get_device_name(0), 'batch': B, 'repeats': a.repeats, 'warmup': a.warmup,
           'words_per_text': [6, 40], 'wordpiece_vocab': len(vocab), 'non_ascii_share': a.non_ascii,
           'mean_text_bytes': float(np.mean([len(t.encode()) for b in batches for t in b]))}

    if a.utf8_shares is not None:
        del res['non_ascii_share'], res['mean_text_bytes']
        finish(utf8_report(a, dev, words, vocab, res), a.out)
        return

    wi = KerasWordIndex({'<OOV>': 1, **{w: i + 2 for i, w in enumerate(words)}}, num_words=10000)
    lstm = {k: FastTextEmotionPredictor(seed=1234, device=dev, word_index=wi, tokenize=k) for k in ('host', 'gpu')}
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, 'vocab.txt'), 'w') as f:
            f.write('\n'.join(vocab) + '\n')
        fast = BertTokenizerFast.from_pretrained(d)
    bert = {k: TextInference(seed=1234, device=dev, tokenizer=fast, precision='f16', tokenize=k)
            for k in ('host', 'gpu')}
    paths = {'bilstm': {k: m._forward for k, m in lstm.items()},
             'bert_f16_packed': {k: (lambda texts, m=m: m.predict_texts(texts, pack=True)) for k, m in bert.items()}}
    for name, fns in paths.items():
        for k, fn in fns.items():  # warm-up: every batch once (packed GEMM shapes autotune per packed row count)
            for texts in batches:
                fn(texts)
            clocked(fn, batches, a.warmup, dev)
        ms = {'host': [], 'gpu': []}
        for r in range(a.repeats):  # the two settings alternate
            for k, fn in fns.items():
                ms[k] += clocked(fn, [batches[r % len(batches)]], 1, dev)
        gt = (lstm if name == 'bilstm' else bert)['gpu'].gpu_tokenizer
        prep = [t.lower().strip() for t in batches[0]] if name == 'bilstm' else batches[0]
        gt.encode(prep)
        res[name] = {'host': summary(ms['host'], B), 'gpu': summary(ms['gpu'], B),
                     'gpu_over_host_speedup': statistics.median(ms['host']) / statistics.median(ms['gpu']),
                     'tok_encode_event_ms': encode_event_ms(gt, prep, 50),
                     'rows_routed_to_host_share': gt.host_rows / B}
        # the tokenizer call alone on the host clock, both settings (strings -> ids on the device, synchronized)
        if name == 'bilstm':
            host_tok = lambda texts: engine.to_device(  # noqa: E731
                wi.padded([t.lower().strip() for t in texts], 128), dev)
            gpu_tok = lambda texts: gt.encode([t.lower().strip() for t in texts])  # noqa: E731
        else:
            host_tok = lambda texts: [engine.to_device(x, dev) for x in bert['host'].encode_batch(texts)]  # noqa: E731
            gpu_tok = gt.encode
        res[name]['tokenize_only'] = {'host': summary(clocked(host_tok, batches, a.repeats, dev), B),
                                      'gpu': summary(clocked(gpu_tok, batches, a.repeats, dev), B)}
    finish(res, a.out)


def finish(res, out):
    print(json.dumps(res))
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
