"""
BiLSTM text inference on the MI355X HIP path — drop-in for the reference's
inference/text_lstm_inference.py (same class, constructor, methods and result dicts).

The model arithmetic (Embedding -> two Bidirectional LSTMs -> three Dense layers -> softmax,
model_training/train_lstm_text_model.py:96-120) runs in the HIP kernels of csrc/text_lstm.hip
through libmec_hip.so; there is no CPU fallback. Tokenization restates Keras'
Tokenizer.texts_to_sequences + pad_sequences(padding='post', truncating='post') as the reference
calls them (:61-62, :101-102): on the host by default (tokenize='host'), or in the HIP kernel of
csrc/tokenizer.hip (tokenize='gpu', engine.GpuTokenizer: the same ids, so the same probabilities bit for bit).

The reference unpickles its tokenizer (`_tokenizer.pkl`). This module never unpickles anything:
it reads the word index from JSON, either Keras' own `tokenizer.to_json()` or a plain
{word: index} dict. Export it once, in the environment that trained the model:

    python -c "import pickle; t = pickle.load(open('models/text_model_tokenizer.pkl', 'rb')); \\
               open('models/text_lstm_tokenizer.json', 'w').write(t.to_json())"

Weights come from text_lstm_weights.npz (tools/convert_text_lstm_h5.py), an explicit `weights`
dict, or a synthetic `seed` (mec.checkpoints.resolve).
"""
import argparse
import json
import os
import time

import numpy as np

from config import Config
from mec import checkpoints, engine

KERAS_FILTERS = '!"#$%&()*+,-./:;<=>?@[\\]^_`{|}~\t\n'  # keras.preprocessing.text.Tokenizer's default


class KerasWordIndex:
    """Tokenizer.texts_to_sequences for a fitted word index: lower-case, every `filters` character
    becomes the split character, split on it, drop empty strings; a word whose index is >= num_words
    and a word not in the index both map to the OOV token's index (dropped when there is no OOV token)."""

    def __init__(self, word_index, num_words=10000, oov_token='<OOV>', filters=KERAS_FILTERS, lower=True, split=' '):
        self.word_index = {str(k): int(v) for k, v in word_index.items()}
        self.num_words = int(num_words) if num_words else None
        self.oov_index = self.word_index.get(oov_token) if oov_token is not None else None
        self.lower, self.split, self.filters = bool(lower), split, filters
        self._table = str.maketrans({c: split for c in filters})

    @classmethod
    def from_json(cls, path):
        if str(path).endswith('.pkl'):
            raise ValueError(f'{path}: a pickled tokenizer is never loaded; export tokenizer.to_json() '
                             '(see this module\'s docstring)')
        with open(path, 'r', encoding='utf-8') as f:
            obj = json.load(f)
        if isinstance(obj, dict) and 'config' in obj and 'word_index' in obj['config']:  # Tokenizer.to_json()
            cfg = obj['config']
            wi = cfg['word_index']
            wi = json.loads(wi) if isinstance(wi, str) else wi
            return cls(wi, cfg.get('num_words'), cfg.get('oov_token'), cfg.get('filters', KERAS_FILTERS),
                       cfg.get('lower', True), cfg.get('split', ' '))
        if not isinstance(obj, dict):
            raise ValueError(f'{path}: expected Tokenizer.to_json() output or a word -> index dict')
        return cls(obj)

    def words(self, text):
        if self.lower:
            text = text.lower()
        return [w for w in text.translate(self._table).split(self.split) if w]

    def sequence(self, text):
        out = []
        for w in self.words(text):
            i = self.word_index.get(w)
            if i is None or (self.num_words and i >= self.num_words):
                if self.oov_index is not None:
                    out.append(self.oov_index)
            else:
                out.append(i)
        return out

    def padded(self, texts, maxlen):
        """pad_sequences(padding='post', truncating='post'): int32 [len(texts), maxlen], 0-padded."""
        ids = np.zeros((len(texts), maxlen), np.int32)
        for r, t in enumerate(texts):
            s = self.sequence(t)[:maxlen]
            ids[r, :len(s)] = s
        return ids


class FastTextEmotionPredictor:
    """Fast LSTM-based text emotion predictor (reference: inference/text_lstm_inference.py:27-131).

    model_path: the reference's .h5 path (its converted text_lstm_weights.npz is read from the same
    directory) or the .npz itself; tokenizer_path: the tokenizer JSON. Added beyond the reference:
    weights / seed / device / word_index (a {word: index} dict instead of a tokenizer file) / tokenize
    ('host', the default: KerasWordIndex.padded; 'gpu': the ids are computed on the device, ValueError
    when the tokenizer's split / filters are not single ASCII characters)."""

    def __init__(self, model_path=None, tokenizer_path=None, weights=None, seed=None, device=None, word_index=None,
                 tokenize='host'):
        if tokenize not in ('host', 'gpu'):
            raise ValueError(f"tokenize must be 'host' or 'gpu', got {tokenize!r}")
        self.model_path = model_path or Config.TEXT_MODEL_PATH
        self.tokenizer_path = tokenizer_path or checkpoints.lstm_tokenizer_path()
        if weights is None and seed is None and model_path is not None:
            npz = model_path if str(model_path).endswith('.npz') else os.path.join(
                os.path.dirname(model_path), 'text_lstm_weights.npz')
            weights = checkpoints.load_text_lstm_npz(npz)
        w = checkpoints.resolve('text_lstm', weights, seed)
        if w is None:  # the reference's load_model raises too: this model has no heuristic fallback
            raise RuntimeError('BiLSTM text model not found: convert the trained .h5 with '
                               'tools/convert_text_lstm_h5.py (text_lstm_weights.npz)')
        # No silent CPU fallback: a missing libmec_hip.so or GPU raises MecError here.
        self.model = engine.LstmTextEncoder(w, device=device)
        self.device = self.model.device
        self.tokenizer = KerasWordIndex(word_index) if word_index is not None else KerasWordIndex.from_json(
            self.tokenizer_path)
        self.emotions = Config.EMOTIONS
        self.max_length = Config.MAX_TEXT_LENGTH
        self.tokenize = tokenize
        self.gpu_tokenizer = engine.GpuTokenizer.from_keras(
            self.tokenizer, device=self.device, max_length=self.max_length) if tokenize == 'gpu' else None

    def _forward(self, texts):
        """-> (probs [n,7] numpy, milliseconds around the synchronized forward)."""
        import torch
        texts = [t.lower().strip() for t in texts]
        if self.gpu_tokenizer is not None:
            ids = self.gpu_tokenizer.encode(texts)[0]
        else:
            ids = engine.to_device(self.tokenizer.padded(texts, self.max_length), self.device)
        torch.cuda.synchronize(self.device)
        start = time.time()
        _, _, probs = self.model.forward(ids)
        torch.cuda.synchronize(self.device)
        ms = (time.time() - start) * 1000
        return probs.cpu().numpy(), ms

    def _result(self, preds):
        idx = int(np.argmax(preds))
        return {'emotion': self.emotions[idx], 'confidence': float(preds[idx]),
                'probabilities': {e: float(p) for e, p in zip(self.emotions, preds)}}

    def predict(self, text):
        """dict with 'emotion', 'confidence', 'probabilities' and 'inference_time_ms'."""
        probs, ms = self._forward([text])
        out = self._result(probs[0])
        out['inference_time_ms'] = ms
        return out

    def predict_batch(self, texts):
        """List of dicts with 'text', 'emotion', 'confidence' and 'probabilities', one per text."""
        if not len(texts):
            return []
        probs, ms = self._forward(list(texts))
        print(f'Batch inference: {ms:.2f}ms total, {ms / len(texts):.2f}ms per sample')
        return [dict(text=t, **self._result(p)) for t, p in zip(texts, probs)]


DEMO_TEXTS = [
    "What a wonderful morning, I feel great",
    "I cannot stand this noise, it makes me furious",
    "Nothing special happened today",
]


def main(argv=None):
    ap = argparse.ArgumentParser(description='Fast LSTM text emotion prediction (HIP)')
    ap.add_argument('text', nargs='?', help='Text to analyze')
    ap.add_argument('--text', dest='text_arg', help='Text to analyze (alternative)')
    ap.add_argument('--model', help='Path to model file')
    ap.add_argument('--batch', action='store_true', help='Run batch demo')
    a = ap.parse_args(argv)
    text = a.text or a.text_arg
    if not text and not a.batch:
        ap.print_usage()
        return
    predictor = FastTextEmotionPredictor(model_path=a.model)
    for r in (predictor.predict_batch(DEMO_TEXTS) if a.batch else [dict(text=text, **predictor.predict(text))]):
        print(f"\nText: '{r['text']}'\nEmotion: {r['emotion'].upper()} ({r['confidence']:.2%})")
        for e, p in sorted(r['probabilities'].items(), key=lambda x: x[1], reverse=True):
            print(f'  {e:10s}: {p:.2%}')


if __name__ == '__main__':
    main()
