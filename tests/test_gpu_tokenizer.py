"""Tokenization on the GPU (mec_tok_*, csrc/tokenizer.hip; engine.GpuTokenizer) against the host tokenizers
it replaces: KerasWordIndex.padded for the BiLSTM path, BertTokenizerFast (through encode_batch) and
transformers 4.30's pure-Python BertTokenizer (BertTokenizerLegacy) for the BERT path. Integers, so every
comparison is exact equality; batches of B = 0, 1 and 67; seeded inputs. Then the two drop-in classes with
tokenize='gpu' against tokenize='host': the same probabilities bit for bit."""
import ctypes
import json

import numpy as np
import pytest
import torch

import tok_cases as tc
from inference.text_inference import TextInference, encode_batch
from inference.text_lstm_inference import FastTextEmotionPredictor, KerasWordIndex
from mec import _lib, engine, tokenize as T
from test_tokenizer import TEXTS

pytestmark = pytest.mark.gpu
L, B = 128, 67


def _np(t):
    return tuple(x.cpu().numpy() for x in t)


def _batches(texts):
    assert len(texts) % B == 0
    return [texts[i:i + B] for i in range(0, len(texts), B)]


def _keras_want(wi, texts):
    prep = [t.lower() for t in texts] if wi.lower else texts
    n = np.array([min(len(wi.sequence(t)), L) for t in prep], np.int32)
    return wi.padded(prep, L), (np.arange(L)[None] < n[:, None]).astype(np.int32), n


def _check_keras(gt, wi, texts):
    got = _np(gt.encode(texts))
    for g, w, name in zip(got, _keras_want(wi, texts), ('ids', 'mask', 'len')):
        assert g.dtype == np.int32 and g.shape == w.shape, name
        bad = np.flatnonzero((g != w).reshape(len(texts), -1).any(1))
        assert not bad.size, (name, int(bad[0]), texts[bad[0]][:80], g[bad[0]], w[bad[0]])
    return got


KNOWN = 'wonderful'  # in tc.KERAS_WORDS


def keras_special_texts():
    w = ['happy', 'zzz', 'sad', 'café']
    words = lambda n: ' '.join(w[i % 4] for i in range(n))  # noqa: E731
    return ['', ' ,.!\t\n;  ', words(127), words(128), words(129),
            'a' * 59 + ' ' + KNOWN + ' sad',                 # bytes 60..68: the word straddles byte 64
            'i ' * 30 + 'hap' + ' ' + KNOWN,                 # ... and starts exactly at byte 64
            'zz ' * 84 + KNOWN + ' love',                    # bytes 252..260: straddles byte 256
            'a' * 8192, 'a' * 8192 + ' happy', 'happy ' + 'b' * 8191 + ',' + KNOWN,  # an 8 KB single word
            'café 日本語 naïve ünïcödé', 'caffè 日本 日本語x ünï', 'x\x00y \x00 happy\x00 x\x00y\x00',
            'rare rarer w0 w1', "don't", 'happy', ' happy', 'happy ', 'i']


@pytest.mark.parametrize('kw', [dict(num_words=10000), dict(num_words=20), dict(oov_token=None),
                                dict(num_words=None, split='-', filters='!. \t\n')], ids=str)
def test_keras_matches_keras_word_index(dev, kw):
    """Every special case and seeded random texts, as one batch of 67 and row by row (B = 1): the same
    integers as KerasWordIndex.padded, whatever the batch. num_words=20 maps an index >= num_words to
    OOV; oov_token=None drops unknown words."""
    wi = KerasWordIndex(tc.keras_word_index(n_extra=40), **kw)
    gt = engine.GpuTokenizer.from_keras(wi, device=dev)
    special = keras_special_texts()
    texts = special + [t.lower().strip() for t in tc.keras_texts(B - len(special), seed=3)]
    ids, mask, n = _check_keras(gt, wi, texts)
    assert n.max() == L and n.min() == 0 and gt.host_rows == 0
    for i, t in enumerate(texts):
        one = _check_keras(gt, wi, [t])
        assert np.array_equal(one[0][0], ids[i]) and one[2][0] == n[i]
    for t in gt.encode([]):
        assert t.shape[0] == 0 and t.dtype == torch.int32


def test_keras_near_duplicate_vocabulary(dev):
    """5000 entries that share prefixes and suffixes (a, aa, ..., a..ab, ba..a): a table that trusted its
    hash, or compared a prefix only, gives a wrong id somewhere."""
    words = ['a' * k for k in range(1, 2001)] + ['a' * k + 'b' for k in range(1, 1501)] + ['b' + 'a' * k
                                                                                             for k in range(1, 1501)]
    wi = KerasWordIndex({'<OOV>': 1, **{w: i + 2 for i, w in enumerate(words)}}, num_words=None)
    gt = engine.GpuTokenizer.from_keras(wi, device=dev)
    rng = np.random.default_rng(17)
    missing = ['a' * 2001, 'ab' * 3, 'b', 'aab' + 'a', 'ba' * 2, 'a' * 1501 + 'b', 'b' * 2 + 'a', 'a' * 1000 + 'c']

    def word():
        r = rng.random()
        if r < 0.2:
            return missing[int(rng.integers(len(missing)))]
        w = words[int(rng.integers(len(words)))]
        return w if r < 0.8 else w[:int(rng.integers(1, 40))]
    texts = [' '.join(word() for _ in range(int(rng.integers(1, 24)))) for _ in range(B)]
    ids, _, n = _check_keras(gt, wi, texts)
    assert (ids == 1).any() and len(np.unique(ids)) > 300


def test_keras_unencodable_text_takes_the_host_row(dev):
    wi = KerasWordIndex(tc.keras_word_index())
    gt = engine.GpuTokenizer.from_keras(wi, device=dev)
    texts = ['happy day', 'sad \ud800 day', 'love']
    got = _np(gt.encode(texts))
    assert gt.host_rows == 1
    assert np.array_equal(got[0], wi.padded(texts, L)) and got[2].tolist() == [2, 3, 1]


@pytest.fixture(scope='module')
def vocab_dir(tmp_path_factory):
    return tc.write_vocab(tmp_path_factory.mktemp('bert_vocab'))


def wordpiece_special_texts():
    return ['x' * 100, 'y' * 101, 'x' * 100 + ' ' + 'y' * 101 + ' happy', 'a' * 99 + 'q',
            'runningz', 'happyly runningz unbelievable', 'qrunning',   # a piece missing: the whole word is [UNK]
            'a ' * 124 + 'b', 'a ' * 125 + 'b', 'a ' * 126 + 'b',      # 125, 126 and 127 pieces
            'running ' * 70, 'ab\x00cd\x1fef\x7fgh', '\x00', ' \t\r\n ', '...', 'Happy A AB aB HAPPY',
            'a' * 63 + ' wonderful', 'a' * 60 + ' wonderfully', 'i ' * 126 + 'wonder' + 'ful', 'x' * 5000 + ' sad',
            'abcdefghij' * 10, 'z' * 64 + 'y' * 36]


@pytest.mark.parametrize('lower', [True, False])
def test_wordpiece_matches_both_bert_tokenizers(dev, vocab_dir, lower):
    """The ten TEXTS of test_tokenizer.py, 200 seeded random 7-bit texts that hold every control byte, the
    edge cases above, and rows routed to the host ('café', 'x[SEP]y') interleaved with GPU rows: ids, mask
    and len equal those of encode_batch with BertTokenizerFast and of BertTokenizerLegacy per text, in
    batches of 67 and row by row."""
    slow, fast = tc.bert_tokenizers(vocab_dir, do_lower_case=lower)
    gt = engine.GpuTokenizer.from_bert(fast, device=dev)
    rand = tc.ascii_texts(200, seed=23)
    assert {chr(c) for c in range(128)} <= set(''.join(rand))
    texts = list(TEXTS) + wordpiece_special_texts()
    for i, t in enumerate(rand):  # a routed row after every eighth random text
        texts.append(t)
        if i % 8 == 0:
            texts.append(['café', 'x[SEP]y', 'so [MASK] happy', 'naïve — day'][i // 8 % 4])
    texts += tc.ascii_texts(-len(texts) % B, seed=29)
    want_ids, want_mask = encode_batch(fast, texts)
    slow_ids, slow_mask = tc.host_rows(slow, texts)
    assert np.array_equal(want_ids, slow_ids) and np.array_equal(want_mask, slow_mask)
    want_n = want_mask.sum(1)
    assert {127, 128, 2}.issubset(want_n.tolist()) and (want_ids == fast.unk_token_id).any()
    routed = 0
    for lo, batch in zip(range(0, len(texts), B), _batches(texts)):
        ids, mask, n = _np(gt.encode(batch))
        routed += gt.host_rows
        bad = np.flatnonzero((ids != want_ids[lo:lo + B]).any(1))
        assert not bad.size, (batch[bad[0]][:100], ids[bad[0]], want_ids[lo + bad[0]])
        assert np.array_equal(mask, want_mask[lo:lo + B]) and np.array_equal(n, want_n[lo:lo + B])
    assert routed >= 25 + 1  # TEXTS holds one non-ASCII text
    for i in range(len(TEXTS) + len(wordpiece_special_texts()) + 4):
        ids, mask, n = _np(gt.encode([texts[i]]))
        assert np.array_equal(ids[0], want_ids[i]) and np.array_equal(mask[0], want_mask[i]), texts[i]
        assert n[0] == want_n[i], texts[i]
    for t in gt.encode([]):
        assert t.shape[0] == 0


def test_abi_error_paths_return_minus_one_with_a_message(dev):
    lib = _lib.load()
    h = ctypes.c_void_p()

    def failed(rc, what):
        assert rc == -1 and what in lib.mec_last_error().decode(), (rc, lib.mec_last_error())
    failed(lib.mec_tok_create(None, dev.index, ctypes.byref(h)), 'null')
    d, keep = T.Table(T.KERAS, [b'a', b'b', b'a'], [1, 2, 3]).desc()
    failed(lib.mec_tok_create(ctypes.byref(d), dev.index, ctypes.byref(h)), 'duplicates')
    assert not h.value
    gt = engine.GpuTokenizer.from_keras(KerasWordIndex(tc.keras_word_index()), device=dev)
    text = torch.zeros(16, dtype=torch.uint8, device=dev)
    off = torch.zeros(5, dtype=torch.int64, device=dev)
    ids = torch.full((4, 513), -7, dtype=torch.int32, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    failed(lib.mec_tok_encode(gt.handle, p(text), p(off), 4, 0, p(ids), None, None, None), 'L must be')
    failed(lib.mec_tok_encode(gt.handle, p(text), p(off), 4, 513, p(ids), None, None, None), 'L must be')
    failed(lib.mec_tok_encode(gt.handle, p(text), p(off), -1, 128, p(ids), None, None, None), 'B < 0')
    failed(lib.mec_tok_encode(gt.handle, None, p(off), 4, 128, p(ids), None, None, None), 'null')
    failed(lib.mec_tok_encode(gt.handle, p(text), None, 4, 128, p(ids), None, None, None), 'null')
    failed(lib.mec_tok_encode(gt.handle, p(text), p(off), 4, 128, None, None, None, None), 'null')
    failed(lib.mec_tok_encode(None, p(text), p(off), 4, 128, p(ids), None, None, None), 'null tokenizer')
    assert lib.mec_tok_encode(gt.handle, None, None, 0, 128, None, None, None, None) == 0  # B == 0: no launch
    torch.cuda.synchronize(dev)
    assert int((ids != -7).sum()) == 0  # nothing was launched
    # mask and len are optional; L = 1 and L = 512 are the bounds
    assert lib.mec_tok_encode(gt.handle, p(text), p(off), 4, 512, p(ids), None, None, None) == 0
    assert lib.mec_tok_encode(gt.handle, p(text), p(off), 4, 1, p(ids), None, None, None) == 0
    torch.cuda.synchronize(dev)
    assert int(ids.reshape(-1)[:4 * 512].abs().sum()) == 0


def test_encode_captures_into_a_graph_and_replays_on_new_bytes(dev):
    """mec_tok_encode allocates nothing and never synchronizes: captured once over static buffers, a
    replay tokenizes whatever bytes and offsets the buffers hold then."""
    wi = KerasWordIndex(tc.keras_word_index())
    gt = engine.GpuTokenizer.from_keras(wi, device=dev)
    batches = [[t.lower().strip() for t in tc.keras_texts(B, seed=s)] for s in (41, 43)]
    text_d = torch.zeros(1 << 17, dtype=torch.uint8, device=dev)
    off_d = torch.zeros(B + 1, dtype=torch.int64, device=dev)
    ids, mask = (torch.zeros((B, L), dtype=torch.int32, device=dev) for _ in range(2))
    n = torch.zeros(B, dtype=torch.int32, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def load(texts):
        blob, off, _ = T.pack_texts(texts)
        assert blob.size <= text_d.numel()
        text_d[:blob.size].copy_(engine.to_device(blob, dev))
        off_d.copy_(engine.to_device(off, dev))

    def encode(stream):
        assert gt.lib.mec_tok_encode(gt.handle, p(text_d), p(off_d), B, L, p(ids), p(mask), p(n),
                                     ctypes.c_void_p(stream.cuda_stream)) == 0
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    load(batches[0])
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(s):
        encode(s)  # warm on the capture stream
    torch.cuda.synchronize(dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        encode(s)
    for texts in (batches[1], batches[0]):
        load(texts)
        ids.zero_()
        torch.cuda.synchronize(dev)
        g.replay()
        torch.cuda.synchronize(dev)
        want = _keras_want(wi, texts)
        for got, w in zip((ids, mask, n), want):
            assert np.array_equal(got.cpu().numpy(), w)


E2E_TEXTS = [t for t in tc.ascii_texts(80, seed=31) if len(t) < 400][:B - 4] + [
    'café au lait', 'so x[SEP]y', '', 'I am so happy today!']


def test_bilstm_dropin_gpu_tokenizer_gives_the_same_bits(dev, tmp_path):
    assert len(E2E_TEXTS) == B
    wi = tc.keras_word_index()
    host = FastTextEmotionPredictor(seed=7, device=dev, word_index=wi)
    gpu = FastTextEmotionPredictor(seed=7, device=dev, word_index=wi, tokenize='gpu')
    assert gpu.gpu_tokenizer is not None and host.gpu_tokenizer is None
    a, b = host.predict_batch(E2E_TEXTS), gpu.predict_batch(E2E_TEXTS)
    assert a == b and len(b) == B
    one = gpu.predict(E2E_TEXTS[-1])
    assert one['probabilities'] == host.predict(E2E_TEXTS[-1])['probabilities']
    path = tmp_path / 'tokenizer.json'  # Tokenizer.to_json()'s form, with a split the kernel cannot express
    path.write_text(json.dumps({'config': {'word_index': json.dumps(wi), 'num_words': 10000, 'oov_token': '<OOV>',
                                           'split': 'é'}}))
    assert FastTextEmotionPredictor(seed=7, device=dev, tokenizer_path=str(path)).tokenizer.split == 'é'
    with pytest.raises(ValueError, match="tokenize='gpu'"):
        FastTextEmotionPredictor(seed=7, device=dev, tokenizer_path=str(path), tokenize='gpu')
    with pytest.raises(ValueError, match='tokenize must be'):
        FastTextEmotionPredictor(seed=7, device=dev, word_index=wi, tokenize='device')


def test_bert_dropin_gpu_tokenizer_gives_the_same_bits(dev, vocab_dir):
    assert len(E2E_TEXTS) == B
    _, fast = tc.bert_tokenizers(vocab_dir)
    host = TextInference(seed=1234, device=dev, tokenizer=fast, precision='f16')
    gpu = TextInference(seed=1234, device=dev, tokenizer=fast, precision='f16', tokenize='gpu')
    ids, mask = gpu.encode_batch(E2E_TEXTS)
    h_ids, h_mask = host.encode_batch(E2E_TEXTS)
    assert ids.device == dev and np.array_equal(ids.cpu().numpy(), h_ids) and np.array_equal(mask.cpu().numpy(), h_mask)
    assert gpu.gpu_tokenizer.host_rows == 2
    assert host.predict_texts(E2E_TEXTS) == gpu.predict_texts(E2E_TEXTS)
    assert host.predict_texts(E2E_TEXTS, pack=True) == gpu.predict_texts(E2E_TEXTS, pack=True)
    assert gpu.model.packed_rows == host.model.packed_rows < B
    assert gpu.predict_texts([]) == []
    with pytest.raises(ValueError, match='tokenize must be'):
        TextInference(seed=1234, device=dev, tokenizer=fast, tokenize='cuda')
