"""Tokenization of non-ASCII text on the GPU (MEC_TOK_WORDPIECE_UTF8: mec_tok_create_utf8,
wordpiece_kernel<true> of csrc/tokenizer.hip; engine.GpuTokenizer.from_bert(unicode=True),
TextInference(tokenize='gpu_utf8')) against the two host tokenizers it replaces, BertTokenizerFast and the
pure-Python BertTokenizerLegacy. Integers, so every comparison is exact equality; batches of B = 0, 1 and 67,
L = 128 and L = 8; no row may take the host's way unless the test says so."""
import ctypes

import numpy as np
import pytest
import torch

import tok_cases as tc
import tok_cases_utf8 as tu
from inference.text_inference import TextInference
from mec import engine, tokenize as T

pytestmark = pytest.mark.gpu
L, B = 128, 67


@pytest.fixture(scope='module')
def vocab_dir(tmp_path_factory):
    return tu.write_vocab(tmp_path_factory.mktemp('bert_vocab_utf8'))


@pytest.fixture(scope='module')
def toks(vocab_dir):
    return tu.bert_tokenizers(vocab_dir)


@pytest.fixture(scope='module')
def gt(dev, toks):
    return engine.GpuTokenizer.from_bert(toks[1], device=dev, unicode=True)


def _np(t):
    return tuple(x.cpu().numpy() for x in t)


def _pad(texts):
    return texts + ['happy'] * (-len(texts) % B)


def check(gt, toks, texts, max_length=L, host_rows=0):
    """Batches of 67: ids, mask and len equal both host tokenizers'; -> (ids, mask, len) of all texts."""
    texts = _pad(list(texts))
    want_ids, want_mask = tc.host_rows(toks[1], texts, max_length)
    slow_ids, slow_mask = tc.host_rows(toks[0], texts, max_length)
    assert np.array_equal(want_ids, slow_ids) and np.array_equal(want_mask, slow_mask)
    got, routed = [], 0
    for lo in range(0, len(texts), B):
        got.append(_np(gt.encode(texts[lo:lo + B])))
        routed += gt.host_rows
    ids, mask, n = (np.concatenate(x) for x in zip(*got))
    bad = np.flatnonzero((ids != want_ids).any(1))
    assert not bad.size, (len(bad), texts[bad[0]][:100], ids[bad[0]][:24], want_ids[bad[0]][:24])
    assert np.array_equal(mask, want_mask) and np.array_equal(n, want_mask.sum(1)) and routed == host_rows
    return ids, mask, n


A, E2, P3, H3, C3, E4 = 'a', 'é', '—', '한', '日', '😀'  # 1, 2, 3, 3, 3 and 4 bytes
ACUTE, ZWSP, ZWJ, VS16, NBSP, LSEP, IDSP = '\u0301', '\u200b', '\u200d', '\ufe0f', '\xa0', '\u2028', '\u3000'


def special_texts():
    t = []
    for k in (60, 61, 62, 63):  # a character of every length starting at each of a chunk's last four bytes
        for ch in (E2, 'ж', 'ß', ACUTE, P3, H3, C3, '豈', LSEP, ZWJ, E4, '😁', '\U0002f800'):
            t += [A * k + ch + 'b', A * (k - 1) + ' ' + ch, 'a ' * (k // 2) + A * (k % 2) + ch + ch + ' sad']
    t += ['abc' + ch for ch in (E2, P3, H3, C3, E4, ACUTE, ZWJ)]  # at the text's last bytes
    t += [E2, P3, H3, C3, E4, ACUTE, NBSP]
    # words of exactly 100 and 101 characters of 1, 2, 3 and 4 bytes; 100 that become 101 by an expansion
    for ch in ('x', 'ж', 'ᄀ', E4):
        t += [ch * 100, ch * 101, ch * 100 + ' ' + ch * 101 + ' happy', 'é' + ch * 99, 'é' + ch * 100]
    t += ['ж' * 98 + '가', 'ж' * 99 + '가', 'ж' * 97 + '각', 'ж' * 98 + '각', '가' * 50, '가' * 50 + 'a', '각' * 33 + 'a',
          '각' * 33 + 'ab']
    # marks inside, before and after a word, alone; the dotted capital I
    t += ['café', 'ca\u0301\u0308fe', ACUTE + 'cafe', 'cafe ' + ACUTE, '\u0301\u0308\u0323', 'a ' + ACUTE + ' b', 'CAFÉ É',
          'İstanbul İ', 'i\u0307', 'hapṕy dày']
    # dropped Cf inside words and emoji sequences, the variation selector
    t += ['hap' + ZWSP + 'py', 'ha' + ZWJ + 'ppy' + ZWJ, ZWSP, '😀' + ZWJ + '😀', '😀' + VS16, '❤\ufe0f\u200d\U0001f525',
          'so\xadft', '\U0001f44d\U0001f3fd']
    # separators
    t += ['happy' + NBSP + 'day', 'happy' + LSEP + 'day\u2029sad', 'happy' + IDSP + 'day', NBSP + LSEP + IDSP, 'i\u2003am\u1680so happy']
    # punctuation next to letters and to ASCII punctuation
    t += ['¿que?', 'so—happy', '—…—', 'happy…!', '"happy"…', '«happy»', 'a·b', '。happy。', '!—!', ';·`', 'it’s']
    # CJK inside Latin words, compatibility ideographs (mapped and isolated), CJK punctuation, fullwidth forms
    t += ['x日y本z', '日本語', 'happy日本', '豈', 'a豈b', '豈更', '\U0002f800x', '日。本', 'ａｂ ＡＢ', '﹗']
    # emoji with and without a vocab entry
    t += ['😀', '😀😀😀', 'a😀', '😁', '😀😁', 'happy 😀 day 😁']
    # truncation at L - 2 inside a multi-piece word
    t += ['a ' * 124 + 'é', 'a ' * 124 + 'жжж', 'a ' * 125 + 'жжж', 'a ' * 123 + '한', 'a ' * 120 + 'straßeßß ßß', 'é ' * 200, '日' * 200,
          '— ' * 130]
    # an entry of more than 64 bytes
    t += [tu.LONG, 'Ж' * 40, 'ж' * 41, 'ж' * 39, tu.LONG + ' ' + tu.LONG + 'ж', 'ж' * 80]
    t += ['straße STRASSE Straße ẞ', 'σοσ ος', 'øre Øø', '', ' ', 'x' * 5000 + ' é', 'é' * 3000 + ' sad', '\x00é\x1f']
    return t


def test_utf8_matches_both_bert_tokenizers(dev, toks, gt):
    """The edge cases above and 201 seeded texts of covered code points, in batches of 67 and (the edge
    cases) row by row: the same integers as both host tokenizers, no row on the host."""
    special = special_texts()
    texts = special + tu.utf8_texts(201, seed=23, cls=gt.cpmap.cls)
    ids, mask, n = check(gt, toks, texts)
    v = toks[1].get_vocab()
    assert {2, 3, 127, 128} <= set(n.tolist()) and (ids == v['[UNK]']).any()
    for piece in ('cafe', 'straße', '日', '豈', '😀', '##😀', '—', '…', '##ᅡ', '##ᆨ', tu.LONG, '##ß', '##ж', 'ａ', '##ｂ'):
        assert (ids == v[piece]).any(), piece
    for i, t in enumerate(special):
        one = _np(gt.encode([t]))
        assert gt.host_rows == 0
        assert np.array_equal(one[0][0], ids[i]) and np.array_equal(one[1][0], mask[i]) and one[2][0] == n[i], t
    for t in gt.encode([]):
        assert t.shape[0] == 0 and t.dtype == torch.int32


def test_utf8_small_row(dev, toks):
    """L = 8: six pieces fit; the cut falls inside words of several pieces."""
    gt8 = engine.GpuTokenizer.from_bert(toks[1], device=dev, max_length=8, unicode=True)
    texts = ['café 日本語 한 😀😀', 'straßeßß', 'жжжжжжжж', '한한한', 'é — é — é — é', '', '😀', 'a\u0301 b\u0301 c d e f g']
    ids, mask, n = check(gt8, toks, texts + tu.utf8_texts(B - len(texts), seed=37, cls=gt8.cpmap.cls), max_length=8)
    assert ids.shape[1] == 8 and {2, 8} <= set(n.tolist())


def test_seven_bit_texts_get_the_rows_of_the_seven_bit_kind(dev, toks, gt):
    old = engine.GpuTokenizer.from_bert(toks[1], device=dev)
    for seed in (23, 29):
        texts = tc.ascii_texts(B, seed=seed)
        a, b = _np(old.encode(texts)), _np(gt.encode(texts))
        assert old.host_rows == 0 and gt.host_rows == 0
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
    check(gt, toks, tc.ascii_texts(B, seed=31))


def test_uncovered_and_special_texts_take_the_host_rows_in_order(dev, toks, gt):
    texts = tu.utf8_texts(B, seed=41, cls=gt.cpmap.cls)
    routed = {3: 'ΟΔΟ\u03a3 café', 17: 'so [MASK] happy —', 18: 'x[SEP]日', 40: '\u03a3', 66: 'café \u1b44'}
    for i, t in routed.items():
        texts[i] = t
    check(gt, toks, texts, host_rows=len(routed))
    check(gt, toks, ['happy', '\u03a3'], host_rows=1)


def test_ill_formed_and_uncovered_rows_are_all_pad(dev, toks, gt):
    """Through the raw C call: such a row is pad_id, mask 0 and len -1; the rows next to it are the host
    tokenizers'. A sequence cut off by its text's end does not borrow the next text's bytes."""
    bad = [b'caf\xc3', b'\x80abc', b'a\xa9 b', b'\xc0\xaf', b'\xc1\xbf', b'\xe0\x80\xaf', b'\xf0\x80\x80\xaf',
           b'\xed\xa0\x80', b'\xf4\x90\x80\x80', b'\xf5\x80\x80\x80', b'a\xe2\x82', b'\xe2\x82 x', b'\xff', b'a\xc3',
           b'\xa9b', '\u03a3'.encode(), 'a\u0378'.encode(), ('happy ' * 200 + '\u03a3').encode(),
           b'a' * 62 + b'\xe2\x82', b'a' * 63 + b'\xe2 \x82', b'a' * 64 + b'\x82', ('é' * 40 + '\ud7ff').encode() + b'\xed\xa0\x80']
    good = ['café 日本', 'happy', '', '😀 — é', 'a' * 62 + '—b']
    datas, is_bad = [], []
    for i, b in enumerate(bad):
        datas += [good[i % len(good)].encode(), b]
        is_bad += [False, True]
    datas.append(good[0].encode())
    is_bad.append(False)
    n_rows = len(datas)
    off = np.zeros(n_rows + 1, np.int64)
    np.cumsum([len(d) for d in datas], out=off[1:])
    text_d = engine.to_device(np.frombuffer(b''.join(datas), np.uint8), dev)
    off_d = engine.to_device(off, dev)
    ids = torch.full((n_rows, L), -7, dtype=torch.int32, device=dev)
    mask, n = torch.full_like(ids, -7), torch.full((n_rows,), -7, dtype=torch.int32, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    assert gt.lib.mec_tok_encode(gt.handle, p(text_d), p(off_d), n_rows, L, p(ids), p(mask), p(n), None) == 0
    torch.cuda.synchronize(dev)
    ids, mask, n = _np((ids, mask, n))
    want_ids, want_mask = tc.host_rows(toks[1], [d.decode() for d, b in zip(datas, is_bad) if not b])
    is_bad = np.array(is_bad)
    assert np.array_equal(ids[~is_bad], want_ids) and np.array_equal(mask[~is_bad], want_mask)
    assert np.array_equal(n[~is_bad], want_mask.sum(1))
    assert (ids[is_bad] == toks[1].pad_token_id).all() and (mask[is_bad] == 0).all() and (n[is_bad] == -1).all()


def test_utf8_encode_captures_into_a_graph(dev, toks, gt):
    texts = tu.utf8_texts(B, seed=43, cls=gt.cpmap.cls)
    want = _np(gt.encode(texts))
    blob, off, host = T.pack_texts(texts)
    assert not host
    text_d, off_d = engine.to_device(blob, dev), engine.to_device(off, dev)
    ids, mask = (torch.zeros((B, L), dtype=torch.int32, device=dev) for _ in range(2))
    n = torch.zeros(B, dtype=torch.int32, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def encode(stream):
        assert gt.lib.mec_tok_encode(gt.handle, p(text_d), p(off_d), B, L, p(ids), p(mask), p(n),
                                     ctypes.c_void_p(stream.cuda_stream)) == 0
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(s):
        encode(s)  # warm on the capture stream
    torch.cuda.synchronize(dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        encode(s)
    for t in (ids, mask, n):
        t.zero_()
    torch.cuda.synchronize(dev)
    g.replay()
    torch.cuda.synchronize(dev)
    for got, w in zip(_np((ids, mask, n)), want):
        assert np.array_equal(got, w)


def test_bert_dropin_gpu_utf8_gives_the_same_bits(dev, toks, vocab_dir):
    _, fast = toks
    texts = [t for t in tu.utf8_texts(120, seed=47, cls=T.wordpiece_cpmap(fast).cls) if len(t.encode()) < 400][:B - 6] + [
        'café au lait', 'so x[SEP]y', '', 'I am so happy today!', 'ΟΔΟ\u03a3', '日本語 😀']
    assert len(texts) == B
    non_ascii = sum(not t.isascii() for t in texts)
    assert non_ascii > B // 2
    host = TextInference(seed=1234, device=dev, tokenizer=fast, precision='f16')
    utf8 = TextInference(seed=1234, device=dev, tokenizer=fast, precision='f16', tokenize='gpu_utf8')
    gpu = TextInference(seed=1234, device=dev, tokenizer=fast, precision='f16', tokenize='gpu')
    ids, mask = utf8.encode_batch(texts)
    h_ids, h_mask = host.encode_batch(texts)
    assert ids.device == dev and np.array_equal(ids.cpu().numpy(), h_ids) and np.array_equal(mask.cpu().numpy(), h_mask)
    assert utf8.gpu_tokenizer.host_rows == 2
    want = host.predict_texts(texts)
    assert want == utf8.predict_texts(texts)
    assert host.predict_texts(texts, pack=True) == utf8.predict_texts(texts, pack=True)
    assert utf8.model.packed_rows == host.model.packed_rows < B
    assert utf8.predict_texts([]) == []
    # the 7-bit setting is what it was: every non-ASCII text and the special literal on the host
    assert want == gpu.predict_texts(texts) and gpu.gpu_tokenizer.host_rows == non_ascii + 1
    with pytest.raises(ValueError, match='tokenize must be'):
        TextInference(seed=1234, device=dev, tokenizer=fast, tokenize='utf8')
    cased = tu.bert_tokenizers(vocab_dir, do_lower_case=False)[1]
    with pytest.raises(ValueError, match='gpu_utf8'):
        TextInference(seed=1234, device=dev, tokenizer=cased, precision='f16', tokenize='gpu_utf8')

