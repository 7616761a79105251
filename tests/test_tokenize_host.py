"""Tokenization on the GPU, the parts that need no GPU: (a) the byte-level specifications of
include/mec.h (mec_tok_*), restated in tests/tok_ref.py, give exactly the integers of the existing
tokenizers (KerasWordIndex.padded; transformers 4.30's pure-Python BertTokenizer, kept as
BertTokenizerLegacy, and BertTokenizerFast) on seeded random texts; (b) the new host code of
mec/tokenize.py: blob / offset packing, the routing predicate, the ValueError cases, the tables' contents;
(c) mec_tok_create's descriptor validation, which runs before the library touches a device."""
import ctypes

import numpy as np
import pytest

import tok_cases as tc
import tok_ref
from inference.text_lstm_inference import KERAS_FILTERS, KerasWordIndex
from mec import _lib, tokenize as T

L = 128


@pytest.fixture(scope='module')
def vocab_dir(tmp_path_factory):
    return tc.write_vocab(tmp_path_factory.mktemp('bert_vocab'))


def _keras_ref(wi, texts, maxlen=L):
    t = T.keras_table(wi)
    table = dict(zip(t.entries, t.ids))
    datas = [x.lower().encode('utf-8') if wi.lower else x.encode('utf-8') for x in texts]
    return tok_ref.rows(tok_ref.keras_row, datas, maxlen, table, t.delim, t.scalars['oov_id'])


@pytest.mark.parametrize('kw', [dict(num_words=10000), dict(num_words=20), dict(num_words=10000, oov_token=None),
                                dict(num_words=None, split='-', filters='!. \t\n')])
def test_keras_spec_matches_keras_word_index(kw):
    wi = KerasWordIndex(tc.keras_word_index(), **kw)
    texts = [t.lower().strip() for t in tc.keras_texts(120, seed=5)] + ['', ' ,.! ', 'x\x00y rare x\x00 y']
    ids, mask, n = _keras_ref(wi, texts)
    want = wi.padded(texts, L)
    assert np.array_equal(ids, want)
    lens = np.array([min(len(wi.sequence(t)), L) for t in texts])
    assert np.array_equal(n, lens) and np.array_equal(mask, (np.arange(L)[None] < lens[:, None]).astype(np.int32))
    assert (n == L).any() and (n == 0).any() and (ids == 1).any() == (wi.oov_index is not None)


def _wordpiece_ref(tok, texts, maxlen=L):
    t = T.wordpiece_table(tok)
    return tok_ref.rows(tok_ref.wordpiece_row, [x.encode('ascii') for x in texts], maxlen,
                        dict(zip(t.entries, t.ids)), **{k: v for k, v in t.scalars.items() if k != 'oov_id'})


@pytest.mark.parametrize('lower', [True, False])
def test_wordpiece_spec_matches_bert_tokenizers(vocab_dir, lower):
    slow, fast = tc.bert_tokenizers(vocab_dir, do_lower_case=lower)
    on_host = T.wordpiece_on_host(fast.all_special_tokens)
    texts = tc.ascii_texts(400, seed=11) + [
        'x' * 100, 'y' * 101, 'a' * 99 + 'q', 'runningz happyly', 'Happy A AB aB', '', ' '.join(['love'] * 200),
        'a ' * 126 + 'b', 'ab\x00cd\x1fef\x7fgh']
    assert not any(on_host(t) for t in texts)
    assert {chr(c) for c in range(128)} <= set(''.join(texts))
    ids, mask, n = _wordpiece_ref(fast, texts)
    for name, tok in (('legacy', slow), ('fast', fast)):
        want_ids, want_mask = tc.host_rows(tok, texts)
        bad = [i for i in range(len(texts)) if not np.array_equal(ids[i], want_ids[i])]
        assert not bad, (name, texts[bad[0]], ids[bad[0]][:20], want_ids[bad[0]][:20])
        assert np.array_equal(mask, want_mask) and np.array_equal(n, want_mask.sum(1))
    assert (n == L).any() and (n == 2).any() and (ids == fast.unk_token_id).any()


def test_pack_texts_blob_offsets_and_unencodable():
    texts = ['ab', '', 'café', 'bad \ud800 surrogate', '日本', 'keep me off']
    blob, off, host = T.pack_texts(texts, on_host=lambda t: t.startswith('keep'))
    assert blob.dtype == np.uint8 and off.dtype == np.int64 and off.shape == (7,)
    assert host == [3, 5]
    want = [t.encode('utf-8') for t in ('ab', '', 'café', '', '日本', '')]
    assert off.tolist() == np.concatenate([[0], np.cumsum([len(w) for w in want])]).tolist()
    assert blob.tobytes() == b''.join(want)
    for i, w in enumerate(want):
        assert blob[off[i]:off[i + 1]].tobytes() == w
    blob, off, host = T.pack_texts([])
    assert blob.size >= 1 and off.tolist() == [0] and host == []  # never a zero-size upload
    blob, off, host = T.pack_texts(['', ''])
    assert blob.size >= 1 and off.tolist() == [0, 0, 0] and host == []


def test_wordpiece_routing_predicate(vocab_dir):
    _, fast = tc.bert_tokenizers(vocab_dir)
    on_host = T.wordpiece_on_host(fast.all_special_tokens)
    assert sorted(fast.all_special_tokens) == ['[CLS]', '[MASK]', '[PAD]', '[SEP]', '[UNK]']
    for t in ('café', 'x[SEP]y', '[CLS]', 'a [MASK] b', 'naïve', '\x80', 'tab\there — dash'):
        assert on_host(t), t
    for t in ('', 'plain text!', '[sep] [ SEP ] [unused0]', 'a\x00b\x7f', 'x' * 500):
        assert not on_host(t), t
    # the predicate is what keeps the specification exact: both tokenizers keep a special-token literal whole
    assert tc.host_rows(fast, ['x[SEP]y'])[0][0, :5].tolist() == [fast.cls_token_id, fast.get_vocab()['x'],
                                                                  fast.sep_token_id, fast.get_vocab()['y'],
                                                                  fast.sep_token_id]


def test_keras_table_contents_and_value_errors():
    wi = KerasWordIndex(tc.keras_word_index(), num_words=20)
    t = T.keras_table(wi)
    table = dict(zip(t.entries, t.ids))
    assert t.kind == T.KERAS and t.scalars['oov_id'] == 1
    assert table == {w.encode('utf-8'): i for w, i in wi.word_index.items()
                     if i < 20 and not set(w) & set(KERAS_FILTERS + ' ')}
    assert b'happy' in table and b'<OOV>' not in table  # '<OOV>' holds filter characters: no word can equal it
    assert 'café'.encode() not in table and wi.word_index['café'] >= 20  # cut off: OOV, as KerasWordIndex has it
    assert [b for b in range(256) if t.delim[b]] == sorted(ord(c) for c in KERAS_FILTERS + ' ')
    assert T.keras_table(KerasWordIndex(tc.keras_word_index(), oov_token=None)).scalars['oov_id'] == -1
    assert len(T.keras_table(KerasWordIndex(tc.keras_word_index(), num_words=None)).entries) == len(wi.word_index) - 1
    for kw in (dict(split='  '), dict(split=''), dict(split='é'), dict(split=None), dict(filters=KERAS_FILTERS + '…')):
        with pytest.raises(ValueError, match="tokenize='gpu'"):
            T.keras_table(KerasWordIndex(tc.keras_word_index(), **kw))


def test_wordpiece_table_contents_and_value_errors(vocab_dir):
    slow, fast = tc.bert_tokenizers(vocab_dir)
    for tok in (slow, fast):
        t = T.wordpiece_table(tok)
        vocab = tok.get_vocab()
        assert t.kind == T.WORDPIECE
        assert dict(zip(t.entries, t.ids)) == {k.encode(): v for k, v in vocab.items() if k.isascii()}
        assert b'##ing' in t.entries and 'café' in vocab and '##é' in vocab  # the '##' form is kept for the library
        assert not any(max(e) >= 0x80 for e in t.entries)
        assert t.scalars == dict(oov_id=-1, lower=1, unk_id=vocab['[UNK]'], cls_id=vocab['[CLS]'],
                                 sep_id=vocab['[SEP]'], pad_id=vocab['[PAD]'], max_word=100)
    plain, cont = tok_ref.split_entries(dict(zip(t.entries, t.ids)))
    assert cont[b'ing'] == vocab['##ing'] and b'##ing' not in plain and plain[b'run'] == vocab['run']
    assert T.wordpiece_table(tc.bert_tokenizers(vocab_dir, do_lower_case=False)[1]).scalars['lower'] == 0
    for kw in (dict(do_lower_case=True, strip_accents=False), dict(do_lower_case=False, strip_accents=True)):
        for tok in tc.bert_tokenizers(vocab_dir, **kw):
            with pytest.raises(ValueError, match='strip_accents'):
                T.wordpiece_table(tok)
    for tok in tc.bert_tokenizers(vocab_dir):
        tok.add_tokens(['lol'])
        with pytest.raises(ValueError, match='added tokens'):
            T.wordpiece_table(tok)


def test_descriptor_matches_header_and_create_validates_on_the_host():
    """mec_tok_create checks the descriptor and builds the table before it touches a device, so its error
    paths run without a GPU: each returns -1 with a message."""
    lib = _lib.load()
    h = ctypes.c_void_p()

    def create(table=None, **over):
        if table is None:
            return lib.mec_tok_create(None, 0, ctypes.byref(h))
        d, keep = table.desc()
        for k, v in over.items():
            setattr(d, k, v)
        rc = lib.mec_tok_create(ctypes.byref(d), 0, ctypes.byref(h))
        return rc

    def failed(rc, what):
        assert rc == -1 and what in lib.mec_last_error().decode(), lib.mec_last_error()
        assert not h.value
    assert ctypes.sizeof(T.TokDesc) == 8 * 4 + 256 + 8 * 4  # kind+pad | 3 pointers | n | delim | 7 ints (+ pad)
    failed(create(), 'null')
    failed(create(T.Table(T.KERAS, [b'a', b'b', b'a'], [1, 2, 3])), 'duplicates')
    failed(create(T.Table(T.KERAS, [b'a', b'b'], [1, -2])), 'id < 0')
    failed(create(T.Table(T.KERAS, [b'a'], [1]), n=-1), 'n < 0')
    failed(create(T.Table(T.KERAS, [b'a'], [1]), off=None), 'null')
    failed(create(T.Table(T.KERAS, [b'a'], [1]), kind=5), 'kind')
    failed(create(T.Table(T.WORDPIECE, ['é'.encode()], [1])), '0x80')
    failed(create(T.Table(T.WORDPIECE, [b'a'], [1], max_word=500)), 'max_word')
    d, keep = T.Table(T.KERAS, [b'ab', b'c'], [1, 2]).desc()
    keep[1][:] = [0, 2, 1]
    assert lib.mec_tok_create(ctypes.byref(d), 0, ctypes.byref(h)) == -1 and b'monotone' in lib.mec_last_error()
    assert lib.mec_tok_create(ctypes.byref(d), 0, None) == -1
    assert lib.mec_tok_encode(None, None, None, 1, 128, None, None, None, None) == -1
    assert lib.mec_tok_destroy(None) == 0
