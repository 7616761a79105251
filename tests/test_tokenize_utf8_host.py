"""MEC_TOK_WORDPIECE_UTF8, the parts that need no GPU: (a) the byte-level specification of include/mec.h,
restated in tests/tok_ref_utf8.py, gives exactly the integers of BertTokenizerLegacy and BertTokenizerFast
on seeded texts drawn from the covered code points; (b) the covered set, the routing predicate and the
ValueError cases of mec/tokenize.py; (c) mec_tok_create_utf8's validation, which runs before the library
touches a device; (d) a 7-bit text gets the row of the 7-bit specification."""
import ctypes
import unicodedata

import numpy as np
import pytest

import tok_cases as tc
import tok_cases_utf8 as tu
import tok_ref
import tok_ref_utf8
from mec import _lib, tokenize as T

L = 128


@pytest.fixture(scope='module')
def toks(tmp_path_factory):
    return tu.bert_tokenizers(tu.write_vocab(tmp_path_factory.mktemp('bert_vocab_utf8')))


@pytest.fixture(scope='module')
def cpmap(toks):
    return T.wordpiece_cpmap(toks[1])  # the fast tokenizer's: the slow one's less what the probe takes away


def ref_rows(tok, cpmap, texts, maxlen=L):
    t = T.wordpiece_table_utf8(tok)
    return tok_ref.rows(tok_ref_utf8.wordpiece_utf8_row, [x.encode('utf-8') for x in texts], maxlen,
                        cpmap.cls, cpmap.outputs, dict(zip(t.entries, t.ids)),
                        **{k: v for k, v in t.scalars.items() if k != 'oov_id'})


EDGE = ['café', 'CAFÉ', 'cafe\u0301', 'Straße STRASSE \u1e9e', 'x日y本z', '日本語', '한글 한', '\uf900', 'a\uf900b',
        '😀😀 😁 a😀', '—…¿que?·。', 'a\u200db\u200bc', '😀\u200d😀\ufe0f', 'a\xa0b\u2028c\u3000d', '\u0130stanbul',
        '\u0301\u0308', 'a\u0301\u0308', '\u0301a', 'ж' * 100, 'ж' * 101, 'Ж' * 40, 'ж' * 41, 'ж' * 99 + '가',
        'ж' * 98 + '가', '😀' * 100, '😀' * 101, 'a ' * 124 + 'жжж', 'ａｂ ＡＢ', 'σοσ ος', '\u037e \u0387 \u1fef', '']


def test_utf8_spec_matches_both_bert_tokenizers(toks, cpmap):
    """Exact equality on every text, none skipped: the generator draws covered code points only, so the
    routing predicate holds for no text."""
    slow, fast = toks
    on_host = T.wordpiece_on_host_utf8(fast.all_special_tokens, cpmap)
    texts = tu.utf8_texts(300, seed=11, cls=cpmap.cls) + EDGE + tc.ascii_texts(40, seed=13)
    assert not any(on_host(t) for t in texts)
    assert sum(not t.isascii() for t in texts) > 280
    ids, mask, n = ref_rows(fast, cpmap, texts)
    assert (n >= 2).all()
    for name, tok in (('legacy', slow), ('fast', fast)):
        want_ids, want_mask = tc.host_rows(tok, texts)
        bad = [i for i in range(len(texts)) if not np.array_equal(ids[i], want_ids[i])]
        assert not bad, (name, len(bad), texts[bad[0]], ids[bad[0]][:24], want_ids[bad[0]][:24])
        assert np.array_equal(mask, want_mask) and np.array_equal(n, want_mask.sum(1))
    v = fast.get_vocab()
    assert (n == L).any() and (n == 2).any() and (ids == fast.unk_token_id).any()
    for piece in ('cafe', 'straße', '日', '😀', '##😀', '—', '##ᅡ', tu.LONG, '豈', '##ß'):
        assert (ids == v[piece]).any(), piece
    first = {t: ids[len(texts) - 40 - len(EDGE) + i, 1:4].tolist() for i, t in enumerate(EDGE)}
    assert first['café'][:2] == first['CAFÉ'][:2] == first['cafe\u0301'][:2] == [v['cafe'], v['[SEP]']]
    assert first['ж' * 100][0] != v['[UNK]'] and first['ж' * 101][:2] == [v['[UNK]'], v['[SEP]']]
    assert first['ж' * 99 + '가'][:2] == [v['[UNK]'], v['[SEP]']] and first['ж' * 98 + '가'][0] == v[tu.LONG]
    assert first['\uf900'][:2] == [v['豈'], v['[SEP]']] and '豈' != '\uf900'


def test_seven_bit_text_gets_the_seven_bit_row(toks, cpmap):
    _, fast = toks
    texts = tc.ascii_texts(200, seed=11) + ['x' * 100, 'y' * 101, 'Happy A AB aB', 'ab\x00cd\x1fef\x7fgh', '']
    t7 = T.wordpiece_table(fast)
    want = tok_ref.rows(tok_ref.wordpiece_row, [x.encode('ascii') for x in texts], L, dict(zip(t7.entries, t7.ids)),
                        **{k: v for k, v in t7.scalars.items() if k != 'oov_id'})
    for got, w in zip(ref_rows(fast, cpmap, texts), want):
        assert np.array_equal(got, w)


def test_ill_formed_and_uncovered_rows_are_invalid(toks, cpmap):
    _, fast = toks
    t = T.wordpiece_table_utf8(fast)
    kw = {k: v for k, v in t.scalars.items() if k != 'oov_id'}
    for data in (b'caf\xc3', b'\x80abc', b'a\xa9', b'\xc0\xaf', b'\xc1\xbf', b'\xe0\x80\xaf', b'\xf0\x80\x80\xaf',
                 b'\xed\xa0\x80', b'\xf4\x90\x80\x80', b'\xf5\x80\x80\x80', b'a\xe2\x82', b'\xe2\x82 x', b'\xff',
                 '\u03a3'.encode(), 'a\u0378'.encode(), 'happy ' * 200 + '\u03a3'):
        data = data.encode() if isinstance(data, str) else data
        ids, mask, n = tok_ref_utf8.wordpiece_utf8_row(data, cpmap.cls, cpmap.outputs, dict(zip(t.entries, t.ids)), 8, **kw)
        assert n == -1 and ids == [kw['pad_id']] * 8 and mask == [0] * 8, data
    assert tok_ref_utf8.decode('aé—😀'.encode()) == [0x61, 0xE9, 0x2014, 0x1F600]


def test_covered_set(toks):
    slow, fast = toks
    model, cp_fast = T.wordpiece_cpmap(slow), T.wordpiece_cpmap(fast)
    sensitive = [cp for cp in range(0x110000) if cp == 0x3A3 or (
        unicodedata.combining(chr(cp)) and unicodedata.category(chr(cp)) != 'Mn')]
    assert len(sensitive) == 24
    unassigned = next(cp for cp in range(0x378, 0x110000) if unicodedata.category(chr(cp)) == 'Cn')
    for m in (model, cp_fast):
        assert not any(m.covered(cp) for cp in sensitive + [unassigned, 0xD800, 0xDFFF, 0xE000, 0x10FFFF])
        assert all(m.covered(ord(c)) for c in 'é—😀\u200d\u2028\xa0ß한日\uf900\u0130')
        assert m.cls[0x200D] == T.CP_DROP and m.cls[0x2028] == T.CP_SPACE and m.cls[0x2014] == T.CP_PUNCT
        assert m.cls[0x65E5] == T.CP_CHAR | T.CP_ISOLATE and m.cls[0xF900] == T.CP_MAPPED | T.CP_ISOLATE
        assert m.outputs(0xE9) == [0x65] and m.outputs(0xD55C) == [0x1112, 0x1161, 0x11AB] and m.outputs(0x301) == []
        assert m.outputs(0x130) == [0x69] and m.outputs(0xF900) == [0x8C48]
    # the model leaves out, of the assigned code points outside Co / Cs, the 24 and the 13 musical symbols
    # whose decompositions hold one of them
    assigned = [cp for cp in range(0x80, 0x110000) if unicodedata.category(chr(cp)) not in ('Cn', 'Co', 'Cs')]
    left_out = [cp for cp in assigned if not model.covered(cp)]
    assert set(sensitive) <= set(left_out) and len(left_out) == 24 + 13
    assert all(0x1D15E <= cp <= 0x1D1C0 for cp in set(left_out) - set(sensitive))
    # the fast tokenizer's own tables are another Unicode version's: a few hundred code points fewer
    fewer = int(((model.cls & 7) != 0).sum() - ((cp_fast.cls & 7) != 0).sum())
    assert 0 < fewer < 2000
    assert T.wordpiece_cpmap(fast) is not cp_fast and len(T._PROBED) == 1  # probed once


def test_utf8_routing_predicate(toks, cpmap):
    _, fast = toks
    on_host = T.wordpiece_on_host_utf8(fast.all_special_tokens, cpmap)
    for t in ('x[SEP]y', '[CLS]', 'café [MASK]', '\u03a3', 'ΟΔΟ\u03a3', 'a\u0378', '\ue000x', 'a\U0001d15e', '\u1b44', 'x\ud800'):
        assert on_host(t), t
    for t in ('', 'plain text!', 'café', 'naïve — day', '[sep] [unused0]', 'a\x00b\x7f', 'σς', '😀\u200d\ufe0f', '한글',
              '日本語', 'x' * 500 + 'é', '\u2028\xa0'):
        assert not on_host(t), t
    rng = np.random.default_rng(5)
    for _ in range(300):  # exactly the texts with an uncovered code point (no special literal among these)
        t = ''.join(chr(int(c)) for c in rng.integers(0x20, 0x30000, int(rng.integers(0, 12))))
        assert on_host(t) == any(not cpmap.covered(ord(c)) for c in t), t


def test_cased_or_accent_keeping_tokenizers_raise(tmp_path):
    d = tu.write_vocab(tmp_path)
    for kw in (dict(do_lower_case=False), dict(do_lower_case=True, strip_accents=False),
               dict(do_lower_case=False, strip_accents=True)):
        for tok in tu.bert_tokenizers(d, **kw):
            with pytest.raises(ValueError, match='gpu_utf8'):
                T.wordpiece_cpmap(tok)
    for tok in tu.bert_tokenizers(d):
        t = T.wordpiece_table_utf8(tok)
        assert t.kind == T.WORDPIECE_UTF8
        assert dict(zip(t.entries, t.ids)) == {k.encode(): v for k, v in tok.get_vocab().items()}
        tok.add_tokens(['lol'])
        with pytest.raises(ValueError, match='added tokens'):
            T.wordpiece_table_utf8(tok)


def test_create_utf8_validates_on_the_host(cpmap):
    """Every rejection of mec_tok_create_utf8 returns -1 with a message, before a device is touched."""
    lib = _lib.load()
    h = ctypes.c_void_p()
    good = T.Table(T.WORDPIECE_UTF8, ['é'.encode(), b'##a', '日'.encode()], [1, 2, 3])

    def create(table=good, cls=None, mapping=None, null_map=False, **over):
        d, keep = table.desc()
        for k, v in over.items():
            setattr(d, k, v)
        m = cpmap if cls is None else T.CpMap(cls, mapping)
        s, keep_m = m.struct()
        return lib.mec_tok_create_utf8(ctypes.byref(d), None if null_map else ctypes.byref(s), 0, ctypes.byref(h))

    def failed(rc, what):
        assert rc == -1 and what in lib.mec_last_error().decode(), lib.mec_last_error()
        assert not h.value

    def edited(**at):
        cls = cpmap.cls.copy()
        for cp, c in at.items():
            cls[int(cp[1:], 16)] = c
        return cls
    mapping = {int(cp): cpmap.outputs(int(cp)) for cp in cpmap.map_cp}
    assert ctypes.sizeof(T.TokCpMap) == 4 * 8 + 8
    failed(lib.mec_tok_create_utf8(None, None, 0, ctypes.byref(h)), 'null')
    failed(create(null_map=True), 'null')
    s, keep = cpmap.struct()
    s.cls = None
    d, keep_d = good.desc()
    failed(lib.mec_tok_create_utf8(ctypes.byref(d), ctypes.byref(s), 0, ctypes.byref(h)), 'cls is null')
    assert lib.mec_tok_create_utf8(ctypes.byref(d), ctypes.byref(cpmap.struct()[0]), 0, None) == -1
    failed(create(kind=T.WORDPIECE), 'kind')
    failed(create(cls=edited(xD800=T.CP_CHAR), mapping=mapping), 'surrogate')
    failed(create(cls=edited(xE9=7), mapping=mapping), 'unknown class')
    failed(create(cls=edited(xE9=T.CP_CHAR), mapping=mapping), 'not MAPPED')      # listed, but not MAPPED
    failed(create(cls=edited(x2014=T.CP_MAPPED), mapping=mapping), 'missing')     # MAPPED, but not listed
    s, keep = cpmap.struct()
    keep[1][[0, 1]] = keep[1][[1, 0]]
    try:
        failed(lib.mec_tok_create_utf8(ctypes.byref(d), ctypes.byref(s), 0, ctypes.byref(h)), 'ascending')
    finally:
        keep[1][[0, 1]] = keep[1][[1, 0]]
    failed(create(cls=cpmap.cls, mapping={**mapping, 0xE9: [0x110000]}), 'no code point')
    failed(create(cls=cpmap.cls, mapping={**mapping, 0xE9: [0xD800]}), 'no code point')
    failed(create(cls=cpmap.cls, mapping={**mapping, 0xE9: [0x65] * 4}), 'more than 3')
    failed(create(cls=cpmap.cls, mapping={**mapping, 0xE9: [0xC9]}), 'not CHAR or PUNCT')   # É is MAPPED itself
    failed(create(cls=cpmap.cls, mapping={**mapping, 0xE9: [0x301]}), 'not CHAR or PUNCT')
    failed(create(cls=cpmap.cls, mapping={**mapping, 0xE9: [0x20]}), '7-bit rules')
    failed(create(cls=cpmap.cls, mapping={**mapping, 0xE9: [0x1F]}), '7-bit rules')
    for entry in (b'caf\xc3', b'\x80', b'\xc0\xaf', b'\xed\xa0\x80', b'\xf4\x90\x80\x80', b'##\xe2\x82'):
        failed(create(T.Table(T.WORDPIECE_UTF8, [b'a', entry], [1, 2])), 'well-formed')
    # everything mec_tok_create rejects
    failed(create(T.Table(T.WORDPIECE_UTF8, [b'a', b'b', b'a'], [1, 2, 3])), 'duplicates')
    failed(create(T.Table(T.WORDPIECE_UTF8, [b'a'], [-1])), 'id < 0')
    failed(create(max_word=129), 'max_word')
    failed(create(sep_id=-1), 'sep_id')
    failed(create(n=-1), 'n < 0')
    failed(create(off=None), 'null')
    # the 7-bit creation call does not take the new kind
    d, keep_d = good.desc()
    assert lib.mec_tok_create(ctypes.byref(d), 0, ctypes.byref(h)) == -1 and b'kind' in lib.mec_last_error()
