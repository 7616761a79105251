"""Host side of tokenization on the GPU (include/mec.h mec_tok_*; the kernels are csrc/tokenizer.hip).

Pure Python / numpy, no GPU: packs strings into the byte blob + offsets that mec_tok_encode reads, decides
which texts the kernel can take and which stay with the host tokenizer (the routing predicate), and turns a
fitted Keras word index or a BERT WordPiece tokenizer into the descriptor mec_tok_create takes. A
tokenizer the byte-level specifications cannot express raises ValueError here: there is no silent
fall-back to the host. engine.GpuTokenizer is the device half."""
from __future__ import annotations

import ctypes

import numpy as np

KERAS, WORDPIECE = 0, 1  # include/mec.h MEC_TOK_*
MAX_WORD = 100           # transformers' WordpieceTokenizer.max_input_chars_per_word


class TokDesc(ctypes.Structure):
    """include/mec.h mec_tok_desc, field for field."""
    _fields_ = [('kind', ctypes.c_int), ('pool', ctypes.c_void_p), ('off', ctypes.c_void_p), ('id', ctypes.c_void_p),
                ('n', ctypes.c_int), ('delim', ctypes.c_uint8 * 256), ('oov_id', ctypes.c_int), ('lower', ctypes.c_int),
                ('unk_id', ctypes.c_int), ('cls_id', ctypes.c_int), ('sep_id', ctypes.c_int), ('pad_id', ctypes.c_int),
                ('max_word', ctypes.c_int)]


def utf8(text):
    """The text's UTF-8 bytes, or None when it has none (a lone surrogate)."""
    try:
        return text.encode('utf-8')
    except UnicodeEncodeError:
        return None


def pack_texts(texts, on_host=None):
    """-> (blob uint8 [max(total, 1)], off int64 [B+1], host int list): text i is blob[off[i]:off[i+1]].
    A text for which on_host(text) holds, and a text without a UTF-8 encoding, contributes no bytes and
    is listed in `host` (ascending): its row is the host tokenizer's to fill."""
    parts, host = [], []
    for i, t in enumerate(texts):
        b = None if (on_host is not None and on_host(t)) else utf8(t)
        if b is None:
            host.append(i)
            b = b''
        parts.append(b)
    off = np.zeros(len(parts) + 1, np.int64)
    np.cumsum([len(b) for b in parts], out=off[1:])
    blob = np.frombuffer(b''.join(parts) or b'\0', np.uint8)
    return blob, off, host


def wordpiece_on_host(specials):
    """The WORDPIECE routing predicate: a text that is not 7-bit, or that holds one of the tokenizer's
    special tokens as a substring (the tokenizers never split those), stays on the host."""
    specials = tuple(s for s in specials if s)

    def on_host(text):
        return not text.isascii() or any(s in text for s in specials)
    return on_host


class Table:
    """A vocabulary in mec_tok_create's form: entries (bytes) -> ids, and the descriptor's scalars."""

    def __init__(self, kind, entries, ids, **scalars):
        self.kind, self.entries, self.ids = kind, list(entries), [int(i) for i in ids]
        self.delim = scalars.pop('delim', bytes(256))
        self.scalars = dict(oov_id=-1, lower=0, unk_id=0, cls_id=0, sep_id=0, pad_id=0, max_word=MAX_WORD)
        self.scalars.update(scalars)

    def desc(self):
        """-> (TokDesc, keepalive): the ctypes descriptor and the arrays it points into."""
        pool = np.frombuffer(b''.join(self.entries) or b'\0', np.uint8)
        off = np.zeros(len(self.entries) + 1, np.int64)
        np.cumsum([len(e) for e in self.entries], out=off[1:])
        ids = np.asarray(self.ids, np.int32).reshape(-1)
        d = TokDesc(kind=self.kind, pool=pool.ctypes.data, off=off.ctypes.data, id=ids.ctypes.data, n=len(self.entries),
                    **self.scalars)
        ctypes.memmove(d.delim, bytes(self.delim), 256)
        return d, (pool, off, ids)


def keras_table(wi) -> Table:
    """The table of a KerasWordIndex-like object (word_index, num_words, oov_index, filters,
    split). Holds only the entries with index < num_words: the rest are OOV to
    texts_to_sequences anyway. ValueError when `split` is not one ASCII character or a filter character
    is not ASCII (the kernel separates words on single bytes)."""
    split = wi.split
    if not isinstance(split, str) or len(split) != 1 or not split.isascii():
        raise ValueError(f"tokenize='gpu': split must be a single ASCII character, got {split!r}")
    filters = list(wi.filters)
    bad = [c for c in filters if not c.isascii()]
    if bad:
        raise ValueError(f"tokenize='gpu': filters holds a non-ASCII character ({bad[0]!r})")
    delim = bytearray(256)
    for c in filters + [split]:
        delim[ord(c)] = 1
    entries, ids = [], []
    for w, i in wi.word_index.items():
        if wi.num_words and i >= wi.num_words:
            continue
        b = utf8(w)
        if not b or any(delim[x] for x in b):  # no word of a text can equal it
            continue
        if i < 0:
            raise ValueError(f"tokenize='gpu': word {w!r} has a negative index")
        entries.append(b)
        ids.append(i)
    oov = wi.oov_index
    if oov is not None and oov < 0:
        raise ValueError("tokenize='gpu': the OOV token has a negative index")
    return Table(KERAS, entries, ids, delim=bytes(delim), oov_id=-1 if oov is None else int(oov))


def wordpiece_table(tokenizer) -> Table:
    """The table of a BERT WordPiece tokenizer (transformers BertTokenizer / BertTokenizerFast): the
    all-ASCII vocab entries in their vocab form ("##" marks a continuation piece; mec_tok_create strips
    it into a flag), which are all a 7-bit text can match. ValueError when the tokenizer has added
    tokens beyond its special tokens, or strip_accents contradicts do_lower_case (BasicTokenizer ties
    them when strip_accents is None; the 7-bit kernel cannot express the untied forms)."""
    vocab = tokenizer.get_vocab()
    specials = set(tokenizer.all_special_tokens)
    added = [t for t in tokenizer.get_added_vocab() if t not in specials]
    if added:
        raise ValueError(f"tokenize='gpu': the tokenizer has added tokens beyond its special tokens ({added[0]!r})")
    lower, strip = _basic_options(tokenizer)
    if strip is not None and bool(strip) != bool(lower):
        raise ValueError(f"tokenize='gpu': strip_accents={strip} contradicts do_lower_case={lower}")
    need = {n: getattr(tokenizer, n + '_token_id') for n in ('unk', 'cls', 'sep', 'pad')}
    missing = [n for n, v in need.items() if v is None]
    if missing:
        raise ValueError(f"tokenize='gpu': the tokenizer has no {missing[0]} token")
    entries, ids = [], []
    for tok, i in vocab.items():
        if tok and tok.isascii():
            entries.append(tok.encode('ascii'))
            ids.append(i)
    return Table(WORDPIECE, entries, ids, lower=int(bool(lower)), unk_id=need['unk'], cls_id=need['cls'],
                 sep_id=need['sep'], pad_id=need['pad'], max_word=MAX_WORD)


def _basic_options(tokenizer):
    """(do_lower_case, strip_accents) of a slow tokenizer (its attributes) or a fast one (its normalizer)."""
    bt = getattr(tokenizer, 'basic_tokenizer', None)
    if bt is not None:
        return bool(bt.do_lower_case), bt.strip_accents
    backend = getattr(tokenizer, 'backend_tokenizer', None)
    if backend is not None and backend.normalizer is not None:
        import json
        st = json.loads(backend.normalizer.__getstate__())
        if st.get('type') != 'BertNormalizer':
            raise ValueError(f"tokenize='gpu': normalizer {st.get('type')!r} is not BertNormalizer")
        return bool(st.get('lowercase')), st.get('strip_accents')
    raise ValueError("tokenize='gpu': not a BERT WordPiece tokenizer (no basic_tokenizer, no BertNormalizer)")
