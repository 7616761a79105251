"""Host side of tokenization on the GPU (include/mec.h mec_tok_*; the kernels are csrc/tokenizer.hip).

Pure Python / numpy, no GPU: packs strings into the byte blob + offsets that mec_tok_encode reads, decides
which texts the kernel can take and which stay with the host tokenizer (the routing predicate), and turns a
fitted Keras word index or a BERT WordPiece tokenizer into the descriptor mec_tok_create takes. A
tokenizer the byte-level specifications cannot express raises ValueError here: there is no silent
fall-back to the host. engine.GpuTokenizer is the device half."""
from __future__ import annotations

import ctypes
import functools
import unicodedata

import numpy as np

KERAS, WORDPIECE, WORDPIECE_UTF8 = 0, 1, 2  # include/mec.h MEC_TOK_*
# include/mec.h MEC_CP_*: a code point's class, or'ed with CP_ISOLATE
CP_UNCOVERED, CP_DROP, CP_SPACE, CP_CHAR, CP_PUNCT, CP_MAPPED, CP_ISOLATE = 0, 1, 2, 3, 4, 5, 8
CP_LIMIT = 0x110000
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
    batch = getattr(on_host, 'batch', None)  # a predicate may decide all texts at once
    flags = batch(texts) if batch is not None else None
    for i, t in enumerate(texts):
        routed = flags[i] if flags is not None else (on_host is not None and on_host(t))
        b = None if routed else utf8(t)
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


def wordpiece_table(tokenizer, unicode: bool = False) -> Table:
    """The table of a BERT WordPiece tokenizer (transformers BertTokenizer / BertTokenizerFast): the
    all-ASCII vocab entries in their vocab form ("##" marks a continuation piece; mec_tok_create strips
    it into a flag), which are all a 7-bit text can match. ValueError when the tokenizer has added
    tokens beyond its special tokens, or strip_accents contradicts do_lower_case (BasicTokenizer ties
    them when strip_accents is None; the 7-bit kernel cannot express the untied forms). unicode: the table of
    wordpiece_table_utf8."""
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
        b = utf8(tok) if unicode else tok.encode('ascii') if tok.isascii() else None
        if b:
            entries.append(b)
            ids.append(i)
    return Table(WORDPIECE_UTF8 if unicode else WORDPIECE, entries, ids, lower=int(bool(lower)), unk_id=need['unk'],
                 cls_id=need['cls'], sep_id=need['sep'], pad_id=need['pad'], max_word=MAX_WORD)


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


# ---- MEC_TOK_WORDPIECE_UTF8: any text, for a lower-casing, accent-stripping BERT tokenizer ----

class TokCpMap(ctypes.Structure):
    """include/mec.h mec_tok_cpmap, field for field."""
    _fields_ = [('cls', ctypes.c_void_p), ('map_cp', ctypes.c_void_p), ('map_off', ctypes.c_void_p),
                ('map_out', ctypes.c_void_p), ('n_map', ctypes.c_int)]


class CpMap:
    """What a code point does (mec_tok_cpmap): cls uint8 [CP_LIMIT], and for the MAPPED ones, ascending in
    map_cp, the outputs map_out[map_off[i]:map_off[i+1]]."""

    def __init__(self, cls, mapping):
        self.cls = np.ascontiguousarray(cls, np.uint8)
        assert self.cls.shape == (CP_LIMIT,)
        cps = sorted(mapping)
        self.map_cp = np.asarray(cps, np.int32).reshape(-1)
        self.map_off = np.zeros(len(cps) + 1, np.int32)
        np.cumsum([len(mapping[c]) for c in cps], out=self.map_off[1:])
        self.map_out = np.asarray([o for c in cps for o in mapping[c]], np.int32).reshape(-1)

    def outputs(self, cp):
        """The output code points of a MAPPED code point."""
        i = int(np.searchsorted(self.map_cp, cp))
        return self.map_out[self.map_off[i]:self.map_off[i + 1]].tolist()

    def covered(self, cp) -> bool:
        return cp < 0x80 or (self.cls[cp] & 7) != CP_UNCOVERED

    def struct(self):
        """-> (TokCpMap, keepalive)."""
        keep = (self.cls, self.map_cp, self.map_off, np.concatenate([self.map_out, np.zeros(1, np.int32)]))
        return TokCpMap(*(a.ctypes.data for a in keep), n_map=len(self.map_cp)), keep


def _is_punctuation(ch):
    """BERT's rule: the ASCII symbols count as punctuation whatever their category."""
    cp = ord(ch)
    if 33 <= cp <= 47 or 58 <= cp <= 64 or 91 <= cp <= 96 or 123 <= cp <= 126:
        return True
    return unicodedata.category(ch).startswith('P')


_CJK = ((0x4E00, 0x9FFF), (0x3400, 0x4DBF), (0x20000, 0x2A6DF), (0x2A700, 0x2B73F), (0x2B740, 0x2B81F),
        (0x2B820, 0x2CEAF), (0xF900, 0xFAFF), (0x2F800, 0x2FA1F))  # BERT's "Chinese character" blocks


@functools.lru_cache(maxsize=1)
def _unicode_model():
    """(cls, {cp: outputs}) by the running interpreter's unicodedata, for a lower-casing, accent-stripping
    BasicTokenizer, whose handling of a code point does not depend on its neighbours: drop U+FFFD and the
    categories C* (U+0000 and \t \n \r are 7-bit), whitespace is Zs and whatever str.isspace holds for, every
    other character stands for NFD(lower(ch)) without its Mn marks, an output that is punctuation is a word of
    its own, and so is a CJK ideograph. Not covered: unassigned, private-use and surrogate code points,
    U+03A3 (its lower case depends on what follows) and the characters outside Mn with a combining class (NFD
    may move them past characters that stay)."""
    cls = np.zeros(CP_LIMIT, np.uint8)
    mapping = {}
    category, combining, normalize = unicodedata.category, unicodedata.combining, unicodedata.normalize
    for cp in range(0x80, CP_LIMIT):
        ch = chr(cp)
        cat = category(ch)
        if cat in ('Cn', 'Co', 'Cs') or cp == 0x3A3 or (cat != 'Mn' and combining(ch)):
            continue
        if cp == 0xFFFD or cat[0] == 'C':
            cls[cp] = CP_DROP
        elif cat == 'Zs' or ch.isspace():
            cls[cp] = CP_SPACE
        else:
            out = [c for c in normalize('NFD', ch.lower()) if category(c) != 'Mn']
            iso = CP_ISOLATE if any(lo <= cp <= hi for lo, hi in _CJK) else 0
            if out == [ch]:
                cls[cp] = (CP_PUNCT if _is_punctuation(ch) else CP_CHAR) | iso
            else:
                cls[cp] = CP_MAPPED | iso
                mapping[cp] = [ord(c) for c in out]
    for cp, out in list(mapping.items()):  # an output stands for itself, or the code point is not covered
        ok = len(out) <= 3 and all((o > 0x20 and o != 0x7F) if o < 0x80 else (cls[o] & 7) in (CP_CHAR, CP_PUNCT)
                                   for o in out)
        if not ok:
            cls[cp] = CP_UNCOVERED
            del mapping[cp]
    cls.setflags(write=False)
    return cls, mapping


def basic_words(text, cpmap: CpMap):
    """The words the model of `cpmap` splits a covered text into (str level; the byte-level statement is
    include/mec.h). What the probe of a fast tokenizer compares with."""
    words, word = [], []

    def end():
        if word:
            words.append(''.join(word))
            word.clear()
    for ch in text:
        cp = ord(ch)
        if cp < 0x80:
            c = (CP_SPACE if ch in ' \t\n\r' else CP_DROP if cp < 0x20 or cp == 0x7F
                 else CP_PUNCT if _is_punctuation(ch) else CP_CHAR)
            outs = (ord(ch.lower()),)
        else:
            c = int(cpmap.cls[cp])
            outs = cpmap.outputs(cp) if c & 7 == CP_MAPPED else (cp,)
        iso, c = c & CP_ISOLATE, c & 7
        if c == CP_UNCOVERED:
            raise ValueError(f'U+{cp:04X} is not covered')
        if c == CP_DROP:
            continue
        if c == CP_SPACE or iso:
            end()
        if c == CP_SPACE:
            continue
        for o in outs:
            if _is_punctuation(chr(o)):
                end()
                words.append(chr(o))
            else:
                word.append(chr(o))
        if iso:
            end()
    end()
    return words


_PROBED = {}  # a fast tokenizer's normalizer + pre-tokenizer state -> the code points it disagrees on


def _fast_disagreements(backend, cpmap: CpMap):
    """The covered code points on which the fast tokenizer's normalizer + pre-tokenizer split otherwise than
    the model, in one of four contexts: between letters, first, last, and between an accented capital and a
    combining mark. (Its tables are another Unicode version's.) Probed once per process and state."""
    norm, pre = backend.normalizer, backend.pre_tokenizer
    key = (norm.__getstate__(), pre.__getstate__())
    if key not in _PROBED:
        bad = []
        normalize, split = norm.normalize_str, pre.pre_tokenize_str
        for cp in np.flatnonzero(cpmap.cls & 7).tolist():
            ch = chr(cp)
            for text in ('a' + ch + 'b', ch + 'b', 'a' + ch, 'Á' + ch + '\u0301B'):
                if [w for w, _ in split(normalize(text))] != basic_words(text, cpmap):
                    bad.append(cp)
                    break
        _PROBED[key] = np.asarray(bad, np.int64)
    return _PROBED[key]


def wordpiece_cpmap(tokenizer) -> CpMap:
    """The code-point table of a BERT tokenizer that lower-cases and strips accents (bert-base-uncased's
    configuration). ValueError for any other: the cased and the accent-keeping forms normalize to NFC, which
    is not a per-code-point operation. For a fast tokenizer the code points on which its own tables disagree
    with the interpreter's unicodedata are left uncovered (_fast_disagreements)."""
    lower, strip = _basic_options(tokenizer)
    if not lower or (strip is not None and not strip):
        raise ValueError(f"tokenize='gpu_utf8' needs do_lower_case and accent stripping (do_lower_case={lower}, "
                         f'strip_accents={strip})')
    cls, mapping = _unicode_model()
    cpmap = CpMap(cls, mapping)
    backend = getattr(tokenizer, 'backend_tokenizer', None) if getattr(tokenizer, 'is_fast', False) else None
    if backend is not None:
        bad = _fast_disagreements(backend, cpmap)
        if bad.size:
            cls = cls.copy()
            cls[bad] = CP_UNCOVERED
            # an output must stay covered too
            mapping = {cp: out for cp, out in mapping.items() if cls[cp] and all(o < 0x80 or cls[o] for o in out)}
            cls[[cp for cp in np.flatnonzero((cls & 7) == CP_MAPPED).tolist() if cp not in mapping]] = CP_UNCOVERED
            cpmap = CpMap(cls, mapping)
    return cpmap


def wordpiece_table_utf8(tokenizer) -> Table:
    """wordpiece_table with every vocab entry that has a UTF-8 encoding (kind WORDPIECE_UTF8)."""
    return wordpiece_table(tokenizer, unicode=True)


def wordpiece_on_host_utf8(specials, covered: CpMap):
    """The WORDPIECE_UTF8 routing predicate: a text that holds one of the tokenizer's special tokens as a
    substring, or a code point `covered` does not cover, stays on the host. The code points of a text that is
    not 7-bit are looked up in one precomputed table, all at once (a `re` character class with ranges above
    U+FFFF is tried range by range: 23 ms for 256 texts). on_host.batch(texts) -> bool [B] decides a whole
    batch with one look-up; pack_texts uses it."""
    specials = tuple(s for s in specials if s)
    uncovered = (covered.cls & 7) == CP_UNCOVERED
    uncovered[:0x80] = False

    def code_points(text):
        return np.frombuffer(text.encode('utf-32-le', 'surrogatepass'), np.uint32)

    def on_host(text):
        return any(s in text for s in specials) or (not text.isascii() and bool(uncovered[code_points(text)].any()))

    def batch(texts):
        hit = np.zeros(len(texts), bool)
        joined = '\0'.join(texts)  # no special token holds U+0000, so none matches across two texts
        if not joined.isascii():
            bad = np.flatnonzero(uncovered[code_points(joined)])
            if bad.size:
                hit[np.searchsorted(np.cumsum([len(t) + 1 for t in texts]), bad, 'right')] = True
        if any(s in joined for s in specials):
            for i, t in enumerate(texts):
                if any(s in t for s in specials):
                    hit[i] = True
        return hit
    on_host.batch = batch
    return on_host
