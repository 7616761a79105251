"""Pure-Python restatement of the two byte-level tokenizer specifications of include/mec.h (mec_tok_*),
in the manner of gemm_ref.py and lstm_ref.py: what the kernels of csrc/tokenizer.hip must compute, byte for
byte, written for reading. tests/test_tokenize_host.py checks it against the host tokenizers."""
import numpy as np


def keras_row(data: bytes, table: dict, delim, oov_id: int, L: int):
    """data: the UTF-8 bytes of the lower-cased text; table: {bytes: id}; delim: 256 flags.
    -> (ids [L], mask [L], len)."""
    out, word = [], bytearray()

    def end_word():
        if word:
            i = table.get(bytes(word), oov_id)
            if i >= 0:
                out.append(i)
            word.clear()
    for b in data:
        if delim[b]:
            end_word()
        else:
            word.append(b)
    end_word()
    out = out[:L]
    n = len(out)
    return out + [0] * (L - n), [1] * n + [0] * (L - n), n


PUNCT = set(range(33, 48)) | set(range(58, 65)) | set(range(91, 97)) | set(range(123, 127))
SPACE = set(b' \t\n\r')


def split_entries(vocab: dict):
    """{vocab form (bytes): id} -> (plain {bytes: id}, continuation {bytes after '##': id})."""
    plain, cont = {}, {}
    for e, i in vocab.items():
        if len(e) > 2 and e[:2] == b'##':
            cont[e[2:]] = i
        else:
            plain[e] = i
    return plain, cont


def wordpiece_word(word: bytes, plain: dict, cont: dict, unk_id: int, max_word: int):
    if len(word) > max_word:
        return [unk_id]
    pieces, s = [], 0
    while s < len(word):
        tab = cont if s else plain
        e = len(word)
        while e > s and word[s:e] not in tab:
            e -= 1
        if e == s:
            return [unk_id]
        pieces.append(tab[word[s:e]])
        s = e
    return pieces


def wordpiece_row(data: bytes, vocab: dict, L: int, lower=1, unk_id=0, cls_id=0, sep_id=0, pad_id=0, max_word=100):
    """data: 7-bit text bytes; vocab: {vocab form (bytes): id}. -> (ids [L], mask [L], len)."""
    plain, cont = split_entries(vocab)
    words, word = [], bytearray()
    for b in data:
        if b in SPACE:
            if word:
                words.append(bytes(word))
                word = bytearray()
        elif b < 0x20 or b == 0x7F:
            continue  # dropped: the bytes around it join
        elif b in PUNCT:
            if word:
                words.append(bytes(word))
                word = bytearray()
            words.append(bytes([b]))
        else:
            word.append(b + 32 if lower and 65 <= b <= 90 else b)
    if word:
        words.append(bytes(word))
    pieces = []
    for w in words:
        pieces += wordpiece_word(w, plain, cont, unk_id, max_word)
    pieces = pieces[:L - 2]
    n = len(pieces) + 2
    return [cls_id] + pieces + [sep_id] + [pad_id] * (L - n), [1] * n + [0] * (L - n), n


def rows(fn, datas, L, *a, **k):
    """fn(data, *a, L, **k) over a batch -> int32 ids [B,L], mask [B,L], len [B]."""
    out = [fn(d, *a, L, **k) for d in datas]
    return (np.array([o[0] for o in out], np.int32).reshape(len(out), L),
            np.array([o[1] for o in out], np.int32).reshape(len(out), L), np.array([o[2] for o in out], np.int32))
