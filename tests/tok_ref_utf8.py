"""Pure-Python restatement of the MEC_TOK_WORDPIECE_UTF8 specification of include/mec.h, in the manner of
tok_ref.py: bytes, the code-point classes and the map in, one row out; what wordpiece_kernel<true> of
csrc/tokenizer.hip must compute, written for reading. tests/test_tokenize_utf8_host.py holds it against the
host tokenizers."""
import tok_ref

UNCOVERED, DROP, SPACE, CHAR, PUNCT, MAPPED, ISOLATE = 0, 1, 2, 3, 4, 5, 8


def decode(data: bytes):
    """The code points of well-formed UTF-8, or None: a byte that can start nothing (0x80-0xC1, 0xF5-0xFF),
    a sequence the text's end cuts off, a byte that does not continue where one must, an overlong form, a
    surrogate, a value above 0x10FFFF."""
    cps, i = [], 0
    while i < len(data):
        b = data[i]
        if b < 0x80:
            cps.append(b)
            i += 1
            continue
        n = 2 if 0xC2 <= b <= 0xDF else 3 if 0xE0 <= b <= 0xEF else 4 if 0xF0 <= b <= 0xF4 else 0
        if n == 0 or i + n > len(data) or any(c & 0xC0 != 0x80 for c in data[i + 1:i + n]):
            return None
        cp = b & (0x7F >> n)
        for c in data[i + 1:i + n]:
            cp = cp << 6 | (c & 0x3F)
        if cp < (0x80, 0x800, 0x10000)[n - 2] or 0xD800 <= cp <= 0xDFFF or cp > 0x10FFFF:
            return None
        cps.append(cp)
        i += n
    return cps


def encode(cp: int) -> bytes:
    return chr(cp).encode('utf-8')


def wordpiece_utf8_row(data: bytes, cls, outputs, vocab: dict, L: int, lower=1, unk_id=0, cls_id=0, sep_id=0,
                       pad_id=0, max_word=100):
    """data: any bytes; cls: 0x110000 classes (entries below 0x80 ignored); outputs(cp): the output code points
    of a MAPPED cp; vocab: {vocab form (bytes): id}. -> (ids [L], mask [L], len); len = -1 marks a row whose
    text is ill-formed or holds an UNCOVERED code point."""
    invalid = [pad_id] * L, [0] * L, -1
    cps = decode(data)
    if cps is None:
        return invalid
    plain, cont = tok_ref.split_entries(vocab)
    words, word = [], []  # a word: its output code points

    def end_word():
        if word:
            words.append(list(word))
            word.clear()
    for cp in cps:
        if cp < 0x80:  # the 7-bit rules of MEC_TOK_WORDPIECE
            if cp in tok_ref.SPACE:
                end_word()
            elif cp < 0x20 or cp == 0x7F:
                pass
            elif cp in tok_ref.PUNCT:
                end_word()
                words.append([cp])
            else:
                word.append(cp + 32 if lower and 65 <= cp <= 90 else cp)
            continue
        c, isolate = cls[cp] & 7, cls[cp] & ISOLATE
        if c == UNCOVERED:
            return invalid
        if c == DROP:
            continue
        if c == SPACE or isolate:
            end_word()
        if c == SPACE:
            continue
        for o in (outputs(cp) if c == MAPPED else [cp]):
            if (o in tok_ref.PUNCT) if o < 0x80 else (cls[o] & 7) == PUNCT:
                end_word()
                words.append([o])
            else:
                word.append(o)
        if isolate:
            end_word()
    end_word()
    pieces = []
    for w in words:
        if len(w) > max_word:  # characters, not bytes
            pieces.append(unk_id)
        else:
            b = b''.join(encode(o) for o in w)
            pieces += tok_ref.wordpiece_word(b, plain, cont, unk_id, len(b))
    pieces = pieces[:L - 2]
    n = len(pieces) + 2
    return [cls_id] + pieces + [sep_id] + [pad_id] * (L - n), [1] * n + [0] * (L - n), n
