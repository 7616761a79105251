"""Seeded inputs shared by tests/test_tokenize_utf8_host.py and tests/test_gpu_tokenizer_utf8.py: tok_cases'
synthetic WordPiece vocab plus entries that non-ASCII text can match once it is lower-cased and stripped of
its accents, and generators of texts drawn from the covered code points only."""
import numpy as np

import tok_cases as tc

JAMO = ['ᄀ', 'ᄒ', 'ᅡ', 'ᅳ', 'ᆨ', 'ᆫ', 'ᆯ']  # U+1100 U+1112 U+1161 U+1173 U+11A8 U+11AB U+11AF
LONG = 'ж' * 40                                 # one entry of 80 bytes
VOCAB = list(dict.fromkeys(
    tc.VOCAB + ['ß', '##ß', 'ø', '##ø', 'straße', '日', '本', '豈', '😀', '##😀', '—', '…', '¿', '·', '。', 'cafe',
                'ж', '##ж', LONG, 'σ', '##σ', '##ς', 'i', '한', '\u1112\u1161\u11ab', 'ａ', '##ｂ']
    + JAMO + ['##' + j for j in JAMO] + ['##글']))
# '한' and '##글' hold precomposed syllables: no text can match them (a syllable is mapped to its jamo)


def write_vocab(d):
    (d / 'vocab.txt').write_text('\n'.join(VOCAB) + '\n', encoding='utf-8')
    return d


def bert_tokenizers(d, **kw):
    return tc.bert_tokenizers(d, **kw)


def covered_pools(cls):
    """Code-point pools, each cut down to what `cls` covers."""
    def pool(*ranges):
        cps = np.concatenate([np.arange(lo, hi + 1) for lo, hi in ranges])
        return cps[(cls[cps] & 7) != 0]
    return dict(latin=pool((0xA0, 0x24F), (0x1E00, 0x1EFF)), marks=pool((0x300, 0x36F), (0x483, 0x489)),
                greek_cyrillic=pool((0x370, 0x52F)), jamo=pool((0x1100, 0x11FF)), syllables=pool((0xAC00, 0xD7A3)),
                cjk=pool((0x3000, 0x303F), (0x4E00, 0x4E7F), (0xF900, 0xF9FF), (0x2F800, 0x2F83F), (0xFF00, 0xFFEF)),
                punct=pool((0x2000, 0x206F), (0xA1, 0xBF)), emoji=pool((0x1F600, 0x1F64F), (0xFE00, 0xFE0F), (0x1F3FB, 0x1F3FF)),
                any=np.flatnonzero((cls & 7) != 0))


KNOWN = ['café', 'CAFÉ', 'cafe\u0301', 'Straße', 'STRASSE', 'straße', 'ßß', 'øre', 'Øø', '日本', '日本語', 'x日y本z', '한', '한글',
         '가각', '😀', '😀😀', 'a😀', '😁', '—', '…', '¿que?', 'жж', 'Ж' * 41, 'σοσ', 'ος', 'İi', 'happy', 'running']


def utf8_texts(n, seed, cls):
    """n seeded texts of covered code points: vocabulary words, accented and multi-output characters, marks,
    punctuation, CJK, Hangul jamo and syllables, emoji, ASCII controls, any covered code point."""
    rng = np.random.default_rng(seed)
    pools = covered_pools(cls)
    names = list(pools)
    seps = ['', ' ', ' ', ' ', '\t', '\n', '\xa0', '\u2028', '\u3000', '\u200b', '\u200d', '\x00', '\ufe0f', ',', '\u2014']
    out = []
    for i in range(n):
        parts = []
        for _ in range(int(rng.integers(0, 90 if i % 7 == 0 else 16))):
            k = int(rng.integers(0, 10))
            if k < 3:
                w = KNOWN[int(rng.integers(len(KNOWN)))]
            elif k < 5:
                w = tc.WORDS[int(rng.integers(len(tc.WORDS)))]
                if rng.random() < 0.5:  # an accent, a mark or a dropped character somewhere inside
                    at = int(rng.integers(0, len(w) + 1))
                    w = w[:at] + ['\u0301', '\u0308\u0323', '\u200d', '\xad'][int(rng.integers(4))] + w[at:]
            else:
                name = names[int(rng.integers(len(names)))]
                w = ''.join(chr(int(c)) for c in rng.choice(pools[name], int(rng.integers(1, 40 if k == 9 else 6))))
            if rng.random() < 0.2 and all(ord(c) < 0x80 or cls[ord(c)] & 7 for c in w.upper()):
                w = w.upper()  # 'σ'.upper() is U+03A3, which is not covered
            parts.append(w)
            parts.append(seps[int(rng.integers(len(seps)))])
        out.append(''.join(parts))
    return out
