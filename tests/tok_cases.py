"""Seeded inputs shared by tests/test_tokenize_host.py and tests/test_gpu_tokenizer.py: a synthetic
WordPiece vocab (the fixture pattern of tests/test_tokenizer.py; no BERT vocab exists offline), a fitted
Keras word index, and text generators."""
import numpy as np

WORDS = ['i', 'am', 'so', 'happy', 'sad', 'today', 'this', 'is', 'the', 'worst', 'day', 'ever', 'what', 'a',
         'wonderful', 'surprise', 'angry', 'fear', 'of', 'dark', 'not', 'sure', 'how', 'feel', 'about', 'it', 'un',
         'believ', 'able', 'love', 'hate', 'you', 'we', 'they', 'run', 'running']
SUB = ['##s', '##ing', '##ed', '##able', '##ly', '##er', '##est', '##y', '##n', '##d', '##e', '##a']
PUNCT = list('.,!?\'"-:;()')
LETTERS = [chr(c) for c in range(ord('a'), ord('z') + 1)]
# no 'q' and no '##z': a word that holds one has an unmatched position and becomes [UNK]
VOCAB = (['[PAD]'] + [f'[unused{i}]' for i in range(5)] + ['[UNK]', '[CLS]', '[SEP]', '[MASK]'] + PUNCT
         + [c for c in LETTERS if c != 'q'] + ['##' + c for c in LETTERS if c != 'z'] + WORDS + SUB
         + ['0', '1', '2', '##0', '##1', 'café', '##é', 'Happy', 'A', '##B'])
VOCAB = list(dict.fromkeys(VOCAB))


def write_vocab(d):
    (d / 'vocab.txt').write_text('\n'.join(VOCAB) + '\n', encoding='utf-8')
    return d


def bert_tokenizers(d, **kw):
    """(BertTokenizerLegacy: transformers 4.30's pure-Python BertTokenizer, BertTokenizerFast) on VOCAB."""
    from transformers import BertTokenizerFast
    from transformers.models.bert.tokenization_bert_legacy import BertTokenizerLegacy
    return BertTokenizerLegacy(str(d / 'vocab.txt'), **kw), BertTokenizerFast.from_pretrained(str(d), **kw)


def host_rows(tokenizer, texts, L=128):
    """The reference's tokenizer call (text_inference.py:78-85) per text -> int32 ids, mask [B,L]."""
    ids, mask = np.zeros((len(texts), L), np.int32), np.zeros((len(texts), L), np.int32)
    for i, t in enumerate(texts):
        enc = tokenizer(t, add_special_tokens=True, max_length=L, padding='max_length', truncation=True,
                        return_tensors='np')
        ids[i], mask[i] = enc['input_ids'][0], enc['attention_mask'][0]
    return ids, mask


def ascii_texts(n, seed):
    """n seeded 7-bit texts: vocabulary words with and without suffixes, random letter strings of 1..120
    characters, upper case, punctuation, every kind of whitespace, and (text i holds byte i % 128) every
    control byte; some long enough to truncate at 128."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        parts = []
        for _ in range(int(rng.integers(0, 150 if i % 7 == 0 else 24))):
            k = int(rng.integers(0, 10))
            if k < 4:
                w = WORDS[int(rng.integers(len(WORDS)))]
                if rng.random() < 0.4:
                    w += SUB[int(rng.integers(len(SUB)))][2:]
            elif k < 6:
                w = ''.join(LETTERS[int(c)] for c in rng.integers(0, 26, int(rng.integers(1, 121 if k == 5 else 8))))
            elif k == 6:
                w = PUNCT[int(rng.integers(len(PUNCT)))] * int(rng.integers(1, 4))
            elif k == 7:
                w = chr(int(rng.integers(0, 128)))
            else:
                w = str(int(rng.integers(0, 3000)))
            if rng.random() < 0.15:
                w = w.upper() if rng.random() < 0.5 else w.capitalize()
            parts.append(w)
            parts.append(['', ' ', ' ', ' ', '  ', '\t', '\n', '\r', '\x00', '\x1f'][int(rng.integers(0, 10))])
        parts.insert(int(rng.integers(0, len(parts) + 1)), chr(i % 128))
        out.append(''.join(parts))
    return out


KERAS_WORDS = WORDS + ['café', 'naïve', '日本語', 'ünïcödé', "don't", 'x\x00y', 'rare', 'rarer']


def keras_word_index(n_extra=0):
    """{word: index} as a fitted keras Tokenizer has it: '<OOV>' is 1, then words by frequency rank."""
    wi = {'<OOV>': 1}
    for w in KERAS_WORDS + [f'w{j}' for j in range(n_extra)]:
        wi[w] = len(wi) + 1
    return wi


def keras_texts(n, seed):
    """n seeded texts of known, unknown and multi-byte words, filter characters and odd whitespace."""
    rng = np.random.default_rng(seed)
    pool = KERAS_WORDS + ['zzz', 'unknown', 'caffè', '日本', 'Ünï', 'HAPPY', 'w3', 'w11']
    seps = [' ', ' ', ' ', '  ', ', ', '. ', '!', '\t', '\n', '-', ' \r ', '\xa0', '…']
    out = []
    for i in range(n):
        k = int(rng.integers(0, 200 if i % 5 == 0 else 30))
        out.append(''.join(pool[int(rng.integers(len(pool)))] + seps[int(rng.integers(len(seps)))] for _ in range(k)))
    return out
