"""CPU: the BiLSTM text model's float64 restatement (tests/lstm_ref.py) against torch.nn.LSTM, the
synthetic spec, the Keras tokenizer restatement, and the argument errors of the two C entries."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import lstm_ref
from mec import _lib, synthetic as syn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _torch_bilstm(w, prefix, x, fin, u):
    """torch.nn.LSTM(bidirectional, batch_first) in float64 with the Keras tensors mapped in:
    weight_ih = W.T, weight_hh = U.T, bias_ih = b, bias_hh = 0 (torch's gate order i, f, g, o is Keras')."""
    m = torch.nn.LSTM(fin, u, batch_first=True, bidirectional=True).double()
    with torch.no_grad():
        for d, suf in (('forward', ''), ('backward', '_reverse')):
            p = f'{prefix}/{d}_lstm/'
            getattr(m, 'weight_ih_l0' + suf).copy_(torch.from_numpy(np.asarray(w[p + 'kernel'], np.float64).T.copy()))
            getattr(m, 'weight_hh_l0' + suf).copy_(
                torch.from_numpy(np.asarray(w[p + 'recurrent_kernel'], np.float64).T.copy()))
            getattr(m, 'bias_ih_l0' + suf).copy_(torch.from_numpy(np.asarray(w[p + 'bias'], np.float64)))
            getattr(m, 'bias_hh_l0' + suf).zero_()
        y, (hn, _) = m(torch.from_numpy(x))
    return y.numpy(), torch.cat([hn[0], hn[1]], dim=1).numpy()


def test_restatement_matches_torch_lstm_f64():
    w = syn.weights('text_lstm', 1234)
    ids = syn.text_lstm_inputs(3, 128, seed=5, ragged=True)
    x = np.asarray(w['embedding/embeddings'], np.float64)[np.clip(ids, 0, syn.LSTM_VOCAB - 1)]
    y1 = lstm_ref.bidirectional(w, 'bidirectional', x, True)
    ty1, _ = _torch_bilstm(w, 'bidirectional', x, 128, 128)
    assert y1.shape == ty1.shape == (3, 128, 256)
    assert np.abs(y1 - ty1).max() <= 1e-12
    h2 = lstm_ref.bidirectional(w, 'bidirectional_1', y1, False)
    _, th2 = _torch_bilstm(w, 'bidirectional_1', ty1, 256, 64)
    assert h2.shape == th2.shape == (3, 128)
    assert np.abs(h2 - th2).max() <= 1e-12


def test_lstm_seq_reverse_is_time_aligned():
    rng = np.random.default_rng(0)
    xz, U = rng.standard_normal((2, 5, 256)), rng.standard_normal((64, 256)) * 0.1
    yf, hf = lstm_ref.lstm_seq(xz[:, ::-1], U, reverse=False)
    yb, hb = lstm_ref.lstm_seq(xz, U, reverse=True)
    assert np.array_equal(yb, yf[:, ::-1]) and np.array_equal(hb, hf) and np.array_equal(hb, yb[:, 0])


def test_margins_of_the_gpu_batch():
    """The float64 top-2 margin of every row of the GPU tests' B = 37 batch is >= 1e-3, 100 times
    their 1e-5 parity bar, so argmax can be compared exactly."""
    p = lstm_ref.forward(syn.weights('text_lstm', 1234), syn.text_lstm_inputs(37, 128, seed=3, ragged=True))[2]
    s = np.sort(p, axis=1)
    assert (s[:, -1] - s[:, -2]).min() >= 1e-3
    assert len(set(p.argmax(1))) >= 3  # not one class for every row


def test_spec_blob_and_inputs():
    lib = _lib.load()
    assert syn.blob_size('text_lstm') == 1_732_743
    assert lib.mec_blob_size(syn.KIND_IDS['text_lstm']) == syn.blob_size('text_lstm')
    names = [n for n, _, _, _ in syn.text_lstm_spec()]
    assert names[0] == 'embedding/embeddings' and names[1] == 'bidirectional/forward_lstm/kernel'
    assert names[4] == 'bidirectional/backward_lstm/kernel' and names[7] == 'bidirectional_1/forward_lstm/kernel'
    assert names[-6:] == ['dense/kernel', 'dense/bias', 'dense_1/kernel', 'dense_1/bias', 'output/kernel', 'output/bias']
    w = syn.weights('text_lstm', 1234)
    b = w['bidirectional/forward_lstm/bias']
    assert 0.9 < b[128:256].mean() < 1.1 and abs(b[:128].mean()) < 0.05  # unit_forget_bias
    ids = syn.text_lstm_inputs(5, 128, seed=3, ragged=True)
    assert ids.dtype == np.int32 and ids.shape == (5, 128)
    assert (ids[0, 8:] > 0).all() and ids[1, 0] > 0 and (ids[1, 1:] == 0).all() and (ids[2] == 0).all()
    assert ids[0, 3] == 9999 and ids[0, 5] >= 10000 and ids[0, 7] < 0
    full = syn.text_lstm_inputs(4, 128, seed=3)
    assert full.min() >= 1 and full.max() < 10000


def test_pack_rejects_a_wrong_shape():
    w = dict(syn.weights('text_lstm', 1234))
    w['bidirectional_1/forward_lstm/recurrent_kernel'] = np.zeros((64, 255), np.float32)
    with pytest.raises(ValueError):
        syn.pack('text_lstm', w)


# ------------------------------------------------------------------ tokenizer, hand-derived cases
WORD_INDEX = {'<OOV>': 1, 'i': 2, 'am': 3, 'happy': 4, 'so': 5, "i'm": 6, 'well': 7, 'known': 8, 'rare': 9}


def _tok(**kw):
    from inference.text_lstm_inference import KerasWordIndex
    return KerasWordIndex(WORD_INDEX, **kw)


def test_tokenizer_punctuation_case_and_oov():
    t = _tok()
    assert t.sequence('I am SO happy!!!') == [2, 3, 5, 4]                 # case, trailing punctuation filtered
    assert t.sequence('well-known') == [7, 8]                             # '-' is a filter: two words
    assert t.sequence("I'm happy, unbelievably") == [6, 4, 1]             # apostrophe kept; unknown -> OOV
    assert t.sequence('') == [] and t.sequence(' \t\n ?! ') == []
    assert t.sequence('happy   happy') == [4, 4]                          # empty splits dropped


def test_tokenizer_num_words_cut_and_no_oov():
    assert _tok(num_words=9).sequence('rare known') == [1, 8]             # index >= num_words -> OOV
    assert _tok(num_words=9, oov_token=None).sequence('rare known zzz') == [8]  # no OOV token: dropped
    assert _tok(num_words=None).sequence('rare') == [9]


def test_tokenizer_padding_and_truncation():
    t = _tok()
    ids = t.padded(['happy ' * 200, 'i am', ''], 128)
    assert ids.dtype == np.int32 and ids.shape == (3, 128)
    assert (ids[0] == 4).all()                                            # truncating='post': first 128 kept
    assert ids[1].tolist() == [2, 3] + [0] * 126 and (ids[2] == 0).all()  # padding='post'
    long = t.padded(['i ' * 127 + 'am happy so'], 128)[0]
    assert long[126] == 2 and long[127] == 3                              # the words past 128 are cut


def test_tokenizer_json_forms_and_no_pickle(tmp_path):
    from inference.text_lstm_inference import KerasWordIndex
    plain = tmp_path / 'plain.json'
    plain.write_text(json.dumps(WORD_INDEX))
    assert KerasWordIndex.from_json(str(plain)).sequence('so happy zzz') == [5, 4, 1]
    keras = tmp_path / 'keras.json'
    keras.write_text(json.dumps({'class_name': 'Tokenizer', 'config': {
        'num_words': 8, 'filters': '!"#$%&()*+,-./:;<=>?@[\\]^_`{|}~\t\n', 'lower': True, 'split': ' ',
        'char_level': False, 'oov_token': '<OOV>', 'document_count': 3, 'word_index': json.dumps(WORD_INDEX)}}))
    t = KerasWordIndex.from_json(str(keras))
    assert t.num_words == 8 and t.sequence('So well KNOWN!') == [5, 7, 1]
    pkl = tmp_path / 'text_model_tokenizer.pkl'
    pkl.write_bytes(b'not read')
    with pytest.raises(ValueError, match='never loaded'):
        KerasWordIndex.from_json(str(pkl))


def test_checkpoint_loader_pads_the_vocabulary(tmp_path, monkeypatch):
    from config import Config
    from mec import checkpoints
    w = {k: v for k, v in syn.weights('text_lstm', 7).items()}
    w['embedding/embeddings'] = w['embedding/embeddings'][:321]
    np.savez(tmp_path / 'text_lstm_weights.npz', **w)
    monkeypatch.setattr(Config, 'TEXT_MODEL_PATH', str(tmp_path / 'text_model.h5'))
    got = checkpoints.load_checkpoint('text_lstm')
    assert list(got) == [n for n, _, _, _ in syn.text_lstm_spec()]
    e = got['embedding/embeddings']
    assert e.shape == (10000, 128) and np.array_equal(e[:321], w['embedding/embeddings']) and not e[321:].any()
    assert checkpoints.lstm_tokenizer_path() == str(tmp_path / 'text_lstm_tokenizer.json')
    assert syn.pack('text_lstm', got).size == syn.blob_size('text_lstm')


# ------------------------------------------------------------------ C entries, without a GPU
def test_c_entries_reject_bad_arguments_without_gpu():
    lib = _lib.load()
    p = ctypes.c_void_p(0x1000)
    assert lib.mec_text_lstm_fwd(None, p, 1, 128, p, p, p, None) == -1
    assert b'null model' in lib.mec_last_error()
    for units, L, rev, msg in ((32, 4, 0, b'units'), (256, 4, 0, b'units'), (64, 0, 0, b'L >= 1'),
                               (128, -3, 0, b'L >= 1'), (64, 4, 2, b'reverse')):
        assert lib.mec_lstm_seq_f32(p, p, 2, L, units, rev, p, p, None) == -1, (units, L, rev)
        assert msg in lib.mec_last_error(), lib.mec_last_error()
    assert lib.mec_lstm_seq_f32(p, p, -1, 4, 64, 0, p, p, None) == -1
    assert lib.mec_lstm_seq_f32(p, p, 0, 4, 64, 0, p, p, None) == 0          # B == 0: nothing launched
    assert lib.mec_lstm_seq_f32(None, p, 2, 4, 64, 0, p, p, None) == -1 and b'null operand' in lib.mec_last_error()
    assert lib.mec_lstm_seq_f32(p, p, 2, 4, 64, 0, None, None, None) == -1 and b'no output' in lib.mec_last_error()
    for v in (1, 4, 2):
        assert lib.mec_set_option(b'lstm_rows', v) == 0
    for v in (0, 3, 8):
        assert lib.mec_set_option(b'lstm_rows', v) == -1 and b'bad value' in lib.mec_last_error()
