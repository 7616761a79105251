"""GPU: the BiLSTM text model (csrc/text_lstm.hip) against the float64 restatement tests/lstm_ref.py:
the recurrent kernel alone (mec_lstm_seq_f32), the model (mec_text_lstm_fwd), row invariance across
batch sizes and across every "lstm_rows" tile, and the drop-in class."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import lstm_ref
from mec import _lib, engine, synthetic as syn

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 1234
ROWS = (1, 2, 4)  # every "lstm_rows" value


def _np(t):
    return t.detach().cpu().numpy()


# ------------------------------------------------------------------ kernel level
def _seq(dev, xz, U, reverse, y=True, h=True, rows=None):
    lib = _lib.load()
    B, L, u4 = xz.shape
    u = u4 // 4
    dxz, dU = engine.to_device(xz, dev), engine.to_device(U, dev)
    ys = torch.full((B, L, u), float('nan'), device=dev) if y else None
    hl = torch.full((B, u), float('nan'), device=dev) if h else None
    if rows is not None:
        assert lib.mec_set_option(b'lstm_rows', rows) == 0
    try:
        rc = lib.mec_lstm_seq_f32(ctypes.c_void_p(dxz.data_ptr()), ctypes.c_void_p(dU.data_ptr()), B, L, u, int(reverse),
                                  ctypes.c_void_p(ys.data_ptr() if y else 0), ctypes.c_void_p(hl.data_ptr() if h else 0),
                                  ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        _lib.check(rc, 'mec_lstm_seq_f32')
        torch.cuda.synchronize(dev)
    finally:
        if rows is not None:
            lib.mec_set_option(b'lstm_rows', 2)
    return (_np(ys) if y else None), (_np(hl) if h else None)


def _seq_case(B, L, u, seed):
    rng = np.random.default_rng(seed)
    # pre-activations of the model's size (|x.W + b| of a few units), recurrent weights of the spec's amplitude
    xz = rng.uniform(-2.0, 2.0, (B, L, 4 * u)).astype(np.float32)
    a = float(np.sqrt(3.0 / (4 * u)))
    U = rng.uniform(-a, a, (u, 4 * u)).astype(np.float32)
    return xz, U


@pytest.mark.parametrize('reverse', [0, 1])
@pytest.mark.parametrize('u', [64, 128])
@pytest.mark.parametrize('L', [1, 3, 128])
@pytest.mark.parametrize('B', [1, 5, 17])
def test_lstm_seq_matches_f64(dev, B, L, u, reverse):
    xz, U = _seq_case(B, L, u, 1000 * B + 10 * L + u + reverse)
    ry, rh = lstm_ref.lstm_seq(xz, U, reverse=bool(reverse))
    y, h = _seq(dev, xz, U, reverse)
    ey, eh = np.abs(y - ry).max(), np.abs(h - rh).max()
    print(f'B={B} L={L} u={u} reverse={reverse}: y_seq max|d| {ey:.3g}, h_last max|d| {eh:.3g}')
    assert np.isfinite(y).all() and np.isfinite(h).all()
    assert ey <= 1e-5 and eh <= 1e-5
    # time alignment: the last state is the output at the last step walked
    assert np.array_equal(h, y[:, 0 if reverse else L - 1])


@pytest.mark.parametrize('u', [64, 128])
def test_lstm_seq_rows_and_outputs_are_bit_identical(dev, u):
    """Every lstm_rows tile, either output alone, and a row run alone give the same bits."""
    xz, U = _seq_case(7, 9, u, 77 + u)
    base_y, base_h = _seq(dev, xz, U, 1, rows=2)
    for rows in ROWS:
        y, h = _seq(dev, xz, U, 1, rows=rows)
        assert np.array_equal(y, base_y) and np.array_equal(h, base_h), rows
    assert np.array_equal(_seq(dev, xz, U, 1, h=False)[0], base_y)
    assert np.array_equal(_seq(dev, xz, U, 1, y=False)[1], base_h)
    y1, h1 = _seq(dev, xz[4:5], U, 1)
    assert np.array_equal(y1[0], base_y[4]) and np.array_equal(h1[0], base_h[4])


# ------------------------------------------------------------------ model
@pytest.fixture(scope='module')
def batch():
    """The B = 37 ragged batch (a full row, a length-1 row, an all-pad row, id 9999, two out-of-range
    ids) and its float64 outputs, computed once."""
    ids = syn.text_lstm_inputs(37, 128, seed=3, ragged=True)
    assert (ids[0] >= 10000).any() and (ids[0] < 0).any() and (ids[0] == 9999).any()
    return ids, lstm_ref.forward(syn.weights('text_lstm', SEED), ids)


@pytest.fixture(scope='module')
def model(dev):
    m = engine.LstmTextEncoder(seed=SEED, device=dev)
    yield m
    m.close()


@pytest.fixture(scope='module')
def full(dev, model, batch):
    out = model.forward(engine.to_device(batch[0], dev))
    torch.cuda.synchronize(dev)
    model.check()
    return [_np(t) for t in out]


@pytest.mark.parametrize('B', [1, 2, 37])
def test_model_matches_f64(dev, model, batch, full, B):
    ids, (rfeat, rlogits, rprobs) = batch
    if B == 37:
        feat, logits, probs = full
    else:
        feat, logits, probs = (_np(t) for t in model.forward(engine.to_device(ids[:B], dev)))
    ep = np.abs(probs - rprobs[:B]).max()
    ef = np.abs(feat - rfeat[:B]).max() / np.abs(rfeat[:B]).max()
    el = np.abs(logits - rlogits[:B]).max()
    print(f'B={B}: probs max|d| {ep:.3g}, feat max rel {ef:.3g}, logits max|d| {el:.3g}')
    assert probs.shape == (B, 7) and feat.shape == (B, 64) and logits.shape == (B, 7)
    assert ep <= 1e-5
    # feat within 1e-5 relative, the project's form: max|d| / max|ref| (ReLU outputs include exact zeros)
    assert ef <= 1e-5
    assert (probs.argmax(1) == rprobs[:B].argmax(1)).all()
    assert np.abs(probs.sum(1) - 1).max() <= 1e-6


def test_rows_do_not_depend_on_the_batch(dev, model, batch, full):
    """Row i of B = 37 is bit-identical to the same row run alone (and in a batch of 2)."""
    ids = batch[0]
    for i in (0, 1, 2, 17, 36):
        alone = [_np(t) for t in model.forward(engine.to_device(ids[i:i + 1], dev))]
        for a, f in zip(alone, full):
            assert np.array_equal(a[0], f[i]), i
    pair = [_np(t) for t in model.forward(engine.to_device(ids[35:37], dev))]
    for a, f in zip(pair, full):
        assert np.array_equal(a, f[35:37])


def test_every_lstm_rows_tile_gives_the_same_bits(dev, batch, full):
    ids = engine.to_device(batch[0], dev)
    for rows in ROWS:
        m = engine.LstmTextEncoder(seed=SEED, device=dev)
        try:
            m.set_option('lstm_rows', rows)
            out = [_np(t) for t in m.forward(ids)]
        finally:
            m.close()
        for a, f in zip(out, full):
            assert np.array_equal(a, f), rows
    with pytest.raises(_lib.MecError):
        model_bad = engine.LstmTextEncoder(seed=SEED, device=dev, opts={'lstm_rows': 3})
        model_bad.close()


def test_argument_errors_raise_before_any_launch(dev, model):
    ids = engine.to_device(syn.text_lstm_inputs(2, 128, seed=1), dev)
    feat, logits, probs = model.forward(ids[:0])
    assert feat.shape == (0, 64) and logits.shape == (0, 7) and probs.shape == (0, 7)
    with pytest.raises(TypeError):
        model.forward(ids.to(torch.int64))
    with pytest.raises(ValueError):
        model.forward(ids.cpu())
    with pytest.raises(ValueError):
        model.forward(ids[:, :64].contiguous())
    with pytest.raises(ValueError):
        model.forward(ids[0])
    bad = ids.clone()
    bad[1, 5] = 10000
    with pytest.raises(ValueError, match='out of range'):
        model.forward(bad, check_ids=True)
    # the C entry itself: wrong L, a handle of another kind
    lib, st = _lib.load(), ctypes.c_void_p(0)
    p = ctypes.c_void_p(ids.data_ptr())
    out = torch.zeros(2, 64, device=dev)
    o = ctypes.c_void_p(out.data_ptr())
    assert lib.mec_text_lstm_fwd(model.handle, p, 2, 64, o, o, o, st) == -1 and b'L must be 128' in lib.mec_last_error()
    speech = engine.SpeechEncoder(seed=SEED, device=dev)
    try:
        assert lib.mec_text_lstm_fwd(speech.handle, p, 2, 128, o, o, o, st) == -1
        assert b'wrong kind' in lib.mec_last_error()
        assert lib.mec_speech_fwd(model.handle, o, 2, o, o, o, st) == -1 and b'wrong kind' in lib.mec_last_error()
    finally:
        speech.close()
    assert lib.mec_text_lstm_fwd(model.handle, p, 0, 128, o, o, o, st) == 0
    torch.cuda.synchronize(dev)
    assert not out.any()


def test_every_precision_setting_is_an_fp32_handle(dev, batch, full):
    m = engine.LstmTextEncoder(seed=SEED, device=dev, precision='fp32x3')
    try:
        assert m.lib.mec_precision(m.handle) == _lib.PRECISIONS['fp32']
        out = [_np(t) for t in m.forward(engine.to_device(batch[0][:4], dev))]
        m.check()
    finally:
        m.close()
    for a, f in zip(out, full):
        assert np.array_equal(a, f[:4])


# ------------------------------------------------------------------ drop-in
def test_dropin_predict_batch_equals_predict(dev):
    from inference.text_lstm_inference import FastTextEmotionPredictor
    from config import Config
    with open(os.path.join(ROOT, 'tests', 'golden', 'lstm_demo_sentences.json')) as f:
        texts = json.load(f)['texts']
    assert len(texts) == 6
    words = []
    for t in texts:
        for w in t.lower().replace('!', ' ').split():
            if w not in words:
                words.append(w)
    word_index = {'<OOV>': 1, **{w: i + 2 for i, w in enumerate(words[:-2])}}  # the last two words stay unknown
    pred = FastTextEmotionPredictor(seed=SEED, device=dev, word_index=word_index)
    batch = pred.predict_batch(texts)
    assert len(batch) == 6
    ids = pred.tokenizer.padded([t.lower().strip() for t in texts], 128)
    assert ids[0, :6].tolist() == [2, 3, 4, 5, 6, 7] and (ids[0, 6:] == 0).all() and (ids[5] == 1).sum() == 2
    ref = lstm_ref.forward(syn.weights('text_lstm', SEED), ids)[2]
    for i, (t, b) in enumerate(zip(texts, batch)):
        one = pred.predict(t)
        assert set(one) == {'emotion', 'confidence', 'probabilities', 'inference_time_ms'}
        assert set(b) == {'text', 'emotion', 'confidence', 'probabilities'}
        assert b['text'] == t and list(b['probabilities']) == list(Config.EMOTIONS)
        assert one['probabilities'] == b['probabilities'] and one['emotion'] == b['emotion']  # bit for bit
        assert one['confidence'] == b['confidence'] == max(b['probabilities'].values())
        assert one['inference_time_ms'] > 0
        got = np.array([b['probabilities'][e] for e in Config.EMOTIONS])
        assert np.abs(got - ref[i]).max() <= 1e-5
        assert b['emotion'] == Config.EMOTIONS[int(ref[i].argmax())]
    assert pred.predict_batch([]) == []
