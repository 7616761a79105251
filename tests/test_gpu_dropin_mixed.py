"""GPU: MultimodalFusion.predict_multimodal_batch on requests built from the two clips, two texts and two PNG
faces of test_gpu_dropin._run_three, arranged into all 7 non-empty modality patterns (the all-three one twice)
plus an empty request. Every request must get the keys and value types predict_multimodal gives it; the
per-modality dicts and the attention 'fusion' dicts are checked against the oracle chain at the bars of
_run_three, an average 'fusion' dict bit for bit against fuse_predictions of the returned per-modality probs.

Oracle-argmax assertions are relied on only where _run_three already holds them: each per-modality dict is one
of its six inputs alone, and the two attention requests are its two (clip i, text i, face i) triples. No other
combination's argmax is compared with the oracle (an average row's label is checked against its own
probabilities), so no further top-2 margin had to be established."""
import numpy as np
import pytest

from mec import synthetic as syn
from oracle import audio as oa, fusion as o_f, image as o_i, speech as o_s, text as o_t
from test_gpu_dropin import (EMO, SPEECH_TOL, TEXTS, TOL, _check_dict, _encode, _legacy_tokenizer, _stub_audio,
                             _write_vocab)

pytestmark = pytest.mark.gpu
# (clip, text, face) indices, None = absent: all-three twice, every pair, every single, none
PICKS = [(0, 0, 0), (None, 1, 1), (1, None, None), (None, None, None), (0, 1, None), (None, 0, None),
         (1, None, 0), (1, 1, 1), (None, None, 1)]


def _same_shape(a, b, where):
    """Same keys in the same order, same value types, same list lengths."""
    assert type(a) is type(b), where
    if isinstance(a, dict):
        assert list(a) == list(b), where
        for k in a:
            _same_shape(a[k], b[k], f'{where}[{k!r}]')
    elif isinstance(a, list):
        assert len(a) == len(b), where
        for x, y in zip(a, b):
            _same_shape(x, y, where)


def _setup(fusion, tmp_path, monkeypatch):
    from PIL import Image
    waves = {f'clip{i}.wav': w for i, w in enumerate(oa.synthetic_clips(2, seed=51))}
    _stub_audio(monkeypatch, waves)
    faces = syn.image_inputs(2, seed=52)
    vocab = _write_vocab(tmp_path)
    fusion.text_inference.tokenizer = _legacy_tokenizer(vocab)
    paths = []
    for i in range(2):
        paths.append(str(tmp_path / f'face{i}.png'))
        Image.fromarray(faces[i], 'L').save(paths[i])
    clips = list(waves)
    reqs = [(None if c is None else clips[c], None if t is None else TEXTS[t], None if f is None else paths[f])
            for c, t, f in PICKS]
    return waves, faces, _legacy_tokenizer(vocab), reqs


def _oracle(waves, faces, tok, wseed=1234):
    w = {k: syn.weights(k, wseed) for k in ('speech', 'text', 'image', 'fusion')}
    ref_feat, _ = oa.features_batch(np.stack(list(waves.values())))
    s = o_s.forward(w['speech'], ref_feat)
    ids, mask = zip(*(_encode(tok, t) for t in TEXTS))
    t = o_t.forward(w['text'], np.concatenate(ids), np.concatenate(mask))
    i = o_i.forward(w['image'], faces)
    return w, s, t, i


@pytest.mark.parametrize('precision', ['fp32', 'f16'])
def test_predict_multimodal_batch_all_patterns(dev, tmp_path, monkeypatch, precision):
    from inference.multimodal_fusion import MultimodalFusion
    fusion = MultimodalFusion(seed=1234, device=dev, precision=precision)
    waves, faces, tok, reqs = _setup(fusion, tmp_path, monkeypatch)
    w, rs, rt, ri = _oracle(waves, faces, tok)
    tol = TOL[precision]
    got = fusion.predict_multimodal_batch(reqs)
    as_dicts = fusion.predict_multimodal_batch([dict(audio_path=a or '', text=t, image_path=i) for a, t, i in reqs])
    assert len(got) == len(reqs)
    for k, (a, b) in enumerate(zip(as_dicts, got)):  # dict requests, '' for absent: routed the same
        _same_shape(a, b, f'dict request {k}')
    for k, ((c, t, f), req, res) in enumerate(zip(PICKS, reqs, got)):
        one = fusion.predict_multimodal(*req)
        _same_shape(res, one, f'request {k}')
        present = [m for m, x in zip(('speech', 'text', 'image'), (c, t, f)) if x is not None]
        assert list(res) == present + (['fusion'] if len(present) > 1 else [])
        if c is not None:
            _check_dict(f'{precision} batch request {k} speech', res['speech'], rs[2][c], SPEECH_TOL)
        if t is not None:
            _check_dict(f'{precision} batch request {k} text', res['text'], rt[2][t], tol)
        if f is not None:
            _check_dict(f'{precision} batch request {k} image', res['image'], ri[2][f], tol)
        if len(present) == 3:
            _, fp, aw, dw = o_f.forward(w['fusion'], rs[0][c:c + 1], rt[0][t:t + 1], ri[0][f:f + 1],
                                        rs[2][c:c + 1], rt[2][t:t + 1], ri[2][f:f + 1])
            _check_dict(f'{precision} batch request {k} fusion (attention)', res['fusion'], fp[0], max(tol, SPEECH_TOL))
            for key, ref in (('attention_weights', aw[0]), ('decision_weights', dw[0])):
                d = res['fusion'][key]
                assert list(d) == ['speech', 'text', 'image'] and all(isinstance(v, float) for v in d.values())
                assert np.abs(np.array(list(d.values())) - ref).max() <= max(tol, SPEECH_TOL), key
        elif len(present) == 2:
            d = res['fusion']
            assert list(d) == ['emotion', 'confidence', 'all_probabilities']
            ref = o_f.fuse_predictions(*(res[m]['all_probabilities'] if m in res else None
                                         for m in ('speech', 'text', 'image')))
            assert d['all_probabilities'] == ref.tolist()  # float64, bit-exact with numpy
            assert d['emotion'] == EMO[int(np.argmax(ref))] and d['confidence'] == float(ref.max())
    assert got[3] == {}


def test_without_fusion_model_errors_and_empty(dev, tmp_path, monkeypatch):
    from inference.multimodal_fusion import MultimodalFusion
    fusion = MultimodalFusion(seed=1234, device=dev, precision='f16')
    _, _, _, reqs = _setup(fusion, tmp_path, monkeypatch)
    assert fusion.predict_multimodal_batch([]) == []
    assert fusion.predict_multimodal_batch([(None, '', None)]) == [{}]
    # an unreadable file: ValueError naming the request, before any GPU work
    with pytest.raises(ValueError, match='request 1'):
        fusion.predict_multimodal_batch([reqs[0], (None, None, str(tmp_path / 'missing.png'))])
    with pytest.raises(ValueError, match='request 2'):
        fusion.predict_multimodal_batch([reqs[0], reqs[1], ('missing.wav', None, None)])
    # no fusion model: every multi-modality request takes the average
    with_model = fusion.predict_multimodal_batch(reqs)
    monkeypatch.setattr(fusion, 'fusion_model', None)
    got = fusion.predict_multimodal_batch(reqs)
    for k, (res, ref) in enumerate(zip(got, with_model)):
        assert list(res) == list(ref)
        if 'fusion' in res:
            assert list(res['fusion']) == ['emotion', 'confidence', 'all_probabilities']
            avg = o_f.fuse_predictions(*(res[m]['all_probabilities'] if m in res else None
                                         for m in ('speech', 'text', 'image')))
            assert res['fusion']['all_probabilities'] == avg.tolist()
            _same_shape(res, fusion.predict_multimodal(*reqs[k]), f'request {k}')
    monkeypatch.setattr(fusion.image_inference, 'model', None)
    with pytest.raises(RuntimeError, match='image model not loaded'):
        fusion.predict_multimodal_batch(reqs)
