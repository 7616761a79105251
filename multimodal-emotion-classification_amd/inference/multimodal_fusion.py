"""
Multimodal fusion on the MI355X HIP path — drop-in for the reference's
inference/multimodal_fusion.py (same class, methods, result dicts).

fuse_with_attention runs the attention-MLP fusion model in one HIP kernel
(csrc/speech_fusion.hip: fusion_kernel); fuse_predictions runs the 0.3/0.35/0.35 weighted
average in float64 on the GPU, bit-identical to the reference's numpy arithmetic.
predict_multimodal follows the reference's control flow (:244-287) but runs each encoder
once: features and probabilities come out of the same forward.

Added beyond the reference: predict_batch(x, ids, mask, gray) -> the whole batched path
(mec.engine.FusedPipeline semantics) on device tensors, and predict_multimodal_batch(requests) ->
predict_multimodal's result dicts for a batch of requests that each carry any subset of the modalities
(one launch set per encoder over the rows that have it, one routed fusion call: mec_fusion_fwd_mixed).
"""

from typing import Dict, Optional

import numpy as np
import torch

from config import Config
from mec import checkpoints, engine
from mec import _lib
from mec._lib import MecError

from inference import speech_inference as _speech
from inference.speech_inference import SpeechInference
from inference.text_inference import TextInference
from inference.image_inference import ImageInference

_MODS = ('speech', 'text', 'image')


class MultimodalFusion:
    def __init__(self, weights=None, seed=None, device=None, precision=None, image_resize='host',
                 image_convert='host', audio_load='host', image_decode='host'):
        weights = weights or {}
        self.emotions = Config.EMOTIONS
        self.weights = [0.3, 0.35, 0.35]  # speech, text, image (reference :23)
        self.fusion_model = None
        self.speech_inference = SpeechInference(weights.get('speech'), seed, device, load=audio_load)
        self.text_inference = TextInference(weights.get('text'), seed, device, precision=precision)
        self.image_inference = ImageInference(weights.get('image'), seed, device, precision=precision,
                                              resize=image_resize, convert=image_convert, decode=image_decode)
        w = checkpoints.resolve('fusion', weights.get('fusion'), seed)
        if w is not None:
            self.fusion_model = engine.FusionHead(w, device=device)  # raises MecError without HIP/GPU
        self.device = (self.fusion_model.device if self.fusion_model is not None
                       else engine.require_gpu(device))

    def fuse_predictions(self, speech_probs, text_probs, image_probs) -> Dict:
        """Weighted average (fallback), float64 like the reference's numpy (:184-199)."""
        def t(p):
            return None if p is None else torch.tensor(np.asarray(p, np.float64).reshape(1, 7), device=self.device)
        weighted = engine.fuse_weighted_f64(t(speech_probs), t(text_probs), t(image_probs),
                                            device=self.device).cpu().numpy()[0]
        idx = int(np.argmax(weighted))
        return {'emotion': self.emotions[idx], 'confidence': float(weighted[idx]),
                'all_probabilities': weighted.tolist()}

    def _fusion_tensors(self, speech_feat, text_feat, image_feat, speech_pred, text_pred, image_pred):
        f = lambda a, d: engine.to_device(np.asarray(a, np.float32).reshape(1, d), self.device)  # noqa: E731
        return (f(speech_feat, 64), f(text_feat, 768), f(image_feat, 512),
                f(speech_pred, 7), f(text_pred, 7), f(image_pred, 7))

    def fuse_with_attention(self, speech_feat, text_feat, image_feat,
                            speech_pred, text_pred, image_pred) -> Dict:
        """Attention-MLP fusion (:201-242)."""
        if self.fusion_model is None:
            return self.fuse_predictions(speech_pred, text_pred, image_pred)
        try:
            logits, probs, aw, dw = self.fusion_model.forward(
                *self._fusion_tensors(speech_feat, text_feat, image_feat, speech_pred, text_pred, image_pred))
            preds, aw, dw = probs.cpu().numpy()[0], aw.cpu().numpy()[0], dw.cpu().numpy()[0]
            idx = int(np.argmax(preds))
            return {
                'emotion': self.emotions[idx],
                'confidence': float(preds[idx]),
                'all_probabilities': preds.tolist(),
                'attention_weights': {m: float(aw[j]) for j, m in enumerate(_MODS)},
                'decision_weights': {m: float(dw[j]) for j, m in enumerate(_MODS)},
            }
        except MecError:
            raise
        except Exception as e:
            print(f"Fusion model error: {e}")
            return self.fuse_predictions(speech_pred, text_pred, image_pred)

    def predict_multimodal(self, audio_path: Optional[str] = None,
                           text: Optional[str] = None,
                           image_path: Optional[str] = None):
        """Any combination of modalities (:244-287)."""
        results = {}
        if audio_path:
            results['speech'] = self.speech_inference.predict(audio_path)
        if text:
            results['text'] = self.text_inference.predict(text)
        if image_path:
            results['image'] = self.image_inference.predict(image_path)

        if len(results) > 1:
            s_probs = results['speech']['all_probabilities'] if 'speech' in results else None
            t_probs = results['text']['all_probabilities'] if 'text' in results else None
            i_probs = results['image']['all_probabilities'] if 'image' in results else None
            if self.fusion_model is not None and audio_path and text and image_path:
                try:
                    s_feat, s_pred = self.speech_inference.extract_features(audio_path)
                    t_feat, t_pred = self.text_inference.extract_features(text)
                    i_feat, i_pred = self.image_inference.extract_features(image_path)
                    if all(x is not None for x in (s_feat, t_feat, i_feat)):
                        results['fusion'] = self.fuse_with_attention(s_feat, t_feat, i_feat, s_pred, t_pred, i_pred)
                    else:
                        results['fusion'] = self.fuse_predictions(s_probs, t_probs, i_probs)
                except MecError:
                    raise
                except Exception as e:
                    print(f"Feature extraction failed: {e}")
                    results['fusion'] = self.fuse_predictions(s_probs, t_probs, i_probs)
            else:
                results['fusion'] = self.fuse_predictions(s_probs, t_probs, i_probs)
        return results

    def predict_batch(self, x_speech, ids, mask, gray):
        """Whole tri-modal batch on device tensors -> dict of (feat, logits, probs) per
        modality and (logits, probs, attn_w, dec_w) for the fusion."""
        for m, obj in (('speech', self.speech_inference), ('text', self.text_inference),
                       ('image', self.image_inference)):
            if obj.model is None:
                raise RuntimeError(f'{m} model not loaded')
        if self.fusion_model is None:
            raise RuntimeError('fusion model not loaded')
        sf, sl, sp = self.speech_inference.model.forward(x_speech)
        # fp32x3 text / image handles: synchronized and checked (a batch outside the planes' range is
        # answered by the fp32 engine before the fusion reads it; TextInference / ImageInference.predict_batch)
        tf, tl, tp = self.text_inference.predict_batch(ids, mask)
        imf, il, ip = self.image_inference.predict_batch(gray)
        fl, fp, aw, dw = self.fusion_model.forward(sf, tf, imf, sp, tp, ip)
        return {'speech': (sf, sl, sp), 'text': (tf, tl, tp), 'image': (imf, il, ip), 'fusion': (fl, fp, aw, dw)}

    def predict_multimodal_batch(self, requests):
        """`predict_multimodal` for a batch: requests is a sequence of (audio_path, text, image_path)
        tuples or dicts with those keys, a falsy entry meaning absent (the reference's `if audio_path:`).
        -> one dict per request with the keys and value types predict_multimodal gives that request:
        'speech' / 'text' / 'image' where present, 'fusion' for two or more modalities (with
        'attention_weights' / 'decision_weights' on the attention route only), {} for an empty request.

        Each encoder runs once over the requests that have its modality and one fusion call routes every
        request (engine.FusionHead.forward_mixed; engine.fuse_mixed without a fusion model, where every
        multi-modality request takes the average); one device-to-host copy at the end. Needs the three
        encoder models (RuntimeError otherwise, as predict_batch). Files are read before any GPU work: one
        that cannot be read raises ValueError naming its request (the heuristic and neutral fallbacks stay
        with the per-request method)."""
        for m, obj in (('speech', self.speech_inference), ('text', self.text_inference),
                       ('image', self.image_inference)):
            if obj.model is None:
                raise RuntimeError(f'{m} model not loaded')
        if self.text_inference.tokenizer is None:
            raise RuntimeError('text tokenizer not loaded')
        reqs = []
        for r in requests:
            a, t, i = (r.get('audio_path'), r.get('text'), r.get('image_path')) if isinstance(r, dict) else r
            reqs.append((a or None, t or None, i or None))
        present = np.array([[x is not None for x in r] for r in reqs], bool).reshape(-1, 3)
        # ---- host: decode every file first
        # (audio_load='gpu': a PCM WAV file's bytes are read here and decoded on the GPU below; any other file
        # is decoded here, per file)
        audio = self.speech_inference.file_batch(bool(present[:, 0].any()))
        images = []  # per compact image row: what ImageInference.file_item makes of the file
        image_req = []  # ... and its request
        ni = 0
        for b, (a, _, i) in enumerate(reqs):
            if a is not None:
                try:
                    audio.add(a)
                except _speech.PreprocessingMissing:  # as today: not a property of the request
                    raise
                except Exception as e:
                    raise ValueError(f'request {b}: cannot read audio {a!r}: {e}') from e
            if i is not None:
                try:
                    # image_decode='gpu': a JPEG file of the GPU decoder's domain is read here and decoded below
                    images.append(self.image_inference.file_item(i))
                    image_req.append(b)
                except MecError:
                    raise
                except Exception as e:
                    raise ValueError(f'request {b}: cannot read image {i!r}: {e}') from e
                ni += 1
        texts = [t for _, t, _ in reqs if t is not None]
        dev = self.device
        # ---- encoders, each over its compact rows
        speech = text = image = None
        if audio.n:
            x = audio.features()
            sf, _, sp = self.speech_inference.model.forward(x)
            speech = (sf, sp)
        if texts:
            ids, mask = self.text_inference.encode_batch(texts)
            if not isinstance(ids, torch.Tensor):
                ids, mask = engine.to_device(ids, dev), engine.to_device(mask, dev)
            tf, _, tp = self.text_inference.model.checked('forward', ids, mask)
            text = (tf, tp)
        if ni:
            # one forward per model-input shape, placed in compact order; with image_resize='gpu' the images
            # the GPU resizes are grouped by channel count and resized in one call per group; with
            # image_convert='gpu' they are converted and tested for gray there too
            unreadable = {}  # a file the GPU decoder gave up and Pillow cannot read either
            image = self.image_inference.forward_routed(images, unreadable)
            for row in sorted(unreadable):
                b = image_req[row]
                raise ValueError(f'request {b}: cannot read image {reqs[b][2]!r}: {unreadable[row]}') from unreadable[row]
        # ---- one routed fusion call
        plan = engine.fusion_mixed_plan(present, self.fusion_model is not None, dev)
        if self.fusion_model is not None:
            fused, _, aw, dw = self.fusion_model.forward_mixed(plan, speech, text, image)
        else:
            fused, _, aw, dw = engine.fuse_mixed(plan, *(None if p is None else p[1] for p in (speech, text, image)))
        # ---- the one device-to-host copy (float32 -> float64 is exact)
        parts = [fused, aw, dw] + [p[1] for p in (speech, text, image) if p is not None]
        host = torch.cat([p.reshape(-1).double() for p in parts]).cpu().numpy()
        self.speech_inference.model.check()
        cut = np.cumsum([0] + [p.numel() for p in parts])
        views = [host[cut[k]:cut[k + 1]].reshape(parts[k].shape) for k in range(len(parts))]
        fused, aw, dw = views[:3]
        probs = dict(zip([m for m, p in zip(_MODS, (speech, text, image)) if p is not None], views[3:]))
        as_dict = SpeechInference._as_dict
        results = []
        for b in range(len(reqs)):
            res = {}
            for m, idx in zip(_MODS, (plan.s_idx, plan.t_idx, plan.i_idx)):
                if idx[b] >= 0:
                    res[m] = as_dict(self.emotions, probs[m][idx[b]])
            if plan.route[b] >= _lib.ROUTE_AVERAGE:
                res['fusion'] = as_dict(self.emotions, fused[b])
            if plan.route[b] == _lib.ROUTE_ATTENTION:
                res['fusion']['attention_weights'] = {m: float(aw[b, j]) for j, m in enumerate(_MODS)}
                res['fusion']['decision_weights'] = {m: float(dw[b, j]) for j, m in enumerate(_MODS)}
            results.append(res)
        return results

    def check(self):
        """After predict_batch: synchronize the device and raise MecError if a kernel flagged an
        after-the-fact error (the speech DNN's expired wait; an fp32x3 activation outside the f16 range)."""
        torch.cuda.synchronize(self.device)
        for obj in (self.speech_inference.model, self.text_inference.model, self.image_inference.model,
                    self.fusion_model):
            if obj is not None:
                obj.check()
