"""
Speech inference on the MI355X HIP path — drop-in for the reference's
inference/speech_inference.py (same class, methods, result dicts).

The model arithmetic (StandardScaler -> 5 x [Dense, BN, ReLU] -> Dense7 -> softmax) runs in
one fused HIP kernel (csrc/speech_fusion.hip) through libmec_hip.so, and the 56-d
MFCC / chroma / spectral features of preprocess_audio (preprocessing/audio_preprocessing.py:
22-46) run on the GPU too (csrc/audio.hip). By default audio decoding and resampling stay in the
reference's untouched preprocessing/ package (load_audio, imported lazily from the tree this
module is dropped into, as the reference does at inference/speech_inference.py:9). With
load='gpu' a PCM WAV file's bytes go up as they are and one kernel decodes, mixes, resamples and
pads them (csrc/audio_load.hip); a file mec.wav declines takes the host load_audio, per file. The
GPU resampler is the library's own float64 polyphase filter: it is not pinned to librosa's soxr_hq.

Added beyond the reference: predict_features(features) for an already-extracted 56-d
vector, predict_batch(x) for a device-resident [B,56] batch, and features_from_waveforms /
predict_waveforms for device-resident [B, n] waveforms, and predict_files(paths) for a batch of files.
"""

from typing import Dict

import numpy as np

from config import Config
from mec import checkpoints, engine


def _preprocessing():
    # reference: from preprocessing.audio_preprocessing import preprocess_audio, ...
    from preprocessing import audio_preprocessing  # noqa: WPS433 (lazy, needs librosa)
    return audio_preprocessing


class PreprocessingMissing(ImportError):
    """The reference's preprocessing package is needed for a file and cannot be imported."""


class _FileBatch:
    """Audio files on their way to raw 56-d features, in the order they were added. add(path) is host work
    only and routes the file: with load='gpu' a file mec.wav takes becomes a clip for the kernel; any other
    file, and every file with load='host', goes through the reference's load_audio, and where that gives
    another rate than Config.SAMPLE_RATE through preprocess_audio, as SpeechInference._file_features does.
    features() then makes one kernel load, one feature call per route and returns device f32 [n, 56]."""

    def __init__(self, si, expect_files):
        self.si, self.n = si, 0
        self.clips, self.clip_at, self.waves, self.wave_at, self.hostf, self.hostf_at = [], [], [], [], [], []
        # load='host' needs the reference's preprocessing for any file, so its absence shows before any work
        self.ap = _preprocessing() if si.load == 'host' and expect_files else None

    def add(self, path):
        clip = self.si._audio_loader().read_one(path) if self.si.load == 'gpu' else None
        if clip is not None:
            self.clips.append(clip)
            self.clip_at.append(self.n)
        else:
            if self.ap is None:
                try:
                    self.ap = _preprocessing()
                except ImportError as e:  # told apart from a file that cannot be read
                    raise PreprocessingMissing(str(e)) from e
            audio, sr = self.ap.load_audio(path)
            if int(sr) != Config.SAMPLE_RATE:
                self.hostf.append(np.asarray(self.ap.preprocess_audio(path), np.float32).reshape(56))
                self.hostf_at.append(self.n)
            else:
                self.waves.append(np.asarray(audio, np.float32).reshape(-1))
                self.wave_at.append(self.n)
        self.n += 1

    def _device(self):
        return self.si.device if self.si.device is not None else engine.require_gpu(None)

    def _place(self, out, at, rows):
        import torch
        out.index_copy_(0, torch.tensor(at, dtype=torch.int64, device=out.device), rows)

    def waveforms(self):
        """device f32 [n, samples] of the clips and the host waveforms (no file may have taken preprocess_audio)."""
        import torch
        dev = self._device()
        wave = torch.empty((self.n, Config.AUDIO_DURATION * Config.SAMPLE_RATE), dtype=torch.float32, device=dev)
        if self.clips:
            self._place(wave, self.clip_at, self.si._audio_loader().load(self.clips))
        if self.waves:
            self._place(wave, self.wave_at, engine.to_device(np.stack(self.waves), dev))
        return wave

    def features(self):
        import torch
        dev = self._device()
        x = torch.empty((self.n, 56), dtype=torch.float32, device=dev)
        if self.clips:
            self._place(x, self.clip_at, self.si.features_from_waveforms(self.si._audio_loader().load(self.clips)))
        if self.waves:
            self._place(x, self.wave_at, self.si.features_from_waveforms(engine.to_device(np.stack(self.waves), dev)))
        if self.hostf:
            self._place(x, self.hostf_at, engine.to_device(np.stack(self.hostf), dev))
        return x


class SpeechInference:
    def __init__(self, weights=None, seed=None, device=None, load='host'):
        if load not in ('host', 'gpu'):
            raise ValueError(f"load must be 'host' or 'gpu', got {load!r}")
        self.load = load
        self.emotions = Config.EMOTIONS
        self.model = None
        self.scaler = None  # the scaler is part of the device model (applied in-kernel)
        w = checkpoints.resolve('speech', weights, seed)
        if w is not None:
            # No silent CPU fallback: a missing libmec_hip.so or GPU raises MecError here.
            self.model = engine.SpeechEncoder(w, device=device)
        self.device = self.model.device if self.model is not None else None
        self._audio = None
        self._loader = None

    def _audio_loader(self):
        if self._loader is None:
            self._loader = engine.AudioLoader(self._featurizer())
        return self._loader

    def file_batch(self, expect_files: bool = True):
        """The files of one batch, routed one by one on the host (`add`) and then turned into raw features
        in one go (`features`): see _FileBatch."""
        return _FileBatch(self, expect_files)

    def load_waveforms(self, paths):
        """load_audio for a list of files -> device f32 [B, n]: the files mec.wav takes by one kernel call
        (load='gpu'), every other by the host load_audio, which must give Config.SAMPLE_RATE."""
        fb = self.file_batch()
        for p in paths:
            fb.add(p)
        if fb.hostf:
            raise ValueError(f'load_audio gave another rate than {Config.SAMPLE_RATE} Hz')
        return fb.waveforms()

    def predict_files(self, paths):
        """predict for a batch of files: each file routed on the host, then one load, one feature call and
        one forward."""
        if self.model is None:
            return [self._heuristic_predict(p) for p in paths]
        fb = self.file_batch()
        for p in paths:
            fb.add(p)
        if not fb.n:
            return []
        probs = self.predict_batch(fb.features())[2].cpu().numpy()
        self.model.check()
        return [self._as_dict(self.emotions, p) for p in probs]

    def _featurizer(self):
        if self._audio is None:
            self._audio = engine.AudioFeaturizer(Config.SAMPLE_RATE, Config.N_MFCC, device=self.device)
        return self._audio

    def _file_features(self, audio_file_path: str) -> np.ndarray:
        # preprocess_audio (audio_preprocessing.py:40-46): load_audio on the host (decode,
        # resample, pad/trim), the feature arithmetic on the GPU; load='gpu': load_audio on the GPU too
        if self.load == 'gpu':
            fb = self.file_batch()
            fb.add(audio_file_path)
            return fb.features().cpu().numpy()[0]
        audio, sr = _preprocessing().load_audio(audio_file_path)
        if int(sr) != Config.SAMPLE_RATE:
            return _preprocessing().preprocess_audio(audio_file_path)
        wave = engine.to_device(np.asarray(audio, np.float32).reshape(1, -1), self.device)
        return self._featurizer().forward(wave).cpu().numpy()[0]

    def features_from_waveforms(self, wave):
        """wave: device f32 [B, n] (load_audio's fixed length) -> raw 56-d features [B, 56]."""
        return self._featurizer().forward(wave)

    def predict_waveforms(self, wave):
        """wave: device f32 [B, n] -> (feat [B,64], logits [B,7], probs [B,7])."""
        return self.predict_batch(self.features_from_waveforms(wave))

    def _heuristic_predict(self, audio_path: str) -> Dict:
        # reference :36-58 — RMS energy / spectral centroid rule
        ap = _preprocessing()
        if self.load == 'gpu':
            audio, sr = self.load_waveforms([audio_path]).cpu().numpy()[0], Config.SAMPLE_RATE
        else:
            audio, sr = ap.load_audio(audio_path)
        zcr, centroid, rolloff, rms = ap.extract_spectral_features(audio, sr)
        if rms > 0.06 and centroid > 2000:
            label = 'angry'
        elif rms < 0.02 and centroid < 1500:
            label = 'sad'
        else:
            label = 'neutral'
        probs = np.ones(len(self.emotions)) * (0.1 / (len(self.emotions) - 1))
        idx = self.emotions.index(label)
        probs[idx] = 0.9
        return {'emotion': label, 'confidence': float(probs[idx]), 'all_probabilities': probs.tolist()}

    def _forward(self, features: np.ndarray):
        x = np.asarray(features, dtype=np.float32).reshape(1, 56)
        feat, logits, probs = self.model.forward(engine.to_device(x, self.device))
        feat, probs = feat.cpu().numpy()[0], probs.cpu().numpy()[0]  # synchronizes the stream
        self.model.check()  # an expired in-kernel wait raises MecError instead of NaN probs
        return feat, probs

    @staticmethod
    def _as_dict(emotions, probs: np.ndarray) -> Dict:
        idx = int(np.argmax(probs))
        return {'emotion': emotions[idx], 'confidence': float(probs[idx]), 'all_probabilities': probs.tolist()}

    def predict_features(self, features) -> Dict:
        """Per-sample prediction from a raw (pre-scaler) 56-d feature vector."""
        return self._as_dict(self.emotions, self._forward(features)[1])

    def predict(self, audio_file_path: str) -> Dict:
        if self.model is None:
            return self._heuristic_predict(audio_file_path)
        return self.predict_features(self._file_features(audio_file_path))

    def extract_features(self, audio_file_path: str):
        """(64-d block-5 ReLU feature, 7 probs) — one forward instead of the reference's three."""
        if self.model is None:
            return None, None
        return self._forward(self._file_features(audio_file_path))

    def predict_batch(self, x):
        """x: device f32 [B,56] raw features -> (feat [B,64], logits [B,7], probs [B,7])."""
        if self.model is None:
            raise RuntimeError('speech model not loaded')
        return self.model.forward(x)
