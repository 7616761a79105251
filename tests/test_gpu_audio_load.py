"""GPU: the audio front end (csrc/audio_load.hip). mec_audio_load_ragged against the numpy /
scipy restatement (tests/resample_ref.py): bit for bit where nothing is resampled, and for resampled clips

    |gpu - f32(ref)| <= ulp32(ref) + 2 * N * 2^-53 * S * peak

with the library's own taps (N taps per output, S the largest per-phase sum of |up * h|, peak = max |x|): one
output rounding plus two float64 summation orders. Then tones, raggedness, the rejections and the drop-in
classes with load='gpu'."""
import sys
import types

import numpy as np
import pytest
import torch

import resample_ref as rr
from mec import engine

pytestmark = pytest.mark.gpu

N_OUT = rr.N_OUT
FORMATS = (rr.U8, rr.S16, rr.S24, rr.S32, rr.F32)


@pytest.fixture(scope='module')
def loader(dev):
    return engine.AudioLoader(engine.AudioFeaturizer(22050, 40, device=dev))


def _noise(frames, ch, seed):
    return np.random.default_rng(seed).uniform(-0.95, 0.95, (frames, ch))


def _clip(fmt, ch, rate, frames, seed=0, upload=None):
    """(bytes, fmt, ch, rate, frames) of seeded noise; `upload` frames of it (default all) are in the bytes."""
    data = rr.encode(_noise(frames if upload is None else upload, ch, seed), fmt)
    return (data, fmt, ch, rate, frames if upload is None else upload)


def _raw_call(loader, dev, src_np, offs, desc, wave, B=None, src_bytes=None, null=()):
    """mec_audio_load_ragged as given (no packing by AudioLoader): for odd offsets and the rejections."""
    src = torch.from_numpy(np.ascontiguousarray(src_np)).to(dev) if src_np is not None and src_np.size else None
    offs = np.asarray(offs, np.int64)
    desc = np.asarray(desc, np.int32).reshape(-1, 4)
    ptr = lambda name, v: None if name in null else v  # noqa: E731
    rc = loader.audio.lib.mec_audio_load_ragged(
        loader.audio.handle, ptr('src', engine._ptr(src)), ptr('offs', offs.ctypes.data), ptr('desc', desc.ctypes.data),
        len(offs) if B is None else B, (src_np.size if src_np is not None else 0) if src_bytes is None else src_bytes,
        ptr('wave', engine._ptr(wave)), wave.shape[1], engine._stream(dev))
    torch.cuda.synchronize(dev)
    return rc


# ---------------------------------------------------------------- exact

def test_identity_rate_is_bit_exact(loader, dev):
    """Rate 22 050: every format x channels x frames {0, 1, 5, 66149, 66150, 66151}, each clip at an odd byte
    offset, equals the numpy decode / mix / pad bit for bit."""
    clips = [_clip(f, ch, 22050, n, seed=7 * f + ch) for f in FORMATS for ch in (1, 2)
             for n in (0, 1, 5, 66149, 66150, 66151)]
    offs, at = [], 1
    for c in clips:
        offs.append(at)
        at += len(c[0]) + (len(c[0]) % 2) + 2  # keeps every offset odd
    src = np.zeros(at, np.uint8)
    for o, c in zip(offs, clips):
        src[o:o + len(c[0])] = np.frombuffer(c[0], np.uint8)
    wave = torch.full((len(clips), N_OUT), 7.0, dtype=torch.float32, device=dev)
    assert _raw_call(loader, dev, src, offs, [c[1:] for c in clips], wave) == 0, loader.audio.lib.mec_last_error()
    got = wave.cpu().numpy()
    for g, c in zip(got, clips):
        ref = rr.fix(rr.decode(*c[:3], c[4]))
        assert np.array_equal(g.view(np.uint32), ref.view(np.uint32)), f'fmt {c[1]} ch {c[2]} frames {c[4]}'


def test_int32_rounds_as_numpy(loader, dev):
    """S32 is the one inexact decode: values around the float32 rounding ties."""
    v = np.array([2 ** 24 + 1, 2 ** 24 + 3, -2 ** 24 - 1, 2 ** 31 - 1, -2 ** 31, 2 ** 30 + 64, 2 ** 30 + 192, 0x7FFFFF40],
                 '<i4')
    got = loader.load([(v.tobytes(), rr.S32, 1, 22050, v.size)]).cpu().numpy()[0, :v.size]
    assert np.array_equal(got, v.astype(np.float32) * np.float32(2.0 ** -31))


# ---------------------------------------------------------------- resampled

def _run_end(rate):
    """A frame count whose output ends inside a workgroup's run and inside a column of it: 1.37 cycles of up."""
    up, down, _ = rr.lib_plan(rate)
    return max(3, int(1.37 * max(up, 256) * down / up))


RESAMPLED = [(rate, frames, fmt, ch) for rate in (44100, 48000, 16000, 8000, 11025, 24414)
             for frames in (1, 2, 1000, _run_end(rate), int(3 * rate) + 5000) for fmt, ch in ((rr.S16, 2), (rr.F32, 1))]


@pytest.fixture(scope='module')
def resampled(loader, dev):
    """One ragged call over every resampled case -> [(case, clip, gpu row)]; clips longer than 3 s upload
    int(3 * rate) frames only, as the caller of the kernel does."""
    clips = [_clip(fmt, ch, rate, frames, seed=rate % 997 + frames % 13, upload=min(frames, int(3 * rate)))
             for rate, frames, fmt, ch in RESAMPLED]
    got = loader.load(clips).cpu().numpy()
    return list(zip(RESAMPLED, clips, got))


@pytest.mark.parametrize('rate', (44100, 48000, 16000, 8000, 11025, 24414))
def test_resampled_within_bound(resampled, rate):
    taps = rr.lib_taps(rate)
    up, down, half = rr.lib_plan(rate)
    N, S = rr.bound_terms(taps, up)
    seen = 0
    for (r, frames, fmt, ch), clip, got in resampled:
        if r != rate:
            continue
        seen += 1
        ref, x = rr.load_ref(*clip, taps)
        peak = float(np.abs(x).max()) if x.size else 0.0
        f32 = ref.astype(np.float32)
        n = min(rr.out_len(clip[4], rate), N_OUT)
        assert not got[n:].any(), f'{rate} Hz frames {frames}: samples past n = {n} are not zero'
        err = np.abs(got.astype(np.float64) - f32.astype(np.float64))
        bound = np.spacing(np.abs(f32)).astype(np.float64) + 2 * N * 2.0 ** -53 * S * peak
        worst = int(np.argmax(err - bound))
        print(f'{rate} Hz fmt {fmt} ch {ch} frames {frames}: max err {err.max():.3g}, slack {2 * N * 2.0 ** -53 * S * peak:.3g}')
        assert (err <= bound).all(), f'{rate} Hz frames {frames} fmt {fmt}: sample {worst} off by {err[worst]:.3g} > {bound[worst]:.3g}'
        assert frames <= 2 or np.abs(got[:n]).max() > 0.01  # the row is a signal, not zeros
    assert seen == 10


def test_tones_from_48k(loader):
    """Amplitude 1 at 48 kHz, away from the ends: 10 kHz comes out as the ideal 22 050 Hz sampling within 1e-6;
    11.6 kHz (past the output's Nyquist) peaks below 1e-6."""
    t = np.arange(144000) / 48000.0
    tone = lambda f: (np.sin(2 * np.pi * f * t).astype('<f4').tobytes(), rr.F32, 1, 48000, t.size)  # noqa: E731
    got = loader.load([tone(10000.0), tone(11600.0)]).cpu().numpy().astype(np.float64)
    m = np.arange(2000, N_OUT - 2000)
    ideal = np.sin(2 * np.pi * 10000.0 * m / 22050.0)
    e_pass, e_stop = np.abs(got[0, m] - ideal).max(), np.abs(got[1, m]).max()
    print(f'10 kHz: {e_pass:.3g}; 11.6 kHz: {e_stop:.3g}')
    assert e_pass <= 1e-6
    assert e_stop < 1e-6


# ---------------------------------------------------------------- ragged

def test_rows_do_not_depend_on_the_batch(loader):
    """All formats, both channel counts, four rates in one call: every row equals its single-clip call bitwise,
    and the same under a permutation."""
    spec = [(rr.U8, 1, 22050, 70000), (rr.S16, 2, 48000, 30011), (rr.S24, 2, 16000, 48000), (rr.S32, 1, 44100, 5),
            (rr.F32, 2, 48000, 144000), (rr.S24, 1, 22050, 0), (rr.U8, 2, 44100, 90001), (rr.F32, 1, 16000, 1),
            (rr.S16, 1, 16000, 20000), (rr.S32, 2, 22050, 66150)]
    clips = [_clip(f, ch, rate, n, seed=i) for i, (f, ch, rate, n) in enumerate(spec)]
    whole = loader.load(clips).cpu().numpy()
    perm = np.random.default_rng(5).permutation(len(clips))
    shuffled = loader.load([clips[i] for i in perm]).cpu().numpy()
    for i, c in enumerate(clips):
        single = loader.load([c]).cpu().numpy()[0]
        assert np.array_equal(whole[i].view(np.uint32), single.view(np.uint32)), f'clip {i}'
    for at, i in enumerate(perm):
        assert np.array_equal(shuffled[at].view(np.uint32), whole[i].view(np.uint32)), f'clip {i} at {at}'
    assert loader.load([]).shape == (0, N_OUT)


# ---------------------------------------------------------------- rejections

def test_rejections_launch_nothing(loader, dev):
    src = np.zeros(64, np.uint8)
    ok = [rr.S16, 2, 48000, 16]  # 64 bytes
    cases = [
        (dict(offs=[0, 0], desc=[ok, [5, 1, 48000, 1]]), 'clip 1 has the unknown format 5'),
        (dict(offs=[0], desc=[[-1, 1, 48000, 1]]), 'clip 0 has the unknown format -1'),
        (dict(offs=[0], desc=[[rr.S16, 3, 48000, 1]]), 'clip 0 has 3 channels'),
        (dict(offs=[0], desc=[[rr.S16, 0, 48000, 1]]), 'clip 0 has 0 channels'),
        (dict(offs=[0, 0, 0], desc=[ok, ok, [rr.S16, 1, 22051, 1]]), 'clip 2 has the rate 22051'),
        (dict(offs=[0], desc=[[rr.S16, 1, 0, 1]]), 'clip 0 has the rate 0'),
        (dict(offs=[0], desc=[[rr.S16, 1, 192001, 1]]), 'clip 0 has the rate 192001'),
        (dict(offs=[0], desc=[[rr.S16, 1, 48000, -1]]), 'clip 0 has frames < 0'),
        (dict(offs=[1], desc=[ok]), 'clip 0 does not lie inside src_bytes'),
        (dict(offs=[-1], desc=[ok]), 'clip 0 does not lie inside src_bytes'),
        (dict(offs=[0], desc=[ok], src_bytes=63), 'clip 0 does not lie inside src_bytes'),
        (dict(offs=[65], desc=[[rr.S16, 1, 48000, 0]]), 'clip 0 does not lie inside src_bytes'),
        (dict(offs=[0], desc=[ok], B=-1), 'B < 0'),
        (dict(offs=[0], desc=[ok], null=('offs',)), 'null'),
        (dict(offs=[0], desc=[ok], null=('desc',)), 'null'),
        (dict(offs=[0], desc=[ok], null=('wave',)), 'null'),
        (dict(offs=[0], desc=[ok], null=('src',)), 'null'),
    ]
    for kw, what in cases:
        wave = torch.full((3, N_OUT), -5.0, dtype=torch.float32, device=dev)
        assert _raw_call(loader, dev, src, wave=wave, **kw) == -1, what
        err = loader.audio.lib.mec_last_error().decode()
        assert err.startswith('requirement failed: mec_audio_load_ragged: ') and what in err, err
        assert bool((wave == -5.0).all()), what
    wave = torch.full((1, N_OUT), -5.0, dtype=torch.float32, device=dev)
    assert _raw_call(loader, dev, src, [], [], wave, B=0) == 0 and bool((wave == -5.0).all())
    assert loader.audio.lib.mec_audio_load_ragged(None, None, None, None, 1, 0, None, N_OUT, None) == -1
    # a zero-frame clip is a zero row
    assert _raw_call(loader, dev, src, [64], [[rr.S16, 2, 48000, 0]], wave) == 0 and not bool(wave.any())


# ---------------------------------------------------------------- end to end

@pytest.fixture(scope='module')
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp('wavs')
    spec = [('a48.wav', rr.S16, 2, 48000, 100000), ('b22.wav', rr.S16, 1, 22050, 40000), ('c24.wav', rr.F32, 1, 24414, 80000),
            ('d22.wav', rr.S24, 2, 22050, 70000)]
    out = []
    for i, (name, fmt, ch, rate, frames) in enumerate(spec):
        data = rr.encode(_noise(frames, ch, 100 + i) * 0.3, fmt)
        (d / name).write_bytes(rr.wav_bytes(data, fmt, ch, rate, extensible=i == 3, before=[(b'LIST', b'xyz')] if i == 0 else ()))
        n = min(frames, int(3 * rate))
        out.append((str(d / name), (data[:n * ch * rr.BYTES[fmt]], fmt, ch, rate, n)))
    return out


def _probs(results):
    return np.array([r['all_probabilities'] for r in results])


def test_predict_files(files, loader, dev):
    from inference.speech_inference import SpeechInference
    si = SpeechInference(seed=11, device=dev, load='gpu')
    res = si.predict_files([p for p, _ in files])
    assert [set(r) for r in res] == [{'emotion', 'confidence', 'all_probabilities'}] * len(files)
    # the kernel-level call's waveform through predict_waveforms, bit for bit
    wave = loader.load([c for _, c in files])
    ref = si.predict_waveforms(wave)[2].cpu().numpy()
    assert np.array_equal(_probs(res), ref.astype(np.float64))
    # 22 050 Hz files: the numpy-loaded waveform, bit for bit
    at = [i for i, (_, c) in enumerate(files) if c[3] == 22050]
    host = np.stack([rr.fix(rr.decode(*files[i][1][:3], files[i][1][4])) for i in at])
    assert np.array_equal(wave.cpu().numpy()[at], host)
    ref22 = si.predict_waveforms(engine.to_device(host, dev))[2].cpu().numpy()
    assert np.array_equal(_probs(si.predict_files([files[i][0] for i in at])), ref22.astype(np.float64))
    # predict / extract_features take the same path, one file at a time
    one = si.predict(files[0][0])
    assert np.array_equal(np.array(one['all_probabilities']),
                          si.predict_waveforms(loader.load([files[0][1]]))[2].cpu().numpy()[0].astype(np.float64))
    assert si.predict_files([]) == []


def test_non_wav_goes_to_the_host_loader(files, dev, tmp_path, monkeypatch):
    """A path mec.wav declines is loaded by preprocessing.audio_preprocessing.load_audio, and only that one."""
    calls = []
    host_wave = (np.random.default_rng(3).uniform(-0.2, 0.2, N_OUT)).astype(np.float32)

    def load_audio(path):
        calls.append(path)
        return host_wave.copy(), 22050

    pkg, mod = types.ModuleType('preprocessing'), types.ModuleType('preprocessing.audio_preprocessing')
    mod.load_audio = load_audio
    pkg.audio_preprocessing = mod
    monkeypatch.setitem(sys.modules, 'preprocessing', pkg)
    monkeypatch.setitem(sys.modules, 'preprocessing.audio_preprocessing', mod)
    other = tmp_path / 'speech.flac'
    other.write_bytes(b'fLaC' + bytes(100))
    from inference.speech_inference import SpeechInference
    si = SpeechInference(seed=11, device=dev, load='gpu')
    paths = [files[0][0], str(other), files[1][0]]
    res = si.predict_files(paths)
    assert calls == [str(other)]
    ref = si.predict_waveforms(engine.to_device(host_wave.reshape(1, -1), dev))[2].cpu().numpy()[0]
    assert np.array_equal(np.array(res[1]['all_probabilities']), ref.astype(np.float64))
    alone = si.predict_files([files[0][0], files[1][0]])
    assert np.array_equal(_probs([res[0], res[2]]), _probs(alone))


def test_multimodal_batch_equals_per_request(files, dev, tmp_path, monkeypatch):
    """audio_load='gpu': predict_multimodal_batch against predict_multimodal on the same files, for every
    pattern of modalities that has audio (audio, audio + text, audio + image, all three, the last twice) among
    requests without it, with the attention model and without one (the average route).

    The speech rows are bitwise equal: the waveform of a file does not depend on its batch (the kernel's
    contract), and the feature kernels and the speech DNN compute each row on its own. The text and image
    encoders and the fusion run GEMMs whose tile, and so summation order, follows the batch size, which is why
    the existing mixed-batch tests hold them to a tolerance; here 1e-6 on fp32 probabilities (a few float32
    roundings of values below 1) and equal labels."""
    from PIL import Image
    from inference.multimodal_fusion import MultimodalFusion
    from mec import synthetic as syn
    from test_gpu_dropin import TEXTS, _legacy_tokenizer, _write_vocab
    mf = MultimodalFusion(seed=1234, device=dev, precision='fp32', audio_load='gpu')
    assert mf.speech_inference.load == 'gpu' and mf.fusion_model is not None
    mf.text_inference.tokenizer = _legacy_tokenizer(_write_vocab(tmp_path))
    faces = syn.image_inputs(2, seed=52)
    png = []
    for k in range(2):
        png.append(str(tmp_path / f'face{k}.png'))
        Image.fromarray(faces[k], 'L').save(png[k])
    wavs = [p for p, _ in files]
    reqs = [(wavs[0], TEXTS[0], png[0]), (wavs[1], None, png[1]), (None, TEXTS[1], png[0]), (wavs[2], TEXTS[1], None),
            (wavs[3], None, None), (None, None, png[1]), (wavs[2], TEXTS[0], png[1]), (None, None, None)]
    keys = [['speech', 'text', 'image', 'fusion'], ['speech', 'image', 'fusion'], ['text', 'image', 'fusion'],
            ['speech', 'text', 'fusion'], ['speech'], ['image'], ['speech', 'text', 'image', 'fusion'], []]

    def compare():
        batch = mf.predict_multimodal_batch(reqs)
        assert [list(b) for b in batch] == keys
        for n, (r, b) in enumerate(zip(reqs, batch)):
            one = mf.predict_multimodal(audio_path=r[0], text=r[1], image_path=r[2])
            assert list(one) == list(b), f'request {n}'
            for k in one:
                assert list(one[k]) == list(b[k]), f'request {n} {k}'
                d = np.abs(np.array(one[k]['all_probabilities']) - np.array(b[k]['all_probabilities'])).max()
                assert d <= 1e-6, f'request {n} {k}: {d}'
                assert one[k]['emotion'] == b[k]['emotion'], f'request {n} {k}'
            if 'speech' in one:
                assert one['speech'] == b['speech'], f'request {n}: speech rows differ'
        return batch

    with_model = compare()
    assert 'attention_weights' in with_model[0]['fusion'] and 'attention_weights' not in with_model[1]['fusion']
    monkeypatch.setattr(mf, 'fusion_model', None)
    without = compare()
    assert 'attention_weights' not in without[0]['fusion']
    # an unreadable audio file names its request, before any GPU work
    with pytest.raises(ValueError, match='request 1'):
        mf.predict_multimodal_batch([reqs[0], (str(tmp_path / 'missing.wav'), None, png[0])])
