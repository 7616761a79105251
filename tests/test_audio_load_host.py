"""Host (no GPU): the resampler's design (csrc/resample_design.h through mec_resample_*), the WAV header reader
(mec/wav.py) and the per-file routing of load='gpu' (DESIGN.md 4.19). The numpy restatement is
tests/resample_ref.py."""
import io

import numpy as np
import pytest

import resample_ref as rr
from mec import _lib, wav
from mec.engine import AudioLoader

RATES = (48000, 44100, 24414, 16000, 11025, 8000, 22050)


@pytest.mark.parametrize('rate', RATES)
def test_plan_matches_restatement(rate):
    assert rr.lib_plan(rate) == rr.plan(rate)
    assert _lib.load().mec_resample_on_gpu(rate, 22050) == 1


def test_issue_table():
    """The plans and tap counts the design was measured at."""
    for rate, up, down, taps in ((48000, 147, 320, 59977), (24414, 3675, 4069, 762615), (16000, 441, 320, 82655),
                                 (44100, 1, 2, 377)):
        u, d, half = rr.lib_plan(rate)
        assert (u, d, 2 * half + 1) == (up, down, taps)
    assert rr.lib_plan(22050) == (1, 1, 0)


@pytest.mark.parametrize('rate', (22051, 0, -1, 192001, 22049))
def test_off_domain(rate):
    lib = _lib.load()
    assert rr.plan(rate) is None if 1 <= rate <= 192000 else True
    assert lib.mec_resample_on_gpu(rate, 22050) == 0
    assert rr.lib_plan(rate) is None
    assert b'mec_resample_plan' in lib.mec_last_error()
    assert not wav.resample_on_gpu(rate)


def test_domain_edges():
    lib = _lib.load()
    assert lib.mec_resample_on_gpu(192000, 22050) == 1 and lib.mec_resample_on_gpu(1, 22050) == 0
    assert lib.mec_resample_on_gpu(22050, 0) == 0
    # taps: a wrong n or a null h is rejected
    h = np.zeros(377)
    assert lib.mec_resample_taps(44100, 22050, h.ctypes.data, 376) == -1
    assert lib.mec_resample_taps(44100, 22050, None, 377) == -1
    assert lib.mec_resample_taps(22050, 22050, None, 0) == 0


@pytest.mark.parametrize('rate', (48000, 44100, 24414, 16000, 11025, 8000))
def test_taps_match_restatement(rate):
    """Within 1e-9 of the centre tap: float noise with a careful sum is below 1e-10, a wrong beta or cutoff
    shows at 1e-4."""
    h, ref = rr.lib_taps(rate), rr.design(rate)
    assert h.shape == ref.shape
    centre = ref[ref.size // 2]
    assert np.abs(h - ref).max() <= 1e-9 * centre
    assert abs(float(np.sum(h.astype(np.longdouble))) - 1.0) <= 1e-12
    assert np.array_equal(h, h[::-1]) or np.abs(h - h[::-1]).max() <= 1e-18


@pytest.mark.parametrize('rate', (48000, 44100, 16000))
def test_response(rate):
    """The library's taps by a DTFT: passband (to 0.913 of the lower Nyquist) within 1e-6 of 1, stopband (from
    1.0 of it) at most -120 dB. The filter runs at rate_in * up; the lower Nyquist is 0.5 / M cycles there."""
    up, down, half = rr.lib_plan(rate)
    h = rr.lib_taps(rate)
    M = max(up, down)
    n = np.arange(-half, half + 1, dtype=np.float64)

    def mag(f):  # |H| at frequencies f (cycles per sample), in blocks to bound the memory
        out = np.empty(f.size)
        for i in range(0, f.size, 64):
            out[i:i + 64] = np.abs(np.cos(2 * np.pi * np.outer(f[i:i + 64], n)) @ h)  # h is symmetric
        return out

    nyq = 0.5 / M
    passband = mag(np.linspace(0, rr.PASS * nyq, 257))
    # the stopband's worst lobes are the first ones: a fine grid over them, a coarser one to 0.5
    lobe = 1.0 / h.size
    stop = np.concatenate([nyq + np.arange(0, 40 * lobe, lobe / 8), np.linspace(nyq + 40 * lobe, 0.5, 1500)])
    stopband = mag(stop[stop <= 0.5])
    print(f'rate {rate}: passband deviation {np.abs(passband - 1).max():.3g}, stopband '
          f'{20 * np.log10(stopband.max()):.2f} dB')
    assert np.abs(passband - 1).max() <= 1e-6
    assert 20 * np.log10(stopband.max()) <= -120.0


def test_reference_length():
    """int(np.ceil(frames * (float(22050) / rate))): frames that land on both sides of an integer."""
    assert rr.out_len(320, 48000) == 147 and rr.out_len(321, 48000) == 148 and rr.out_len(319, 48000) == 147
    assert rr.out_len(144000, 48000) == 66150 and rr.out_len(2, 44100) == 1 and rr.out_len(3, 44100) == 2
    assert rr.out_len(4069, 24414) in (3675, 3676) and rr.out_len(0, 8000) == 0
    assert rr.out_len(73242, 24414) == int(np.ceil(73242 * (22050.0 / 24414)))


# ---------------------------------------------------------------- mec/wav.py

def _probe(b):
    return wav.probe(io.BytesIO(b))


def _clip(fmt, ch, frames=10, seed=0):
    x = np.random.default_rng(seed).uniform(-0.9, 0.9, (frames, ch))
    return rr.encode(x, fmt)


@pytest.mark.parametrize('fmt', range(5))
@pytest.mark.parametrize('ch', (1, 2))
def test_wav_plain(fmt, ch):
    d = _clip(fmt, ch, 11)
    got = _probe(rr.wav_bytes(d, fmt, ch, 24414))
    assert got == (fmt, ch, 24414, 11, 44)


def test_wav_chunks_before_data_and_pad_bytes():
    d = _clip(rr.S16, 2, 7)
    b = rr.wav_bytes(d, rr.S16, 2, 48000, before=[(b'LIST', b'abc'), (b'fact', b'\1\0\0\0')])
    fmt, ch, rate, frames, off = _probe(b)
    assert (fmt, ch, rate, frames) == (rr.S16, 2, 48000, 7) and b[off:off + len(d)] == d
    assert off == 12 + 24 + (8 + 3 + 1) + (8 + 4) + 8


@pytest.mark.parametrize('fmt', (rr.S24, rr.F32, rr.U8))
def test_wav_extensible(fmt):
    d = _clip(fmt, 2, 5)
    b = rr.wav_bytes(d, fmt, 2, 44100, extensible=True)
    fmt_, ch, rate, frames, off = _probe(b)
    assert (fmt_, ch, rate, frames) == (fmt, 2, 44100, 5) and b[off:off + len(d)] == d


def test_wav_data_size_past_the_end():
    d = _clip(rr.S16, 2, 9) + b'\x01\x02\x03'  # 9 frames and a torn tenth
    b = rr.wav_bytes(d, rr.S16, 2, 16000, data_size=0xFFFFFFFF)
    assert _probe(b)[:4] == (rr.S16, 2, 16000, 9)


def test_wav_declines():
    d = _clip(rr.S16, 1, 4)
    good = rr.wav_bytes(d, rr.S16, 1, 22050)
    assert _probe(good) is not None
    assert _probe(b'') is None and _probe(b'OggS' + good[4:]) is None and _probe(good[:8] + b'AVI ' + good[12:]) is None
    codec = bytearray(good)
    codec[20:22] = (2).to_bytes(2, 'little')  # ADPCM
    assert _probe(bytes(codec)) is None
    f64 = bytearray(rr.wav_bytes(b'\0' * 32, rr.F32, 1, 22050))
    f64[32:36] = (8).to_bytes(2, 'little') + (64).to_bytes(2, 'little')  # block align 8, 64 bits
    assert _probe(bytes(f64)) is None
    three = bytearray(good)
    three[22:24] = (3).to_bytes(2, 'little')
    assert _probe(bytes(three)) is None
    assert _probe(rr.wav_bytes(d, rr.S16, 1, 22051)) is None  # a rate outside mec_resample_on_gpu
    assert _probe(good[:36]) is None  # no data chunk
    other_guid = bytearray(rr.wav_bytes(d, rr.S16, 1, 22050, extensible=True))
    other_guid[12 + 8 + 30] ^= 0xFF
    assert _probe(bytes(other_guid)) is None


def test_read_clip_reads_three_seconds(tmp_path):
    rate, frames = 8000, 3 * 8000 + 5000
    d = _clip(rr.U8, 2, frames)
    p = tmp_path / 'long.wav'
    p.write_bytes(rr.wav_bytes(d, rr.U8, 2, rate))
    data, fmt, ch, r, n = wav.read_clip(str(p))
    assert (fmt, ch, r, n) == (rr.U8, 2, rate, 3 * rate) and data == d[:3 * rate * 2]
    q = tmp_path / 'not.wav'
    q.write_bytes(b'ID3\x03' + bytes(64))
    assert wav.read_clip(str(q)) is None


# ---------------------------------------------------------------- routing

class _FakeLoader:
    """engine.AudioLoader without a GPU or a handle: read(), the routing, is the real one."""
    sample_rate, n_out = 22050, 66150
    read, read_one = AudioLoader.read, AudioLoader.read_one


def test_routing_per_file(tmp_path):
    """AudioLoader.read: WAV files the kernel takes are clips, everything else is declined, per file and in
    order; a missing file raises."""
    paths = []
    for name, b in (('a.wav', rr.wav_bytes(_clip(rr.S16, 2, 30), rr.S16, 2, 48000)), ('b.mp3', b'ID3' + bytes(50)),
                    ('c.wav', rr.wav_bytes(_clip(rr.F32, 1, 12), rr.F32, 1, 22050)),
                    ('d.wav', rr.wav_bytes(_clip(rr.S16, 1, 12), rr.S16, 1, 22051))):
        (tmp_path / name).write_bytes(b)
        paths.append(str(tmp_path / name))
    clips, at, declined = _FakeLoader().read(paths)
    assert at == [0, 2] and declined == [1, 3]
    assert [c[1:] for c in clips] == [(rr.S16, 2, 48000, 30), (rr.F32, 1, 22050, 12)]
    with pytest.raises(OSError):
        _FakeLoader().read([str(tmp_path / 'missing.wav')])


def test_load_argument():
    from inference.speech_inference import SpeechInference
    with pytest.raises(ValueError, match="load must be 'host' or 'gpu'"):
        SpeechInference(load='device')
    import inspect
    from inference.multimodal_fusion import MultimodalFusion
    assert inspect.signature(SpeechInference.__init__).parameters['load'].default == 'host'
    assert inspect.signature(MultimodalFusion.__init__).parameters['audio_load'].default == 'host'
