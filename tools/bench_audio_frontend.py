"""Measure the audio front end (csrc/audio_load.hip, load='gpu'): 256 in-memory 3-s stereo S16 WAV files at
48 000 Hz and at 24 414 Hz, taken to speech probabilities. Writes profiles/audio_frontend_bench.json.

Per rate: the kernel's time (mec_audio_load_prof_read), end-to-end files/s of the GPU path (header parse,
packing, upload, kernel, features, model, probabilities on the host), and for comparison files/s of a host
restatement of the same arithmetic: numpy decode and mono mean, scipy.signal.resample_poly with the library's
taps, then the same features and model on the GPU. That host figure is the restatement, NOT librosa / soxr,
which are not installed where this runs. Recorded, not judged: there is no threshold.

    python tools/bench_audio_frontend.py [--files 256] [--reps 5] [--host-files 32]
"""
import argparse
import ctypes
import io
import json
import os
import statistics
import struct
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'multimodal-emotion-classification_amd'))

import torch  # noqa: E402
from scipy.signal import resample_poly  # noqa: E402

from inference.speech_inference import SpeechInference  # noqa: E402
from mec import _lib, engine, wav  # noqa: E402

N_OUT = 66150


def plan_and_taps(rate, rate_out=22050):
    """(up, down, half, taps) from the library (mec_resample_plan, mec_resample_taps)."""
    lib = _lib.load()
    up, down, half = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    _lib.check(lib.mec_resample_plan(rate, rate_out, ctypes.byref(up), ctypes.byref(down), ctypes.byref(half)),
               'mec_resample_plan')
    h = np.zeros(2 * half.value + 1, np.float64)
    _lib.check(lib.mec_resample_taps(rate, rate_out, h.ctypes.data, h.size), 'mec_resample_taps')
    return up.value, down.value, half.value, h


def wav_s16_stereo(x, rate):
    """x float [frames, 2] in [-1, 1] -> the bytes of a plain 16-bit stereo WAV file."""
    data = np.clip(np.round(x * 32768), -32768, 32767).astype('<i2').tobytes()
    fmt = struct.pack('<HHIIHH', 1, 2, rate, rate * 4, 4, 16)
    body = b'WAVE' + b'fmt ' + struct.pack('<I', len(fmt)) + fmt + b'data' + struct.pack('<I', len(data)) + data
    return b'RIFF' + struct.pack('<I', len(body)) + body


def host_load(data, rate, frames, up, down, taps):
    """The kernel's arithmetic on the host for a stereo S16 clip: numpy decode and float32 mono mean, float64
    resample_poly with the library's taps, librosa's length, pad / trim; one rounding to float32."""
    x = np.frombuffer(data, '<i2', frames * 2).astype(np.float32).reshape(frames, 2) / np.float32(32768)
    y = resample_poly(np.mean(x, axis=1, dtype=np.float32).astype(np.float64), up, down, window=taps)
    n = min(int(np.ceil(frames * (float(22050) / rate))), N_OUT)
    out = np.zeros(N_OUT, np.float32)
    out[:n] = y[:n]
    return out


def make_files(rate, count, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(3 * rate) / rate
    out = []
    for _ in range(count):
        f0 = rng.uniform(80, 400)
        x = 0.4 * np.sin(2 * np.pi * f0 * t)[:, None] + 0.1 * rng.standard_normal((t.size, 2))
        out.append(wav_s16_stereo(np.clip(x, -1, 1), rate))
    return out


def clip_of(b):
    fmt, ch, rate, frames, off = wav.probe(io.BytesIO(b))
    frames = min(frames, int(3.0 * rate))
    return memoryview(b)[off:off + frames * ch * wav.BYTES[fmt]], fmt, ch, rate, frames


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--files', type=int, default=256)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--host-files', type=int, default=32, help='files of the host restatement (it is slow)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'audio_frontend_bench.json'))
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    si = SpeechInference(seed=1234, device=dev, load='gpu')
    loader = si._audio_loader()
    result = {'arch': torch.cuda.get_device_properties(0).gcnArchName,
              'device_name_reported': torch.cuda.get_device_name(0),
              'device_note': 'gfx950 is the AMD Instinct MI355X (CDNA4); the runtime may report a generic name', 'files': a.files, 'reps': a.reps, 'seconds_per_file': 3,
              'format': 'stereo S16 WAV, in memory',
              'host_note': 'host_files_per_s is the numpy decode + scipy.signal.resample_poly restatement with the '
                           "library's taps (float64), followed by the same GPU features and model; it is NOT "
                           'librosa / soxr_hq, which are not installed here',
              'rates': {}}
    for rate in (48000, 24414):
        files = make_files(rate, a.files, seed=rate)

        def gpu_path():
            wave = loader.load([clip_of(b) for b in files])
            return si.predict_waveforms(wave)[2].cpu().numpy()

        gpu_path()  # builds the rate's tap table, settles the allocator
        gpu_path()
        engine.audio_load_prof(True)
        times = []
        for _ in range(a.reps):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            probs = gpu_path()
            times.append(time.perf_counter() - t0)
        ms, calls = engine.audio_load_prof_read()
        engine.audio_load_prof(False)
        up, down, half, taps = plan_and_taps(rate)
        host_files = files[:a.host_files]

        def host_path():
            waves = []
            for b in host_files:
                data, _, _, _, frames = clip_of(b)
                waves.append(host_load(data, rate, frames, up, down, taps))
            return si.predict_waveforms(engine.to_device(np.stack(waves), dev))[2].cpu().numpy()

        host_path()
        htimes = []
        for _ in range(max(1, a.reps // 2)):
            t0 = time.perf_counter()
            hprobs = host_path()
            htimes.append(time.perf_counter() - t0)
        result['rates'][str(rate)] = {
            'plan': f'{up}/{down}', 'taps': 2 * half + 1,
            'kernel_ms_per_call': ms / calls, 'kernel_calls': calls,
            'gpu_end_to_end_s': statistics.median(times), 'gpu_files_per_s': a.files / statistics.median(times),
            'gpu_end_to_end_s_all': times,
            'host_files': len(host_files), 'host_end_to_end_s': statistics.median(htimes),
            'host_files_per_s': len(host_files) / statistics.median(htimes),
            'probs_max_abs_diff_gpu_vs_host': float(np.abs(probs[:len(host_files)] - hprobs).max()),
        }
        print(rate, json.dumps(result['rates'][str(rate)]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(result, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
