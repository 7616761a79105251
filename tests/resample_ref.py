"""The audio front end restated in numpy / scipy (csrc/resample_design.h, csrc/audio_load.hip):
the filter design, the library's own taps through ctypes, PCM encoders for the test clips, and load_ref, the
float64 reference of mec_audio_load_ragged for one clip."""
import ctypes
import math
import struct

import numpy as np

from mec import _lib

RATE_OUT = 22050
N_OUT = 66150
ATTEN, PASS = 125.0, 0.913
U8, S16, S24, S32, F32 = range(5)
BYTES = {U8: 1, S16: 2, S24: 3, S32: 4, F32: 4}


def plan(rate_in, rate_out=RATE_OUT):
    """(up, down, half) of the design, or None outside the domain; half 0 is the identity plan."""
    if not (1 <= rate_in <= 192000):
        return None
    g = math.gcd(rate_in, rate_out)
    up, down = rate_out // g, rate_in // g
    M = max(up, down)
    if M > 8192:
        return None
    if M == 1:
        return 1, 1, 0
    half = math.ceil((ATTEN - 7.95) / (2.285 * (1 - PASS) * math.pi / M) / 2)
    if 2 * half + 1 > 2 ** 21:
        return None
    return up, down, half


def design(rate_in, rate_out=RATE_OUT):
    """The 2 * half + 1 taps, float64, unit sum (math.fsum: exact)."""
    up, down, half = plan(rate_in, rate_out)
    M = max(up, down)
    fc = (PASS + 1) / 2 / M
    beta = 0.1102 * (ATTEN - 8.7)
    n = np.arange(-half, half + 1, dtype=np.float64)
    h = fc * np.sinc(fc * n) * np.i0(beta * np.sqrt(np.maximum(0.0, 1 - (n / half) ** 2))) / np.i0(beta)
    return h / math.fsum(h)


def lib_plan(rate_in, rate_out=RATE_OUT):
    lib = _lib.load()
    up, down, half = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    rc = lib.mec_resample_plan(rate_in, rate_out, ctypes.byref(up), ctypes.byref(down), ctypes.byref(half))
    return None if rc else (up.value, down.value, half.value)


_TAPS = {}


def lib_taps(rate_in, rate_out=RATE_OUT):
    """The library's taps (mec_resample_taps), cached and read-only."""
    key = (rate_in, rate_out)
    if key not in _TAPS:
        _, _, half = lib_plan(rate_in, rate_out)
        h = np.zeros(2 * half + 1 if half else 0, np.float64)
        _lib.check(_lib.load().mec_resample_taps(rate_in, rate_out, h.ctypes.data, h.size), 'mec_resample_taps')
        h.setflags(write=False)
        _TAPS[key] = h
    return _TAPS[key]


def out_len(frames, rate_in, rate_out=RATE_OUT):
    """librosa 0.10.0 resample, literally."""
    return int(np.ceil(frames * (float(rate_out) / rate_in)))


def encode(x, fmt):
    """x: float64 [frames, ch] in [-1, 1) -> the little-endian interleaved PCM bytes of format fmt."""
    x = np.asarray(x, np.float64)
    if fmt == U8:
        return np.clip(np.round(x * 128) + 128, 0, 255).astype(np.uint8).tobytes()
    if fmt == S16:
        return np.clip(np.round(x * 2 ** 15), -2 ** 15, 2 ** 15 - 1).astype('<i2').tobytes()
    if fmt == S24:
        v = np.clip(np.round(x * 2 ** 23), -2 ** 23, 2 ** 23 - 1).astype('<i4')
        return v.view(np.uint8).reshape(-1, 4)[:, :3].tobytes()
    if fmt == S32:
        return np.clip(np.round(x * 2 ** 31), -2 ** 31, 2 ** 31 - 1).astype('<i4').tobytes()
    return x.astype('<f4').tobytes()


def decode(data, fmt, ch, frames):
    """libsndfile's normalisation to float32 and librosa's to_mono (np.mean over channels, float32)."""
    raw = np.frombuffer(data, np.uint8, frames * ch * BYTES[fmt])
    if fmt == U8:
        x = (raw.astype(np.float32) - np.float32(128)) / np.float32(128)
    elif fmt == S16:
        x = raw.view('<i2').astype(np.float32) / np.float32(2 ** 15)
    elif fmt == S24:
        b = raw.reshape(-1, 3).astype(np.int32)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        x = (v - ((v & 0x800000) << 1)).astype(np.float32) / np.float32(2 ** 23)
    elif fmt == S32:
        x = raw.view('<i4').astype(np.float32) * np.float32(2.0 ** -31)
    else:
        x = raw.view('<f4').astype(np.float32)
    x = x.reshape(frames, ch)
    return x[:, 0].copy() if ch == 1 else np.mean(x, axis=1, dtype=np.float32)


def fix(y, n=N_OUT):
    out = np.zeros(n, y.dtype)
    out[:min(n, y.size)] = y[:n]
    return out


def load_ref(data, fmt, ch, rate, frames, taps, rate_out=RATE_OUT, n_out=N_OUT):
    """-> (float64 [n_out] before the output rounding, the decoded mono float32 signal)."""
    from scipy.signal import resample_poly
    x = decode(data, fmt, ch, frames)
    up, down, half = plan(rate, rate_out)
    if half == 0:
        return fix(x.astype(np.float64), n_out), x
    n = out_len(frames, rate, rate_out)
    y = resample_poly(x.astype(np.float64), up, down, window=taps) if frames else np.zeros(0)
    return fix(fix(y, n), n_out), x


def bound_terms(taps, up):
    """(N, S): taps per output and the largest per-phase sum of |up * h|."""
    half = (taps.size - 1) // 2
    N = -(-taps.size // up)
    S = max(float(np.abs(up * taps[(half + p) % up::up]).sum()) for p in range(up))
    return N, S


def wav_bytes(data, fmt, ch, rate, extensible=False, before=(), data_size=None):
    """A RIFF/WAVE file: `before` = [(chunk id, body)] ahead of `data`; data_size overrides the data chunk's."""
    tag = 3 if fmt == F32 else 1
    bits = BYTES[fmt] * 8
    align = ch * BYTES[fmt]
    body = struct.pack('<HHIIHH', 0xFFFE if extensible else tag, ch, rate, rate * align, align, bits)
    if extensible:
        body += struct.pack('<HHIH', 22, bits, 3 if ch == 2 else 4, tag) + bytes.fromhex('000000001000800000aa00389b71')
    chunks = [(b'fmt ', body)] + list(before)
    out = b''
    for cid, b in chunks:
        out += cid + struct.pack('<I', len(b)) + b + (b'\0' if len(b) & 1 else b'')
    out += b'data' + struct.pack('<I', len(data) if data_size is None else data_size) + data
    if len(data) & 1 and data_size is None:
        out += b'\0'
    return b'RIFF' + struct.pack('<I', 4 + len(out)) + b'WAVE' + out
