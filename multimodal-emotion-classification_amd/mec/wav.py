"""RIFF/WAVE headers, read without the samples: what the GPU audio front end (csrc/audio_load.hip,
engine.AudioLoader) needs to know about a file before its bytes go up as they are.

probe(f) walks the chunks of a file object and returns (fmt, channels, rate, frames, data_offset) for
little-endian PCM the kernel decodes -- U8, S16, S24, S32 or float32, one or two channels, a rate inside
mec_resample_on_gpu -- and None for everything else (not RIFF, another codec, float64, more channels, a rate
outside the domain): the caller routes those files to the host loader. read_clip(path) adds the bytes of the
frames load_audio would read, min(frames, int(3 * rate)).
"""
import struct

from . import _lib

# include/mec.h MEC_PCM_*
PCM_U8, PCM_S16, PCM_S24, PCM_S32, PCM_F32 = 0, 1, 2, 3, 4
BYTES = {PCM_U8: 1, PCM_S16: 2, PCM_S24: 3, PCM_S32: 4, PCM_F32: 4}

_FORMAT_PCM, _FORMAT_FLOAT, _FORMAT_EXTENSIBLE = 0x0001, 0x0003, 0xFFFE
# the tail every KSDATAFORMAT_SUBTYPE GUID of a wave format tag shares: xxxxxxxx-0000-0010-8000-00aa00389b71
_GUID_TAIL = bytes.fromhex('000000001000800000aa00389b71')
_PCM_BITS = {8: PCM_U8, 16: PCM_S16, 24: PCM_S24, 32: PCM_S32}


def resample_on_gpu(rate: int, rate_out: int = 22050) -> bool:
    """mec_resample_on_gpu: whether the kernel resamples rate -> rate_out (host only, no GPU needed)."""
    return 1 <= rate < 2 ** 31 and bool(_lib.load().mec_resample_on_gpu(int(rate), int(rate_out)))


def _format(body: bytes):
    """(fmt, channels, rate, block_align) of a `fmt ` chunk's body, or None."""
    if len(body) < 16:
        return None
    tag, channels, rate, _, align, bits = struct.unpack('<HHIIHH', body[:16])
    if tag == _FORMAT_EXTENSIBLE:
        # cbSize, valid bits, channel mask, sub-format GUID; the container size is `bits`
        if len(body) < 40 or struct.unpack('<H', body[16:18])[0] < 22 or body[26:40] != _GUID_TAIL:
            return None
        tag = struct.unpack('<H', body[24:26])[0]
    if tag == _FORMAT_PCM:
        fmt = _PCM_BITS.get(bits)
    elif tag == _FORMAT_FLOAT:
        fmt = PCM_F32 if bits == 32 else None
    else:
        fmt = None
    if fmt is None or channels not in (1, 2) or align != channels * BYTES[fmt]:
        return None
    return fmt, channels, rate, align


def probe(f, rate_out: int = 22050):
    """f: a binary file object positioned at the start of a file. -> (fmt, channels, rate, frames,
    data_offset) or None. A chunk of odd size is followed by a pad byte; chunks before `data` (LIST, fact,
    ...) are skipped; a `data` size that runs past the end of the file is cut to whole frames."""
    head = f.read(12)
    if len(head) < 12 or head[:4] != b'RIFF' or head[8:12] != b'WAVE':
        return None
    f.seek(0, 2)
    end = f.tell()
    at, spec = 12, None
    while at + 8 <= end:
        f.seek(at)
        cid, size = struct.unpack('<4sI', f.read(8))
        body = at + 8
        if cid == b'fmt ':
            spec = _format(f.read(min(size, 40)))
            if spec is None:
                return None
        elif cid == b'data':
            if spec is None:
                return None
            fmt, channels, rate, align = spec
            if not resample_on_gpu(rate, rate_out):
                return None
            frames = min(size, end - body) // align
            return fmt, channels, rate, frames, body
        at = body + size + (size & 1)
    return None


def read_clip(path, rate_out: int = 22050, duration: float = 3.0):
    """-> (bytes, fmt, channels, rate, frames) of the frames load_audio reads from `path`,
    min(frames, int(duration * rate)) as soundfile counts them, or None where probe declines the file. A file
    that cannot be opened raises as open() does."""
    with open(path, 'rb') as f:
        got = probe(f, rate_out)
        if got is None:
            return None
        fmt, channels, rate, frames, off = got
        frames = min(frames, int(duration * rate))
        f.seek(off)
        data = f.read(frames * channels * BYTES[fmt])
    frames = len(data) // (channels * BYTES[fmt])
    return data[:frames * channels * BYTES[fmt]], fmt, channels, rate, frames
