"""The JPEG front end's host side: which files the GPU decodes (mec_jpeg_probe; csrc/jpeg_probe.h) and what it
needs of them.

Nothing here needs a GPU: the probe is a host function of libmec_hip.so. The domain is stated once, in
include/mec.h: baseline, 8-bit, one scan, gray or YCbCr 4:4:4 / 4:2:2 / 4:2:0, no Adobe segment, inside the GPU
resize's domain. Every other file is decoded by Pillow on the host.
"""
import ctypes

import numpy as np

from . import _lib
from .image import PIX_L, PIX_RGB

# include/mec.h MEC_JPEG_ST_*: why the kernels gave an image up (its file then goes to the host)
ST_OK, ST_BAD_CODE, ST_DC_CATEGORY, ST_AC_SIZE, ST_COEF_INDEX, ST_SEGMENT_END, ST_IDCT_RANGE, ST_COEF_RANGE = range(8)


class Blob:
    """A file the GPU decodes: its bytes, its descriptor (_lib.JpegDesc) and its restart segments (int64
    [nseg, 2]: offset in the file, length). `span` is the byte range of the file the kernels read."""

    def __init__(self, data, desc, segs):
        self.data, self.desc, self.segs = data, desc, segs
        self.H, self.W, self.C = int(desc.H), int(desc.W), int(desc.ncomp)
        self.fmt = PIX_L if self.C == 1 else PIX_RGB
        self.span = (int(segs[0, 0]), int(segs[-1, 0] + segs[-1, 1]))

    @property
    def out_bytes(self) -> int:
        return self.H * self.W * self.C

    def scan(self) -> np.ndarray:
        """The entropy-coded bytes (restart markers included), u8."""
        return np.frombuffer(self.data, np.uint8, self.span[1] - self.span[0], self.span[0])


def probe(data, seg_cap: int = 64):
    """bytes -> Blob for a file inside mec_jpeg_probe's domain, None for one the host decodes. Safe on any
    bytes."""
    data = bytes(data)
    lib = _lib.load()
    desc = _lib.JpegDesc()
    segs = np.zeros((max(int(seg_cap), 1), 2), np.int64)
    rc = lib.mec_jpeg_probe(data, len(data), ctypes.byref(desc), segs.ctypes.data, len(segs))
    if rc == 1 and desc.nseg > len(segs):
        segs = np.zeros((desc.nseg, 2), np.int64)
        rc = lib.mec_jpeg_probe(data, len(data), ctypes.byref(desc), segs.ctypes.data, len(segs))
    if rc < 0:
        _lib.check(rc, 'mec_jpeg_probe')
    if rc != 1:
        return None
    return Blob(data, desc, np.ascontiguousarray(segs[:desc.nseg]))


def desc_array(descs):
    """A list of _lib.JpegDesc -> the contiguous ctypes array mec_jpeg_decode_ragged takes."""
    arr = (_lib.JpegDesc * max(len(descs), 1))()
    for i, d in enumerate(descs):
        ctypes.memmove(ctypes.byref(arr, i * ctypes.sizeof(_lib.JpegDesc)), ctypes.byref(d), ctypes.sizeof(_lib.JpegDesc))
    return arr


def workspace_bytes(descs) -> int:
    """The device workspace a batch of descriptors needs (mec_jpeg_workspace_bytes)."""
    arr = desc_array(descs)
    n = _lib.load().mec_jpeg_workspace_bytes(ctypes.addressof(arr), len(descs))
    if n < 0:
        _lib.check(-1, 'mec_jpeg_workspace_bytes')
    return int(n)
