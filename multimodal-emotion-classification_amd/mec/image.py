"""The image front end's host side: which images the GPU resizes (csrc/resize.hip), and Pillow's taps.

Nothing here needs a GPU: the predicate and the tap builder are host functions of libmec_hip.so.
"""
import numpy as np

from . import _lib

OUT = 224  # IMAGE_SIZE: the one target the GPU resize has


def resize_on_gpu(H, W) -> bool:
    """True for an image the ragged GPU resize covers (include/mec.h: 1 <= H, W <= 4096 and H <= 100 W;
    for taller strips Pillow's bytes are not those of its documented pass order). Every
    other image is resized by PIL on the host. The domain is stated once, in the library."""
    H, W = int(H), int(W)
    if not (0 <= H < 2 ** 31 and 0 <= W < 2 ** 31):
        return False
    return bool(_lib.load().mec_resize_on_gpu(H, W))


def resize_taps(in_size: int, out_size: int = OUT, kmax: int | None = None):
    """Pillow's bilinear 8-bit taps for one extent (mec_resize_taps): (xmin int32 [out], n int32 [out],
    k int32 [out, kmax]); kmax defaults to the extent's ksize."""
    if kmax is None:
        kmax = 2 * int(np.ceil(max(in_size / out_size, 1.0))) + 1
    xmin, n = np.zeros(out_size, np.int32), np.zeros(out_size, np.int32)
    k = np.zeros((out_size, kmax), np.int32)
    _lib.check(_lib.load().mec_resize_taps(int(in_size), int(out_size), xmin.ctypes.data, n.ctypes.data,
                                           k.ctypes.data, int(kmax)), 'mec_resize_taps')
    return xmin, n, k
