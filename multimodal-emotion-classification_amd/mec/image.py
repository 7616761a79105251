"""The image front end's host side: which images the GPU resizes (csrc/resize.hip) and converts
(csrc/image_canon.hip), and Pillow's taps.

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


# include/mec.h MEC_PIX_*: the native pixel formats the GPU ingest converts (csrc/image_canon.hip), their bytes
# per pixel, and the Pillow modes they are
PIX_L, PIX_LA, PIX_RGB, PIX_RGBA, PIX_P = range(5)
PIX_BPP = (1, 2, 3, 4, 1)
PIX_MODES = {'L': PIX_L, 'LA': PIX_LA, 'RGB': PIX_RGB, 'RGBA': PIX_RGBA, 'P': PIX_P}


def native_pixels(image):
    """PIL image -> (u8 pixels as decoded, fmt, palette u8 [768] or None) when the GPU ingest covers it: mode
    L, LA, RGB or RGBA, or P with a palette whose getpalette('RGB') is not empty (zero-padded to 256 entries, as
    convert('RGB') looks indices up), and a size inside resize_on_gpu's domain. None for every other image
    (modes 1, I, I;16, F, CMYK, YCbCr, PA, RGBX, HSV, LAB, P without a palette, sizes outside the domain): those
    are converted on the host. Nothing is converted or compared here."""
    fmt = PIX_MODES.get(image.mode)
    W, H = image.size
    if fmt is None or not resize_on_gpu(H, W):
        return None
    pal = None
    if fmt == PIX_P:
        flat = image.getpalette('RGB')
        if not flat or len(flat) > 768:
            return None
        pal = np.zeros(768, np.uint8)
        pal[:len(flat)] = flat
    a = np.asarray(image)
    if a.dtype != np.uint8 or a.shape[:2] != (H, W):
        return None
    return a, fmt, pal


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
