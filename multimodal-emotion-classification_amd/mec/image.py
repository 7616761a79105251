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


PAL_BYTES = 768  # a PIX_P image's palette: 256 RGB entries, zero-padded
# the model-input shapes (engine.ImageEncoder.forward_u8), in the order engine.ingest_ragged returns its batches
MODEL_SHAPES = ((48, 48, 1), (OUT, OUT, 1), (OUT, OUT, 3))


def pad16(n) -> int:
    return (int(n) + 15) // 16 * 16


def pack_layout(sizes, blobs=()):
    """Where a ragged batch lies in its one staging buffer: images of `sizes` bytes, then `blobs` (bytes objects:
    the palettes) -> (offs int64 [B], {blob: offset}, end). Every image starts on a 16-byte boundary; the
    distinct blobs follow the last image's padded end back to back, unpadded, each stored once. `end` is the end
    of the last thing stored, not padded: engine.resize_ragged's total as it is, engine.ingest_ragged's src_total
    once padded (the converted images follow it)."""
    offs, at, end = [], 0, 0
    for n in sizes:
        offs.append(at)
        end = at + int(n)
        at = pad16(end)
    stored = {}
    for b in blobs:
        if b not in stored:
            stored[b] = at
            end = at = at + len(b)
    return np.asarray(offs, np.int64), stored, end


def check_image(i, a, C=None, fmt=None, pal=None):
    """Image i of a ragged batch -> its u8 array [H,W,C] ([H,W] becomes [H,W,1]). With `fmt` (a PIX_*; ValueError
    for another value) the array must hold that format's bytes per pixel and `pal` must be given for PIX_P and for
    no other; without it the array must have C channels where C is given. TypeError for another dtype, rank or
    bytes per pixel; ValueError for another channel count and outside resize_on_gpu's domain."""
    a = np.asarray(a)
    if a.ndim == 2:
        a = a[..., None]
    if fmt is None:
        if a.dtype != np.uint8 or a.ndim != 3:
            raise TypeError(f'image {i}: expected a u8 array [H,W,C], got {a.dtype} {a.shape}')
        if C is not None and a.shape[2] != C:
            raise ValueError(f'image {i}: {a.shape[2]} channels in a batch of C = {C}')
    else:
        if not isinstance(fmt, (int, np.integer)) or not 0 <= fmt < len(PIX_BPP):
            raise ValueError(f'image {i}: unknown fmt {fmt!r}')
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != PIX_BPP[fmt]:
            raise TypeError(f'image {i}: expected a u8 array [H,W,{PIX_BPP[fmt]}] for fmt {fmt}, got {a.dtype} {a.shape}')
    if not resize_on_gpu(a.shape[0], a.shape[1]):
        raise ValueError(f'image {i}: {a.shape[0]} x {a.shape[1]} is outside the GPU resize\'s domain')
    if fmt is not None and (fmt == PIX_P) != (pal is not None):
        raise ValueError(f'image {i}: a palette goes with fmt PIX_P and with no other')
    return a


def canon_room(fmt, H, W) -> int:
    """The most an image's converted copy can take behind the sources: an L image is read as it is unless it is a
    face (gathered); RGB and LA shrink to one channel at most; RGBA and P may become RGB."""
    if fmt == PIX_L and (H, W) != (48, 48):
        return 0
    return pad16(H * W * (3 if fmt in (PIX_RGBA, PIX_P) else 1))


def canon_plan(gray, hw, fmts, offs, src_total):
    """engine.ingest_ragged's host step between the gray flags and the conversion: what each image's consumer
    reads, and where -> (face, chan, c_out, dst_offs, read_at). face: gray and 48 x 48 (gathered into one
    contiguous batch); chan: 1 for a gray image, 3 for any other; c_out: chan where the image is converted, 0
    where its native bytes are what its consumer reads (gray L, coloured RGB, no face); dst_offs: the converted
    copies' offsets behind src_total, the faces first and contiguous, each on a 16-byte boundary; read_at: where
    the resize reads each image, its source or its converted copy."""
    face = gray & (hw[:, 0] == 48) & (hw[:, 1] == 48)
    chan = np.where(gray, 1, 3).astype(np.int32)
    asis = ~face & (((fmts == PIX_L) & gray) | ((fmts == PIX_RGB) & ~gray))
    c_out = np.where(asis, 0, chan).astype(np.int32)
    npix = hw[:, 0].astype(np.int64) * hw[:, 1]
    dst_offs, read_at, at = np.zeros(len(gray), np.int64), np.array(offs, np.int64), 0
    for i in list(np.flatnonzero(face)) + list(np.flatnonzero(~face & ~asis)):
        dst_offs[i], read_at[i] = at, src_total + at
        at += pad16(npix[i] * c_out[i])
    return face, chan, c_out, dst_offs, read_at


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
