"""Test infrastructure: Pillow's 8-bit bilinear resize to 224 x 224, restated for any input size, and the
inputs of the ragged-resize tests.

`resize_hfirst` is oracle/resize.py's statement (horizontal pass into a u8 intermediate, then the vertical
pass, each clip8((2^21 + sum px * k) >> 22) on oracle.resize.coeffs' 22-bit taps) for any size and channel
count, with tap j of all 224 outputs applied in one numpy step.

Pillow 12.2's bytes equal this order for H <= 100 W; for H > 100 W with H > 224 they equal the vertical-first
order, which is not restated; tests/golden/image_resize_ragged.json pins the former."""
import hashlib

import numpy as np

from oracle.resize import PRECISION_BITS, coeffs

OUT = 224
PATTERNS = ('formula', 'white', 'checker')


def _pass(src_u8: np.ndarray, in_size: int) -> np.ndarray:
    """Resample the LAST axis (in_size long) of a u8 array to 224 with Pillow's taps: output xx sums its
    n[xx] samples from xmin[xx] on. Tap j of every output is applied at once; an output with fewer than j + 1
    taps takes tap 0 again with the coefficient 0 that coeffs leaves there (the index is never clamped)."""
    xmins, ns, kk = coeffs(in_size, OUT)
    src = src_u8.astype(np.int64)
    acc = np.full(src.shape[:-1] + (OUT,), 1 << (PRECISION_BITS - 1), np.int64)
    for j in range(kk.shape[1]):
        live = j < ns
        assert not kk[~live, j].any()
        acc += src[..., np.where(live, xmins + j, xmins)] * np.where(live, kk[:, j], 0).astype(np.int64)
    return np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)


def resize_hfirst(img: np.ndarray) -> np.ndarray:
    """u8 [H,W,C] -> u8 [224,224,C]: horizontal pass first, as ImagingResample orders them."""
    img = np.asarray(img, np.uint8)
    H, W, _ = img.shape
    tmp = _pass(np.ascontiguousarray(img.transpose(0, 2, 1)), W)   # [H,C,224]
    out = _pass(np.ascontiguousarray(tmp.transpose(2, 1, 0)), H)   # [224(x),C,224(y)]
    return np.ascontiguousarray(out.transpose(2, 0, 1))       # [224(y),224(x),C]


def make_input(H: int, W: int, pattern: str) -> np.ndarray:
    """u8 [H,W,3], a closed integer formula of (y, x, c): 'formula' a multiplicative hash (all byte values,
    no structure the filter could hide behind), 'white' all 255 (the upper clamp), 'checker' 0 / 255."""
    y, x, c = np.meshgrid(np.arange(H, dtype=np.uint64), np.arange(W, dtype=np.uint64),
                          np.arange(3, dtype=np.uint64), indexing='ij')
    if pattern == 'white':
        return np.full((H, W, 3), 255, np.uint8)
    if pattern == 'checker':
        return (((y + x + c) & np.uint64(1)) * np.uint64(255)).astype(np.uint8)
    assert pattern == 'formula'
    h = (y * np.uint64(73856093)) ^ (x * np.uint64(19349663)) ^ (c * np.uint64(83492791))
    return (((h * np.uint64(2654435761)) >> np.uint64(13)) & np.uint64(255)).astype(np.uint8)


def digest(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a, np.uint8).tobytes()).hexdigest()
