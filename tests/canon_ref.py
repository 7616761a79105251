"""A numpy restatement of Pillow's convert('RGB') for the five modes the GPU ingest covers (csrc/image_canon.hip;
DESIGN.md 4.15), of the gray test of inference/image_inference.py::_route on the converted pixels, and the
packing the C entry points take. test_image_canon_host.py holds it equal to the installed Pillow."""
import numpy as np

L, LA, RGB, RGBA, P = range(5)  # include/mec.h MEC_PIX_*
BPP = {L: 1, LA: 2, RGB: 3, RGBA: 4, P: 1}
MODES = {'L': L, 'LA': LA, 'RGB': RGB, 'RGBA': RGBA, 'P': P}


def pad_palette(palette) -> np.ndarray:
    """getpalette('RGB') (a flat list of at most 768 values) -> u8 [768], zero-padded."""
    pal = np.zeros(768, np.uint8)
    flat = np.asarray(palette, np.uint8).reshape(-1)
    pal[:flat.size] = flat
    return pal


def canon(fmt, pixels, palette=None):
    """(fmt, u8 pixels [H,W] or [H,W,bpp], u8 palette [768] for P) -> (u8 RGB [H,W,3], gray flag)."""
    a = np.asarray(pixels, np.uint8)
    if a.ndim == 2:
        a = a[..., None]
    assert a.shape[2] == BPP[fmt], (fmt, a.shape)
    if fmt in (L, LA):
        rgb = np.repeat(a[..., :1], 3, axis=2)
    elif fmt in (RGB, RGBA):
        rgb = a[..., :3]
    else:
        rgb = np.asarray(palette, np.uint8).reshape(256, 3)[a[..., 0]]
    rgb = np.ascontiguousarray(rgb)
    gray = bool((rgb[..., 0] == rgb[..., 1]).all() and (rgb[..., 0] == rgb[..., 2]).all())
    return rgb, gray


def formula(H, W, C, salt=0):
    """A deterministic u8 [H,W,C] whose channels differ."""
    y, x, c = np.meshgrid(np.arange(H), np.arange(W), np.arange(C), indexing='ij')
    return ((y * 131 + x * 31 + c * 71 + salt * 17 + (y * x) % 7) % 256).astype(np.uint8)


def pack(items, start=1, pad=0, odd=False):
    """items: [(fmt, pixels, palette or None)] -> (blob u8, offs int64, hw int32 [B,2], fmt int32, pal_off int64).
    Images back to back from byte `start` on, `pad` bytes between them (`odd`: and each at an odd offset); the
    distinct palettes behind them."""
    offs, hw, fmts, chunks, at = [], [], [], [], start
    step = (lambda n: (n + pad) | 1) if odd else (lambda n: n + pad)
    for fmt, px, _ in items:
        px = np.asarray(px, np.uint8)
        offs.append(at)
        hw.append(px.shape[:2])
        fmts.append(fmt)
        chunks.append((at, px.reshape(-1)))
        at = step(at + px.size)
    pal_at, pal_off = {}, []
    for fmt, _, pal in items:
        if fmt != P:
            pal_off.append(-1)
            continue
        key = np.asarray(pal, np.uint8).tobytes()
        if key not in pal_at:
            pal_at[key] = at
            chunks.append((at, np.frombuffer(key, np.uint8)))
            at = step(at + 768)
        pal_off.append(pal_at[key])
    blob = np.zeros(at, np.uint8)
    for o, b in chunks:
        blob[o:o + b.size] = b
    return (blob, np.asarray(offs, np.int64), np.asarray(hw, np.int32).reshape(-1, 2), np.asarray(fmts, np.int32),
            np.asarray(pal_off, np.int64))
