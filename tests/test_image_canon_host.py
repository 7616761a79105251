"""CPU: the GPU image ingest's host side (csrc/image_canon.hip). The numpy restatement
(tests/canon_ref.py) against the installed Pillow's convert('RGB'); the predicate that routes an image to the GPU
ingest or to the host; and the descriptor checks of the two entry points, which all precede the first device
call and so run without a GPU."""
import numpy as np
import pytest

import canon_ref as cr
from mec import _lib, image as mimage

SHAPES = [(1, 1), (1, 7), (7, 1), (5, 3), (48, 48), (33, 65)]


def _palette(n, salt=0):
    """n RGB entries, the odd ones gray."""
    e = np.arange(n)
    pal = np.stack([(e * 7 + salt) % 256, (e * 13 + 5) % 256, (e * 29 + 11) % 256], 1).astype(np.uint8)
    pal[1::2, 1:] = pal[1::2, :1]
    return pal


def _pil_cases(H, W):
    """[(name, PIL image)] over the covered modes and palette kinds."""
    from PIL import Image
    out = [('L', Image.fromarray(cr.formula(H, W, 1)[..., 0], 'L')),
           ('LA', Image.fromarray(cr.formula(H, W, 2), 'LA')),
           ('RGB', Image.fromarray(cr.formula(H, W, 3), 'RGB')),
           ('RGBA', Image.fromarray(cr.formula(H, W, 4), 'RGBA'))]
    full = Image.fromarray(cr.formula(H, W, 1, 3)[..., 0], 'P')
    full.putpalette(_palette(256).reshape(-1).tolist())
    out.append(('P full', full))
    short = Image.fromarray(cr.formula(H, W, 1, 5)[..., 0], 'P')  # indices up to 255, ten entries: the rest are 0
    short.putpalette(_palette(10, 9).reshape(-1).tolist())
    out.append(('P 10 entries', short))
    rgba = Image.fromarray(cr.formula(H, W, 1, 7)[..., 0], 'P')
    rgba.putpalette(np.concatenate([_palette(256, 4), cr.formula(256, 1, 1)[:, 0]], 1).reshape(-1).tolist(), 'RGBA')
    out.append(('P RGBA palette', rgba))
    tr = Image.fromarray(cr.formula(H, W, 1, 9)[..., 0], 'P')
    tr.putpalette(_palette(256, 2).reshape(-1).tolist())
    tr.info['transparency'] = 3
    out.append(('P transparency', tr))
    return out


@pytest.mark.parametrize('shape', SHAPES)
def test_restatement_equals_live_pillow(shape):
    pytest.importorskip('PIL.Image')
    for name, im in _pil_cases(*shape):
        native = mimage.native_pixels(im)
        assert native is not None, name
        a, fmt, pal = native
        assert fmt == cr.MODES[im.mode] and (pal is not None) == (im.mode == 'P'), name
        ref = np.asarray(im.convert('RGB'))
        rgb, gray = cr.canon(fmt, a, pal)
        assert rgb.shape == shape + (3,) and np.array_equal(rgb, ref), name
        assert gray == bool((ref[..., 0] == ref[..., 1]).all() and (ref[..., 0] == ref[..., 2]).all()), name


def test_restatement_gray_flag():
    g = cr.formula(5, 3, 1)
    assert cr.canon(cr.L, g)[1] and cr.canon(cr.LA, cr.formula(5, 3, 2))[1]
    assert cr.canon(cr.RGB, np.repeat(g, 3, 2))[1] and not cr.canon(cr.RGB, cr.formula(5, 3, 3))[1]
    rgba = np.concatenate([np.repeat(g, 3, 2), cr.formula(5, 3, 1, 4)], 2)
    assert cr.canon(cr.RGBA, rgba)[1]
    pal = cr.pad_palette(_palette(256))
    assert cr.canon(cr.P, np.full((5, 3), 1, np.uint8), pal)[1]  # an odd entry: gray
    assert not cr.canon(cr.P, np.full((5, 3), 2, np.uint8), pal)[1]


def test_routing_predicate():
    Image = pytest.importorskip('PIL.Image')
    for name, im in _pil_cases(5, 3):  # the five covered modes go native
        assert mimage.native_pixels(im) is not None, name
    host = [Image.new('1', (8, 8)), Image.new('CMYK', (8, 8)), Image.new('I;16', (8, 8)), Image.new('F', (8, 8)),
            Image.new('YCbCr', (8, 8)), Image.new('PA', (8, 8)), Image.new('RGBX', (8, 8)), Image.new('I', (8, 8)),
            Image.new('HSV', (8, 8)), Image.new('LAB', (8, 8)),
            Image.fromarray(cr.formula(301, 3, 3), 'RGB'), Image.fromarray(cr.formula(301, 3, 1)[..., 0], 'L')]
    for im in host:
        assert mimage.native_pixels(im) is None, (im.mode, im.size)
    bare = Image.frombytes('P', (4, 4), bytes(16))  # mode P, no palette attached
    if not bare.getpalette('RGB'):
        assert mimage.native_pixels(bare) is None
    a, fmt, pal = mimage.native_pixels(Image.fromarray(cr.formula(300, 3, 3), 'RGB'))  # the last in-domain strip
    assert fmt == mimage.PIX_RGB and a.shape == (300, 3, 3) and pal is None


def test_constants_mirror_the_restatement():
    assert (mimage.PIX_L, mimage.PIX_LA, mimage.PIX_RGB, mimage.PIX_RGBA, mimage.PIX_P) == (cr.L, cr.LA, cr.RGB, cr.RGBA, cr.P)
    assert mimage.PIX_MODES == cr.MODES and list(mimage.PIX_BPP) == [cr.BPP[f] for f in range(5)]


# ---- the entry points' descriptor checks. A batch of an RGBA 10 x 20 (800 B at 0), a P 10 x 20 (200 B at 800) and
# an L 10 x 20 (200 B at 1008), one palette at 1216; src_bytes 1984. The canon call writes RGB 600 B at dst + 0, RGB
# 600 B at dst + 608, nothing for the L image; dst_bytes 1216.
GOOD = dict(offs=[0, 800, 1008], hw=[[10, 20]] * 3, fmt=[cr.RGBA, cr.P, cr.L], pal_off=[-1, 1216, -1], B=3,
            src_bytes=1984, c_out=[3, 3, 0], dst_offs=[0, 608, 0], dst_bytes=1216, src=0x10000, dst=0x20000, gray=0x30000)
PTRS = ('src', 'offs', 'hw', 'fmt', 'pal_off', 'c_out', 'dst_offs', 'dst', 'gray')


def _call(lib, which, null=(), **kw):
    a = {**GOOD, **kw}
    keep = {'offs': np.asarray(a['offs'], np.int64), 'hw': np.asarray(a['hw'], np.int32), 'fmt': np.asarray(a['fmt'], np.int32),
            'pal_off': np.asarray(a['pal_off'], np.int64), 'c_out': np.asarray(a['c_out'], np.int32),
            'dst_offs': np.asarray(a['dst_offs'], np.int64)}
    p = {k: (None if k in null else keep[k].ctypes.data if k in keep else a[k]) for k in PTRS}
    if which == 'gray':
        return lib.mec_image_gray_ragged_u8(p['src'], p['offs'], p['hw'], p['fmt'], p['pal_off'], a['B'], a['src_bytes'],
                                            p['gray'], None)
    return lib.mec_image_canon_ragged_u8(p['src'], p['offs'], p['hw'], p['fmt'], p['pal_off'], p['c_out'], p['dst_offs'],
                                         a['B'], a['src_bytes'], p['dst'], a['dst_bytes'], None)


BOTH = {  # name -> (kwargs, a fragment of the message): what both calls reject
    'B < 0': (dict(B=-1), b'B < 0'),
    'null src': (dict(null=('src',)), b'null'),
    'null offs': (dict(null=('offs',)), b'null'),
    'null hw': (dict(null=('hw',)), b'null'),
    'null fmt': (dict(null=('fmt',)), b'null'),
    'null pal_off': (dict(null=('pal_off',)), b'null'),
    'fmt 5': (dict(fmt=[cr.RGBA, 5, cr.L]), b'image 1 has the unknown fmt 5'),
    'fmt -1': (dict(fmt=[-1, cr.P, cr.L]), b'image 0 has the unknown fmt'),
    'image past src_bytes': (dict(offs=[0, 800, 1785]), b'image 2 does not lie inside src_bytes'),
    'negative offset': (dict(offs=[-1, 800, 1008]), b'image 0 does not lie inside src_bytes'),
    'offset past src_bytes': (dict(offs=[0, 1 << 50, 1008]), b'image 1 does not lie inside src_bytes'),
    'palette past src_bytes': (dict(pal_off=[-1, 1217, -1]), b'image 1 has a palette that does not lie inside'),
    'P without a palette': (dict(pal_off=[-1, -1, -1]), b'image 1 is MEC_PIX_P and has no palette'),
    'palette on RGBA': (dict(pal_off=[1216, 1216, -1]), b'image 0 is not MEC_PIX_P and names a palette'),
    'pal_off -2 on L': (dict(pal_off=[-1, 1216, -2]), b'image 2 is not MEC_PIX_P'),
    'H = 0': (dict(hw=[[10, 20], [0, 20], [10, 20]]), b'image 1 is 0 x 20, outside'),
    'W = 4097': (dict(hw=[[10, 20], [10, 20], [1, 4097]], src_bytes=1 << 40), b'image 2 is 1 x 4097, outside'),
    'H > 100 W': (dict(hw=[[301, 3], [10, 20], [10, 20]], src_bytes=1 << 40), b'image 0 is 301 x 3, outside'),
}
CANON = {  # what the canon call alone rejects
    'null c_out': (dict(null=('c_out',)), b'null'),
    'null dst_offs': (dict(null=('dst_offs',)), b'null'),
    'null dst': (dict(null=('dst',)), b'null'),
    'misaligned dst': (dict(dst=0x20004), b'dst must be 16-byte aligned'),
    'c_out 2': (dict(c_out=[3, 2, 0]), b'image 1 has c_out 2'),
    'c_out 4': (dict(c_out=[4, 3, 0]), b'image 0 has c_out 4'),
    'c_out -1': (dict(c_out=[3, 3, -1]), b'image 2 has c_out -1'),
    'dst_off 8': (dict(dst_offs=[8, 608, 0]), b'image 0 has a dst_off that is negative or not a multiple of 16'),
    'negative dst_off': (dict(dst_offs=[0, -16, 0]), b'image 1 has a dst_off'),
    'output past dst_bytes': (dict(dst_bytes=1207), b'image 1 has an output that does not lie inside dst_bytes'),
    'dst_off past dst_bytes': (dict(dst_offs=[0, 1 << 50, 0]), b'image 1 has an output that does not lie inside'),
    'two outputs overlap': (dict(dst_offs=[0, 592, 0]), b'overlaps'),
    'output on its own input': (dict(dst=0x10000), b'overlaps'),
    'output on another input': (dict(dst=0x10000, dst_offs=[1008, 0, 0], dst_bytes=4096, c_out=[3, 0, 0]), b'overlaps'),
    'output on the palette': (dict(dst=0x10000, dst_offs=[1216, 0, 0], dst_bytes=4096, c_out=[1, 0, 0]), b'overlaps'),
    'output on an image with c_out 0': (dict(dst=0x10000, dst_offs=[0, 0, 0], dst_bytes=4096, c_out=[0, 0, 1]), b'overlaps'),
}


@pytest.mark.parametrize('which', ['gray', 'canon'])
@pytest.mark.parametrize('case', list(BOTH))
def test_both_entries_reject_invalid_sources_without_gpu(which, case):
    """Every check precedes the first device call: the fake device pointers are never touched."""
    lib = _lib.load()
    kw, msg = BOTH[case]
    assert _call(lib, which, **kw) == -1
    err = lib.mec_last_error()
    assert msg in err and (b'mec_image_gray_ragged_u8' if which == 'gray' else b'mec_image_canon_ragged_u8') in err, err


@pytest.mark.parametrize('case', list(CANON))
def test_canon_entry_rejects_invalid_outputs_without_gpu(case):
    lib = _lib.load()
    kw, msg = CANON[case]
    assert _call(lib, 'canon', **kw) == -1
    assert msg in lib.mec_last_error(), lib.mec_last_error()


def test_gray_entry_null_flags_and_large_batches_without_gpu():
    lib = _lib.load()
    assert _call(lib, 'gray', null=('gray',)) == -1 and b'null' in lib.mec_last_error()
    n = 65536
    big = dict(offs=[0] * n, hw=[[1, 1]] * n, fmt=[cr.L] * n, pal_off=[-1] * n, B=n, c_out=[0] * n, dst_offs=[0] * n)
    for which in ('gray', 'canon'):
        assert _call(lib, which, **big) == -1 and b'at most 65535' in lib.mec_last_error(), which


def test_in_place_destination_is_accepted_up_to_the_launch():
    """dst inside the source allocation, behind the palette: no descriptor check objects, so the call goes on to
    the device. With every c_out 0 nothing is launched and it returns 0 without a GPU."""
    lib = _lib.load()
    assert _call(lib, 'canon', dst=0x10000 + 1984, c_out=[0, 0, 0]) == 0
    assert _call(lib, 'canon', dst=0x10000, dst_offs=[0, 0, 0], c_out=[0, 0, 0]) == 0  # unused dst_offs are not checked


def test_empty_batch_without_gpu():
    lib = _lib.load()
    assert lib.mec_image_gray_ragged_u8(None, None, None, None, None, 0, 0, None, None) == 0
    assert lib.mec_image_canon_ragged_u8(None, None, None, None, None, None, None, 0, 0, None, 0, None) == 0
    assert lib.mec_image_gray_ragged_u8(None, None, None, None, None, -1, 0, None, None) == -1


def test_convert_gpu_requires_resize_gpu():
    from inference.image_inference import ImageInference
    from inference.multimodal_fusion import MultimodalFusion
    with pytest.raises(ValueError, match="requires resize='gpu'"):
        ImageInference(convert='gpu', resize='host')
    with pytest.raises(ValueError, match="requires resize='gpu'"):
        ImageInference(convert='gpu')
    with pytest.raises(ValueError, match='convert must be'):
        ImageInference(convert='device', resize='gpu')
    with pytest.raises(ValueError, match="requires resize='gpu'"):
        MultimodalFusion(image_convert='gpu')
