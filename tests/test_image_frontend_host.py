"""CPU: the ragged image front end's host bookkeeping, none of which needs a GPU: the staging
layout (mec.image.pack_layout), the array check (mec.image.check_image) and the per-shape batch plan of
ImageInference.forward_routed (inference.image_inference.plan_batches)."""
import numpy as np
import pytest

from mec import image as mimage

SIZES = [1, 15, 16, 17, 2304, 3 * 301 * 3]
PAL_A = bytes(range(256)) * 3
PAL_B = bytes(reversed(range(256))) * 3


def _restated_layout(sizes, blobs):
    """The rules, written out again: an image starts at the next multiple of 16 behind its predecessor's end; the
    distinct blobs follow the padded end of the images back to back."""
    offs, pos = [], 0
    for n in sizes:
        offs.append(pos)
        pos = -(-(pos + n) // 16) * 16
    end = offs[-1] + sizes[-1] if sizes else 0
    at = {}
    for b in blobs:
        if b not in at:
            at[b] = pos
            end = pos = pos + 768
    return offs, at, end


@pytest.mark.parametrize('blobs', [[], [PAL_A], [PAL_A, PAL_A], [PAL_A, PAL_B, PAL_A]], ids=['0', '1', '1 twice', '2'])
@pytest.mark.parametrize('order', [1, -1])
def test_pack_layout(order, blobs):
    sizes = SIZES[::order]
    offs, at, end = mimage.pack_layout(sizes, blobs)
    assert offs.dtype == np.int64 and offs.shape == (len(sizes),) and (offs % 16 == 0).all() and offs[0] == 0
    ranges = [(int(o), int(o) + n) for o, n in zip(offs, sizes)] + [(o, o + 768) for o in at.values()]
    assert all(a[1] <= b[0] for a, b in zip(ranges, ranges[1:])), 'ranges overlap or do not ascend'
    assert list(at) == list(dict.fromkeys(blobs)), 'a repeated palette is stored once, in order of first use'
    images_end = int(offs[-1]) + sizes[-1]
    if blobs:  # the palettes follow the images' padded end, unpadded
        assert list(at.values()) == [mimage.pad16(images_end) + 768 * k for k in range(len(at))]
        assert end == mimage.pad16(images_end) + 768 * len(at)
    else:  # resize_ragged's total: not padded; ingest_ragged's src_total pads it
        assert end == images_end
    assert mimage.pad16(end) % 16 == 0 and 0 <= mimage.pad16(end) - end < 16
    r_offs, r_at, r_end = _restated_layout(sizes, blobs)
    assert offs.tolist() == r_offs and at == r_at and end == r_end


def test_pack_layout_empty():
    offs, at, end = mimage.pack_layout([])
    assert offs.shape == (0,) and offs.dtype == np.int64 and at == {} and end == 0
    assert [mimage.pad16(n) for n in (0, 1, 15, 16, 17)] == [0, 16, 16, 16, 32]


def test_check_image_accepts():
    a = mimage.check_image(0, np.zeros((5, 7), np.uint8))
    assert a.shape == (5, 7, 1) and a.dtype == np.uint8
    assert mimage.check_image(1, np.zeros((5, 7, 3), np.uint8), 3).shape == (5, 7, 3)
    assert mimage.check_image(2, np.zeros((300, 3, 3), np.uint8), 3).shape == (300, 3, 3)
    assert mimage.check_image(3, np.zeros((5, 7), np.uint8), fmt=mimage.PIX_P, pal=np.zeros(768, np.uint8)).shape == (5, 7, 1)
    assert mimage.check_image(4, np.zeros((5, 7, 4), np.uint8), fmt=mimage.PIX_RGBA).shape == (5, 7, 4)


def test_check_image_rejections():
    u8 = lambda *s: np.zeros(s, np.uint8)  # noqa: E731
    with pytest.raises(TypeError, match='image 3: expected a u8 array'):  # wrong dtype
        mimage.check_image(3, np.zeros((5, 5, 3), np.float32))
    for fmt in (None, mimage.PIX_L):  # wrong rank
        with pytest.raises(TypeError, match='expected a u8 array'):
            mimage.check_image(0, u8(5), fmt=fmt)
        with pytest.raises(TypeError, match='expected a u8 array'):
            mimage.check_image(0, u8(2, 5, 5, 3), fmt=fmt)
    with pytest.raises(ValueError, match='image 1: 1 channels in a batch of C = 3'):  # mixed channel counts
        mimage.check_image(1, u8(5, 5, 1), 3)
    with pytest.raises(TypeError, match=r'expected a u8 array \[H,W,4\] for fmt 3'):  # bytes per pixel of the format
        mimage.check_image(0, u8(5, 5, 3), fmt=mimage.PIX_RGBA)
    with pytest.raises(ValueError, match='unknown fmt'):
        mimage.check_image(0, u8(5, 5, 3), fmt=5)
    for kw in ({}, {'C': 3}, {'fmt': mimage.PIX_RGB}):  # 301 x 3: outside the domain
        with pytest.raises(ValueError, match="image 2: 301 x 3 is outside the GPU resize's domain"):
            mimage.check_image(2, u8(301, 3, 3), **kw)
    with pytest.raises(ValueError, match='palette'):  # a palette on a non-P format
        mimage.check_image(0, u8(5, 5, 3), fmt=mimage.PIX_RGB, pal=u8(768))
    with pytest.raises(ValueError, match='palette'):  # a P format without one
        mimage.check_image(0, u8(5, 5), fmt=mimage.PIX_P)


F, G1, G3 = (48, 48, 1), (224, 224, 1), (224, 224, 3)
# tests/test_gpu_image_canon.py _pil_batch(): each image's model-input shape, and whether the device makes its row
# with resize='gpu' (a 48 x 48 gray face and the 301 x 3 strip are the host's) and with convert='gpu' as well (the
# strip alone is; the mode-1 and the CMYK image are converted on the host and resized on the device in both)
PIL_SHAPES = [G3, F, G3, G3, F, G3, G1, G1, F, G1, G3, G1, G1]
PIL_RESIZE = [s != F and k != 3 for k, s in enumerate(PIL_SHAPES)]
PIL_CONVERT = [k != 3 for k in range(13)]
# tests/test_gpu_resize_ragged.py _arrays()
ARR_SHAPES = [G3, F, G1, G3, G3, G1, G1, G3]
ARR_RESIZE = [s != F and k != 3 for k, s in enumerate(ARR_SHAPES)]
ARR_CONVERT = [k != 3 for k in range(8)]
PLANS = {'pil resize': (PIL_SHAPES, PIL_RESIZE), 'pil convert': (PIL_SHAPES, PIL_CONVERT),
         'pil host': (PIL_SHAPES, [False] * 13), 'arrays resize': (ARR_SHAPES, ARR_RESIZE),
         'arrays convert': (ARR_SHAPES, ARR_CONVERT), 'arrays host': (ARR_SHAPES, [False] * 8),
         'empty': ([], []), 'one shape': ([G1] * 4, [True, False, False, True]),
         'all on the device': ([G3, F, G3, G3], [True, False, True, True])}


@pytest.mark.parametrize('name', list(PLANS))
def test_plan_batches(name):
    from inference.image_inference import plan_batches
    shapes, on_device = PLANS[name]
    plan = plan_batches(list(zip(shapes, on_device)))
    assert list(plan) == [F, G1, G3]
    seen = []
    for shape, (rows, dev_at, host_at) in plan.items():
        assert rows == [r for r, s in enumerate(shapes) if s == shape], 'the rows of the shape, ascending'
        assert sorted(dev_at + host_at) == list(range(len(rows))), "the parts' slots partition the batch"
        dev_rows = [r for r in rows if on_device[r]]  # what each part holds, in its own (ascending) order
        host_rows = [r for r in rows if not on_device[r]]
        assert len(dev_at) == len(dev_rows) and len(host_at) == len(host_rows)
        placed = [None] * len(rows)
        for slots, part in ((dev_at, dev_rows), (host_at, host_rows)):
            for k, r in zip(slots, part):
                placed[k] = r
        assert placed == rows, "placing the parts' rows at their slots gives the ascending row list"
        seen += rows
    assert sorted(seen) == list(range(len(shapes)))
    if name == 'all on the device':
        assert plan[G3] == ([0, 2, 3], [0, 1, 2], []) and plan[F] == ([1], [], [0]) and plan[G1] == ([], [], [])
