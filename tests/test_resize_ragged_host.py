"""CPU: the ragged GPU resize's host side (csrc/resize.hip). The restatement
(tests/resize_ref.py, horizontal pass first) against Pillow 12.2's recorded digests and against the installed
Pillow; the domain predicate; the library's tap builder against oracle.resize.coeffs; and the batch entry's
descriptor checks, which all precede the first device call and so run without a GPU."""
import json
import os

import numpy as np
import pytest

import resize_ref
from conftest import GOLDEN
from mec import _lib, image as mimage
from oracle.resize import coeffs

with open(os.path.join(GOLDEN, 'image_resize_ragged.json')) as _f:
    FIXTURE = json.load(_f)
CASES = FIXTURE['cases']


def test_restatement_equals_pillow_digests():
    assert len(CASES) == 57 and FIXTURE['pillow'].startswith('12.2')
    for case in CASES:
        H, W = case['H'], case['W']
        assert mimage.resize_on_gpu(H, W), (H, W)
        for p in resize_ref.PATTERNS:
            got = resize_ref.resize_hfirst(resize_ref.make_input(H, W, p))
            assert got.shape == (224, 224, 3) and resize_ref.digest(got) == case['sha256'][p], (H, W, p)


# the explicit shapes of the fixture and the last in-domain strip at W = 3; the installed Pillow may be any
# version whose 8-bit resample is Pillow 12.2's
LIVE = [(c['H'], c['W']) for c in CASES[:17]] + [(300, 3)]


def test_restatement_equals_live_pillow():
    Image = pytest.importorskip('PIL.Image')
    for H, W in LIVE:
        for p in resize_ref.PATTERNS:
            a = resize_ref.make_input(H, W, p)
            ref = np.asarray(Image.fromarray(a, 'RGB').resize((224, 224), Image.BILINEAR))
            assert np.array_equal(resize_ref.resize_hfirst(a), ref), (H, W, p)
    gray = resize_ref.make_input(37, 61, 'formula')[..., 0]
    ref = np.asarray(Image.fromarray(gray, 'L').resize((224, 224), Image.BILINEAR))
    assert np.array_equal(resize_ref.resize_hfirst(gray[..., None])[..., 0], ref)


def test_domain_predicate():
    for hw in ((301, 3), (4097, 100), (0, 5), (5, 0), (100, 4097), (-1, 5), (101, 1), (2 ** 40, 2 ** 40)):
        assert mimage.resize_on_gpu(*hw) is False, hw
    for hw in ((300, 3), (100, 1), (1, 1), (4096, 41), (4096, 4096), (1, 4096), (2, 4096)):
        assert mimage.resize_on_gpu(*hw) is True, hw


@pytest.mark.parametrize('extent', [1, 2, 3, 48, 223, 224, 225, 449, 640, 4096])
def test_library_taps_equal_oracle_coeffs(extent):
    xmin, n, kk = coeffs(extent, 224)
    ks = kk.shape[1]
    assert ks <= 39
    gx, gn, gk = mimage.resize_taps(extent, 224, 39)  # the widest table the domain needs
    assert np.array_equal(gx, xmin) and np.array_equal(gn, n)
    assert np.array_equal(gk[:, :ks], kk) and not gk[:, ks:].any()
    for xx in range(224):  # nothing past an output's n taps, nothing outside the source
        assert not gk[xx, gn[xx]:].any() and gx[xx] >= 0 and gx[xx] + gn[xx] <= extent and gn[xx] >= 1
    tx, tn, tk = mimage.resize_taps(extent, 224)  # kmax = the extent's own ksize
    assert tk.shape[1] == ks and np.array_equal(tk, kk) and np.array_equal(tx, xmin) and np.array_equal(tn, n)


def test_library_taps_argument_errors():
    lib = _lib.load()
    keep = np.zeros(224 * 39, np.int32)
    buf = keep.ctypes.data
    assert lib.mec_resize_taps(0, 224, buf, buf, buf, 39) == -1 and b'at least 1' in lib.mec_last_error()
    assert lib.mec_resize_taps(48, 0, buf, buf, buf, 39) == -1
    assert lib.mec_resize_taps(48, 224, None, buf, buf, 39) == -1 and b'null' in lib.mec_last_error()
    assert lib.mec_resize_taps(4096, 224, buf, buf, buf, 38) == -1 and b'kmax' in lib.mec_last_error()
    assert lib.mec_resize_taps(4096, 224, buf, buf, buf, 39) == 0


def _call(lib, offs, hw, B, C, src_bytes, tmp_bytes, src=0x1000, tmp=0x2000, out=0x3000, null=()):
    offs = np.asarray(offs, np.int64)
    hw = np.asarray(hw, np.int32)
    p = {'src': src, 'tmp': tmp, 'out': out, 'offs': offs.ctypes.data, 'hw': hw.ctypes.data}
    for k in null:
        p[k] = None
    return lib.mec_resize_ragged_u8(p['src'], p['offs'], p['hw'], B, C, src_bytes, p['tmp'], tmp_bytes, p['out'], None)


# name -> (kwargs of _call for a batch of two 10 x 20 RGB images, a fragment of the message)
GOOD = dict(offs=[0, 608], hw=[[10, 20], [10, 20]], B=2, C=3, src_bytes=1208, tmp_bytes=2 * 10 * 224 * 3)
BAD = {
    'B < 0': (dict(B=-1), b'B < 0'),
    'C = 2': (dict(C=2), b'C must be 1 or 3'),
    'C = 0': (dict(C=0), b'C must be 1 or 3'),
    'null src': (dict(null=('src',)), b'null'),
    'null offs': (dict(null=('offs',)), b'null'),
    'null hw': (dict(null=('hw',)), b'null'),
    'null tmp': (dict(null=('tmp',)), b'null'),
    'null out': (dict(null=('out',)), b'null'),
    'misaligned tmp': (dict(tmp=0x2001), b'aligned'),
    'H = 0': (dict(hw=[[10, 20], [0, 20]]), b'image 1'),
    'W = 0': (dict(hw=[[10, 0], [10, 20]]), b'image 0'),
    'H = 4097': (dict(hw=[[10, 20], [4097, 100]], src_bytes=1 << 40, tmp_bytes=1 << 40), b'outside'),
    'W = 4097': (dict(hw=[[10, 20], [10, 4097]], src_bytes=1 << 40, tmp_bytes=1 << 40), b'outside'),
    'H > 100 W': (dict(hw=[[10, 20], [301, 3]], src_bytes=1 << 40, tmp_bytes=1 << 40), b'outside'),
    'negative H': (dict(hw=[[-10, 20], [10, 20]]), b'image 0'),
    'negative offset': (dict(offs=[-1, 608]), b'inside src_bytes'),
    'image past src_bytes': (dict(src_bytes=1207), b'inside src_bytes'),
    'offset past src_bytes': (dict(offs=[0, 1 << 50]), b'inside src_bytes'),
    'tmp one byte short': (dict(tmp_bytes=2 * 10 * 224 * 3 - 1), b'tmp_bytes'),
}


@pytest.mark.parametrize('case', list(BAD))
def test_ragged_entry_rejects_invalid_descriptors_without_gpu(case):
    """Every check precedes the first device call: the fake device pointers are never touched."""
    lib = _lib.load()
    kw, msg = BAD[case]
    assert _call(lib, **{**GOOD, **kw}) == -1
    assert msg in lib.mec_last_error(), lib.mec_last_error()


def test_ragged_entry_empty_batch_without_gpu():
    lib = _lib.load()
    assert lib.mec_resize_ragged_u8(None, None, None, 0, 3, 0, None, 0, None, None) == 0
    assert lib.mec_resize_ragged_u8(None, None, None, 0, 1, 0, None, 0, None, None) == 0
    assert lib.mec_resize_ragged_u8(None, None, None, 0, 2, 0, None, 0, None, None) == -1

