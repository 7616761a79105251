"""GPU: mode conversion and the gray test of ragged image batches (csrc/image_canon.hip). The
kernels on the raw C ABI against the numpy restatement (tests/canon_ref.py, which test_image_canon_host.py holds
equal to the installed Pillow) byte for byte and flag for flag, and the drop-in classes with convert='gpu'
against convert='host' (both resize='gpu') bit for bit.

A tile is 4096 pixels: the 13 x 11 images are one tile each at every phase of the 16-byte loads, the 200 x 200
ones ten tiles with a ragged last one."""
import ctypes

import numpy as np
import pytest
import torch

import canon_ref as cr
from mec import _lib, engine

pytestmark = pytest.mark.gpu


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _gray_flags(dev, items, start=1):
    """The gray call on `items` packed back to back from byte `start` on -> int32 [B] numpy."""
    lib = _lib.load()
    blob, offs, hw, fmt, pal_off = cr.pack(items, start)
    src = engine.to_device(blob, dev)
    gray = torch.full((len(items),), 7, dtype=torch.int32, device=dev)
    _lib.check(lib.mec_image_gray_ragged_u8(_p(src), offs.ctypes.data, hw.ctypes.data, fmt.ctypes.data, pal_off.ctypes.data,
                                            len(items), blob.size, _p(gray), ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)),
               'mec_image_gray_ragged_u8')
    return gray.cpu().numpy()


def _gray_palette():
    """256 entries: the even ones gray, the odd ones coloured in G (1, 5, 9 ...) or in B (3, 7, 11 ...)."""
    e = np.arange(256)
    pal = np.repeat(((e * 37 + 11) % 256).astype(np.uint8)[:, None], 3, 1)
    pal[1::4, 1] ^= 0x10
    pal[3::4, 2] ^= 0x01
    return pal.reshape(-1)


def _gray_image(fmt, H, W):
    """A gray image of the format: (pixels, palette or None). P uses even (gray) palette entries only."""
    v = cr.formula(H, W, 1, 2)
    if fmt == cr.RGB:
        return np.repeat(v, 3, 2), None
    if fmt == cr.RGBA:
        return np.concatenate([np.repeat(v, 3, 2), cr.formula(H, W, 1, 5)], 2), None
    return (v[..., 0] & 0xFE), _gray_palette()


def _coloured(fmt, px, y, x, ch):
    """A copy of the gray image with exactly pixel (y, x) coloured in channel ch (1: G != R, 2: B != R)."""
    c = px.copy()
    if fmt == cr.P:
        c[y, x] = (c[y, x] & 0xFC) | (1 if ch == 1 else 3)  # a palette entry coloured in that channel
    else:
        c[y, x, ch] ^= 0x80
    return c


@pytest.mark.parametrize('fmt', [cr.RGB, cr.RGBA, cr.P])
def test_gray_flags_exhaustive_over_phase(dev, fmt):
    """13 x 11: the all-gray original and one copy per pixel position and per differing channel, 287 images in one
    call, back to back at odd offsets (13 * 11 * bpp is odd for RGB and P, so the images start at every phase;
    RGBA starts at the odd phases 1, 5, 9, 13): every coloured image has gray neighbours and the reverse."""
    H, W = 13, 11
    px, pal = _gray_image(fmt, H, W)
    items = [(fmt, px, pal)]
    for ch in (1, 2):
        for y in range(H):
            for x in range(W):
                items.append((fmt, _coloured(fmt, px, y, x, ch), pal))
                if (y * W + x) % 9 == 4:
                    items.append((fmt, px, pal))  # gray neighbours among the coloured
    assert sum(1 for it in items if it[1] is not px) == 286
    ref = np.array([cr.canon(*it)[1] for it in items], np.int32)
    assert ref[0] == 1 and (ref == 0).sum() == 286
    got = _gray_flags(dev, items)
    bad = np.flatnonzero(got != ref)
    assert not len(bad), f'fmt {fmt}: images {bad[:10]} differ: got {got[bad[:10]]}, expected {ref[bad[:10]]}'


def test_gray_flags_tile_seams(dev):
    """200 x 200 (ten tiles, the last of 3136 pixels) per format: the original, and copies with one coloured pixel
    at the first pixel, the last pixel and 8 seeded positions; all formats in one call."""
    H = W = 200
    rng = np.random.default_rng(20240607)
    pos = [(0, 0), (H - 1, W - 1)] + [(int(p) // W, int(p) % W) for p in rng.integers(0, H * W, 8)]
    items, names = [], []
    for fmt in (cr.RGB, cr.RGBA, cr.P):
        px, pal = _gray_image(fmt, H, W)
        items.append((fmt, px, pal))
        names.append((fmt, 'gray'))
        for k, (y, x) in enumerate(pos):
            items.append((fmt, _coloured(fmt, px, y, x, 1 + k % 2), pal))
            names.append((fmt, (y, x)))
    ref = np.array([cr.canon(*it)[1] for it in items], np.int32)
    assert ref.sum() == 3
    got = _gray_flags(dev, items)
    bad = [names[i] for i in np.flatnonzero(got != ref)]
    assert not bad, f'wrong flags for (fmt, position) {bad}; seeded positions {pos[2:]}'


def test_gray_flags_other_cases(dev):
    v = cr.formula(37, 29, 1, 1)
    pal_a, pal_b = _gray_palette(), cr.pad_palette(_gray_palette()[::-1][:30].copy())  # pal_b: 10 entries, zero-padded
    assert cr.canon(cr.P, np.arange(256, dtype=np.uint8)[None], pal_b)[1] is False
    unused = (v[..., 0] & 0xFE)  # even entries only: palette a's coloured entries are unused
    used = unused.copy()
    used[36, 28] = 1
    zeros_b = np.full((9, 9), 200, np.uint8)  # palette b's padding: black, gray
    col_b = zeros_b.copy()
    col_b[4, 4] = int(np.flatnonzero((pal_b.reshape(256, 3)[:, 0] != pal_b.reshape(256, 3)[:, 1]))[0])
    items = [(cr.RGBA, np.concatenate([np.repeat(v, 3, 2), cr.formula(37, 29, 1, 8)], 2), None),  # alpha alone varies
             (cr.P, unused, pal_a), (cr.P, used, pal_a), (cr.P, zeros_b, pal_b), (cr.P, col_b, pal_b),
             (cr.L, v[..., 0], None), (cr.LA, cr.formula(37, 29, 2, 3), None), (cr.P, unused, pal_a),
             (cr.RGB, cr.formula(3, 300, 3), None)]
    ref = np.array([cr.canon(*it)[1] for it in items], np.int32)
    assert ref.tolist() == [1, 1, 0, 1, 0, 1, 1, 1, 0]
    assert _gray_flags(dev, items).tolist() == ref.tolist()
    assert _gray_flags(dev, items[5:7], start=3).tolist() == [1, 1]  # a call that launches no tile kernel


CANON_SHAPES = [(1, 1), (1, 7), (7, 1), (5, 3), (48, 48), (33, 65), (3, 300)]
GUARD = 0xA5


def _canon_items():
    pal = cr.pad_palette((np.arange(768) * 53 % 251).astype(np.uint8))
    items = []
    for k, (H, W) in enumerate(CANON_SHAPES):
        for fmt in range(5):
            px = cr.formula(H, W, cr.BPP[fmt], k + fmt)
            items.append((fmt, px[..., 0] if cr.BPP[fmt] == 1 else px, pal if fmt == cr.P else None))
    return items


def _expected(item, C):
    rgb = cr.canon(*item)[0]
    return rgb if C == 3 else rgb[..., :1]


def _run_canon(dev, items, c_out, in_place):
    """The canon call on `items` packed at odd offsets; the outputs 16-byte aligned with 16 guard bytes between
    them, in a buffer of their own or behind the sources in the same allocation. -> (whole dst region numpy,
    dst_offs, the source region after the call, the blob)."""
    lib = _lib.load()
    blob, offs, hw, fmt, pal_off = cr.pack(items, start=1, pad=2, odd=True)
    assert (offs % 2 == 1).all()
    c_out = np.asarray(c_out, np.int32)
    sizes = hw[:, 0].astype(np.int64) * hw[:, 1] * c_out
    dst_offs, at = np.zeros(len(items), np.int64), 16
    for i, n in enumerate(sizes):
        if n:
            dst_offs[i] = at
            at += (int(n) + 15) // 16 * 16 + 16
    src_room = (blob.size + 15) // 16 * 16
    whole = torch.full((src_room + at,), GUARD, dtype=torch.uint8, device=dev)
    whole[:blob.size].copy_(engine.to_device(blob, dev))
    if in_place:
        src_ptr, dst_ptr, dst = whole.data_ptr(), whole.data_ptr() + src_room, whole[src_room:]
    else:
        dst = torch.full((at,), GUARD, dtype=torch.uint8, device=dev)
        src_ptr, dst_ptr = whole.data_ptr(), dst.data_ptr()
    _lib.check(lib.mec_image_canon_ragged_u8(ctypes.c_void_p(src_ptr), offs.ctypes.data, hw.ctypes.data, fmt.ctypes.data,
                                             pal_off.ctypes.data, c_out.ctypes.data, dst_offs.ctypes.data, len(items), blob.size,
                                             ctypes.c_void_p(dst_ptr), at, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)),
               'mec_image_canon_ragged_u8')
    return dst.cpu().numpy(), dst_offs, whole[:blob.size].cpu().numpy(), blob


@pytest.mark.parametrize('in_place', [False, True])
def test_canon_bytes_and_guards(dev, in_place):
    """Every (fmt, c_out) over the shape list in one call: c_out 3, 1 and 0 in turn over the items, each item
    three times, so that every pair is served and a third of the images write nothing."""
    base = _canon_items()
    items, c_out = [], []
    for k, it in enumerate(base):
        for r in range(3):
            items.append(it)
            c_out.append((3, 1, 0)[(k + r) % 3])
    got, dst_offs, src_after, blob = _run_canon(dev, items, c_out, in_place)
    assert np.array_equal(src_after, blob), 'the call wrote into its sources'
    untouched = np.ones(got.size, bool)
    for i, (it, C) in enumerate(zip(items, c_out)):
        if not C:
            continue
        ref = _expected(it, C).reshape(-1)
        o = int(dst_offs[i])
        untouched[o:o + ref.size] = False
        bad = np.flatnonzero(got[o:o + ref.size] != ref)
        assert not len(bad), f'image {i} fmt {it[0]} shape {np.asarray(it[1]).shape} c_out {C}: {len(bad)} bytes differ, first at {bad[0]}'
    assert (got[untouched] == GUARD).all(), 'a byte outside the written ranges changed'
    assert untouched.sum() >= 16 * sum(1 for c in c_out if c)


def test_canon_c_out_0_writes_nothing(dev):
    items = _canon_items()[:10]
    got, _, src_after, blob = _run_canon(dev, items, [0] * len(items), False)
    assert (got == GUARD).all() and np.array_equal(src_after, blob)


def test_canon_gathers_faces(dev):
    """48 x 48 L images scattered among others at odd offsets -> one contiguous [n,48,48,1] batch (L -> 1)."""
    lib = _lib.load()
    faces = [cr.formula(48, 48, 1, s)[..., 0] for s in range(5)]
    items = []
    for k, f in enumerate(faces):
        items.append((cr.L, f, None))
        items.append((cr.RGB, cr.formula(5 + k, 7, 3, k), None))
    blob, offs, hw, fmt, pal_off = cr.pack(items, start=3)
    c_out = np.array([1, 0] * 5, np.int32)
    dst_offs = np.array([k // 2 * 2304 if k % 2 == 0 else 0 for k in range(10)], np.int64)
    src = engine.to_device(blob, dev)
    out = torch.full((5, 48, 48, 1), GUARD, dtype=torch.uint8, device=dev)
    _lib.check(lib.mec_image_canon_ragged_u8(_p(src), offs.ctypes.data, hw.ctypes.data, fmt.ctypes.data, pal_off.ctypes.data,
                                             c_out.ctypes.data, dst_offs.ctypes.data, 10, blob.size, _p(out), out.numel(),
                                             ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), 'mec_image_canon_ragged_u8')
    assert np.array_equal(out.cpu().numpy()[..., 0], np.stack(faces))


def test_ingest_ragged_groups(dev):
    """engine.ingest_ragged against the host's route on the restatement's pixels: the flags, the three groups'
    rows, and the batches' bytes (the resized ones against engine.resize_ragged on the converted pixels)."""
    pal = _gray_palette()
    g48 = cr.formula(48, 48, 1, 1)
    items = [(cr.RGB, cr.formula(60, 80, 3), None), (cr.L, g48[..., 0], None), (cr.RGBA, cr.formula(50, 70, 4), None),
             (cr.RGB, np.repeat(g48, 3, 2), None), (cr.P, cr.formula(40, 30, 1)[..., 0] & 0xFE, pal),
             (cr.P, cr.formula(40, 30, 1)[..., 0], pal), (cr.LA, cr.formula(20, 90, 2), None),
             (cr.L, cr.formula(100, 64, 1)[..., 0], None),
             (cr.RGBA, np.concatenate([np.repeat(g48, 3, 2), cr.formula(48, 48, 1, 4)], 2), None),
             (cr.RGB, np.repeat(cr.formula(31, 33, 1), 3, 2), None)]
    conv = [cr.canon(*it) for it in items]
    gray, groups = engine.ingest_ragged([(px, fmt, pal) for fmt, px, pal in items], dev)
    assert gray.tolist() == [g for _, g in conv]
    (f48, r48), (x1, r1), (x3, r3) = groups
    assert r48 == [1, 3, 8] and r1 == [4, 6, 7, 9] and r3 == [0, 2, 5]
    assert np.array_equal(f48.cpu().numpy(), np.stack([conv[i][0][..., :1] for i in r48]))
    assert torch.equal(x1, engine.resize_ragged([conv[i][0][..., :1] for i in r1], dev))
    assert torch.equal(x3, engine.resize_ragged([conv[i][0] for i in r3], dev))
    gray0, groups0 = engine.ingest_ragged([], dev)
    assert gray0.shape == (0,) and [tuple(t.shape) for t, _ in groups0] == [(0, 48, 48, 1), (0, 224, 224, 1), (0, 224, 224, 3)]
    with pytest.raises(ValueError, match='domain'):
        engine.ingest_ragged([(cr.formula(301, 3, 3), cr.RGB, None)], dev)
    with pytest.raises(ValueError, match='palette'):
        engine.ingest_ragged([(cr.formula(5, 3, 1)[..., 0], cr.P, None)], dev)


def _pil_batch():
    """One image of every route, as PIL images (the issue's list, in a mixed order)."""
    from PIL import Image
    f = cr.formula
    g48 = f(48, 48, 1, 6)
    p_col = Image.fromarray(f(90, 70, 1, 2)[..., 0], 'P')
    p_col.putpalette((np.arange(768) * 53 % 251).astype(np.uint8).tolist())
    p_gray = Image.fromarray(f(64, 100, 1, 3)[..., 0] & 0xFE, 'P')
    p_gray.putpalette(_gray_palette().tolist())
    cmyk = Image.fromarray(f(80, 60, 4, 1), 'CMYK')
    return [Image.fromarray(f(120, 160, 3), 'RGB'),  # a colour photo
            Image.fromarray(g48[..., 0], 'L'),  # a 48 x 48 L face
            Image.fromarray(f(75, 55, 4, 2), 'RGBA'),  # colour RGBA
            Image.fromarray(f(301, 3, 3), 'RGB'),  # the strip: outside the domain, the host's
            Image.fromarray(np.repeat(g48, 3, 2), 'RGB'),  # a 48 x 48 gray-valued RGB face
            p_col, Image.fromarray(f(200, 150, 1, 4)[..., 0], 'L'),  # an L photo
            Image.fromarray(f(57, 83, 1, 5)[..., 0] > 127),  # mode 1: the host's
            Image.fromarray(np.concatenate([np.repeat(g48, 3, 2), f(48, 48, 1, 9)], 2), 'RGBA'),  # a gray RGBA face
            p_gray, cmyk, Image.fromarray(np.repeat(f(130, 90, 1, 7), 3, 2), 'RGB'),  # a gray-valued RGB photo
            Image.fromarray(f(66, 44, 2, 8), 'LA')]


COVERED = ('L', 'LA', 'RGB', 'RGBA', 'P')


@pytest.mark.parametrize('precision', ['f16', 'fp32x3'])
def test_image_inference_convert_gpu_equals_host(dev, precision, monkeypatch):
    from PIL import Image
    from inference.image_inference import ImageInference, Native
    inf = ImageInference(seed=1234, device=dev, precision=precision, resize='gpu')
    assert inf.convert == 'host'
    images = _pil_batch()
    assert [im.mode for im in images].count('1') == 1 and any(im.mode == 'CMYK' for im in images)
    arrays = [np.asarray(im) for im in images if im.mode in ('L', 'RGB')] + [cr.formula(30, 40, 1, 1)]  # [H,W], [H,W,3], [H,W,1]
    host_items = [inf.route(im) for im in images]
    assert not any(isinstance(it, Native) for it in host_items)
    inf.forward_routed(host_items)  # the handle's GEMM autotuner settles on these first passes
    inf.extract_features_arrays(arrays)
    ref_pil = [t.cpu().numpy() for t in inf.forward_routed(host_items)]
    ref_arr = inf.extract_features_arrays(arrays)
    ref_dicts = inf.predict_arrays(arrays)

    real = Image.Image.convert

    def convert(self, *a, **k):
        # the strip is an RGB image outside the domain: the host converts it in both settings
        assert self.mode not in COVERED or self.size == (3, 301), f'convert() on a {self.mode} image {self.size}'
        return real(self, *a, **k)

    inf.convert = 'gpu'
    monkeypatch.setattr(Image.Image, 'convert', convert)
    items = [inf.route(im) for im in images]
    assert [isinstance(it, Native) for it in items] == [im.mode in COVERED and im.size != (3, 301) for im in images]
    got_pil = [t.cpu().numpy() for t in inf.forward_routed(items)]
    got_arr = inf.extract_features_arrays(arrays)
    got_dicts = inf.predict_arrays(arrays)
    monkeypatch.undo()
    assert got_pil[0].shape == (len(images), 512) and got_pil[1].shape == (len(images), 7)
    for g, r in zip(got_pil + list(got_arr), ref_pil + list(ref_arr)):
        assert g.dtype == r.dtype and np.array_equal(g, r)
    assert got_dicts == ref_dicts and inf.predict_arrays([]) == []
    with pytest.raises(ValueError):
        inf.extract_features_arrays([np.zeros((5, 5, 2), np.uint8)])


def test_forward_routed_merges_every_shape(dev):
    """Nine small images such that every model-input shape's batch interleaves host-made and device-made rows,
    under both sources of the device-made rows (engine.resize_ragged per channel count, engine.ingest_ragged):
    (48,48,1) rows 1, 4; (224,224,1) rows 2, 6, 8; (224,224,3) rows 0, 3, 5, 7. The three settings' results are
    equal bit for bit."""
    from PIL import Image
    from inference.image_inference import ImageInference, Native
    f = cr.formula
    images = [Image.fromarray(f(100, 120, 3), 'RGB'),  # an RGB photo: the device's
              Image.fromarray(f(48, 48, 1, 5)[..., 0] > 127),  # a mode-1 face: converted on the host, its own kernel
              Image.fromarray(f(60, 80, 1, 4)[..., 0], 'L'),  # an L photo: the device's
              Image.fromarray(f(301, 3, 3), 'RGB'),  # the strip, outside the domain: the host's
              Image.fromarray(f(48, 48, 1, 6)[..., 0], 'L'),  # an L face: the host's, ingested with convert='gpu'
              Image.fromarray(f(80, 60, 4, 1), 'CMYK'),  # converted on the host, resized on the device
              Image.fromarray(f(301, 3, 1, 2)[..., 0], 'L'),  # a gray strip: the host's
              Image.fromarray(f(75, 55, 4, 2), 'RGBA'),  # colour RGBA: the device's
              Image.fromarray(np.repeat(f(90, 70, 1, 7), 3, 2), 'RGB')]  # a gray-valued RGB photo: the device's
    inf = ImageInference(seed=1234, device=dev, precision='f16')

    def run(resize, convert):
        inf.resize, inf.convert = resize, convert
        items = [inf.route(im) for im in images]
        made = ['native' if isinstance(it, Native) else 'ragged' if it[1] else it[0].shape for it in items]
        return made, [t.cpu().numpy() for t in inf.forward_routed(items)]

    F, G1, G3 = (48, 48, 1), (224, 224, 1), (224, 224, 3)
    run('host', 'host')  # the handle's GEMM autotuner settles on this first pass
    made_h, ref = run('host', 'host')
    assert made_h == [G3, F, G1, G3, F, G3, G1, G3, G1]
    made_r, got_r = run('gpu', 'host')
    assert made_r == ['ragged', F, 'ragged', G3, F, 'ragged', G1, 'ragged', 'ragged']
    made_c, got_c = run('gpu', 'gpu')
    assert made_c == ['native', F, 'native', G3, 'native', 'ragged', G1, 'native', 'native']
    assert ref[0].shape == (9, 512) and ref[1].shape == (9, 7)
    for got in (got_r, got_c):
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])


def test_predict_and_extract_features_on_files(dev, tmp_path):
    from PIL import Image
    from inference.image_inference import ImageInference
    inf = ImageInference(seed=1234, device=dev, precision='f16', resize='gpu', convert='gpu')
    assert inf.convert == 'gpu'
    p_im = Image.fromarray(cr.formula(70, 90, 1, 2)[..., 0] % 40, 'P')
    p_im.putpalette((np.arange(120) * 53 % 251).astype(np.uint8).tolist())  # 40 entries
    imgs = [Image.fromarray(cr.formula(90, 120, 1)[..., 0], 'L'), Image.fromarray(cr.formula(80, 100, 4), 'RGBA'), p_im,
            Image.fromarray(cr.formula(48, 48, 1, 3)[..., 0], 'L')]
    paths = []
    for k, im in enumerate(imgs):
        paths.append(str(tmp_path / f'im{k}.png'))
        im.save(paths[-1])
    with Image.open(paths[2]) as im:
        assert im.mode == 'P'
    inf.convert = 'host'
    for p in paths:  # the handle's GEMM autotuner settles on this first pass
        inf.predict(p)
    host = [(inf.predict(p), inf.extract_features(p)) for p in paths]
    inf.convert = 'gpu'
    for p, (d, (feat, probs)) in zip(paths, host):
        assert inf.predict(p) == d
        f, q = inf.extract_features(p)
        assert np.array_equal(f, feat) and np.array_equal(q, probs)


def test_predict_multimodal_batch_convert_gpu_equals_host(dev, tmp_path, monkeypatch):
    """B = 5 requests with mixed presence and image modes (an L face, an RGBA image, a P image, a mode-1 image, an
    RGB photo): the result dicts of image_convert='gpu' equal those of 'host'."""
    from PIL import Image
    from inference.multimodal_fusion import MultimodalFusion
    from oracle import audio as oa
    from test_gpu_dropin import TEXTS, _legacy_tokenizer, _stub_audio, _write_vocab
    fusion = MultimodalFusion(seed=1234, device=dev, precision='f16', image_resize='gpu', image_convert='gpu')
    assert fusion.image_inference.convert == 'gpu' and fusion.image_inference.resize == 'gpu'
    waves = {f'clip{i}.wav': w for i, w in enumerate(oa.synthetic_clips(2, seed=51))}
    _stub_audio(monkeypatch, waves)
    fusion.text_inference.tokenizer = _legacy_tokenizer(_write_vocab(tmp_path))
    p_im = Image.fromarray(cr.formula(70, 50, 1, 2)[..., 0], 'P')
    p_im.putpalette((np.arange(768) * 53 % 251).astype(np.uint8).tolist())
    imgs = [Image.fromarray(cr.formula(48, 48, 1)[..., 0], 'L'), Image.fromarray(cr.formula(150, 200, 4), 'RGBA'), p_im,
            Image.fromarray(cr.formula(60, 40, 1)[..., 0] > 100), Image.fromarray(cr.formula(333, 240, 3), 'RGB')]
    paths = []
    for k, im in enumerate(imgs):
        paths.append(str(tmp_path / f'im{k}.png'))
        im.save(paths[-1])
    clips = list(waves)
    reqs = [(clips[0], TEXTS[0], paths[1]), (None, TEXTS[1], paths[0]), (clips[1], None, paths[2]),
            (None, None, paths[3]), (clips[0], TEXTS[1], paths[4])]
    fusion.predict_multimodal_batch(reqs)  # the handles' GEMM autotuners settle on this first pass
    got = fusion.predict_multimodal_batch(reqs)
    fusion.image_inference.convert = 'host'
    ref = fusion.predict_multimodal_batch(reqs)
    assert len(got) == 5 and got == ref
    assert 'attention_weights' in got[0]['fusion'] and list(got[3]) == ['image']
