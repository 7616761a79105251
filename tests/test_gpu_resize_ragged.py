"""GPU: the ragged PIL-exact resize (csrc/resize.hip). The kernels against the numpy
restatement (tests/resize_ref.py, which test_resize_ragged_host.py pins to Pillow 12.2's digests) byte for byte,
and the drop-in classes with resize='gpu' against resize='host' bit for bit.

Shapes: the fixture's 57 (sides 1 .. 4096: up- and downscale on either axis, ksize 3 .. 39, row tiles of 2 ..
32 rows with and without a remainder of the 4-row step, row tiles that start at every 16-byte phase) with
the hash input; the 17 explicit ones again all-255 and as a 0 / 255 checkerboard."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import resize_ref
from conftest import GOLDEN
from mec import _lib, engine

pytestmark = pytest.mark.gpu

with open(os.path.join(GOLDEN, 'image_resize_ragged.json')) as _f:
    CASES = [(c['H'], c['W']) for c in json.load(_f)['cases']]
FIXED = CASES[:17]


@pytest.fixture(scope='module')
def batch():
    """[(name, input u8 [H,W,3], restatement u8 [224,224,3])], computed once and never written to."""
    items = [(H, W, 'formula') for H, W in CASES] + [(H, W, p) for H, W in FIXED for p in ('white', 'checker')]
    out = []
    for H, W, p in items:
        a = resize_ref.make_input(H, W, p)
        r = resize_ref.resize_hfirst(a)
        a.setflags(write=False)
        r.setflags(write=False)
        out.append((f'{H}x{W} {p}', a, r))
    return out


def _check(batch, got, pick):
    got = got.cpu().numpy()
    assert got.shape[0] == len(batch)
    for (name, _, ref), g in zip(batch, got):
        ref = pick(ref)
        bad = np.argwhere(g != ref)
        assert not len(bad), f'{name}: {len(bad)} bytes differ, first at {bad[0]}: {g[tuple(bad[0])]} vs {ref[tuple(bad[0])]}'


def test_whole_shape_list_rgb(dev, batch):
    got = engine.resize_ragged([a for _, a, _ in batch], dev)
    assert got.shape == (len(batch), 224, 224, 3) and got.dtype == torch.uint8
    _check(batch, got, lambda r: r)


def test_whole_shape_list_gray(dev, batch):
    """C = 1 (the other instantiation of both kernels) on channel 1 of the same inputs; the restatement treats
    the channels independently, so its channel 1 is the gray image's result."""
    got = engine.resize_ragged([np.ascontiguousarray(a[..., 1:2]) for _, a, _ in batch], dev)
    assert got.shape == (len(batch), 224, 224, 1)
    _check(batch, got, lambda r: r[..., 1:2])


def test_48x48_equals_the_fast_path(dev, batch):
    lib = _lib.load()
    name, a, _ = batch[CASES.index((48, 48))]
    assert name == '48x48 formula'
    gray = np.ascontiguousarray(a[..., 0])
    x = engine.to_device(gray[None], dev)
    fast = torch.empty((1, 224, 224), dtype=torch.uint8, device=dev)
    _lib.check(lib.mec_resize_u8(ctypes.c_void_p(x.data_ptr()), 1, 48, 48, ctypes.c_void_p(fast.data_ptr()), 224, 224,
                                 ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), 'mec_resize_u8')
    got = engine.resize_ragged([gray], dev)
    assert torch.equal(got[0, :, :, 0], fast[0])


def test_empty_and_single(dev, batch):
    for C in (1, 3):
        e = engine.resize_ragged([], dev, channels=C)
        assert e.shape == (0, 224, 224, C) and e.dtype == torch.uint8 and e.device == dev
    name, a, ref = batch[CASES.index((480, 640))]
    got = engine.resize_ragged([a], dev)
    assert got.shape == (1, 224, 224, 3) and np.array_equal(got[0].cpu().numpy(), ref), name


def test_c_abi_packed_at_odd_offsets(dev, batch):
    """The C entry on images packed back to back from byte 1 on (no image starts on a 16-byte boundary, the
    last ends with the buffer), an exact-size tmp, and a stream of its own."""
    lib = _lib.load()
    picks = [batch[CASES.index(hw)] for hw in ((5, 3), (37, 1000), (1, 7), (223, 225), (300, 3))]
    sizes = [a.size for _, a, _ in picks]
    offs = np.cumsum([1] + sizes[:-1]).astype(np.int64)
    total = int(offs[-1] + sizes[-1])
    blob = np.zeros(total, np.uint8)
    for (_, a, _), o in zip(picks, offs):
        blob[o:o + a.size] = a.reshape(-1)
    hw = np.array([a.shape[:2] for _, a, _ in picks], np.int32)
    tmp_bytes = int(hw[:, 0].sum()) * 224 * 3
    src = engine.to_device(blob, dev)
    tmp = torch.empty(tmp_bytes, dtype=torch.uint8, device=dev)
    out = torch.empty((len(picks), 224, 224, 3), dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    for _ in range(2):  # the second call re-uses the library's staging buffer behind the first one's kernels
        _lib.check(lib.mec_resize_ragged_u8(p(src), offs.ctypes.data, hw.ctypes.data, len(picks), 3, total, p(tmp),
                                            tmp_bytes, p(out), ctypes.c_void_p(stream.cuda_stream)), 'mec_resize_ragged_u8')
    stream.synchronize()
    _check(picks, out, lambda r: r)


def test_white_stays_white(dev):
    shapes = [(1, 1), (7, 1), (300, 3), (480, 640), (4096, 41), (2, 4096), (1000, 37)]
    for C in (1, 3):
        got = engine.resize_ragged([np.full((H, W, C), 255, np.uint8) for H, W in shapes], dev)
        assert int(got.min()) == 255, C


def test_engine_argument_errors(dev):
    with pytest.raises(ValueError, match='domain'):
        engine.resize_ragged([np.zeros((301, 3, 3), np.uint8)], dev)
    with pytest.raises(ValueError, match='channels'):
        engine.resize_ragged([np.zeros((5, 5, 3), np.uint8), np.zeros((5, 5, 1), np.uint8)], dev)
    with pytest.raises(TypeError):
        engine.resize_ragged([np.zeros((5, 5, 3), np.float32)], dev)


def _arrays():
    """Small images of every route: 48x48 gray (its own kernel), gray and RGB inside the GPU resize's domain
    (up- and downscale, one already 224x224), and one RGB strip outside it (301 > 100 * 3: host)."""
    f = resize_ref.make_input
    rgb = [f(100, 130, 'formula'), f(224, 224, 'formula'), f(300, 449, 'checker'), f(301, 3, 'formula')]
    gray = [f(48, 48, 'formula')[..., 0], f(60, 80, 'formula')[..., 2], f(30, 20, 'formula')[..., :1]]
    gray3 = np.repeat(f(257, 131, 'formula')[..., :1], 3, axis=2)  # RGB storage, gray content: one channel
    return [rgb[0], gray[0], gray[1], rgb[3], rgb[1], gray3, gray[2], rgb[2]]


@pytest.mark.parametrize('precision', ['f16', 'fp32x3'])
def test_image_inference_gpu_equals_host(dev, precision, monkeypatch):
    from inference.image_inference import ImageInference
    with pytest.raises(ValueError):
        ImageInference(seed=1234, device=dev, resize='device')
    inf = ImageInference(seed=1234, device=dev, precision=precision)
    assert inf.resize == 'host'
    arrays = _arrays()
    inf.extract_features_arrays(arrays)  # the handle's GEMM autotuner settles on this first pass
    feat_h, probs_h = inf.extract_features_arrays(arrays)
    dicts_h = inf.predict_arrays(arrays)
    calls = []
    real = engine.resize_ragged
    monkeypatch.setattr(engine, 'resize_ragged',
                        lambda arrs, *a, **k: calls.append([x.shape for x in arrs]) or real(arrs, *a, **k))
    assert not calls
    inf.resize = 'gpu'
    feat_g, probs_g = inf.extract_features_arrays(arrays)
    # every in-domain image went through the GPU resize, grouped by channel count; 48x48 gray and the strip did not
    assert sorted(calls) == [[(60, 80, 1), (257, 131, 1), (30, 20, 1)], [(100, 130, 3), (224, 224, 3), (300, 449, 3)]]
    assert feat_g.shape == (8, 512) and probs_g.shape == (8, 7)
    assert np.array_equal(feat_g, feat_h) and np.array_equal(probs_g, probs_h)
    assert inf.predict_arrays(arrays) == dicts_h
    assert inf.predict_arrays([]) == []


def test_predict_and_extract_features_gpu_equals_host(dev, tmp_path):
    from PIL import Image
    from inference.image_inference import ImageInference
    inf = ImageInference(seed=1234, device=dev, precision='f16')
    a = resize_ref.make_input(90, 120, 'formula')
    paths = []
    for k, img in enumerate((Image.fromarray(a, 'RGB'), Image.fromarray(a[..., 0], 'L'),
                             Image.fromarray(resize_ref.make_input(301, 3, 'formula'), 'RGB'))):
        paths.append(str(tmp_path / f'im{k}.png'))
        img.save(paths[-1])
    for p in paths:  # the handle's GEMM autotuner settles on this first pass
        inf.predict(p)
    host = [(inf.predict(p), inf.extract_features(p)) for p in paths]
    inf.resize = 'gpu'
    for p, (d, (feat, probs)) in zip(paths, host):
        assert inf.predict(p) == d
        f, q = inf.extract_features(p)
        assert np.array_equal(f, feat) and np.array_equal(q, probs)


def test_predict_multimodal_batch_gpu_equals_host(dev, tmp_path, monkeypatch):
    """B = 5 requests with mixed presence and mixed image shapes (a 48x48 face, an RGB photo, a gray photo, an
    out-of-domain strip): the result dicts of image_resize='gpu' equal those of 'host'."""
    from PIL import Image
    from inference.multimodal_fusion import MultimodalFusion
    from oracle import audio as oa
    from test_gpu_dropin import TEXTS, _legacy_tokenizer, _stub_audio, _write_vocab
    fusion = MultimodalFusion(seed=1234, device=dev, precision='f16', image_resize='gpu')
    assert fusion.image_inference.resize == 'gpu'
    waves = {f'clip{i}.wav': w for i, w in enumerate(oa.synthetic_clips(2, seed=51))}
    _stub_audio(monkeypatch, waves)
    fusion.text_inference.tokenizer = _legacy_tokenizer(_write_vocab(tmp_path))
    f = resize_ref.make_input
    imgs = [Image.fromarray(f(48, 48, 'formula')[..., 0], 'L'), Image.fromarray(f(150, 200, 'formula'), 'RGB'),
            Image.fromarray(f(70, 50, 'formula')[..., 1], 'L'), Image.fromarray(f(301, 3, 'formula'), 'RGB'),
            Image.fromarray(f(333, 240, 'checker'), 'RGB')]
    paths = []
    for k, im in enumerate(imgs):
        paths.append(str(tmp_path / f'im{k}.png'))
        im.save(paths[-1])
    clips = list(waves)
    reqs = [(clips[0], TEXTS[0], paths[1]), (None, TEXTS[1], paths[0]), (clips[1], None, paths[2]),
            (None, None, paths[3]), (clips[0], TEXTS[1], paths[4])]
    fusion.predict_multimodal_batch(reqs)  # the handles' GEMM autotuners settle on this first pass
    got = fusion.predict_multimodal_batch(reqs)
    fusion.image_inference.resize = 'host'
    ref = fusion.predict_multimodal_batch(reqs)
    assert len(got) == 5 and got == ref
    assert 'attention_weights' in got[0]['fusion'] and list(got[3]) == ['image']
