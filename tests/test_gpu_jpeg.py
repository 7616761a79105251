"""GPU: baseline JPEG decoding of ragged batches (csrc/jpeg.hip). Kernel level: the whole fixture
as one batch against the numpy restatement (tests/jpeg_ref.py, itself held against Pillow's digests by
tests/test_jpeg_host.py), independence of batch size and position, canaries around every output; ill-formed
streams, whose purpose is the clean status; then the drop-in classes, decode='gpu' against decode='host'."""
import ctypes
import io

import numpy as np
import pytest
import torch

import jpeg_ref
from mec import _lib, engine, jpeg as mjpeg

pytestmark = pytest.mark.gpu

CANARY = 0xA5
GAP = 32  # canary bytes in front of every output and behind the last


class Entry:
    """One image of a kernel-level batch: descriptor, the bytes that go up and its segments inside them."""

    def __init__(self, desc, data, segs):
        self.desc, self.data, self.segs = desc, bytes(data), np.asarray(segs, np.int64).reshape(-1, 2)
        self.out_bytes = int(desc.H) * int(desc.W) * int(desc.ncomp)
        self.shape = (int(desc.H), int(desc.W), int(desc.ncomp))


@pytest.fixture(scope='module')
def fixture(golden):
    """[(name, Entry, reference pixels)] for every file of the fixture: computed once, never changed."""
    z = golden('jpeg_cases.npz')
    data, offs = z['data'].tobytes(), z['offs']
    out = []
    for k, name in enumerate(z['names']):
        d = data[offs[k]:offs[k + 1]]
        blob = mjpeg.probe(d)
        desc, st, px = jpeg_ref.decode_file(d)
        assert blob is not None and st == 0
        px.setflags(write=False)
        out.append((str(name), Entry(blob.desc, d, blob.segs), px))
    return out


def run(dev, entries):
    """mec_jpeg_decode_ragged on `entries` -> (images, status, canaries untouched). Sources at odd byte phases;
    outputs 16-byte aligned with GAP canary bytes between them, sources and outputs in one allocation."""
    lib = _lib.load()
    B = len(entries)
    src_offs, at = [], 0
    for i, e in enumerate(entries):
        at = (at + 15) // 16 * 16 + (5 * i) % 16
        src_offs.append(at)
        at += len(e.data)
    src_total = (at + 15) // 16 * 16
    dst_offs, at = [], 0
    for e in entries:
        at += GAP
        dst_offs.append(at)
        at = (at + e.out_bytes + 15) // 16 * 16
    room = at + GAP
    host = np.full(src_total + room, CANARY, np.uint8)
    for e, o in zip(entries, src_offs):
        host[o:o + len(e.data)] = np.frombuffer(e.data, np.uint8)
    buf = torch.from_numpy(host).to(dev)
    descs = mjpeg.desc_array([e.desc for e in entries])
    segs = np.ascontiguousarray(np.concatenate([e.segs + np.array([[o, 0]], np.int64) for e, o in zip(entries, src_offs)]))
    ws_bytes = mjpeg.workspace_bytes([e.desc for e in entries])
    ws = torch.empty(ws_bytes + 64, dtype=torch.uint8, device=dev)
    ws[ws_bytes:] = CANARY
    status = torch.full((B,), -1, dtype=torch.int32, device=dev)
    dst_offs = np.asarray(dst_offs, np.int64)
    with torch.cuda.device(dev):
        rc = lib.mec_jpeg_decode_ragged(buf.data_ptr(), src_total, ctypes.addressof(descs), segs.ctypes.data, B,
                                        buf.data_ptr() + src_total, dst_offs.ctypes.data, room, ws.data_ptr(), ws_bytes,
                                        status.data_ptr(), engine._stream(dev))
        _lib.check(rc, 'mec_jpeg_decode_ragged')
        torch.cuda.synchronize(dev)
    got = buf.cpu().numpy()
    keep = np.ones(src_total + room, bool)
    images = []
    for e, o in zip(entries, dst_offs):
        lo = src_total + int(o)
        keep[lo:lo + e.out_bytes] = False
        images.append(got[lo:lo + e.out_bytes].reshape(e.shape))
    clean = bool(np.array_equal(got[keep], host[keep])) and bool((ws[ws_bytes:] == CANARY).all())
    return images, status.cpu().numpy(), clean


def test_fixture_as_one_shuffled_batch(dev, fixture):
    order = np.random.default_rng(7).permutation(len(fixture))
    images, status, clean = run(dev, [fixture[k][1] for k in order])
    assert clean, 'a byte outside the outputs changed'
    assert not status.any(), [(fixture[k][0], int(s)) for k, s in zip(order, status) if s]
    for k, im in zip(order, images):
        assert np.array_equal(im, fixture[k][2]), fixture[k][0]


def test_rows_depend_on_neither_batch_size_nor_position(dev, fixture):
    picks = [3, 20, 41, 59, 83]
    for k in picks:  # B = 1
        images, status, clean = run(dev, [fixture[k][1]])
        assert clean and status.tolist() == [0] and np.array_equal(images[0], fixture[k][2]), fixture[k][0]
    order = np.random.default_rng(8).permutation(len(fixture))[::-1]  # another order, twice in the batch
    images, status, clean = run(dev, [fixture[k][1] for k in list(order) + picks])
    assert clean and not status.any()
    for k, im in zip(list(order) + picks, images):
        assert np.array_equal(im, fixture[k][2]), fixture[k][0]


def test_profile_hook_counts_the_three_kernels(dev, fixture):
    engine.jpeg_prof(True)
    try:
        run(dev, [fixture[k][1] for k in (5, 50)])
        e, i, c, n = engine.jpeg_prof_read()
    finally:
        engine.jpeg_prof(False)
    assert n == 1 and e > 0 and i > 0 and c > 0


# ---- ill-formed streams (after the tests above): the status is the point, and that nothing else is touched

def _ref_status(entry):
    d = jpeg_ref.Desc()
    c = entry.desc
    d.H, d.W, d.ncomp, d.restart = c.H, c.W, c.ncomp, c.restart
    for k in range(c.ncomp):
        d.hs.append(c.hs[k])
        d.vs.append(c.vs[k])
        d.qt.append(list(c.qt[k]))
        d.dc.append((list(c.dc[k].counts), list(c.dc[k].vals)))
        d.ac.append((list(c.ac[k].counts), list(c.ac[k].vals)))
    d.segs = [tuple(s) for s in entry.segs.tolist()]
    return jpeg_ref.decode(d, entry.data)[0]


def _cut(entry, seg, new_len):
    segs = entry.segs.copy()
    segs[seg, 1] = new_len
    return Entry(entry.desc, entry.data, segs)


def _codes(table):
    """{symbol: bit string} of a Huffman table (16 counts, values)."""
    out, code, p = {}, 0, 0
    for l in range(16):
        for _ in range(table.counts[l]):
            out[table.vals[p]] = format(code, f'0{l + 1}b')
            code += 1
            p += 1
        code <<= 1
    return out


def _bad_entries(fixture):
    """[(what, Entry)], every one with a nonzero status by the restatement."""
    by_name = {n: e for n, e, _ in fixture}
    plain = by_name['48x48_420_q75_opt1_rst0_random']  # one segment
    scan_off, scan_len = (int(v) for v in plain.segs[0])
    out = [('cut mid-MCU', _cut(plain, 0, scan_len // 2)), ('cut to nothing', _cut(plain, 0, 0))]
    scan = plain.data[scan_off:scan_off + scan_len]
    stuffed = scan.find(b'\xff\x00', 16)
    assert stuffed > 0
    out.append(('cut inside a stuffed FF 00', _cut(plain, 0, stuffed + 1)))
    for name, e, _ in fixture:  # a restart segment that loses its last byte, where that byte holds more than padding
        if '_rst1_' in name or '_rst3_' in name:
            cand = _cut(e, 0, int(e.segs[0, 1]) - 1)
            if _ref_status(cand):
                out.append(('a segment cut at its last byte', cand))
                break
    # a block whose runs lead past coefficient 63: DC 0, then (run 15, size 1) five times
    gray = by_name['16x16_gray_q30_opt0_rst0_smooth']
    dc, ac = _codes(gray.desc.dc[0]), _codes(gray.desc.ac[0])
    bits = dc[0] + (ac[0xF1] + '1') * 5
    bits += '1' * (-len(bits) % 8) + '1' * 64
    raw = bytes(int(bits[i:i + 8], 2) for i in range(0, len(bits), 8)).replace(b'\xff', b'\xff\x00')
    out.append(('runs past coefficient 63', Entry(gray.desc, raw, [[0, len(raw)]])))
    # an AC size above 10 cannot be coded with the encoder's tables; a DC category above 11 neither
    assert [w for w, _ in out][3] == 'a segment cut at its last byte' and len(out) == 5
    return out


def test_ill_formed_streams_give_a_status_and_touch_nothing_else(dev, fixture):
    bad = _bad_entries(fixture)
    want = [_ref_status(e) for _, e in bad]
    assert all(want), list(zip([w for w, _ in bad], want))
    assert want[0] and want[2] == jpeg_ref.SEGMENT_END and want[4] == jpeg_ref.COEF_INDEX
    good = [3, 34, 59, 70, 83]
    entries = []
    for j, k in enumerate(good):  # each bad file between good ones
        entries.append(fixture[k][1])
        entries.append(bad[j][1])
    images, status, clean = run(dev, entries)
    assert clean, 'a byte outside the outputs changed'
    for j, k in enumerate(good):
        assert status[2 * j] == 0 and np.array_equal(images[2 * j], fixture[k][2]), fixture[k][0]
        assert status[2 * j + 1] != 0, bad[j][0]
        assert status[2 * j + 1] == want[j], (bad[j][0], int(status[2 * j + 1]), want[j])  # one segment, one problem


def test_out_of_range_coefficients_are_given_up(dev, fixture):
    """A DC-only 8 x 8 gray block of 2047 * 255: the dequantized coefficient leaves int16, where libjpeg-turbo's
    SIMD code wraps; with a table value of 16 it fits and the IDCT result leaves [-512, 511]."""
    gray = {n: e for n, e, _ in fixture}['8x8_gray_q100_opt0_rst0_smooth']
    dc, ac = _codes(gray.desc.dc[0]), _codes(gray.desc.ac[0])
    bits = dc[11] + '1' * 11 + ac[0]  # category 11, value 2047, end of block
    bits += '1' * (-len(bits) % 8)
    raw = bytes(int(bits[i:i + 8], 2) for i in range(0, len(bits), 8)).replace(b'\xff', b'\xff\x00')
    entries, want = [], []
    for q0, code in ((255, jpeg_ref.COEF_RANGE), (16, jpeg_ref.IDCT_RANGE)):
        desc = _lib.JpegDesc.from_buffer_copy(gray.desc)
        desc.qt[0][0] = q0
        entries.append(Entry(desc, raw, [[0, len(raw)]]))
        assert _ref_status(entries[-1]) == code
        want.append(code)
    images, status, clean = run(dev, entries + [gray])
    assert clean and status.tolist() == want + [0]


# ---- the drop-in classes

def _files(tmp_path, fixture):
    """The fixture's files plus a PNG, a progressive JPEG and a truncated JPEG -> (paths, index of the truncated)."""
    from PIL import Image
    paths = []
    for k in range(0, len(fixture), 3):
        paths.append(str(tmp_path / f'case{k}.jpg'))
        with open(paths[-1], 'wb') as f:
            f.write(fixture[k][1].data)
    rng = np.random.default_rng(3)
    rgb = rng.integers(0, 256, (40, 56, 3)).astype(np.uint8)
    paths.append(str(tmp_path / 'extra.png'))
    Image.fromarray(rgb, 'RGB').save(paths[-1])
    paths.append(str(tmp_path / 'progressive.jpg'))
    Image.fromarray(rgb, 'RGB').save(paths[-1], progressive=True)
    paths.append(str(tmp_path / 'face.jpg'))
    Image.fromarray(rgb[:, :, 0].repeat(2, 0)[:48, :48].copy(), 'L').save(paths[-1], quality=90)  # a 48 x 48 gray face
    paths.append(str(tmp_path / 'truncated.jpg'))
    with open(paths[-1], 'wb') as f:
        f.write(fixture[-1][1].data[:-200])
    return paths, len(paths) - 1


def test_image_inference_decode_gpu_equals_host(dev, fixture, tmp_path, monkeypatch):
    from inference.image_inference import ImageInference
    inf = ImageInference(seed=1234, device=dev, precision='f16', resize='gpu', convert='gpu', decode='gpu')
    assert inf.decode == 'gpu'
    paths, trunc = _files(tmp_path, fixture)
    good = paths[:trunc]
    inf.decode = 'host'
    inf.predict_files(paths)  # the handle's GEMM autotuner settles on these first passes
    for p in (paths[0], paths[5]):
        inf.predict(p)
    ref = inf.predict_files(paths)
    ref_feat = inf.extract_features_files(good)
    ref_one = [inf.predict(p) for p in (paths[0], paths[5], paths[trunc])]
    assert ref[trunc] == inf._fallback() and ref_one[2] == inf._fallback()
    assert sum(d == inf._fallback() for d in ref) == 1

    uploaded = []
    real = engine.ingest_ragged_files

    def spy(items, device=None):
        uploaded.append(sum(isinstance(it, mjpeg.Blob) for it in items))
        return real(items, device)

    monkeypatch.setattr(engine, 'ingest_ragged_files', spy)
    inf.decode = 'gpu'
    got = inf.predict_files(paths)
    assert uploaded == [trunc - 2]  # every fixture file and the face went up undecoded; the PNG and the progressive did not
    got_feat = inf.extract_features_files(good)
    assert got == ref
    for g, r in zip(got_feat, ref_feat):
        assert g.dtype == r.dtype and g.shape == r.shape and np.array_equal(g, r)
    assert [inf.predict(p) for p in (paths[0], paths[5], paths[trunc])] == ref_one
    f, q = inf.extract_features(paths[5])
    inf.decode = 'host'
    f0, q0 = inf.extract_features(paths[5])
    assert np.array_equal(f, f0) and np.array_equal(q, q0)
    # a single file is its batch row: same label, probabilities within the f16 path's 1e-3 of the oracle, twice
    for k in (0, 5):
        one = ref_one[(0, 5).index(k)]
        assert one['emotion'] == ref[k]['emotion']
        assert np.allclose(one['all_probabilities'], ref[k]['all_probabilities'], atol=2e-3)
    with pytest.raises(Exception):
        inf.extract_features_files([paths[trunc]])
    assert inf.predict_files([]) == []


def test_a_file_the_kernels_give_up_takes_the_host_route(dev, fixture, tmp_path):
    """A file that passes the probe and whose scan is damaged (bytes zeroed in the middle): whatever the kernels
    make of it, the result is decode='host''s, which is Pillow's reading of the same bytes."""
    from inference.image_inference import ImageInference
    inf = ImageInference(seed=1234, device=dev, precision='f16', resize='gpu', convert='gpu', decode='gpu')
    name, e, _ = fixture[81]
    assert name.startswith('64x80_422') and '_rst0_' in name
    lo, n = (int(v) for v in e.segs[0])
    damaged = bytearray(e.data)
    damaged[lo + n // 2:lo + n // 2 + 8] = bytes(8)
    assert mjpeg.probe(bytes(damaged)) is not None
    paths = []
    for k, d in enumerate((fixture[10][1].data, bytes(damaged), fixture[40][1].data)):
        paths.append(str(tmp_path / f'f{k}.jpg'))
        with open(paths[-1], 'wb') as f:
            f.write(d)
    got = inf.predict_files(paths)
    inf.decode = 'host'
    inf.predict_files(paths)
    assert got == inf.predict_files(paths)


def test_multimodal_fusion_image_decode_gpu_equals_host(dev, fixture, tmp_path, monkeypatch):
    from inference.multimodal_fusion import MultimodalFusion
    from oracle import audio as oa
    from test_gpu_dropin import TEXTS, _legacy_tokenizer, _stub_audio, _write_vocab
    fusion = MultimodalFusion(seed=1234, device=dev, precision='f16', image_resize='gpu', image_convert='gpu',
                              image_decode='gpu')
    assert fusion.image_inference.decode == 'gpu'
    waves = {f'clip{i}.wav': w for i, w in enumerate(oa.synthetic_clips(2, seed=51))}
    _stub_audio(monkeypatch, waves)
    fusion.text_inference.tokenizer = _legacy_tokenizer(_write_vocab(tmp_path))
    paths, _ = _files(tmp_path, fixture)
    png, face = paths[-4], paths[-2]
    clips = list(waves)
    reqs = [(clips[0], TEXTS[0], paths[27]), (None, TEXTS[1], face), (clips[1], None, png), (None, None, paths[2]),
            (clips[0], TEXTS[1], paths[16]), (clips[1], TEXTS[0], None)]
    fusion.predict_multimodal_batch(reqs)  # the handles' GEMM autotuners settle on this first pass
    got = fusion.predict_multimodal_batch(reqs)
    one = fusion.predict_multimodal(None, None, paths[27])
    fusion.image_inference.decode = 'host'
    ref = fusion.predict_multimodal_batch(reqs)
    assert len(got) == 6 and got == ref
    assert 'attention_weights' in got[0]['fusion'] and list(got[3]) == ['image'] and 'image' not in got[5]
    assert one == fusion.predict_multimodal(None, None, paths[27])


def test_constructor_rejects_decode_without_the_gpu_front_end():
    from inference.image_inference import ImageInference
    from inference.multimodal_fusion import MultimodalFusion
    for kw in (dict(decode='gpu'), dict(decode='gpu', resize='gpu'), dict(decode='gpu', convert='gpu'),
               dict(decode='device', resize='gpu', convert='gpu')):
        with pytest.raises(ValueError):
            ImageInference(seed=None, **kw)
    with pytest.raises(ValueError):
        MultimodalFusion(seed=None, image_decode='gpu')
