"""CPU: the JPEG front end's host side (csrc/jpeg_probe.h, csrc/jpeg.hip). The restatement
(tests/jpeg_ref.py) against Pillow 12.2's recorded digests and against the installed Pillow where it runs on
libjpeg-turbo; the probe's routing and descriptors, library against restatement; and the decode entry's checks,
which all precede the first device call and so run without a GPU."""
import ctypes
import hashlib
import io

import numpy as np
import pytest

import jpeg_ref
from mec import _lib, jpeg as mjpeg


@pytest.fixture(scope='module')
def cases(golden):
    z = golden('jpeg_cases.npz')
    data = z['data'].tobytes()
    offs = z['offs']
    return [(str(n), data[offs[k]:offs[k + 1]], tuple(z['hw'][k]), int(z['chan'][k]), str(z['sha'][k]))
            for k, n in enumerate(z['names'])]


def test_restatement_reproduces_every_digest(cases):
    assert len(cases) == 84
    for name, data, hw, chan, sha in cases:
        desc, st, px = jpeg_ref.decode_file(data)
        assert desc is not None and st == 0, name
        assert px.shape == hw + (chan,), name
        assert hashlib.sha256(px.tobytes()).hexdigest() == sha, name


def _encode(a, **kw):
    from PIL import Image
    f = io.BytesIO()
    Image.fromarray(a[..., 0] if a.shape[2] == 1 else a, 'L' if a.shape[2] == 1 else 'RGB').save(f, 'JPEG', **kw)
    return f.getvalue()


def _pil(data):
    from PIL import Image
    a = np.asarray(Image.open(io.BytesIO(data)))
    return a[..., None] if a.ndim == 2 else a


def _image(H, W, C, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    a = np.stack([(5 * yy + 3 * xx + 60 * c) % 256 for c in range(C)], -1) + rng.integers(-20, 21, (H, W, C))
    return np.clip(a, 0, 255).astype(np.uint8)


def test_restatement_equals_live_pillow_on_width_sweep():
    features = pytest.importorskip('PIL.features')
    if not features.check_feature('libjpeg_turbo'):
        pytest.skip('the installed Pillow does not decode with libjpeg-turbo')
    for sub in (1, 2):
        for H in (2, 17):
            for W in list(range(5, 82)) + [127, 128, 129, 130]:
                data = _encode(_image(H, W, 3, W * 7 + H), quality=(30, 75, 95)[W % 3], subsampling=sub,
                               restart_marker_blocks=(0, 1, 3)[(W + H) % 3])
                desc, st, px = jpeg_ref.decode_file(data)
                assert desc is not None and st == 0, (sub, H, W)
                assert np.array_equal(px, _pil(data)), (sub, H, W)


def _same_desc(blob, ref):
    d = blob.desc
    assert (d.H, d.W, d.ncomp, d.restart, d.nseg) == (ref.H, ref.W, ref.ncomp, ref.restart, len(ref.segs))
    for c in range(ref.ncomp):
        assert (d.hs[c], d.vs[c]) == (ref.hs[c], ref.vs[c])
        assert list(d.qt[c]) == ref.qt[c]
        for got, want in ((d.dc[c], ref.dc[c]), (d.ac[c], ref.ac[c])):
            assert list(got.counts) == want[0] and list(got.vals)[:len(want[1])] == want[1]
    assert blob.segs.tolist() == [list(s) for s in ref.segs]


def test_probe_gives_the_restatements_descriptors(cases):
    for name, data, hw, chan, _ in cases:
        blob, ref = mjpeg.probe(data, seg_cap=4), jpeg_ref.probe(data)  # a small seg_cap: the second call
        assert blob is not None and ref is not None, name
        _same_desc(blob, ref)
        assert (blob.H, blob.W, blob.C) == hw + (chan,)
        sampling = {'gray': (1, 1), '444': (1, 1), '422': (2, 1), '420': (2, 2)}[name.split('_')[1]]
        assert (blob.desc.hs[0], blob.desc.vs[0]) == sampling, name
        if 'rst1' in name and chan == 3:
            mx = -(-hw[1] // (8 * sampling[0]))
            my = -(-hw[0] // (8 * sampling[1]))
            assert blob.desc.restart == 1 and blob.desc.nseg == mx * my, name


def _both(data):
    a, b = mjpeg.probe(data), jpeg_ref.probe(data)
    assert (a is None) == (b is None)
    return a


def test_probe_routes_to_the_host():
    Image = pytest.importorskip('PIL.Image')
    rgb = _image(24, 40, 3, 1)
    assert _both(_encode(rgb, quality=80)) is not None
    assert _both(_encode(rgb, quality=80, progressive=True)) is None
    base = _encode(rgb, quality=80, subsampling=1)
    sof = base.index(b'\xff\xc0')
    assert base[sof + 11] == 0x21  # luma 2 x 1; the probe reads the header only
    for sampling in (0x12, 0x41, 0x22, 0x11, 0x21):  # 4:4:0 and 4:1:1 go to the host
        assert (_both(base[:sof + 11] + bytes([sampling]) + base[sof + 12:]) is None) == (sampling in (0x12, 0x41))
    f = io.BytesIO()
    Image.fromarray(np.dstack([rgb, rgb[..., :1]]), 'CMYK').save(f, 'JPEG')
    assert _both(f.getvalue()) is None
    for sub in (1, 2):
        assert _both(_encode(_image(9, 4, 3, 2), subsampling=sub)) is None  # subsampled, W = 4
        assert _both(_encode(_image(9, 5, 3, 2), subsampling=sub)) is not None
    assert _both(_encode(_image(9, 4, 3, 2), subsampling=0)) is not None
    assert _both(_encode(_image(301, 3, 1, 3))) is None  # outside the GPU resize's domain
    assert _both(b'') is None and _both(b'\xff\xd8') is None and _both(b'\x89PNG\r\n\x1a\n' + bytes(40)) is None


def test_probe_rejects_damaged_restart_markers_and_foreign_segments():
    data = _encode(_image(16, 48, 3, 4), quality=75, subsampling=2, restart_marker_blocks=1)
    blob = _both(data)
    assert blob is not None and blob.desc.nseg == 3
    at = [i for i in range(blob.span[0], len(data) - 1) if data[i] == 0xFF and 0xD0 <= data[i + 1] <= 0xD7]
    assert len(at) == 2
    removed = data[:at[0]] + data[at[0] + 2:]
    assert _both(removed) is None  # a restart marker removed: wrong count
    swapped = bytearray(data)
    swapped[at[0] + 1], swapped[at[1] + 1] = swapped[at[1] + 1], swapped[at[0] + 1]
    assert _both(bytes(swapped)) is None  # out of cyclic order
    filled = data[:at[0]] + b'\xff\xff' + data[at[0]:]
    ok = _both(filled)  # fill bytes before a marker are skipped
    assert ok is not None and ok.segs[0].tolist() == blob.segs[0].tolist() and ok.segs[1, 0] == blob.segs[1, 0] + 2
    assert _both(data[:-2]) is None and _both(data[:-2] + b'\xff\xda') is None  # no EOI; a second scan
    adobe = data[:2] + b'\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x00' + data[2:]
    assert _both(adobe) is None
    comment = data[:2] + b'\xff\xfe\x00\x05abc' + data[2:]
    assert _both(comment) is not None
    sof = data.index(b'\xff\xc0')
    twelve = bytearray(data)
    twelve[sof + 4] = 12
    assert _both(bytes(twelve)) is None
    dnl = bytearray(data)
    dnl[sof + 5:sof + 7] = b'\x00\x00'  # H = 0: the height comes in a DNL segment
    assert _both(bytes(dnl)) is None


def test_probe_header_cut_at_every_byte(cases):
    for name, data, *_ in cases[::9]:
        for n in range(len(data)):
            assert _both(data[:n]) is None, (name, n)


def test_probe_is_safe_on_arbitrary_bytes(cases):
    rng = np.random.default_rng(5)
    data = cases[40][1]
    for _ in range(300):
        b = bytearray(data)
        for _ in range(int(rng.integers(1, 4))):
            b[int(rng.integers(2, len(b)))] = int(rng.integers(0, 256))
        _both(bytes(b))  # the library and the restatement agree on what stays on the GPU
    lib = _lib.load()
    d = _lib.JpegDesc()
    assert lib.mec_jpeg_probe(None, 0, ctypes.byref(d), None, 0) == -1 and b'null' in lib.mec_last_error()
    assert lib.mec_jpeg_probe(data, len(data), None, None, 0) == -1
    assert lib.mec_jpeg_probe(data, len(data), ctypes.byref(d), None, 4) == -1 and b'seg_cap' in lib.mec_last_error()
    assert lib.mec_jpeg_probe(data, len(data), ctypes.byref(d), None, 0) == 1 and d.nseg >= 1


# ---- mec_jpeg_decode_ragged's preconditions: fake device pointers, never touched

def _good(cases):
    blobs = [mjpeg.probe(cases[k][1]) for k in (38, 61)]
    segs, src_bytes = [], 0
    for b in blobs:
        segs.append(b.segs + np.array([[src_bytes, 0]], np.int64))
        src_bytes += (len(b.data) + 15) // 16 * 16
    sizes = [(b.out_bytes + 15) // 16 * 16 for b in blobs]
    return dict(blobs=blobs, segs=np.concatenate(segs), src_bytes=src_bytes, dst_offs=[0, sizes[0]],
                dst_bytes=sum(sizes), ws_bytes=mjpeg.workspace_bytes([b.desc for b in blobs]))


def _call(lib, blobs, segs, src_bytes, dst_offs, dst_bytes, ws_bytes, B=None, src=0x100000, dst=0x200000, ws=0x300000,
          status=0x400000, null=(), edit=None):
    descs = mjpeg.desc_array([b.desc for b in blobs])
    if edit:
        edit(descs)
    segs = np.ascontiguousarray(segs, np.int64)
    dst_offs = np.asarray(dst_offs, np.int64)
    p = {'src': src, 'descs': ctypes.addressof(descs), 'segs': segs.ctypes.data, 'dst': dst, 'dst_offs': dst_offs.ctypes.data,
         'ws': ws, 'status': status}
    for k in null:
        p[k] = None
    return lib.mec_jpeg_decode_ragged(p['src'], src_bytes, p['descs'], p['segs'], len(blobs) if B is None else B, p['dst'],
                                      p['dst_offs'], dst_bytes, p['ws'], ws_bytes, p['status'], None)


def _set(i, field, value, index=None):
    def edit(descs):
        if index is None:
            setattr(descs[i], field, value)
        else:
            getattr(descs[i], field)[index] = value
    return edit


def _bad_huffman(descs):
    descs[0].dc[0].counts[0] = 3  # three codes of one bit


BAD = {
    'B < 0': (dict(B=-1), b'B < 0'),
    'B > 65535': (dict(B=65536), b'at most 65535'),
    'null src': (dict(null=('src',)), b'null'),
    'null descs': (dict(null=('descs',)), b'null'),
    'null segs': (dict(null=('segs',)), b'null'),
    'null dst': (dict(null=('dst',)), b'null'),
    'null dst_offs': (dict(null=('dst_offs',)), b'null'),
    'null ws': (dict(null=('ws',)), b'null'),
    'null status': (dict(null=('status',)), b'null'),
    'misaligned dst': (dict(dst=0x200004), b'dst must be 16-byte aligned'),
    'misaligned ws': (dict(ws=0x300008), b'ws must be 16-byte aligned'),
    'ncomp 2': (dict(edit=_set(1, 'ncomp', 2)), b'image 1 has ncomp 2'),
    'H = 0': (dict(edit=_set(0, 'H', 0)), b'image 0 is 0 x'),
    'W = 4097': (dict(edit=_set(0, 'W', 4097)), b'outside'),
    'luma 1 x 2': (dict(edit=lambda d: (_set(0, 'hs', 1, 0)(d), _set(0, 'vs', 2, 0)(d))), b'image 0 has a sampling'),
    'chroma 2 x 1': (dict(edit=_set(0, 'hs', 2, 1)), b'image 0 has a sampling'),
    'Huffman counts': (dict(edit=_bad_huffman), b'image 0 has a Huffman table'),
    'quantization value': (dict(edit=lambda d: d[1].qt[0].__setitem__(5, 256)), b'image 1 has a quantization value'),
    'restart < 0': (dict(edit=_set(0, 'restart', -1)), b'restart interval'),
    'segment count': (dict(edit=lambda d: setattr(d[1], 'nseg', d[1].nseg + 1)), b'segments where its MCUs'),
    'restart without its segments': (dict(edit=_set(0, 'restart', 1)), b'image 0 has'),
    'segment past src_bytes': (dict(src_bytes=100), b'segment that does not lie inside src_bytes'),
    'negative segment offset': (dict(segs='negated'), b'image 0 has a segment'),
    'negative dst_off': (dict(dst_offs=[-16, 4096]), b'image 0 has a dst_off'),
    'misaligned dst_off': (dict(dst_offs=[0, 4100]), b'image 1 has a dst_off'),
    'output past dst_bytes': (dict(dst_bytes=100), b'does not lie inside dst_bytes'),
    'overlapping outputs': (dict(dst_offs=[0, 16]), b'overlaps'),
    'output over a segment': (dict(dst=0x100000), b'overlaps'),
    'workspace over an output': (dict(ws=0x200000), b'overlaps'),
    'short workspace': (dict(ws_bytes='one short'), b'ws_bytes'),
}


@pytest.mark.parametrize('case', list(BAD))
def test_decode_entry_rejects_invalid_arguments_without_gpu(cases, case):
    """Every check precedes the first device call: the fake device pointers are never touched."""
    lib = _lib.load()
    good = _good(cases)
    assert good['blobs'][0].C == 3 and good['blobs'][0].desc.restart == 0, 'the cases below edit a colour file without restarts'
    kw, msg = BAD[case]
    kw = dict(kw)
    if isinstance(kw.get('segs'), str):
        kw['segs'] = good['segs'] * np.array([[-1, 1]], np.int64)
    if isinstance(kw.get('ws_bytes'), str):
        kw['ws_bytes'] = good['ws_bytes'] - 1
    if case == 'overlapping outputs':
        kw['dst_bytes'] = 1 << 20
    if case == 'output over a segment':
        kw['src_bytes'] = 1 << 20
    assert _call(lib, **{**good, **kw}) == -1
    err = lib.mec_last_error()
    assert err.startswith(b'requirement failed: mec_jpeg_decode_ragged') and msg in err, err


def test_decode_entry_empty_batch_and_workspace_without_gpu(cases):
    lib = _lib.load()
    assert lib.mec_jpeg_decode_ragged(None, 0, None, None, 0, None, None, 0, None, 0, None, None) == 0
    assert lib.mec_jpeg_workspace_bytes(None, 0) == 0
    assert lib.mec_jpeg_workspace_bytes(None, 1) == -1
    for name, data, hw, chan, _ in cases:
        b = mjpeg.probe(data)
        h, v = b.desc.hs[0], b.desc.vs[0]
        mx, my = -(-hw[1] // (8 * h)), -(-hw[0] // (8 * v))
        assert mjpeg.workspace_bytes([b.desc]) == 192 * mx * my * (1 if chan == 1 else h * v + 2), name
    bad = mjpeg.probe(cases[0][1]).desc
    bad.ncomp = 4
    with pytest.raises(_lib.MecError, match='image 0 has ncomp 4'):
        mjpeg.workspace_bytes([bad])
