"""Time the image path from decoded images to probabilities with resize='host', resize='gpu' and
resize='gpu' + convert='gpu'.

    python3 tools/bench_image_frontend.py --out profiles/image_frontend_convert_bench.json

Everything is measured on the GPU host in one run. Four workloads of --batch seeded images: 'uniform' (RGB u8
arrays, every image 480 x 640), 'ragged' (RGB arrays, sides U[96, 1080], one image in ten gray), 'rgba' (PIL
images of mode RGBA, 480 x 640) and 'gray_rgb' (480 x 640 gray photos stored as RGB arrays).
ImageInference.predict_arrays (ResNet50 f16; for the PIL images route + forward_routed, which is what predict_arrays
runs) runs on each with the three settings alternating in one process, after a warm-up; a host clock
runs from the list of images to the result dicts (so it ends behind a device synchronisation). A window is
--repeats alternating calls per setting and gives each setting's median; --windows windows are taken and their
median, minimum and maximum reported. The results of the three settings are asserted equal first.

Also reported per workload: the resize step alone on the host clock (host: PIL's resize of every image and the
upload of the u8 224 x 224 batch; gpu: engine.resize_ragged, pack + one copy + two kernels, synchronised), and
the two kernels' device-event times (mec_resize_prof_*) with the bytes each must move: the horizontal pass
reads sum H W C and writes sum H 224 C, the vertical pass reads sum H 224 C and writes B 224 224 C. For the
convert='gpu' setting: engine.ingest_ragged alone on the host clock (pack, one copy, the gray kernel, the flags'
read-back, the conversion kernel, the resizes), and the gray and conversion kernels' device-event times
(mec_image_canon_prof_*) with their bytes: the gray kernel reads the RGB / RGBA / P images, the conversion kernel
reads the images it converts and writes H W c_out for each.

The decode comparison (--decode-kinds) goes from files to probabilities, ImageInference.predict_files with decode='gpu'
against decode='host' (both with resize='gpu' and convert='gpu') alternating in the same run: 'jpeg_420' is --batch
480 x 640 4:2:0 quality-75 JPEG files of smooth-plus-noise synthetic content, 'jpeg_face' --batch 48 x 48 gray
JPEG files, all made by Pillow at run time in a temporary directory. Also reported: the file bytes, the restart
segments (one wave each in the entropy kernel), engine.decode_jpeg_ragged alone on the host clock and the three
kernels' device-event times per call (mec_jpeg_prof_*).
Prints one JSON line; --out also writes it to a file.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'multimodal-emotion-classification_amd'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mec import engine  # noqa: E402


KINDS = ('uniform', 'ragged', 'rgba', 'gray_rgb')
SETTINGS = {'host': ('host', 'host'), 'gpu': ('gpu', 'host'), 'gpu_convert': ('gpu', 'gpu')}  # (resize, convert)


def make_images(kind, B, rng):
    out = []
    for _ in range(B):
        H, W = (int(rng.integers(96, 1081)), int(rng.integers(96, 1081))) if kind == 'ragged' else (480, 640)
        a = rng.integers(0, 256, (H, W, 4 if kind == 'rgba' else 3), dtype=np.uint8)
        if kind == 'gray_rgb' or (kind == 'ragged' and rng.random() < 0.1):
            a = np.repeat(a[..., :1], 3, axis=2)
        if kind == 'rgba':
            from PIL import Image
            a = Image.fromarray(a, 'RGBA')
        out.append(a)
    return out


def clock(fn, device):
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize(device)
    return (time.perf_counter() - t0) * 1e3, r


def windows(fns, n_windows, repeats, device):
    """fns: {setting: callable}. -> {setting: per-window medians (ms)}, the settings alternating call by call."""
    med = {k: [] for k in fns}
    for _ in range(n_windows):
        ms = {k: [] for k in fns}
        for _ in range(repeats):
            for k, fn in fns.items():
                ms[k].append(clock(fn, device)[0])
        for k in fns:
            med[k].append(statistics.median(ms[k]))
    return med


def summary(meds, B):
    m = statistics.median(meds)
    return {'ms_per_batch': m, 'window_medians_min_max': [min(meds), max(meds)], 'images_per_s': B / m * 1e3}


def host_resize(arrays, device):
    from PIL import Image
    r = np.stack([np.asarray(Image.fromarray(a, 'RGB').resize((224, 224), Image.BILINEAR)) for a in arrays])
    return engine.to_device(r, device)


def kernel_events(arrays, device, iters):
    """Device-event time of the two kernels per call (the upload and the host packing are outside the events)."""
    for _ in range(3):
        engine.resize_ragged(arrays, device)
    torch.cuda.synchronize(device)
    engine.resize_prof(True)
    for _ in range(iters):
        engine.resize_ragged(arrays, device)
    torch.cuda.synchronize(device)
    h_ms, v_ms, n = engine.resize_prof_read()
    engine.resize_prof(False)
    assert n == iters
    C = arrays[0].shape[2]
    src = sum(a.shape[0] * a.shape[1] * C for a in arrays)
    tmp = sum(a.shape[0] * 224 * C for a in arrays)
    out = len(arrays) * 224 * 224 * C
    h, v = h_ms / n, v_ms / n
    return {'iters': n,
            'horizontal': {'ms': h, 'bytes_read': src, 'bytes_written': tmp, 'GB_per_s': (src + tmp) / h / 1e6},
            'vertical': {'ms': v, 'bytes_read': tmp, 'bytes_written': out, 'GB_per_s': (tmp + out) / v / 1e6}}


def canon_events(inf, images, device, iters):
    """engine.ingest_ragged on what convert='gpu' hands it: the host clock of the call, and the device-event time
    of the gray and conversion kernels per call with the bytes they move."""
    from mec import image as mimage
    inf.resize, inf.convert = SETTINGS['gpu_convert']
    route = inf.route if not isinstance(images[0], np.ndarray) else inf.route_array
    items = [tuple(route(x)) for x in images]
    assert all(len(it) == 3 for it in items)
    for _ in range(3):
        gray, _ = engine.ingest_ragged(items, device)
    host_ms = [clock(lambda: engine.ingest_ragged(items, device), device)[0] for _ in range(iters)]
    torch.cuda.synchronize(device)
    engine.canon_prof(True)
    for _ in range(iters):
        engine.ingest_ragged(items, device)
    torch.cuda.synchronize(device)
    g_ms, g_n, c_ms, c_n = engine.canon_prof_read()
    engine.canon_prof(False)
    scan = conv_r = conv_w = 0
    for (a, fmt, _), g in zip(items, gray):
        hw = a.shape[0] * a.shape[1]
        if fmt not in (mimage.PIX_L, mimage.PIX_LA):
            scan += hw * mimage.PIX_BPP[fmt]
        face = g and a.shape[:2] == (48, 48)
        asis = not face and ((fmt == mimage.PIX_L and g) or (fmt == mimage.PIX_RGB and not g))
        if not asis:
            conv_r += hw * mimage.PIX_BPP[fmt]
            conv_w += hw * (1 if g else 3)
    out = {'iters': iters, 'gray_images': int(gray.sum()), 'upload_bytes': sum(a.size for a, _, _ in items),
           'ingest_ragged_host_clock_ms': {'median': statistics.median(host_ms), 'min_max': [min(host_ms), max(host_ms)]},
           'gray_kernel': {'launches': g_n, 'bytes_read': scan},
           'canon_kernel': {'launches': c_n, 'bytes_read': conv_r, 'bytes_written': conv_w}}
    if g_n:
        out['gray_kernel'].update(ms=g_ms / g_n, GB_per_s=scan / (g_ms / g_n) / 1e6)
    if c_n:
        out['canon_kernel'].update(ms=c_ms / c_n, GB_per_s=(conv_r + conv_w) / (c_ms / c_n) / 1e6)
    return out


DECODE_KINDS = ('jpeg_420', 'jpeg_face')


def make_files(kind, B, rng, folder):
    """B JPEG files made by Pillow: smooth content (a few sinusoids per channel) plus noise."""
    from PIL import Image
    H, W = (480, 640) if kind == 'jpeg_420' else (48, 48)
    C = 3 if kind == 'jpeg_420' else 1
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    paths = []
    for i in range(B):
        a = np.zeros((H, W, C), np.float32)
        for c in range(C):
            fy, fx, ph = rng.uniform(0.5, 4, 2), rng.uniform(0.5, 4, 2), rng.uniform(0, 6.28, 2)
            a[..., c] = 128 + 50 * np.sin(fy[0] * yy / H * 6.28 + ph[0]) * np.cos(fx[0] * xx / W * 6.28) \
                + 40 * np.sin(fx[1] * xx / W * 6.28 + fy[1] * yy / H * 6.28 + ph[1])
        a = np.clip(a + rng.normal(0, 6, a.shape), 0, 255).astype(np.uint8)
        paths.append(os.path.join(folder, f'{kind}_{i}.jpg'))
        if C == 3:
            Image.fromarray(a, 'RGB').save(paths[-1], quality=75, subsampling=2)
        else:
            Image.fromarray(a[..., 0], 'L').save(paths[-1], quality=75)
    return paths


def decode_bench(inf, kind, a, dev, rng):
    from mec import jpeg as mjpeg
    B = a.batch
    with tempfile.TemporaryDirectory() as folder:
        paths = make_files(kind, B, rng, folder)
        inf.resize, inf.convert = 'gpu', 'gpu'

        def predict(decode):
            inf.decode = decode
            return inf.predict_files(paths)

        fns = {k: (lambda k=k: predict(k)) for k in ('host', 'gpu')}
        for _ in range(a.warmup):
            got = {k: fn() for k, fn in fns.items()}
        assert got['host'] == got['gpu'], f'{kind}: the settings disagree'
        med = windows(fns, a.windows, a.repeats, dev)
        blobs = []
        for p in paths:
            with open(p, 'rb') as f:
                blobs.append(mjpeg.probe(f.read()))
        inf.decode = 'host'
    assert all(b is not None for b in blobs), f'{kind}: a file is outside the GPU decoder\'s domain'
    for _ in range(3):
        _, status = engine.decode_jpeg_ragged(blobs, dev)
    assert not status.cpu().numpy().any()
    host_ms = [clock(lambda: engine.decode_jpeg_ragged(blobs, dev), dev)[0] for _ in range(a.event_iters)]
    engine.jpeg_prof(True)
    for _ in range(a.event_iters):
        engine.decode_jpeg_ragged(blobs, dev)
    torch.cuda.synchronize(dev)
    e_ms, i_ms, c_ms, n = engine.jpeg_prof_read()
    engine.jpeg_prof(False)
    assert n == a.event_iters
    out_bytes = sum(b.out_bytes for b in blobs)
    ws = mjpeg.workspace_bytes([b.desc for b in blobs])
    return {'files': B, 'file_bytes': sum(len(b.data) for b in blobs), 'scan_bytes': sum(b.span[1] - b.span[0] for b in blobs),
            'restart_segments': sum(len(b.segs) for b in blobs), 'decoded_bytes': out_bytes, 'workspace_bytes': ws,
            'files_to_probabilities': {k: summary(med[k], B) for k in med},
            'gpu_over_host_speedup': statistics.median(med['host']) / statistics.median(med['gpu']),
            'decode_jpeg_ragged_host_clock_ms': {'median': statistics.median(host_ms), 'min_max': [min(host_ms), max(host_ms)]},
            'kernels_ms_per_call': {'iters': n, 'entropy': e_ms / n, 'idct': i_ms / n, 'colour': c_ms / n}}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--repeats', type=int, default=3, help='alternating calls per setting in a window')
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--event-iters', type=int, default=20)
    ap.add_argument('--kinds', default=','.join(KINDS), help='comma-separated workloads')
    ap.add_argument('--decode-kinds', default=','.join(DECODE_KINDS), help='comma-separated file workloads (may be empty)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_image_frontend: no GPU visible (nothing is measured on the CPU)')
    import PIL
    from inference.image_inference import ImageInference
    dev = torch.device('cuda', 0)
    B = a.batch
    inf = ImageInference(seed=1234, device=dev, precision='f16', resize='gpu')  # the settings are switched per call
    res = {'device': torch.cuda.get_device_name(0), 'batch': B, 'windows': a.windows, 'repeats_per_window': a.repeats,
           'warmup': a.warmup, 'pillow': PIL.__version__, 'precision': 'f16', 'backbone': 'resnet50',
           'host_threads': torch.get_num_threads()}

    def predict(setting, images):
        inf.resize, inf.convert = SETTINGS[setting]
        if isinstance(images[0], np.ndarray):
            return inf.predict_arrays(images)
        probs = inf.forward_routed([inf.route(im) for im in images])[1].cpu().numpy()
        return [inf._as_dict(inf.emotions, p) for p in probs]

    rng = np.random.default_rng(0)
    for kind in [k for k in a.kinds.split(',') if k]:
        images = make_images(kind, B, rng)
        fns = {k: (lambda k=k: predict(k, images)) for k in SETTINGS}
        for _ in range(a.warmup):
            got = {k: fn() for k, fn in fns.items()}
        assert got['host'] == got['gpu'] == got['gpu_convert'], f'{kind}: the settings disagree'
        med = windows(fns, a.windows, a.repeats, dev)
        arrays = [np.ascontiguousarray(np.asarray(x)[..., :3]) for x in images]  # the RGB pixels the resize step works on
        rgb = [x for x in arrays if not (x[..., 0] == x[..., 1]).all()]  # one channel count per resize call
        parts = windows({'host': lambda: host_resize(rgb, dev), 'gpu': lambda: engine.resize_ragged(rgb, dev)},
                        a.windows, a.repeats, dev) if rgb else {}
        res[kind] = {'pixels_per_image_mean': float(np.mean([x.shape[0] * x.shape[1] for x in arrays])),
                     'gray_share': 1 - len(rgb) / B,
                     'arrays_to_probabilities': {k: summary(med[k], B) for k in med},
                     'gpu_over_host_speedup': statistics.median(med['host']) / statistics.median(med['gpu']),
                     'gpu_convert_over_gpu_speedup': statistics.median(med['gpu']) / statistics.median(med['gpu_convert']),
                     'convert_gpu': canon_events(inf, images, dev, a.event_iters),
                     'resize_only_rgb_images': {'images': len(rgb), **{k: summary(parts[k], len(rgb)) for k in parts}},
                     'kernels_rgb_images': kernel_events(rgb, dev, a.event_iters) if rgb else None}
    for kind in [k for k in a.decode_kinds.split(',') if k]:
        res[kind] = decode_bench(inf, kind, a, dev, rng)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
