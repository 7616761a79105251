"""Time the image path from in-memory u8 arrays to probabilities with resize='host' and resize='gpu'.

    python3 tools/bench_image_frontend.py --out profiles/image_frontend_bench.json

Everything is measured on the GPU host in one run. Two workloads of --batch seeded RGB u8 arrays: 'uniform'
(every image 480 x 640) and 'ragged' (sides U[96, 1080], one image in ten gray). ImageInference.predict_arrays
(ResNet50 f16) runs on each with the two settings alternating in one process, after a warm-up; a host clock
runs from the list of arrays to the result dicts (so it ends behind a device synchronisation). A window is
--repeats alternating calls per setting and gives each setting's median; --windows windows are taken and their
median, minimum and maximum reported. The results of the two settings are asserted equal first.

Also reported per workload: the resize step alone on the host clock (host: PIL's resize of every image and the
upload of the u8 224 x 224 batch; gpu: engine.resize_ragged, pack + one copy + two kernels, synchronised), and
the two kernels' device-event times (mec_resize_prof_*) with the bytes each must move: the horizontal pass
reads sum H W C and writes sum H 224 C, the vertical pass reads sum H 224 C and writes B 224 224 C.
Prints one JSON line; --out also writes it to a file.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'multimodal-emotion-classification_amd'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mec import engine  # noqa: E402


def make_images(kind, B, rng):
    out = []
    for _ in range(B):
        H, W = (480, 640) if kind == 'uniform' else (int(rng.integers(96, 1081)), int(rng.integers(96, 1081)))
        a = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        if kind == 'ragged' and rng.random() < 0.1:
            a = np.repeat(a[..., :1], 3, axis=2)
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


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--repeats', type=int, default=3, help='alternating calls per setting in a window')
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--event-iters', type=int, default=20)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_image_frontend: no GPU visible (nothing is measured on the CPU)')
    import PIL
    from inference.image_inference import ImageInference
    dev = torch.device('cuda', 0)
    B = a.batch
    inf = ImageInference(seed=1234, device=dev, precision='f16')
    res = {'device': torch.cuda.get_device_name(0), 'batch': B, 'windows': a.windows, 'repeats_per_window': a.repeats,
           'warmup': a.warmup, 'pillow': PIL.__version__, 'precision': 'f16', 'backbone': 'resnet50',
           'host_threads': torch.get_num_threads()}

    def predict(setting, arrays):
        inf.resize = setting
        return inf.predict_arrays(arrays)

    rng = np.random.default_rng(0)
    for kind in ('uniform', 'ragged'):
        arrays = make_images(kind, B, rng)
        fns = {k: (lambda k=k: predict(k, arrays)) for k in ('host', 'gpu')}
        for _ in range(a.warmup):
            got = {k: fn() for k, fn in fns.items()}
        assert got['host'] == got['gpu'], f'{kind}: the two settings disagree'
        med = windows(fns, a.windows, a.repeats, dev)
        rgb = [x for x in arrays if not (x[..., 0] == x[..., 1]).all()]  # one channel count per resize call
        parts = windows({'host': lambda: host_resize(rgb, dev), 'gpu': lambda: engine.resize_ragged(rgb, dev)},
                        a.windows, a.repeats, dev)
        res[kind] = {'pixels_per_image_mean': float(np.mean([x.shape[0] * x.shape[1] for x in arrays])),
                     'gray_share': 1 - len(rgb) / B,
                     'arrays_to_probabilities': {k: summary(med[k], B) for k in med},
                     'gpu_over_host_speedup': statistics.median(med['host']) / statistics.median(med['gpu']),
                     'resize_only_rgb_images': {'images': len(rgb), **{k: summary(parts[k], len(rgb)) for k in parts}},
                     'kernels_rgb_images': kernel_events(rgb, dev, a.event_iters)}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
