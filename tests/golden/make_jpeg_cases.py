"""Makes tests/golden/jpeg_cases.npz: encoder-made baseline JPEG files and the SHA-256 of the pixels Pillow decodes
from them (made with Pillow 12.2.0 on libjpeg-turbo; the digests pin that decoder's bytes, the files do not depend
on the decoder). Run from the repository root:  python tests/golden/make_jpeg_cases.py

names[k] says how file k was made; data holds the files back to back, file k at data[offs[k]:offs[k + 1]]; hw[k],
chan[k] its decoded shape; sha[k] the hex digest of its decoded u8 pixels [H, W, C]."""
import hashlib
import io
import os

import numpy as np
from PIL import Image

SIZES = [(1, 1), (7, 9), (8, 8), (15, 17), (16, 16), (17, 33), (33, 47), (48, 48), (3, 31), (31, 5), (64, 80)]  # (H, W)
MODES = [('gray', None), ('444', 0), ('422', 1), ('420', 2)]
QUALITY = [30, 75, 95, 100]
RESTART = [0, 1, 3, 'row']


def content(rng, H, W, C, smooth):
    yy, xx = np.mgrid[0:H, 0:W]
    if smooth:
        a = np.stack([(3 * yy + 2 * xx + 70 * c) % 256 for c in range(C)], -1) + rng.integers(-5, 6, (H, W, C))
    else:
        a = rng.integers(0, 256, (H, W, C))
    return np.clip(a, 0, 255).astype(np.uint8)


def cases():
    rng = np.random.default_rng(20261021)
    k = 0
    for H, W in SIZES:
        for mode, sub in MODES:
            if sub in (1, 2) and W < 5:
                continue  # outside the GPU decoder's domain
            for variant in range(2):
                q = QUALITY[(k + k // 4) % 4]
                opt = bool((k // 2) % 2)
                rst = RESTART[(k + k // 16 + 2 * variant) % 4]
                smooth = bool((k // 4) % 2)
                a = content(rng, H, W, 1 if sub is None else 3, smooth)
                im = Image.fromarray(a[..., 0], 'L') if sub is None else Image.fromarray(a, 'RGB')
                kw = {'quality': q, 'optimize': opt}
                if sub is not None:
                    kw['subsampling'] = sub
                if rst == 'row':
                    kw['restart_marker_rows'] = 1
                elif rst:
                    kw['restart_marker_blocks'] = rst
                f = io.BytesIO()
                im.save(f, 'JPEG', **kw)
                name = f'{H}x{W}_{mode}_q{q}_opt{int(opt)}_rst{rst}_{"smooth" if smooth else "random"}'
                yield name, f.getvalue()
                k += 1


def main():
    names, blobs, hw, chan, sha = [], [], [], [], []
    for name, data in cases():
        px = np.asarray(Image.open(io.BytesIO(data)))
        px = px[..., None] if px.ndim == 2 else px
        names.append(name)
        blobs.append(np.frombuffer(data, np.uint8))
        hw.append(px.shape[:2])
        chan.append(px.shape[2])
        sha.append(hashlib.sha256(np.ascontiguousarray(px).tobytes()).hexdigest())
    offs = np.cumsum([0] + [len(b) for b in blobs]).astype(np.int64)
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'jpeg_cases.npz')
    np.savez_compressed(out, names=np.array(names), data=np.concatenate(blobs), offs=offs, hw=np.array(hw, np.int32),
                        chan=np.array(chan, np.int32), sha=np.array(sha))
    print(len(names), 'files', int(offs[-1]), 'bytes ->', out, os.path.getsize(out), 'bytes')


if __name__ == '__main__':
    main()
