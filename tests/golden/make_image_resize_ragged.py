"""Writes tests/golden/image_resize_ragged.json: SHA-256 digests of what Pillow's
`Image.fromarray(a).resize((224, 224), Image.BILINEAR)` returns for the shapes and inputs of the ragged-resize
tests. No pixel data is stored: the inputs are tests/resize_ref.make_input, a closed formula of (y, x, c).

Run with the Pillow version the digests are to pin (12.2):  python tests/golden/make_image_resize_ragged.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, 'tests'), ROOT]

import resize_ref  # noqa: E402

# (H, W): every shape lies in the GPU resize's domain (H <= 100 W, sides 1..4096)
FIXED = [(1, 1), (1, 7), (7, 1), (5, 3), (100, 1), (200, 2), (48, 48),
         (223, 225), (225, 223), (224, 224), (449, 300), (300, 3),
         (2, 4096), (4096, 41), (37, 1000), (480, 640), (300, 449)]


def lcg_shapes(n=40, lo=48, hi=1200):
    """n shapes in [lo, hi]^2 from a linear congruential sequence (no RNG library, so the list is the formula's)."""
    s, out = 12345, []
    for _ in range(n):
        s = (s * 1103515245 + 12345) % (1 << 31)
        h = lo + (s >> 8) % (hi - lo + 1)
        s = (s * 1103515245 + 12345) % (1 << 31)
        out.append((h, lo + (s >> 8) % (hi - lo + 1)))
    return out


def main():
    import PIL
    from PIL import Image
    shapes = FIXED + lcg_shapes()
    cases = []
    for H, W in shapes:
        d = {}
        for p in resize_ref.PATTERNS:
            a = resize_ref.make_input(H, W, p)
            d[p] = resize_ref.digest(np.asarray(Image.fromarray(a, 'RGB').resize((224, 224), Image.BILINEAR)))
        cases.append({'H': H, 'W': W, 'sha256': d})
    with open(os.path.join(HERE, 'image_resize_ragged.json'), 'w') as f:
        json.dump({'pillow': PIL.__version__, 'target': [224, 224], 'filter': 'BILINEAR', 'cases': cases}, f, indent=1)
        f.write('\n')
    print(f'{len(cases)} shapes x {len(resize_ref.PATTERNS)} inputs, Pillow {PIL.__version__}')


if __name__ == '__main__':
    main()
