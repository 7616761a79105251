"""Edited copies of the seeded weights and the holed-mask text batch, shared by the tests that need them
(tests/test_gpu_fp32x3.py, tests/test_gpu_text_masks.py, tests/test_oracle.py). Test infrastructure only."""
import functools

import numpy as np

from mec import synthetic as syn


def edit(kind, edits):
    """A copy of the seeded weights with edits {name: factor | (index, value)} applied (syn.weights
    returns the cached dict every handle shares)."""
    w = dict(syn.weights(kind))
    for name, e in edits.items():
        a = np.array(w[name], np.float32)
        if isinstance(e, tuple):
            a.flat[e[0]] = e[1]
        else:
            a = (a * np.float32(e)).astype(np.float32)
        w[name] = a
    return w


SHARPEN = 4.0


@functools.lru_cache(maxsize=None)
def sharpened_text():
    """The seeded BERT with every layer's query and key weights x 4: score std about 5 and max |score| about
    22 in place of 0.3 and 1.7, the softmax of a fine-tuned checkpoint rather than a nearly flat one."""
    return edit('text', {f'bert.encoder.layer.{i}.attention.self.{n}.weight': SHARPEN
                         for i in range(12) for n in ('query', 'key')})


@functools.lru_cache(maxsize=None)
def mask_batch():
    """ids, mask [8, 128]: the ragged batch of seed 900 with the masks of rows 2-6 replaced by
    Bernoulli(0.5) holes (key 0 kept), only key 127, no key at all, all but key 0, only key 0. The ids stay."""
    ids, mask = syn.text_inputs(8, 128, seed=900, ragged=True)
    mask = mask.copy()
    mask[2] = np.random.default_rng(900).integers(0, 2, 128)
    mask[2, 0] = 1
    mask[3] = 0
    mask[3, 127] = 1
    mask[4] = 0
    mask[5] = 1
    mask[5, 0] = 0
    mask[6] = 0
    mask[6, 0] = 1
    for a in (ids, mask):
        a.setflags(write=False)
    return ids, mask
