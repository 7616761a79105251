"""GPU: the BERT text path on attention masks that are no prefixes and on a peaked softmax, through the
model. Batch (tests/text_edits.py mask_batch): the ragged batch of seed 900 with rows 2-6 masked by
Bernoulli(0.5) holes (key 0 kept), only key 127, no key at all (transformers attends uniformly there:
finfo.min absorbs every score), all but key 0, only key 0. Reference: oracle.text.forward on the same
ids, mask and weights, at the project's bars -- f16: probs 1e-3, cls 1e-2 absolute; fp32 / fp32x3: probs
1e-5, cls 2e-5 relative to max |cls|; argmax equal on every row.

Sharpened weights: every layer's query and key weights x 4 (score std about 5, max |score| about 22).
The fp32 bars hold for the reference alone with room there (tests/test_oracle.py pins the fp32 oracle
against its float64 form on exactly this batch: cls 5.4e-6, probs 1.6e-6, smallest top-2 margin 0.14).
f16 has no derivable bar at x 4 (the kernel-level bound of tests/test_gpu_attention.py carries its
precision): finite outputs and the argmax on all 8 rows are asserted, the errors printed.
Measured on an MI355X, f16 at x 4: probs max|d| 8.9e-4, cls max|d| 4.5e-3 (8.6e-4 of max |cls|), argmax 8/8
(seeded weights on the same batch: probs 7.2e-4, cls 2.6e-3; fp32 / fp32x3 at x 4: probs 1.9e-6 / 3.2e-6, cls
1.1e-5 / 7.2e-6 absolute at max |cls| 5.2).
"""
import functools

import numpy as np
import pytest
import torch

from mec import engine, synthetic as syn
from oracle import text as o_t
from text_edits import mask_batch, sharpened_text

pytestmark = pytest.mark.gpu

PROB_TOL = {'f16': 1e-3, 'fp32': 1e-5, 'fp32x3': 1e-5}
F16_CLS_TOL, CLS_RTOL = 1e-2, 2e-5
DEFAULTS = {'bert_qkv_attn': 1, 'bert_cls_last': 1}  # csrc/mec_common.h


@functools.lru_cache(maxsize=None)
def _oracle(sharp):
    ids, mask = mask_batch()
    return o_t.forward(sharpened_text() if sharp else syn.weights('text'), ids, mask)


@pytest.fixture(scope='module')
def encoders(dev):
    made = {}

    def get(precision):
        if precision not in made:
            made[precision] = engine.TextEncoder(device=dev, precision=precision)
        return made[precision]
    yield get
    for m in made.values():
        m.close()


def _forward(enc, dev):
    ids, mask = mask_batch()
    out = enc.forward(engine.to_device(np.array(ids), dev), engine.to_device(np.array(mask), dev))
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def _errors(what, cls, probs, ref):
    rc, _, rp = ref
    dc, dp = float(np.abs(cls - rc).max()), float(np.abs(probs - rp).max())
    agree = int((probs.argmax(1) == rp.argmax(1)).sum())
    print(f'{what}: probs max|d| {dp:.3g}, cls max|d| {dc:.3g} ({dc / np.abs(rc).max():.3g} of max |cls|), '
          f'argmax {agree}/{len(rp)}')
    return dc, dp, agree


def _assert_bars(precision, what, cls, probs, ref):
    assert np.isfinite(cls).all() and np.isfinite(probs).all(), what
    dc, dp, agree = _errors(what, cls, probs, ref)
    assert agree == len(probs), what
    assert dp <= PROB_TOL[precision], what
    assert dc <= (F16_CLS_TOL if precision == 'f16' else CLS_RTOL * np.abs(ref[0]).max()), what


@pytest.mark.parametrize('cls_last', [0, 1])
@pytest.mark.parametrize('fused', [0, 1])
@pytest.mark.parametrize('precision', ['f16', 'fp32', 'fp32x3'])
def test_holed_masks_vs_oracle(encoders, dev, precision, fused, cls_last):
    enc = encoders(precision)
    enc.set_option('bert_qkv_attn', fused)
    enc.set_option('bert_cls_last', cls_last)
    try:
        cls, _, probs = _forward(enc, dev)
        enc.check()
    finally:
        for k, v in DEFAULTS.items():
            enc.set_option(k, v)
    _assert_bars(precision, f'{precision} bert_qkv_attn {fused} bert_cls_last {cls_last}', cls, probs, _oracle(False))


@pytest.mark.parametrize('precision', ['fp32', 'fp32x3'])
def test_sharpened_weights_vs_oracle(dev, precision):
    """Query / key weights x 4 at the fp32 bars; fp32x3's plane exponents follow the larger Q / K bounds, so
    check() stays clean, with the fused QKV + attention kernel and without it."""
    enc = engine.TextEncoder(sharpened_text(), device=dev, precision=precision)
    try:
        for fused in (1, 0):
            enc.set_option('bert_qkv_attn', fused)
            cls, _, probs = _forward(enc, dev)
            enc.check()
            _assert_bars(precision, f'{precision} x 4, bert_qkv_attn {fused}', cls, probs, _oracle(True))
    finally:
        enc.close()


def test_sharpened_weights_f16_argmax(dev):
    enc = engine.TextEncoder(sharpened_text(), device=dev, precision='f16')
    try:
        cls, _, probs = _forward(enc, dev)
    finally:
        enc.close()
    assert np.isfinite(cls).all() and np.isfinite(probs).all()
    _, _, agree = _errors('f16 x 4', cls, probs, _oracle(True))
    assert agree == len(probs)
