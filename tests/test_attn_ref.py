"""CPU: the float64 attention reference of tests/attn_ref.py against torch's float64 softmax with the
additive finfo(f32).min mask, and the sensitivity of its bound: reference outputs mutated the way
attention kernels go wrong must be rejected on the peaked, planted and adversarial-mask inputs. What
the same mutations do to the diffuse inputs, all that the model-level tests ever produce, is printed:
their errors there are 100-1000 x smaller relative to the bound than on the other cases (at this
module's per-element bound they are still rejected; the model-level bars sit twelve layers away)."""
import numpy as np
import pytest
import torch

import attn_ref as ar


def _torch_ref(q, k, v, valid):
    """softmax(s + (1 - m) finfo(f32).min) @ v in float64 (finfo(f32).min absorbs a finite score in float64
    too: its ulp there is 7.6e22), batched over sequences and heads."""
    q, k, v = (torch.from_numpy(np.asarray(t, np.float64)) for t in (q, k, v))
    ext = (1.0 - torch.from_numpy(valid[:, None].astype(np.float64))) * torch.finfo(torch.float32).min
    return (torch.softmax(q @ k.transpose(-1, -2) / 8.0 + ext, dim=-1) @ v).numpy()


@pytest.mark.parametrize('name', ['random', 'holed', 'all_masked', 'segments'])
def test_reference_equals_torch_float64(name):
    g = np.random.default_rng(11)
    c = ar.case_random(2, 3.0, seed=12)
    if name == 'holed':
        c['mask'] = g.integers(0, 2, (2, ar.L)).astype(np.int32)
    elif name == 'all_masked':
        c['mask'][1] = 0
    valid = ar.valid_of(c)
    if name == 'segments':
        valid = ar.valid_from_segments(g.integers(0, 3, (2, ar.L)).astype(np.uint8))
    ref = ar.attention(c['q'], c['k'], c['v'], valid)
    want = _torch_ref(c['q'], c['k'], c['v'], valid)
    assert np.abs(ref['o'] - want).max() <= 1e-12
    assert (ref['pav'] >= np.abs(ref['o']) - 1e-12).all()
    if name == 'all_masked':  # the uniform mean of all 128 V rows
        assert np.abs(ref['o'][1] - np.asarray(c['v'][1], np.float64).mean(axis=1, keepdims=True)).max() <= 1e-12
        assert (ref['A'][1] == 0).all()


def test_planted_reference_is_the_planted_row():
    c = ar.case_planted(R=1)
    ref = ar.attention(c['q'], c['k'], c['v'], ar.valid_of(c))
    want = np.stack([c['v'][0, h][c['pi'][0, h]] for h in range(ar.HEADS)])
    assert np.abs(ref['o'][0] - want).max() <= 1e-9


def test_split_helpers_round_trip():
    x = np.random.default_rng(13).standard_normal((64, 768)).astype(np.float32) * 3
    for s in (0, 3, -2):
        hi, lo = ar.split(x, s)
        assert np.abs(ar.value(hi, lo, s) - x).max() <= 2.0 ** -21 * np.abs(x).max()
        buf, off = ar.planar(hi, lo)
        assert off % 8 == 0 and np.array_equal(buf[off:].numpy().reshape(hi.shape), lo)
        p = ar.paired(hi, lo)
        assert p.shape == (64, 1536)
        assert np.array_equal(p[:, 64:96].numpy(), hi[:, 32:64]) and np.array_equal(p[:, 96:128].numpy(), lo[:, 32:64])
    rows = ar.to_rows(np.arange(2 * 12 * 128 * 64).reshape(2, 12, 128, 64))
    assert rows[130, 3 * 64 + 5] == ((1 * 12 + 3) * 128 + 2) * 64 + 5
    assert np.array_equal(ar.from_rows(rows), np.arange(2 * 12 * 128 * 64).reshape(2, 12, 128, 64))


def _cases():
    masks = ar.case_masks()
    keep = [2, 10, 11, 13]  # prefix 31, holes, only key 127, key 0 masked
    masks = {n: (masks[n][keep] if isinstance(masks[n], np.ndarray) else masks[n]) for n in masks}
    peaked, planted = ar.case_peaked(R=1), ar.case_planted(R=1)
    diffuse = ar.case_diffuse(R=1)
    for c in (diffuse, peaked, planted):  # a ragged mask, so that a masked key exists to be let through
        c['mask'][:, 100:] = 0
    return {'diffuse': diffuse, 'peaked': peaked, 'planted': planted, 'masks': masks}


@pytest.fixture(scope='module')
def sensitivity():
    out = {}
    for name, c in _cases().items():
        c = ar.f16_exact(c)
        valid = ar.valid_of(c)
        ref = ar.attention(c['q'], c['k'], c['v'], valid)
        out[name] = {}
        for m in ar.MUTATIONS:
            bad = ar.attention(c['q'], c['k'], c['v'], valid, mutate=m)['o']
            out[name][m] = {p: ar.ratio(bad, ref, p) for p in ar.PRECS}
            out[name][m + ' abs'] = float(np.abs(bad - ref['o']).max())
        out[name]['none'] = {p: ar.ratio(ref['o'], ref, p) for p in ar.PRECS}
    return out


@pytest.mark.parametrize('case', ['peaked', 'planted', 'masks'])
@pytest.mark.parametrize('mutation', ar.MUTATIONS)
def test_bound_rejects_mutation(sensitivity, case, mutation):
    r = sensitivity[case][mutation]
    print(f'{case} / {mutation}: max err / bound ' + ', '.join(f'{p} {v:.3g}' for p, v in r.items()))
    assert all(v > 1.0 for v in r.values()), r
    assert all(v == 0.0 for v in sensitivity[case]['none'].values())


def test_diffuse_record(sensitivity):
    """For the record: what the mutations do to the diffuse inputs (score std 0.3, what the seeded weights give
    every model-level test): the largest error of one context element, against this module's f16 bound and
    against 0.01, the model-level f16 bar on the CLS feature that twelve layers of such contexts feed. No
    assertion on the list beyond its being printed."""
    r = sensitivity['diffuse']
    for m in ar.MUTATIONS:
        print(f'diffuse / {m}: max |err| {r[m + " abs"]:.3g} ({"above" if r[m + " abs"] > 0.01 else "BELOW"} 0.01), '
              f'max err / f16 bound {r[m]["f16"]:.3g} -> {"rejected" if r[m]["f16"] > 1 else "LET THROUGH"}')
    assert all(v == 0.0 for v in r['none'].values())
