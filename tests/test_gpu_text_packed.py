"""GPU: the packed BERT text path (mec_text_fwd_packed, engine.TextEncoder.forward_packed): short
sentences share 128-slot rows, position ids restart per sentence and a key counts only for the queries
of its own sentence. The reference is the untouched oracle on the PADDED ids and prefix mask: padded
keys there and other-segment keys here both get weight exactly 0, so the packed outputs are the padded
ones to the precision's rounding. Bars are the unpacked path's own (tests/test_gpu_fp32x3.py: probs
1e-5, CLS 1e-4 relative, argmax exact; tests/test_gpu_parity.py for f16: probs 1e-3, CLS 1e-2 absolute,
argmax exact), on every sample.

Shapes: [128, 8, 60, 60, 9] packs to a full row, a row with a segment ending at slot 127 and one over
slots 60-119 (across the 32-query wave split and the 64-key lane-half split), and a row with 119 unused
slots; [2]*64 + [3] packs 64 segments into one row beside a nearly empty one; the ragged 9 is the
synthetic generator's own mix."""
import functools

import numpy as np
import pytest
import torch

from mec import engine, synthetic as syn
from oracle import text as o_t

pytestmark = pytest.mark.gpu

PRECISIONS = ('f16', 'fp32', 'fp32x3')
# probs max|d|, CLS error (relative to max|cls| for the fp32 family, absolute for f16)
PROB_TOL = {'f16': 1e-3, 'fp32': 1e-5, 'fp32x3': 1e-5}
FEAT_RTOL, F16_CLS_TOL = 1e-4, 1e-2
HEADS_OPT = {'f16': 'bert_qkv_attn_heads', 'fp32x3': 'bert_qkv_attn_x3_heads'}
HEADS_DEFAULT = 1  # csrc/mec_common.h


def _with_lens(lens, seed):
    """Padded ids / prefix mask [B,128] with the given lengths ([CLS] first, [SEP] last, 0 padding)."""
    lens = np.asarray(lens, np.int64)
    ids, _ = syn.text_inputs(len(lens), 128, seed=seed)
    mask = (np.arange(128)[None, :] < lens[:, None]).astype(np.int32)
    ids[np.arange(len(lens)), lens - 1] = 102
    ids[mask == 0] = 0
    return ids, mask


@functools.lru_cache(maxsize=None)
def _case(name):
    """(ids, mask, lens, oracle outputs on the padded batch): computed once, shared, never modified."""
    if name == 'rows':
        ids, mask = _with_lens([128, 8, 60, 60, 9], seed=611)
    elif name == 'many':
        ids, mask = _with_lens([2] * 64 + [3], seed=612)
    elif name == 'ragged9':
        ids, mask = syn.text_inputs(9, 128, seed=613, ragged=True)
    elif name == 'alone':
        ids, mask = _with_lens([9], seed=614)
    elif name == 'behind':  # sample 0 of 'alone', now behind a 100-token neighbour (off = 100)
        ids, mask = _with_lens([9, 100], seed=614)
    else:
        raise KeyError(name)
    for a in (ids, mask):
        a.setflags(write=False)
    return ids, mask, mask.sum(1).astype(np.int32), o_t.forward(syn.weights('text'), ids, mask)


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


def _np(ts):
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in ts]


def _packed(m, dev, ids, lens):
    out = _np(m.forward_packed(engine.to_device(ids, dev), lens=lens))
    m.check()  # a raised fp32x3 range flag is an error here, never a silent fp32 re-run
    return out


def _assert_bars(tag, precision, got, ref):
    (cls, logits, probs), (rc, rl, rp) = got, ref
    err = float(np.abs(probs - rp).max())
    aerr = float(np.abs(cls - rc).max())
    ferr = aerr / float(np.abs(rc).max())
    agree = int((probs.argmax(1) == rp.argmax(1)).sum())
    s = np.sort(rp, axis=1)
    print(f'{tag} {precision}: probs max|d| {err:.3g}, cls max|d| {aerr:.3g} (rel {ferr:.3g}), argmax {agree}/{len(rp)}, '
          f'min top-2 margin {(s[:, -1] - s[:, -2]).min():.3g}')
    assert np.isfinite(cls).all() and np.isfinite(probs).all()
    assert err <= PROB_TOL[precision]
    assert (aerr <= F16_CLS_TOL) if precision == 'f16' else (ferr <= FEAT_RTOL)
    assert agree == len(rp)  # every sample


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('case,bp', [('rows', 3), ('many', 2), ('ragged9', None)])
def test_packed_vs_oracle_on_padded_batch(dev, encoders, precision, case, bp):
    ids, mask, lens, ref = _case(case)
    m = encoders(precision)
    got = _packed(m, dev, ids, lens)
    if bp is not None:
        assert m.packed_rows == bp
    assert m.packed_rows <= len(lens)
    _assert_bars(case, precision, got, ref)
    assert m.x3_reruns == 0


@pytest.mark.parametrize('precision', ['fp32', 'fp32x3'])
def test_identity_plan_equals_forward_bit_for_bit(dev, encoders, precision):
    """Every length >= 65: one sentence per row at offset 0, so real slots see the padded path's
    arithmetic exactly; only pad-slot rows differ (they attend to each other instead of to the
    sentence), and no output reads them."""
    ids, mask = _with_lens([128, 65, 100, 127], seed=615)
    m = encoders(precision)
    d_ids, d_mask = engine.to_device(ids, dev), engine.to_device(mask, dev)
    want = _np(m.forward(d_ids, d_mask))
    got = _np(m.forward_packed(d_ids, d_mask))  # lengths from the mask
    assert m.packed_rows == 4
    for name, a, b in zip(('cls', 'logits', 'probs'), want, got):
        np.testing.assert_array_equal(a, b, err_msg=f'{precision} {name}')
    m.check()


@pytest.mark.parametrize('precision', ['f16', 'fp32x3'])
@pytest.mark.parametrize('case', ['rows', 'many'])
def test_packed_fused_and_unfused_attention_bit_identical(dev, encoders, precision, case):
    """As the unpacked path (test_text_qkv_attn_bit_identical, test_text_fp32x3_fused_qkv_attention_bit_identical):
    the fused QKV + attention kernel with two heads per workgroup and with one, and the QKV GEMM followed
    by the attention kernel, give identical outputs on a packed batch."""
    ids, mask, lens, _ = _case(case)
    m = encoders(precision)
    outs = []
    for fused, heads in ((1, 2), (1, 1), (0, 2)):
        m.set_option('bert_qkv_attn', fused)
        m.set_option(HEADS_OPT[precision], heads)
        try:
            outs.append(_packed(m, dev, ids, lens))
        finally:
            m.set_option('bert_qkv_attn', 1)
            m.set_option(HEADS_OPT[precision], HEADS_DEFAULT)
    for o in outs[1:]:
        for a, b in zip(outs[0], o):
            np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('case', ['rows', 'many'])
def test_packed_cls_last_bit_identical_to_full_layer(dev, encoders, precision, case):
    """bert_cls_last 1 (the last layer on the samples' [CLS] slots only, K / V of their packed rows) against
    0 (the full last layer, then one gather of the [CLS] rows): identical outputs, as unpacked."""
    ids, mask, lens, _ = _case(case)
    m = encoders(precision)
    try:
        m.set_option('bert_cls_last', 0)
        full = _packed(m, dev, ids, lens)
    finally:
        m.set_option('bert_cls_last', 1)
    pruned = _packed(m, dev, ids, lens)
    for name, a, b in zip(('cls', 'logits', 'probs'), full, pruned):
        np.testing.assert_array_equal(a, b, err_msg=f'{precision} {name}')


@pytest.mark.parametrize('precision', PRECISIONS)
def test_sample_independent_of_neighbour_and_offset(dev, encoders, precision):
    """A 9-token sentence packed alone (slots 0-8) and behind a 100-token neighbour (slots 100-108): the
    same answer within the precision's oracle bar. Bit equality is NOT required: the key's slot decides
    which MFMA k group its product is summed in (and which partial sums the softmax adds first), so the
    same terms are added in another order."""
    ids_a, _, lens_a, ref_a = _case('alone')
    ids_b, _, lens_b, ref_b = _case('behind')
    np.testing.assert_array_equal(ids_a[0], ids_b[0])
    m = encoders(precision)
    alone = _packed(m, dev, ids_a, lens_a)
    assert m.packed_rows == 1
    behind = _packed(m, dev, ids_b, lens_b)
    assert m.packed_rows == 1
    d = float(np.abs(alone[2][0] - behind[2][0]).max())
    print(f'{precision}: probs of the sample alone vs behind a neighbour max|d| {d:.3g}')
    assert d <= PROB_TOL[precision]
    _assert_bars('alone', precision, alone, ref_a)
    _assert_bars('behind', precision, behind, ref_b)


def test_fp32x3_range_flag_stays_clear_on_mostly_empty_rows(dev, encoders):
    """Unused slots are a segment of their own (they attend to each other), so every row of every tensor is
    an ordinary LayerNorm / projection output inside the plane bounds: padding never raises the range flag."""
    m = encoders('fp32x3')
    for lens in ([1], [3, 128], [2] * 64 + [3]):
        ids, _ = _with_lens(lens, seed=616)
        cls, logits, probs = _np(m.checked('forward_packed', engine.to_device(ids, dev), None, np.asarray(lens, np.int32)))
        assert np.isfinite(probs).all()
        m.check()
    assert m.x3_reruns == 0


def test_forward_packed_argument_errors_and_packed_rows(dev, encoders):
    m = encoders('f16')
    ids, mask, lens, _ = _case('rows')
    d_ids, d_mask = engine.to_device(ids, dev), engine.to_device(mask, dev)
    holes = mask.copy()
    holes[2, 5] = 0  # not a prefix mask
    with pytest.raises(ValueError, match='prefix'):
        m.forward_packed(d_ids, engine.to_device(holes, dev))
    short = torch.zeros(2, 64, dtype=torch.int32, device=dev)
    with pytest.raises(ValueError):
        m.forward_packed(short, short)
    with pytest.raises(ValueError, match=r'\[1,128\]'):
        m.forward_packed(d_ids, lens=np.array([128, 0, 60, 60, 9], np.int32))
    empty = mask.copy()
    empty[1] = 0  # a length of 0 read from the mask
    with pytest.raises(ValueError, match=r'\[1,128\]'):
        m.forward_packed(d_ids, engine.to_device(empty, dev))
    with pytest.raises(ValueError):
        m.forward_packed(d_ids, lens=np.array([128, 8], np.int32))
    with pytest.raises(ValueError):
        m.forward_packed(d_ids)
    row, off, bp = m.pack_plan(lens)
    m.forward_packed(d_ids, d_mask)
    assert m.packed_rows == bp == 3
    out = m.forward_packed(d_ids[:0], lens=np.zeros(0, np.int32))
    assert out[2].shape == (0, 7) and m.packed_rows == 0
    torch.cuda.synchronize()


def test_predict_texts_pack_matches_unpacked(dev, tmp_path):
    from inference.text_inference import TextInference
    from test_gpu_dropin import _legacy_tokenizer, _write_vocab
    ti = TextInference(seed=1234, device=dev, tokenizer=_legacy_tokenizer(_write_vocab(tmp_path)), precision='fp32')
    texts = ['I am so happy today!', 'This is the WORST day ever... not sure how I feel about it', 'wow',
             'sad and blue', 'I feel nervous about it', 'not sure']
    plain = ti.predict_texts(texts)
    packed = ti.predict_texts(texts, pack=True)
    assert ti.model.packed_rows == 1
    for a, b in zip(plain, packed):
        assert a['emotion'] == b['emotion']
        d = float(np.abs(np.array(a['all_probabilities']) - np.array(b['all_probabilities'])).max())
        assert d <= PROB_TOL['fp32'], d
    ids, mask = ti.encode_batch(texts)
    got = _np(ti.predict_batch(engine.to_device(ids, dev), engine.to_device(mask, dev), pack=True))[2]
    np.testing.assert_array_equal(got.astype(np.float64), np.array([p['all_probabilities'] for p in packed]))
    assert ti.predict_texts(texts) == plain  # the default path is unchanged by a packed call in between
    ti.model.close()


@pytest.mark.parametrize('precision,tol', [('f16', 1e-3), ('fp32x3', 1e-5)])
def test_fused_pipeline_text_lens(dev, precision, tol):
    """The text leg packed inside the fused step (first call serial, second on the text stream): fused
    probabilities within the fused bar (the smoke run's: 1e-3 at f16, 1e-5 at fp32x3) of the run without
    text_lens, and check() clean with no fp32 re-run."""
    B = 8
    pipe = engine.FusedPipeline(device=dev, precision=precision)
    ids, mask = syn.text_inputs(B, 128, seed=617, ragged=True)
    lens = mask.sum(1).astype(np.int32)
    args = tuple(engine.to_device(a, dev) for a in (syn.speech_inputs(B, seed=617), ids, mask,
                                                    syn.image_inputs(B, seed=617)))
    pipe.forward(*args)
    want = pipe.forward(*args)
    pipe.wait()
    assert pipe.check() == []
    want = {k: [t.clone() for t in v] for k, v in want.items()}
    for it in range(2):
        got = pipe.forward(*args, text_lens=lens)
        pipe.wait()
        assert pipe.check() == []
        assert 1 <= pipe.text.packed_rows < B
        for key, idx in (('fusion', 1), ('text', 2)):
            d = float((got[key][idx] - want[key][idx]).abs().max())
            print(f'{precision} call {it}: {key} probs packed vs padded max|d| {d:.3g}')
            assert d <= tol
        for key in ('speech', 'image'):
            assert torch.equal(got[key][2], want[key][2])
    assert pipe.text.x3_reruns == 0
