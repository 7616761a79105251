"""GPU: BERT's self-attention kernels, one launch at a time through mec_bert_attn, against the float64
reference of tests/attn_ref.py on inputs the model-level tests never produce: a peaked softmax, a
planted key per query, a common +-200 on every score of a row, masks with holes / one key / no key
whose masked keys carry the row's largest raw scores and V = 1000, packed rows of up to 64 segments,
and fp32x3 planes at nonzero exponents. Every output element is held to the bound derived in
attn_ref's docstring (no tuned factor); the [CLS]-only form and the fused QKV + attention kernels are
held to the bits of the kernels they claim to equal.

Kernel instantiations reached (24): bert_attention_kernel<PACK> and bert_attention_f32_kernel<0,0,PACK>
and bert_attention_x3_kernel<0,PACK> by test_unfused_vs_float64 (PACK = 1: the packed case);
bert_attention_cls_kernel<PACK>, bert_attention_f32_kernel<0,1,PACK>, bert_attention_x3_kernel<1,PACK> by
test_cls_form_has_the_full_forms_bits; bert_qkv_attn_kernel<0,HP,PACK> and
bert_qkv_attn_x3_kernel<HP,PACK,PAIRED> by test_fused_has_the_unfused_chains_bits.

Operands are what the kernel reads: f16-exact values on the f16 path, hi + lo of the planes on fp32x3.

max(err / bound) measured on an MI355X (a value above 1 would be a finding):
                      f16     fp32      fp32x3 (planar = paired)
  diffuse             0.214   0.0081    0.0062
  peaked              0.522   0.035     0.357
  planted             2e-11   6e-10     6e-10     (p = 1 on one key: the arithmetic is exact)
  offset              0.258   0.0035    0.013
  masks               0.652   0.097     0.057
  packed              0.640   0.026     0.018
  [CLS] peaked        0.457   0.018     0.027
  [CLS] masks         0.640   0.021     0.016
  [CLS] packed        0.640   0.014     0.010
  GEMM + attention    0.53 / 0.58 (packed)        0.213 / 0.48 (packed)
  fp32x3 peaked at exponents (2, -1, 3): 0.781 (0.357 at zero exponents; [CLS] 0.0054). The largest ratios of
  fp32x3 sit on elements with |O 2^s_v| < 2^-3, where the bound is the lo output plane's subnormal half step
  2^-25 2^-s_v and the error is that rounding itself, which cannot exceed it.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import attn_ref as ar
from mec import _lib, x3pair

pytestmark = pytest.mark.gpu

FORMS = ('f16', 'fp32', 'x3 planar', 'x3 paired')
PREC = {'f16': 'f16', 'fp32': 'fp32', 'x3 planar': 'x3', 'x3 paired': 'x3'}
PREC_ID = {'f16': _lib.PRECISIONS['f16'], 'fp32': _lib.PRECISIONS['fp32'], 'x3': _lib.PRECISIONS['fp32x3']}
CASES = {'diffuse': ar.case_diffuse, 'peaked': ar.case_peaked, 'planted': ar.case_planted, 'offset': ar.case_offset,
         'masks': ar.case_masks, 'packed': ar.case_packed}
NO_EXPS = (0, 0, 0)


@functools.lru_cache(maxsize=None)
def _case(name):
    c = CASES[name]()
    for a in c.values():
        a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def _operands(name, prec, exps=NO_EXPS):
    """The case's Q, K, V as the precision's kernels read them -- per tensor a list of planes ([f16], [f32] or
    [hi, lo] at 2^s) -- and the float64 reference on exactly those values. Computed once, shared, never modified."""
    c = _case(name)
    planes, vals = {}, {}
    for n, s in zip('qkv', exps):
        if prec == 'f16':
            planes[n] = [c[n].astype(np.float16)]
            vals[n] = planes[n][0].astype(np.float64)
        elif prec == 'fp32':
            planes[n] = [c[n]]
            vals[n] = c[n].astype(np.float64)
        else:
            planes[n] = list(ar.split(c[n], s))
            vals[n] = ar.value(*planes[n], s)
    return planes, ar.attention(vals['q'], vals['k'], vals['v'], ar.valid_of(c))


class Dev:
    """One [rows, K] tensor on the device in a form's layout: an f16 or f32 array, or fp32x3 planes -- planar
    (one buffer, the lo plane self.lo elements after the hi plane) or paired (self.lo = -1). planes = None: an
    output, filled with NaN so that an element no kernel wrote fails the check."""

    def __init__(self, form, dev, rows, K, planes=None):
        self.form, self.rows, self.K = form, rows, K
        self.lo = 0
        if form in ('f16', 'fp32'):
            dt = torch.float16 if form == 'f16' else torch.float32
            t = (torch.full((rows, K), float('nan'), dtype=dt) if planes is None
                 else torch.from_numpy(np.ascontiguousarray(planes[0])).reshape(rows, K))
        else:
            if planes is None:
                nan = np.full((rows, K), np.nan, np.float16)
                planes = [nan, nan]
            hi, lo = (np.ascontiguousarray(p).reshape(rows, K) for p in planes)
            if form == 'x3 planar':
                t, self.lo = ar.planar(hi, lo)
            else:
                t, self.lo = ar.paired(hi, lo), _lib.X3_PAIRED
        self.t = t.to(dev)

    def planes(self):
        """The tensor's planes as CPU tensors [rows, K] (its bits)."""
        torch.cuda.synchronize()
        t = self.t.cpu()
        if self.form in ('f16', 'fp32'):
            return [t]
        if self.form == 'x3 paired':
            return list(x3pair.unpair(t))
        n = self.rows * self.K
        return [t[:n].reshape(self.rows, self.K), t[self.lo:].reshape(self.rows, self.K)]

    def value(self, s=0):
        p = [x.numpy() for x in self.planes()]
        return p[0].astype(np.float64) if len(p) == 1 else ar.value(p[0], p[1], s)


def _launch(lib, dev, **fields):
    a = _lib.AttnArgs(**{k: (v.data_ptr() if isinstance(v, torch.Tensor) else v) for k, v in fields.items()})
    _lib.check(lib.mec_bert_attn(ctypes.byref(a), ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)),
               'mec_bert_attn')


def _mask_fields(c, dev):
    """The descriptor's mask fields for a case; the tensors stay alive in the returned dict."""
    if 'seg' in c:
        return dict(packed=1, mask=torch.from_numpy(np.array(c['seg'])).to(dev))
    return dict(packed=0, mask=torch.from_numpy(np.array(c['mask'], np.int32)).to(dev))


def _cat(planes, names):
    """[rows, 768 len(names)] per plane: the named tensors' token rows side by side."""
    return [np.concatenate([ar.to_rows(planes[n][p]) for n in names], axis=1) for p in range(len(planes[names[0]]))]


def _slots(c):
    """The [CLS]-only form's samples as flat slots row * 128 + slot."""
    return c['cidx'] if 'cidx' in c else np.arange(c['q'].shape[0], dtype=np.int32) * ar.L


def _run(lib, dev, form, name, cls=False, exps=NO_EXPS):
    """One unfused launch of the case. Returns (the context Dev, its float64 values in the reference's shape,
    the reference restricted to the rows the launch computes)."""
    prec, c = PREC[form], _case(name)
    planes, ref = _operands(name, prec, exps)
    R = c['q'].shape[0]
    mf = _mask_fields(c, dev)
    x3 = dict(qks=float(np.ldexp(0.125, -(exps[0] + exps[1])))) if prec == 'x3' else {}
    if not cls:
        qkv = Dev(form, dev, R * ar.L, 3 * ar.H, _cat(planes, 'qkv'))
        ctx = Dev(form, dev, R * ar.L, ar.H)
        _launch(lib, dev, precision=PREC_ID[prec], form=0, qkv=qkv.t, qkv_lo=qkv.lo, ctx=ctx.t, ctx_lo=ctx.lo, rows=R,
                **mf, **x3)
        return ctx, ar.from_rows(ctx.value(exps[2])), ref
    slots = _slots(c)
    rr, ss = slots // ar.L, slots % ar.L
    kv = Dev(form, dev, R * ar.L, 2 * ar.H, _cat(planes, 'kv'))
    qc = Dev(form, dev, len(slots), ar.H, [p[slots] for p in _cat(planes, 'q')])
    ctx = Dev(form, dev, len(slots), ar.H)
    cidx = dict(cidx=torch.from_numpy(np.array(slots, np.int32)).to(dev)) if 'cidx' in c else {}
    _launch(lib, dev, precision=PREC_ID[prec], form=1, qkv=kv.t, qkv_lo=kv.lo, qc=qc.t, qc_lo=qc.lo, ctx=ctx.t,
            ctx_lo=ctx.lo, rows=R, ns=len(slots), **mf, **cidx, **x3)
    sub = {n: (a[rr, :, ss][:, :, None, :] if a.ndim == 4 else a[rr, :, ss][:, :, None]) for n, a in ref.items()}
    return ctx, ctx.value(exps[2]).reshape(len(slots), ar.HEADS, 1, ar.DH), sub


def _held(what, got, ref, prec, s_v=0):
    r = ar.ratio(got, ref, prec, s_v)
    print(f'{what}: max err / bound {r:.3g} (max |err| {np.abs(np.asarray(got, np.float64) - ref["o"]).max():.3g})')
    assert r <= 1.0, what


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('case', list(CASES))
def test_unfused_vs_float64(dev, case, form):
    lib = _lib.load()
    _, got, ref = _run(lib, dev, form, case)
    _held(f'{case} / {form}', got, ref, PREC[form])
    if case == 'planted':  # O[i] = V[pi(i)]: the other 127 keys weigh at most 127 e^(-(72 - max other score))
        c = _case(case)
        planes, _ = _operands(case, PREC[form])
        v = planes['v'][0].astype(np.float64) + (planes['v'][1].astype(np.float64) if len(planes['v']) > 1 else 0.0)
        want = np.take_along_axis(v, c['pi'][..., None], axis=2)
        assert np.abs(ref['o'] - want).max() <= 1e-9
        assert (np.abs(got - want) <= ar.bound(ref, PREC[form]) + 1e-9).all()


@pytest.mark.parametrize('form', ('x3 planar', 'x3 paired'))
@pytest.mark.parametrize('exps', [(2, -1, 3), NO_EXPS])
def test_x3_plane_exponents(dev, exps, form):
    """Q, K, V planes at 2^s_q, 2^s_k, 2^s_v with qks = 2^-(s_q + s_k) / 8: the context planes (at V's scale)
    stand for the reference on the unscaled values."""
    lib = _lib.load()
    for cls in (False, True):
        _, got, ref = _run(lib, dev, form, 'peaked', cls=cls, exps=exps)
        _held(f'peaked at exponents {exps} / {form}{" [CLS]" if cls else ""}', got, ref, 'x3', exps[2])


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('case', ['peaked', 'planted', 'masks', 'packed'])
def test_cls_form_has_the_full_forms_bits(dev, case, form):
    """The [CLS]-only form (K | V of every token, one query per sample, compact context) writes the bits of the
    full form's row at that sample's slot: slot 0 of row b unpacked, cidx[b] packed (rows out of order, slots
    0 / 60 / 120)."""
    lib = _lib.load()
    full, _, _ = _run(lib, dev, form, case)
    one, got, sub = _run(lib, dev, form, case, cls=True)
    slots = torch.from_numpy(np.asarray(_slots(_case(case)), np.int64))
    for a, b in zip(full.planes(), one.planes()):
        assert torch.equal(a[slots].view(torch.int16 if a.dtype == torch.float16 else torch.int32),
                           b.view(torch.int16 if b.dtype == torch.float16 else torch.int32))
    _held(f'{case} / {form} [CLS]', got, sub, PREC[form])


# ------------------------------------------------------------------ fused QKV + attention
# 25 rows: the one-head kernels launch 25 x 12 = 300 workgroups. qkv_x3_late_dma moves the stage refill only in
# workgroups whose blockIdx.x has bit 8 set (csrc/bert.hip: every other 256-block), so fewer than 22 rows would run
# the knob's three settings on identical instructions; here blocks 256..299 take the late path. The five masks
# (and the five packed rows) repeat five times over different token rows. The float64 reference is computed on
# the first FUSED_REF_ROWS rows (one of each mask); every row is held to the unfused chain's bits.
FUSED_ROWS, FUSED_REF_ROWS = 25, 5


@functools.lru_cache(maxsize=None)
def _fused_inputs():
    """hs [25 * 128, 768] ~ N(0, 1), Wq and Wk ~ N(0, 0.125^2) (q, k std 3.5: score std 12, a peaked softmax),
    Wv ~ N(0, 0.036^2), biases ~ N(0, 0.1^2); the masks with holes, one key and no key, and the packed rows,
    each set of five tiled to the 25 rows."""
    g = np.random.default_rng(77)
    hs = g.standard_normal((FUSED_ROWS * ar.L, ar.H)).astype(np.float32)
    w = g.standard_normal((3 * ar.H, ar.H)).astype(np.float32)
    w[:2 * ar.H] *= np.float32(0.125)
    w[2 * ar.H:] *= np.float32(0.036)
    b = (g.standard_normal(3 * ar.H) * 0.1).astype(np.float32)
    reps = FUSED_ROWS // FUSED_REF_ROWS
    masks = dict(mask=np.tile(_case('masks')['mask'][len(ar.PREFIX_LENS):], (reps, 1)))
    return hs, w, b, masks, dict(seg=np.tile(_case('packed')['seg'], (reps, 1)))


def _set(lib, key, value):
    _lib.check(lib.mec_set_option(key, value), f'{key.decode()} {value}')


@pytest.mark.parametrize('packed', [0, 1])
@pytest.mark.parametrize('form', ('f16', 'x3 planar', 'x3 paired'))
def test_fused_has_the_unfused_chains_bits(dev, form, packed):
    """The fused QKV projection + attention kernels write the bits of the QKV GEMM (mec_gemm_f16 /
    mec_gemm_f16x3 / mec_gemm_f16x3_paired) followed by the unfused attention, at one and two heads per
    workgroup and, on the one-head fp32x3 form, every qkv_x3_late_dma (300 workgroups, so that blocks 256..299
    run the late refill: see FUSED_ROWS); the chain's context is held to the float64 reference on the Q, K, V
    the GEMM wrote, on the first five rows."""
    lib = _lib.load()
    prec = PREC[form]
    hs, w, b, masks, segs = _fused_inputs()
    mf = _mask_fields(segs if packed else masks, dev)
    M, N, K = FUSED_ROWS * ar.L, 3 * ar.H, ar.H
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    split = (lambda x: [x.astype(np.float16)]) if prec == 'f16' else (lambda x: list(ar.split(x)))
    hsd, wd = Dev(form, dev, M, K, split(hs)), Dev(form, dev, N, K, split(w))
    bd = torch.from_numpy(b).to(dev)
    qkv, ctx = Dev(form, dev, M, N), Dev(form, dev, M, K)
    if form == 'f16':
        rc = lib.mec_gemm_f16(hsd.t.data_ptr(), wd.t.data_ptr(), bd.data_ptr(), None, 0, qkv.t.data_ptr(), None, M, N, K,
                              0, stream)
    elif form == 'x3 planar':
        rc = lib.mec_gemm_f16x3(hsd.t.data_ptr(), hsd.lo, wd.t.data_ptr(), wd.lo, 1.0, bd.data_ptr(), None,
                                qkv.t.data_ptr(), qkv.lo, None, M, N, K, 0, stream)
    else:
        rc = lib.mec_gemm_f16x3_paired(hsd.t.data_ptr(), wd.t.data_ptr(), 1.0, bd.data_ptr(), None, qkv.t.data_ptr(), 1,
                                       0, None, M, N, K, 0, stream)
    _lib.check(rc, 'QKV GEMM')
    _launch(lib, dev, precision=PREC_ID[prec], form=0, qkv=qkv.t, qkv_lo=qkv.lo, ctx=ctx.t, ctx_lo=ctx.lo,
            rows=FUSED_ROWS, **mf)
    want = ctx.planes()
    n = FUSED_REF_ROWS
    vals = qkv.value()[:n * ar.L]
    q, k, v = (ar.from_rows(vals[:, i * ar.H:(i + 1) * ar.H]) for i in range(3))
    ref = ar.attention(q, k, v, ar.valid_of(segs if packed else masks)[:n])
    _held(f'QKV GEMM + attention / {form} packed {packed}', ar.from_rows(ctx.value()[:n * ar.L]), ref, prec)
    assert all(torch.isfinite(p.float()).all() for p in want)
    heads_key = b'bert_qkv_attn_heads' if form == 'f16' else b'bert_qkv_attn_x3_heads'
    settings = [(1, 0), (2, 0)] if form == 'f16' else [(1, 0), (1, 1), (1, 2), (2, 0)]
    try:
        for heads, dma in settings:
            _set(lib, heads_key, heads)
            if form != 'f16':
                _set(lib, b'qkv_x3_late_dma', dma)
            out = Dev(form, dev, M, K)
            _launch(lib, dev, precision=PREC_ID[prec], form=0, fused=1, hs=hsd.t, hs_lo=hsd.lo, wqkv=wd.t, w_lo=wd.lo,
                    bqkv=bd, ctx=out.t, ctx_lo=out.lo, rows=FUSED_ROWS, **mf)
            for a, bb in zip(want, out.planes()):
                assert torch.equal(a.view(torch.int16), bb.view(torch.int16)), (heads, dma)
    finally:  # the process defaults of csrc/mec_common.h (Options): one head per workgroup, late_dma 0
        _set(lib, heads_key, 1)
        _set(lib, b'qkv_x3_late_dma', 0)
