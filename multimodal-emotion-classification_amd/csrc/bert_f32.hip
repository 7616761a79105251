// BERT-base in fp32 end to end (mec_create_ex(..., MEC_PREC_FP32)): the reference's own
// precision (transformers BertForSequenceClassification in fp32, inference/text_inference.py:
// 41, :92-93). Every GEMM runs on the fp32 engine (gemm_f32.hip, v_mfma_f32_32x32x2_f32) and
// the attention on f32 MFMAs; LayerNorm, GELU (libm erff), softmax and the residual stream are
// fp32 as on the f16 path. Per layer (M = B*L rows):
//   qkv32 = h32 . Wqkv^T + b                   gemm_f32 (N = 2304)
//   ctx32 = softmax(QK^T/8 + mask_bias) V      bert_attention_f32_kernel
//   t32   = ctx32 . Wo^T + bo + h32            gemm_f32, residual fused
//   h32   = LN(t32)                            bert_layernorm_kernel (f32 out only)
//   i32   = GELU(h32 . Wi^T + bi)              gemm_f32 (N = 3072), exact erf
//   t32   = i32 . Wo2^T + bo2 + h32            gemm_f32
//   h32   = LN(t32)
// Head as on the f16 path (pooler tanh + classifier + softmax, block_ops.h).
#include "bert_model.h"

namespace mec {

// K rows in LDS: 16 chunks of 16 B per 256-B row, chunk c stored at c ^ (row & 15), so the 16
// rows of a ds_read_b128 lane group cover all 64 banks.
__device__ __forceinline__ int kswz(int row, int c) { return c ^ (row & 15); }

// One workgroup per (sequence, head), 4 waves; wave w owns queries 32w .. 32w+31.
// S^T = K Q^T on v_mfma_f32_32x32x2_f32 (A = K rows from LDS, B = Q^T from registers), so each
// lane holds one query's scores over 64 keys (the other 64 in lane ^ 32): the row softmax is
// lane-local plus one shuffle. O^T = V^T P^T: A = V[key][d] read as one f32 per lane (row-major
// V, 32 consecutive d per half wave), B = the lane's own probabilities, in the k order the
// score tile left them (two keys per MFMA: key f(e) + 4h of block t for lane half h).
// SPLIT (fp32x3 path): ctx is written as f16 hi / lo planes (ctx16, ctx16 + lo) for the split
// O-projection GEMM instead of f32.
// CLS = 1 (the last layer with bert_cls_last): qkv holds K | V only ([B*128, 1536]), the [CLS] query
// row comes from qc ([B, 768]) and the context is written compact ([B, 768]); wave 0 computes
// queries 0..31 with Q zero for all but query 0 (an MFMA output column depends only on its own B
// column: the [CLS] context has the full kernel's bits), waves 1-3 only stage K and V.
// PACK (the packed text path): mask = the rows' uint8 segment ids (block_ops.h stage_mask) and a key
// counts only in the query's own segment; with CLS, workgroup (b, h) serves sample b, whose [CLS] slot is
// cidx[b] = row * 128 + off (K / V and segment ids of packed row `row`, the query's segment that of `off`).
template <int SPLIT = 0, int CLS = 0, int PACK = 0>
__global__ __launch_bounds__(256, 2) void bert_attention_f32_kernel(const float* __restrict__ qkv,
                                                                    const int32_t* __restrict__ mask,
                                                                    float* __restrict__ ctx, f16* __restrict__ ctx16,
                                                                    long long lo, const float* __restrict__ qc,
                                                                    const int32_t* __restrict__ cidx) {
  constexpr int LD = CLS ? 2 * BH : 3 * BH, KO = CLS ? 0 : BH;
  __shared__ __attribute__((aligned(16))) float sK[ATT_L * BDH];
  __shared__ __attribute__((aligned(16))) float sV[ATT_L * BDH];
  __shared__ float sBias[ATT_L];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x / BHEADS, h = blockIdx.x - (blockIdx.x / BHEADS) * BHEADS;
  const int cs = (CLS && PACK) ? cidx[b] : 0;
  const int bk = (CLS && PACK) ? cs >> 7 : b;  // the row whose K / V are staged
  const float* base = qkv + (size_t)bk * ATT_L * LD + h * BDH;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int c = tid + 256 * i;
    const int row = c >> 4, kc = c & 15;
    const float* src = base + (size_t)row * LD + kc * 4;
    const float4 k = *reinterpret_cast<const float4*>(src + KO);
    const float4 v = *reinterpret_cast<const float4*>(src + KO + BH);
    *reinterpret_cast<float4*>(sK + row * BDH + kswz(row, kc) * 4) = k;
    *reinterpret_cast<float4*>(sV + row * BDH + kc * 4) = v;
  }
  stage_mask<PACK>(sBias, mask, bk, tid);
  const int lr = lane & 31, lh = lane >> 5;
  const int q = 32 * wave + lr;
  float4 qf[8];  // Q[q][8s + 4lh .. +3]
  if constexpr (CLS) {
    const bool own = wave == 0 && lr == 0;
    const float* qrow = qc + (size_t)b * BH + h * BDH;
#pragma unroll
    for (int s = 0; s < 8; ++s)
      qf[s] = own ? *reinterpret_cast<const float4*>(qrow + (2 * s + lh) * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
  } else {
#pragma unroll
    for (int s = 0; s < 8; ++s) qf[s] = *reinterpret_cast<const float4*>(base + (size_t)q * LD + (2 * s + lh) * 4);
  }
  __syncthreads();
  if (CLS && wave != 0) return;
  const int qseg = mask_qseg<PACK>(sBias, CLS ? (cs & 127) : q);

  floatx16 st[4];  // st[t][e] = S[q][key 32t + (e&3) + 8(e>>2) + 4lh]
#pragma unroll
  for (int t = 0; t < 4; ++t) {
#pragma unroll
    for (int e = 0; e < 16; ++e) st[t][e] = 0.f;
    const int rk = 32 * t + lr;
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const float4 kf = *reinterpret_cast<const float4*>(sK + rk * BDH + kswz(rk, 2 * s + lh) * 4);
      st[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.x, qf[s].x, st[t], 0, 0, 0);
      st[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.y, qf[s].y, st[t], 0, 0, 0);
      st[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.z, qf[s].z, st[t], 0, 0, 0);
      st[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.w, qf[s].w, st[t], 0, 0, 0);
    }
  }
  // scores / sqrt(64) + additive mask (HF eager order), softmax over the 128 keys
  float mx = -INFINITY;
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int key = 32 * t + (e & 3) + 8 * (e >> 2) + 4 * lh;
      const float v = st[t][e] * 0.125f + mask_term<PACK>(sBias, key, qseg);
      st[t][e] = v;
      mx = fmaxf(mx, v);
    }
  mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
  float sum = 0.f;
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const float p = expf(st[t][e] - mx);
      st[t][e] = p;
      sum += p;
    }
  sum += __shfl_xor(sum, 32, 64);
  const float inv = 1.0f / sum;

  floatx16 o[2];  // o[u][e] = O[q][d = 32u + (e&3) + 8(e>>2) + 4lh]
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int e = 0; e < 16; ++e) o[u][e] = 0.f;
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int key = 32 * t + (e & 3) + 8 * (e >> 2) + 4 * lh;
      const float p = st[t][e] * inv;
#pragma unroll
      for (int u = 0; u < 2; ++u) o[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(sV[key * BDH + 32 * u + lr], p, o[u], 0, 0, 0);
    }
  if (CLS && lr != 0) return;
  const size_t obase = ((size_t)b * (CLS ? 1 : ATT_L) + q) * BH + h * BDH;
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const size_t oi = obase + 32 * u + 8 * g + 4 * lh;
      if constexpr (SPLIT) {
        half4 hh, hl;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          hh[e] = (f16)o[u][4 * g + e];
          hl[e] = (f16)(o[u][4 * g + e] - (float)hh[e]);
        }
        *reinterpret_cast<half4*>(ctx16 + oi) = hh;
        *reinterpret_cast<half4*>(ctx16 + lo + oi) = hl;
      } else {
        *reinterpret_cast<float4*>(ctx + oi) =
            make_float4(o[u][4 * g + 0], o[u][4 * g + 1], o[u][4 * g + 2], o[u][4 * g + 3]);
      }
    }
}

// kv: K | V of every token [rows * 128, 1536]; qc, ctx: the samples' [CLS] query / context rows [NS, 768];
// cidx (or null): the packed form (mask = segment ids, sample b's [CLS] slot cidx[b])
int launch_bert_attention_f32_cls(const float* kv, const int32_t* mask, const float* qc, float* ctx, int NS,
                                  hipStream_t s, const int32_t* cidx) {
  if (cidx)
    hipLaunchKernelGGL((bert_attention_f32_kernel<0, 1, 1>), dim3(NS * BHEADS), dim3(256), 0, s, kv, mask, ctx, nullptr,
                       0LL, qc, cidx);
  else
    hipLaunchKernelGGL((bert_attention_f32_kernel<0, 1, 0>), dim3(NS * BHEADS), dim3(256), 0, s, kv, mask, ctx, nullptr,
                       0LL, qc, nullptr);
  MEC_LAUNCH_CHECK();
  return 0;
}

// packed: mask holds the rows' uint8 segment ids and B counts packed rows
int launch_bert_attention_f32(const float* qkv, const int32_t* mask, float* ctx, int B, hipStream_t s, bool packed) {
  if (packed)
    hipLaunchKernelGGL((bert_attention_f32_kernel<0, 0, 1>), dim3(B * BHEADS), dim3(256), 0, s, qkv, mask, ctx, nullptr,
                       0LL, nullptr, nullptr);
  else
    hipLaunchKernelGGL((bert_attention_f32_kernel<0, 0, 0>), dim3(B * BHEADS), dim3(256), 0, s, qkv, mask, ctx, nullptr,
                       0LL, nullptr, nullptr);
  MEC_LAUNCH_CHECK();
  return 0;
}

namespace {
// The fp32 forward's form of TailRows (bert_model.h): no f16 operands, no deferred LayerNorm
struct TailRowsF32 {
  int n;
  float *h32, *t32;  // the stream pair: both GEMMs add h32 into t32, both LayerNorms write t32 -> h32
  float *ctx, *ffn;  // the context (in), the FFN intermediate
  bool tagged;
};
}  // namespace

int TextModel::forward_f32(const int32_t* ids, const int32_t* mask, int B, int L, float* cls, float* logits,
                           float* probs, hipStream_t s, const TextPack* pk) {
  MEC_REQUIRE(wts32.p, "text: fp32 weights missing (handle created at f16 precision)");
  // workspace: h32 | t32 | ctx32 (f32 [M,768]) ; big32 f32 [M,3072] (qkv [M,2304], then FFN) ; pooled [NS,768] ;
  // the [CLS]-row buffers of the last layer (bert_cls_last): h32c | t32c | qc | ctxc [NS,768], fc [NS,3072]
  float *h32, *t32, *ctx32, *big32, *pooled, *h32c, *t32c, *qc, *ctxc, *fc;
  TextBatch tb;
  MEC_TRY(text_prologue(tb, ws, ids, mask, B, pk, s, [&](Carver& c) {
    const size_t M = tb.M, NS = tb.NS;
    h32 = c.take<float>(M * BH);
    t32 = c.take<float>(M * BH);
    ctx32 = c.take<float>(M * BH);
    big32 = c.take<float>(M * BI);
    pooled = c.take<float>(NS * BH);
    h32c = c.take<float>(NS * BH);
    t32c = c.take<float>(NS * BH);
    qc = c.take<float>(NS * BH);
    ctxc = c.take<float>(NS * BH);
    fc = c.take<float>(NS * BI);
  }));
  const int M = tb.M, NS = tb.NS;
  const bool cls_last = opt().bert_cls_last != 0;
  const float* W = wts32.as<float>();
  const float* P = prm.as<float>();

  auto tail = [&](int l, const TailRowsF32& r) -> int {
    const LayerWeights<const float> w = layer_weights(W, l);
    const LayerParams<const float> p = layer_params(P, l);
    auto tag = [&](int t) { return r.tagged ? t : (int)TAG_NONE; };
    GemmParams g;
    g.A = r.ctx; g.B32 = w.wo; g.bias = p.bo; g.R = r.h32; g.r_f32 = 1; g.C32 = r.t32; g.M = r.n; g.N = BH; g.K = BH;
    MEC_TRY(launch_gemm_f32(g, s, &prof, tag(TAG_BERT_OPROJ)));
    MEC_TRY(prof.begin(tag(TAG_BERT_LN), s));
    MEC_TRY(launch_bert_layernorm(r.t32, r.n, p.g1, p.b1, r.h32, nullptr, nullptr, s));
    MEC_TRY(prof.end(tag(TAG_BERT_LN), s));
    g = GemmParams();
    g.A = r.h32; g.B32 = w.wi; g.bias = p.bi; g.act = ACT_GELU_EXACT; g.C32 = r.ffn; g.M = r.n; g.N = BI; g.K = BH;
    MEC_TRY(launch_gemm_f32(g, s, &prof, tag(TAG_BERT_FFN1)));
    g = GemmParams();
    g.A = r.ffn; g.B32 = w.wo2; g.bias = p.bo2; g.R = r.h32; g.r_f32 = 1; g.C32 = r.t32; g.M = r.n; g.N = BH; g.K = BI;
    MEC_TRY(launch_gemm_f32(g, s, &prof, tag(TAG_BERT_FFN2)));
    MEC_TRY(prof.begin(tag(TAG_BERT_LN), s));
    MEC_TRY(launch_bert_layernorm(r.t32, r.n, p.g2, p.b2, r.h32, nullptr, nullptr, s));
    MEC_TRY(prof.end(tag(TAG_BERT_LN), s));
    return 0;
  };

  MEC_TRY(launch_bert_embed_ln(tb.ids, M, L, emb.as<float>(), h32, nullptr, s, 0, 1.f, tb.posid));
  for (int l = 0; l < BLAYERS; ++l) {
    const LayerWeights<const float> w = layer_weights(W, l);
    const LayerParams<const float> p = layer_params(P, l);
    GemmParams g;
    if (cls_last && l == BLAYERS - 1) {
      // [CLS]-only last layer (TextModel::forward): K / V for every token, the rest on the [CLS] rows
      MEC_TRY(gather_cls_rows(tb, {{h32, h32c, BH * 4}}, s));
      g.A = h32; g.B32 = w.wqkv + (size_t)BH * BH; g.bias = p.bqkv + BH; g.C32 = big32; g.M = M; g.N = 2 * BH; g.K = BH;
      MEC_TRY(launch_gemm_f32(g, s, &prof, TAG_NONE));  // K | V [M, 1536]
      g = GemmParams();
      g.A = h32c; g.B32 = w.wqkv; g.bias = p.bqkv; g.C32 = qc; g.M = NS; g.N = BH; g.K = BH;
      MEC_TRY(launch_gemm_f32(g, s, &prof, TAG_NONE));  // Q of the [CLS] rows
      MEC_TRY(launch_bert_attention_f32_cls(big32, tb.mask, qc, ctxc, NS, s, tb.cidx));
      MEC_TRY(tail(l, {NS, h32c, t32c, ctxc, fc, /*tagged=*/false}));
      break;
    }
    g.A = h32; g.B32 = w.wqkv; g.bias = p.bqkv; g.C32 = big32; g.M = M; g.N = BQKV; g.K = BH;
    MEC_TRY(launch_gemm_f32(g, s, &prof, TAG_BERT_QKV));
    MEC_TRY(prof.begin(TAG_BERT_ATTN, s));
    MEC_TRY(launch_bert_attention_f32(big32, tb.mask, ctx32, B, s, pk != nullptr));
    MEC_TRY(prof.end(TAG_BERT_ATTN, s));
    MEC_TRY(tail(l, {M, h32, t32, ctx32, big32, /*tagged=*/true}));
  }
  return text_outputs(tb, P, h32, h32c, cls_last, pooled, cls, logits, probs, s);
}

// fp32x3 path: the fp32 path's structure with every GEMM on split-f16 operands (gemm_glds.hip
// split mode, three f16 MFMA passes into one fp32 accumulator). Per layer (M = B*L rows):
//   qkv hi/lo   = [h_hi|h_lo] . [Wqkv_hi|Wqkv_lo]^T 2^-e + b        split GEMM, split out
//   ctx hi/lo   = softmax(QK^T/8 + mask_bias) V                     bert_attention_x3_kernel (split
//                                                                    MFMA products, fp32 softmax)
//   t32         = ctx . Wo^T 2^-e + bo + LN2'(h32)                  split GEMM, f32 residual (deferred LN)
//   h hi/lo, st1 = LN(t32)                                          bert_layernorm_kernel (lo plane, stats)
//   i hi/lo     = GELU(h . Wi^T 2^-e + bi)                          split GEMM, exact erf, split out
//   h32         = i . Wo2^T 2^-e + bo2 + LN1'(t32)                  split GEMM (deferred LN)
//   h hi/lo, st2 = LN(h32)
int TextModel::forward_x3(const int32_t* ids, const int32_t* mask, int B, int L, float* cls, float* logits,
                          float* probs, hipStream_t s, const TextPack* pk) {
  MEC_REQUIRE(wts.p && x3_lo && x3_layers.size() == (size_t)BLAYERS, "text: fp32x3 weights missing");
  // workspace: h32 | t32 (f32 [M,768]) ; h hi|lo, ctx hi|lo (f16 2x[M,768]) ; big: qkv hi|lo
  // (f16 2x[M,2304]), then the FFN intermediate hi|lo (f16 2x[M,3072]) ; pooled [NS,768]
  // + the [CLS]-row buffers of the last layer (bert_cls_last): h32c | t32c (f32 [NS,768]) ; hsc | qsc | csc
  // (f16 planes 2x[NS,768]) ; fsc (f16 planes 2x[NS,3072])
  // + the LayerNorm row stats st1 | st2 ([M] float2 each; deferred LayerNorm, below) and st1c | st2c ([NS])
  float *h32, *t32, *pooled, *h32c, *t32c;
  f16 *hs, *cs, *bigs, *hsc, *qsc, *csc, *fsc;
  float2 *st1, *st1c;
  TextBatch tb;
  MEC_TRY(text_prologue(tb, ws, ids, mask, B, pk, s, [&](Carver& c) {
    const size_t M = tb.M, NS = tb.NS;
    h32 = c.take<float>(M * BH);
    t32 = c.take<float>(M * BH);
    hs = c.take<f16>(M * BH * 2);
    cs = c.take<f16>(M * BH * 2);
    bigs = c.take<f16>(M * BI * 2);
    pooled = c.take<float>(NS * BH);
    h32c = c.take<float>(NS * BH);
    t32c = c.take<float>(NS * BH);
    hsc = c.take<f16>(NS * BH * 2);
    qsc = c.take<f16>(NS * BH * 2);
    csc = c.take<f16>(NS * BH * 2);
    fsc = c.take<f16>(NS * BI * 2);
    st1 = c.take<float2>(M * 2);
    st1c = c.take<float2>(NS * 2);
  }));
  const int M = tb.M, NS = tb.NS;
  // x3_layout 1: every split tensor below (weights, LN outputs, context, FFN intermediate, the last layer's
  // K | V and [CLS]-row buffers) is paired ([rows][2K], mec_common.h x3_pair_index) in the same buffers; a
  // lo-plane offset is then kX3Paired and the weight matrices sit at twice their planar offsets
  const bool pr = x3_paired;
  auto plo = [&](long long planar) { return pr ? kX3Paired : planar; };
  const long long MH = plo((long long)M * BH), NSH = plo((long long)NS * BH);  // lo planes of [M,768] / [NS,768]
  float2* st2 = st1 + M;
  float2* st2c = st1c + NS;
  const bool cls_last = opt().bert_cls_last != 0;
  const int gelu_act = opt().gelu_x3 ? ACT_GELU_F32 : ACT_GELU_EXACT;  // FFN1's erf GELU
  const f16* W = wts.as<f16>();
  const float* P = prm.as<float>();
  const long long wlo = plo((long long)x3_lo);
  auto wmat = [&](const f16* w) { return pr ? W + 2 * (w - W) : w; };  // a weight matrix of layer_weights(W, l)
  // split operands A (lo plane a_lo on) and weight matrix w of g, planar or paired
  auto operands = [&](GemmParams& g, const f16* A, long long a_lo, const f16* w) {
    g.split = 1; g.A = A; g.B = wmat(w);
    if (pr) { g.a_pair = g.b_pair = 1; } else { g.a_lo = a_lo; g.b_lo = wlo; }
  };
  auto planes_out = [&](GemmParams& g, f16* C, long long c_lo) {
    g.C16 = C;
    if (pr) g.c_pair = 1; else g.c_lo = c_lo;
  };

  // Deferred LayerNorm (as on the f16 path): the LN kernels write the GEMM operand planes and the row
  // (mean, rstd) only; the f32 LN output is needed only as the next residual, which the O-proj / FFN2
  // epilogue re-derives from the pre-LN sum with the LN kernel's own expression (GemmParams::r_stats):
  // same bits, two 100-MB f32 writes per layer fewer at B = 256. The f32 stream ping-pongs, so no GEMM
  // reads its own output. Plane scales (TextModel::create): LN outputs 2^s_ln1 / 2^s_ln2, FFN intermediate
  // cscale 2^s_ffn; each GEMM's oscale undoes its operands' (X3Layer::scale).
  auto tail = [&](int l, const TailRows& r) -> int {
    const LayerWeights<const f16> w = layer_weights(W, l);
    const LayerParams<const float> p = layer_params(P, l);
    const X3Layer& x = x3_layers[l];
    const long long nh = (long long)r.n * BH, nf = (long long)r.n * BI;
    auto tag = [&](int t) { return r.tagged ? t : (int)TAG_NONE; };
    GemmParams g;
    operands(g, r.ctx, nh, w.wo); g.oscale = x.scale[1];
    g.bias = p.bo; g.R = r.h32; g.r_f32 = 1; g.C32 = r.t32; g.M = r.n; g.N = BH; g.K = BH;
    if (r.deferred_in) { g.r_stats = r.st2; g.r_g = layer_params(P, l - 1).g2; g.r_b = layer_params(P, l - 1).b2; }
    MEC_TRY(launch_gemm(g, s, &prof, tag(TAG_BERT_OPROJ)));
    MEC_TRY(prof.begin(tag(TAG_BERT_LN), s));
    MEC_TRY(launch_bert_layernorm(r.t32, r.n, p.g1, p.b1, nullptr, r.op, r.st1, s, plo(nh), std::ldexp(1.0f, x.s_ln1)));
    MEC_TRY(prof.end(tag(TAG_BERT_LN), s));
    g = GemmParams();
    operands(g, r.op, nh, w.wi); g.oscale = x.scale[2];
    g.bias = p.bi; g.act = gelu_act; planes_out(g, r.ffn, nf); g.cscale = std::ldexp(1.0f, x.s_ffn);
    g.M = r.n; g.N = BI; g.K = BH;
    MEC_TRY(launch_gemm(g, s, &prof, tag(TAG_BERT_FFN1)));
    g = GemmParams();
    operands(g, r.ffn, nf, w.wo2); g.oscale = x.scale[3];
    g.bias = p.bo2; g.R = r.t32; g.r_f32 = 1; g.r_stats = r.st1; g.r_g = p.g1; g.r_b = p.b1; g.C32 = r.h32;
    g.M = r.n; g.N = BH; g.K = BI;
    MEC_TRY(launch_gemm(g, s, &prof, tag(TAG_BERT_FFN2)));
    MEC_TRY(prof.begin(tag(TAG_BERT_LN), s));
    MEC_TRY(launch_bert_layernorm(r.h32, r.n, p.g2, p.b2, r.full_out ? r.h32 : nullptr, r.op, r.st2, s, plo(nh),
                                  std::ldexp(1.0f, x.s_ln2)));
    MEC_TRY(prof.end(tag(TAG_BERT_LN), s));
    return 0;
  };

  MEC_TRY(launch_bert_embed_ln(tb.ids, M, L, emb.as<float>(), h32, hs, s, MH, std::ldexp(1.0f, x3_s_emb), tb.posid));
  for (int l = 0; l < BLAYERS; ++l) {
    const LayerWeights<const f16> w = layer_weights(W, l);
    const X3Layer& x = x3_layers[l];
    // Q / K / V planes carry 2^s_q | 2^s_k | 2^s_v through the pre-scaled Wqkv planes and bqkv (x3b); the
    // scores are scaled back by qks = 1/8 2^-(s_q + s_k)
    const float* bqkv = x3b.as<float>() + (size_t)BQKV * l;
    const float qks = std::ldexp(0.125f, -(x.s_q + x.s_k));
    const bool last = l == BLAYERS - 1;
    GemmParams g;
    if (cls_last && last) {
      // [CLS]-only last layer (TextModel::forward): K / V for every token, the rest on the [CLS] rows
      if (pr)  // a paired row holds both planes
        MEC_TRY(gather_cls_rows(tb, {{h32, h32c, BH * 4}, {hs, hsc, BH * 4}, {st2, st2c, 8}}, s));
      else
        MEC_TRY(gather_cls_rows(
            tb, {{h32, h32c, BH * 4}, {hs, hsc, BH * 2}, {hs + MH, hsc + NSH, BH * 2}, {st2, st2c, 8}}, s));
      const long long kvlo = plo((long long)M * 2 * BH);
      operands(g, hs, MH, w.wqkv + (size_t)BH * BH); g.oscale = x.scale[0];
      g.bias = bqkv + BH; planes_out(g, bigs, kvlo); g.M = M; g.N = 2 * BH; g.K = BH;
      MEC_TRY(launch_gemm(g, s, &prof, TAG_NONE));  // K | V planes [M, 1536]
      g = GemmParams();
      operands(g, hsc, NSH, w.wqkv); g.oscale = x.scale[0];
      g.bias = bqkv; planes_out(g, qsc, NSH); g.M = NS; g.N = BH; g.K = BH;
      MEC_TRY(launch_gemm(g, s, &prof, TAG_NONE));  // Q planes of the [CLS] rows
      MEC_TRY(launch_bert_attention_x3_cls(bigs, kvlo, tb.mask, qsc, NSH, csc, NSH, NS, qks, s, tb.cidx));
      MEC_TRY(tail(l, {NS, h32c, t32c, csc, hsc, fsc, st1c, st2c, /*deferred_in=*/true, /*full_out=*/true, /*tagged=*/false}));
      break;
    }
    // QKV projection + attention fused (Q / K / V stay on chip). The fused kernel sums in the K-interleaved
    // term order only, so with gemm_x3_order 0 (pass-major) the split GEMM + attention pair runs instead
    // and every split product of the forward keeps one term order
    if (opt().bert_qkv_attn == 1 && L == ATT_L && opt().gemm_x3_order == 1) {
      MEC_TRY(prof.begin(TAG_BERT_QKV, s));
      MEC_TRY(launch_bert_qkv_attn_x3(hs, MH, wmat(w.wqkv), wlo, x.scale[0], bqkv, tb.mask, cs, MH, B, qks, s, pk != nullptr));
      MEC_TRY(prof.end(TAG_BERT_QKV, s));
    } else {
      const long long qlo = plo((long long)M * BQKV);
      operands(g, hs, MH, w.wqkv); g.oscale = x.scale[0];
      g.bias = bqkv; planes_out(g, bigs, qlo); g.M = M; g.N = BQKV; g.K = BH;
      MEC_TRY(launch_gemm(g, s, &prof, TAG_BERT_QKV));
      MEC_TRY(prof.begin(TAG_BERT_ATTN, s));
      MEC_TRY(launch_bert_attention_x3(bigs, qlo, tb.mask, cs, MH, B, qks, s, pk != nullptr));
      MEC_TRY(prof.end(TAG_BERT_ATTN, s));
    }
    MEC_TRY(tail(l, {M, h32, t32, cs, hs, bigs, st1, st2, /*deferred_in=*/l != 0, /*full_out=*/last, /*tagged=*/true}));
  }
  return text_outputs(tb, P, h32, h32c, cls_last, pooled, cls, logits, probs, s);
}

}  // namespace mec
