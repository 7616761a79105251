// BERT-base encoder + sequence-classification head (the arithmetic the reference runs
// through transformers' BertForSequenceClassification: inference/text_inference.py:41,
// :92-93, :124-128; transformers==4.30.0 eager attention, requirements.txt:16).
//
// Per layer (M = B*L token rows; residual stream kept in fp32, GEMM operands in f16):
//   qkv16  = h16 . Wqkv^T + b                    gemm (N=2304)
//   ctx16  = softmax(QK^T/8 + mask_bias) V       bert_attention_kernel (MFMA, LDS)
//   t32    = ctx16 . Wo^T + bo + h               gemm, f32 out (residual fused)
//   h      = LN(t32)  -> h16 + (mean, rstd)      layernorm_kernel (eps 1e-12)
//   i16    = GELU(h16 . Wi^T + bi)               gemm (N=3072), erf-GELU fused
//   t32    = i16 . Wo2^T + bo2 + h               gemm, f32 out
//   h      = LN(t32)
// The f32 LN output h is never written (except after the embedding and the last layer):
// the residual add that consumes it reads the pre-LN sum and the row (mean, rstd) and
// re-evaluates the LN expression in its epilogue. The pre-LN sums alternate between two
// f32 buffers (O-proj: h32 -> t32, FFN2: t32 -> h32). Saves a 4-byte write per element
// per LayerNorm.
// Head: cls = h32[:,0,:] (pre-pooler CLS feature, text_inference.py:125);
//       probs = softmax(Wc tanh(Wp cls + bp) + bc).
#include "bert_model.h"

namespace mec {

// ----------------------------------------------------------------------------- embed+LN
// One wave per token row; each lane owns 12 of the 768 features (3 float4).
__global__ __launch_bounds__(256) void bert_embed_ln_kernel(const int32_t* __restrict__ ids, int M, int L,
                                                            const float* __restrict__ word,
                                                            const float* __restrict__ pos,
                                                            const float* __restrict__ type,
                                                            const float* __restrict__ g,
                                                            const float* __restrict__ b, float* h32,
                                                            f16* h16, long long lo, float up, unsigned* flag,
                                                            const int32_t* __restrict__ posid) {
  // posid (or null): the position id of every row in place of row % L (the packed path: a token's
  // offset inside its own sentence)
  // lo != 0 (the fp32x3 path): h16 is a hi plane and h16 + lo the lo plane of y up (hi = f16(y up),
  // lo = f16(y up - hi); up = 2^s, the planes' scale); a value outside the f16 range raises `flag`
  // (x3_raise)
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  int id = ids[row];
  id = id < 0 ? 0 : (id >= BVOCAB ? BVOCAB - 1 : id);
  const int l = posid ? min(max(posid[row], 0), BMAXPOS - 1) : row % L;
  float v[12];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int c = j * 256 + lane * 4;
    const float4 w = *reinterpret_cast<const float4*>(word + (size_t)id * BH + c);
    const float4 t = *reinterpret_cast<const float4*>(type + c);
    const float4 p = *reinterpret_cast<const float4*>(pos + (size_t)l * BH + c);
    // HF: (inputs_embeds + token_type_embeddings) + position_embeddings
    v[4 * j + 0] = (w.x + t.x) + p.x;
    v[4 * j + 1] = (w.y + t.y) + p.y;
    v[4 * j + 2] = (w.z + t.z) + p.z;
    v[4 * j + 3] = (w.w + t.w) + p.w;
  }
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 12; ++i) s += v[i];
  const float mean = wave_sum(s) * (1.0f / BH);
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < 12; ++i) { const float d = v[i] - mean; q += d * d; }
  const float rstd = 1.0f / sqrtf(wave_sum(q) * (1.0f / BH) + 1e-12f);
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int c = j * 256 + lane * 4;
    float4 o;
    o.x = (v[4 * j + 0] - mean) * rstd * g[c + 0] + b[c + 0];
    o.y = (v[4 * j + 1] - mean) * rstd * g[c + 1] + b[c + 1];
    o.z = (v[4 * j + 2] - mean) * rstd * g[c + 2] + b[c + 2];
    o.w = (v[4 * j + 3] - mean) * rstd * g[c + 3] + b[c + 3];
    *reinterpret_cast<float4*>(h32 + (size_t)row * BH + c) = o;
    if (h16 && lo) {
      const float4 u = make_float4(o.x * up, o.y * up, o.z * up, o.w * up);
      const half4 hh = {(f16)u.x, (f16)u.y, (f16)u.z, (f16)u.w};
      const half4 hl = {(f16)(u.x - (float)hh[0]), (f16)(u.y - (float)hh[1]), (f16)(u.z - (float)hh[2]),
                        (f16)(u.w - (float)hh[3])};
      *reinterpret_cast<half4*>(h16 + x3_at(lo, row, c, BH, 0)) = hh;  // (lo = kX3Paired: paired planes)
      *reinterpret_cast<half4*>(h16 + x3_at(lo, row, c, BH, 1)) = hl;
      x3_raise(flag, x3_out_of_range4(u));
    } else if (h16) {  // f16 path (null on the fp32 path)
      const half4 hh = {(f16)o.x, (f16)o.y, (f16)o.z, (f16)o.w};
      *reinterpret_cast<half4*>(h16 + (size_t)row * BH + c) = hh;
    }
  }
}

// ----------------------------------------------------------------------------- LayerNorm
// RW rows per wave (RW = 2: both rows' loads in flight before either reduction; option
// bert_ln_rows). Each row's arithmetic is the same at any RW: same bits.
template <int RW>
__global__ __launch_bounds__(256) void bert_layernorm_kernel(const float* x, int M,
                                                             const float* __restrict__ g,
                                                             const float* __restrict__ b, float* h32,
                                                             f16* h16, float2* stats, long long lo,
                                                             float up, unsigned* flag) {
  // h32 may be null: the consumer of the f32 output (the next residual add) then
  // re-derives it from x and `stats` in its GEMM epilogue (GemmParams::r_stats)
  const int lane = threadIdx.x & 63;
  const int row0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * RW;
  if (row0 >= M) return;
  float v[RW][12];
  float4 gg[3], bb[3];
#pragma unroll
  for (int r = 0; r < RW; ++r) {
    const int row = min(row0 + r, M - 1);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const float4 t = *reinterpret_cast<const float4*>(x + (size_t)row * BH + j * 256 + lane * 4);
      v[r][4 * j + 0] = t.x; v[r][4 * j + 1] = t.y; v[r][4 * j + 2] = t.z; v[r][4 * j + 3] = t.w;
    }
  }
  // gamma/beta issued together with the row loads: after the reductions they would sit
  // behind the (possibly aliasing) stores, one load->store round trip per float4
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    gg[j] = *reinterpret_cast<const float4*>(g + j * 256 + lane * 4);
    bb[j] = *reinterpret_cast<const float4*>(b + j * 256 + lane * 4);
  }
#pragma unroll
  for (int r = 0; r < RW; ++r) {
    const int row = row0 + r;
    if (row >= M) break;
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 12; ++i) s += v[r][i];
    const float mean = wave_sum(s) * (1.0f / BH);
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < 12; ++i) { const float d = v[r][i] - mean; q += d * d; }
    const float rstd = 1.0f / sqrtf(wave_sum(q) * (1.0f / BH) + 1e-12f);
    if (stats && lane == 0) stats[row] = make_float2(mean, rstd);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int c = j * 256 + lane * 4;
      float4 o;
      o.x = __builtin_fmaf((v[r][4 * j + 0] - mean) * rstd, gg[j].x, bb[j].x);
      o.y = __builtin_fmaf((v[r][4 * j + 1] - mean) * rstd, gg[j].y, bb[j].y);
      o.z = __builtin_fmaf((v[r][4 * j + 2] - mean) * rstd, gg[j].z, bb[j].z);
      o.w = __builtin_fmaf((v[r][4 * j + 3] - mean) * rstd, gg[j].w, bb[j].w);
      if (h32) *reinterpret_cast<float4*>(h32 + (size_t)row * BH + c) = o;
      if (h16 && lo) {  // fp32x3 path: planes of o up (up = 2^s, the planes' scale) and the range guard
        const float4 u = make_float4(o.x * up, o.y * up, o.z * up, o.w * up);
        const half4 hh = {(f16)u.x, (f16)u.y, (f16)u.z, (f16)u.w};
        const half4 hl = {(f16)(u.x - (float)hh[0]), (f16)(u.y - (float)hh[1]), (f16)(u.z - (float)hh[2]),
                          (f16)(u.w - (float)hh[3])};
        *reinterpret_cast<half4*>(h16 + x3_at(lo, row, c, BH, 0)) = hh;  // (lo = kX3Paired: paired planes)
        *reinterpret_cast<half4*>(h16 + x3_at(lo, row, c, BH, 1)) = hl;
        x3_raise(flag, x3_out_of_range4(u));
      } else if (h16) {  // f16 path (null on the fp32 path)
        const half4 hh = {(f16)o.x, (f16)o.y, (f16)o.z, (f16)o.w};
        *reinterpret_cast<half4*>(h16 + (size_t)row * BH + c) = hh;
      }
    }
  }
}

static void launch_ln_rows(const float* x, int M, const float* g, const float* b, float* h32, f16* h16, float2* st,
                           hipStream_t s, long long lo, float up) {
  unsigned* fl = lo ? range_flag() : nullptr;
  if (opt().bert_ln_rows == 4)
    hipLaunchKernelGGL(bert_layernorm_kernel<4>, dim3((M + 15) / 16), dim3(256), 0, s, x, M, g, b, h32, h16, st, lo, up,
                       fl);
  else if (opt().bert_ln_rows == 2)
    hipLaunchKernelGGL(bert_layernorm_kernel<2>, dim3((M + 7) / 8), dim3(256), 0, s, x, M, g, b, h32, h16, st, lo, up,
                       fl);
  else
    hipLaunchKernelGGL(bert_layernorm_kernel<1>, dim3((M + 3) / 4), dim3(256), 0, s, x, M, g, b, h32, h16, st, lo, up,
                       fl);
}

// Host launchers (also used by the fp32 path, bert_f32.hip). One wave per token row.
int launch_bert_embed_ln(const int32_t* ids, int M, int L, const float* emb, float* h32, f16* h16, hipStream_t s,
                         long long lo, float up, const int32_t* posid) {
  const float* word = emb;
  const float* pos = word + (size_t)BVOCAB * BH;
  const float* type = pos + (size_t)BMAXPOS * BH;
  const float* lng = type + 2 * BH;
  const float* lnb = lng + BH;
  hipLaunchKernelGGL(bert_embed_ln_kernel, dim3((M + 3) / 4), dim3(256), 0, s, ids, M, L, word, pos, type, lng, lnb,
                     h32, h16, lo, up, lo ? range_flag() : nullptr, posid);
  MEC_LAUNCH_CHECK();
  return 0;
}

// ----------------------------------------------------------------------------- sentence packing
// The packed text path (mec_text_fwd_packed): sample i's len[i] tokens sit in slots off[i] .. off[i] +
// len[i] - 1 of the 128-slot row row[i]. One workgroup per packed row, one thread per slot: the slot's
// owner is the sample of this row with the largest off <= slot (the plan fills a row from slot 0 with
// no gaps), its segment id the number of this row's samples that start before the owner. From the
// padded ids [B, 128] it writes per slot the token id (0 when unused), the position id (the offset
// inside the sentence; an unused slot's own index) and the uint8 segment id (255 when unused: the
// unused slots attend only to each other, so their rows stay finite and inside the fp32x3 plane
// bounds, which hold for any LayerNorm output); and per sample its [CLS] slot row * 128 + off. Every
// index read from the plan is clamped, so a bad plan gives wrong numbers, not a bad address.
__global__ __launch_bounds__(128) void bert_pack_kernel(const int32_t* __restrict__ ids,
                                                        const int32_t* __restrict__ row,
                                                        const int32_t* __restrict__ off,
                                                        const int32_t* __restrict__ len, int B, int Bp,
                                                        int32_t* __restrict__ pids, int32_t* __restrict__ ppos,
                                                        uint8_t* __restrict__ seg, int32_t* __restrict__ cidx) {
  const int r = blockIdx.x, t = threadIdx.x;
  int owner = -1, ooff = -1, before = 0;
  for (int i = 0; i < B; ++i) {
    if (row[i] != r) continue;
    const int o = off[i];
    if (o > t) continue;
    ++before;
    if (o > ooff) { ooff = o; owner = i; }
  }
  int id = 0, ps = t, sg = 255;
  if (owner >= 0 && t - ooff < len[owner] && ooff >= 0) {
    id = ids[(size_t)owner * ATT_L + (t - ooff)];
    ps = t - ooff;
    sg = min(before - 1, 254);
  }
  const size_t slot = (size_t)r * ATT_L + t;
  pids[slot] = id;
  ppos[slot] = ps;
  seg[slot] = (uint8_t)sg;
  for (int i = r * ATT_L + t; i < B; i += Bp * ATT_L)
    cidx[i] = min(max(row[i], 0), Bp - 1) * ATT_L + min(max(off[i], 0), ATT_L - 1);
}

int launch_bert_pack(const int32_t* ids, const TextPack& pk, int Bp, int32_t* pids, int32_t* ppos, uint8_t* seg,
                     int32_t* cidx, hipStream_t s) {
  hipLaunchKernelGGL(bert_pack_kernel, dim3(Bp), dim3(ATT_L), 0, s, ids, pk.row, pk.off, pk.len, pk.ns, Bp, pids,
                     ppos, seg, cidx);
  MEC_LAUNCH_CHECK();
  return 0;
}

int launch_bert_layernorm(const float* x, int M, const float* g, const float* b, float* h32, f16* h16, float2* stats,
                          hipStream_t s, long long lo, float up) {
  launch_ln_rows(x, M, g, b, h32, h16, stats, s, lo, up);
  MEC_LAUNCH_CHECK();
  return 0;
}

// ----------------------------------------------------------------------------- attention
// One workgroup per (sequence, head), L = 128 (padding='max_length', text_inference.py:
// 81-83). Wave w owns queries 32w..32w+31. S^T = K Q^T is computed so that each lane holds
// one query's scores (keys in registers): the row softmax is lane-local plus one
// cross-half shuffle, and the f32 score tile becomes the B operand of O^T = V^T P^T with
// no LDS round trip (k order permuted; V^T is read to match). V stays row-major in LDS
// (one 16-B write per loaded chunk); its V^T fragments come from ds_read_b64_tr_b16, the
// gfx950 transposed read (4 keys x 16 d per 16-lane group, delivered column-major).
__device__ __forceinline__ int aswz(int row, int kc) { return kc ^ ((row >> 1) & 7); }
// V rows: chunk kc ^ 4 on rows with bit 1 set, so a 32-lane half's four rows x 64 B of a
// transposed read cover all 64 banks
__device__ __forceinline__ int vswz(int row, int kc) { return kc ^ (((row >> 1) & 1) << 2); }
typedef short s16x4 __attribute__((__vector_size__(4 * sizeof(short))));
__device__ __forceinline__ half4 lds_tr16(const f16* p) {
  const s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)p);
  return __builtin_bit_cast(half4, v);
}

// One (sequence, head) on 4 waves (wave w: queries 32w .. 32w+31) from Q, K (aswz rows)
// and V (vswz rows) in LDS; sQ's rows are reused to stage the output, which is written to
// ctx_row0 (query row 0 of this sequence and head, row stride BH).
// NOUT < 32: only the wave's first NOUT query rows are stored (the [CLS]-only last layer: 1).
// PACK: sBias holds the row's segment ids (stage_mask<1>); the query's own slot is 32 wave + lr, or
// cls_slot for the [CLS]-only form.
template <int NOUT = 32, int PACK = 0>
__device__ __forceinline__ void attn_head(f16* sQ, const f16* sK, const f16* sV, const float* sBias, int wave,
                                          int lane, f16* ctx_row0, int cls_slot = 0) {
  const int lr = lane & 31, lh = lane >> 5;
  const int qseg = mask_qseg<PACK>(sBias, NOUT == 32 ? 32 * wave + lr : cls_slot);
  floatx16 s[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
#pragma unroll
    for (int e = 0; e < 16; ++e) s[t][e] = 0.f;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const int kc = 2 * kk + lh;
      const int rk = 32 * t + lr, rq = 32 * wave + lr;
      const half8 a = *reinterpret_cast<const half8*>(sK + rk * BDH + aswz(rk, kc) * 8);
      const half8 bq = *reinterpret_cast<const half8*>(sQ + rq * BDH + aswz(rq, kc) * 8);
      s[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, bq, s[t], 0, 0, 0);
    }
  }
  // s[t][e] = S[query 32w+lr][key 32t + (e&3) + 8(e>>2) + 4lh]
  float mx = -INFINITY;
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int key = 32 * t + (e & 3) + 8 * (e >> 2) + 4 * lh;
      const float v = s[t][e] * 0.125f + mask_term<PACK>(sBias, key, qseg);  // /sqrt(64) then + additive mask
      s[t][e] = v;
      mx = fmaxf(mx, v);
    }
  mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
  float sum = 0.f;
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      // exp(v - mx) as one v_exp_f32 of (v - mx) log2(e): the libm expf's range reduction and
      // denormal fix-ups cost ~4x the instructions (64 exps per lane per head)
      const float p = __builtin_amdgcn_exp2f((s[t][e] - mx) * 1.44269504088896341f);
      s[t][e] = p;
      sum += p;
    }
  sum += __shfl_xor(sum, 32, 64);
  const float inv = 1.0f / sum;

  floatx16 o[2];
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int e = 0; e < 16; ++e) o[u][e] = 0.f;
  // transposed-read lane roles: lane 4q + p of each 16-lane group addresses key row q of the
  // block, d columns 4p .. 4p+3; the group's 16 columns are d = 32u + 16 ((lane >> 4) & 1) + ..
  const int tq = (lane >> 2) & 3, tp = lane & 3, tg = (lane >> 4) & 1;
#pragma unroll
  for (int st = 0; st < 8; ++st) {
    const int t = st >> 1, sp = st & 1;
    half8 pb;
#pragma unroll
    for (int j = 0; j < 8; ++j) pb[j] = (f16)(s[t][8 * sp + j] * inv);
    const int kq = 32 * t + 16 * sp + 4 * lh + tq;  // keys kb..kb+3 (j<4) and kb+8..kb+11 (j>=4)
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int dc = 32 * u + 16 * tg + 4 * tp;
      // lane gets V[kb + 0..3][d = 32u + lr] and V[kb + 8..11][d]
      const half4 lo = lds_tr16(sV + kq * BDH + vswz(kq, dc >> 3) * 8 + (dc & 7));
      const half4 hi = lds_tr16(sV + (kq + 8) * BDH + vswz(kq + 8, dc >> 3) * 8 + (dc & 7));
      half8 va = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      o[u] = __builtin_amdgcn_mfma_f32_32x32x16_f16(va, pb, o[u], 0, 0, 0);
    }
  }
  // o[u][e] = O[query 32w+lr][d = 32u + (e&3) + 8(e>>2) + 4lh]. Staged through this wave's
  // own 32 rows of sQ (only this wave read them, in S^T), then written as whole 128-B head
  // rows: 8-B stores straight from the MFMA layout touch 32 rows per instruction.
  {
    f16* so = sQ + (32 * wave + lr) * BDH;
    const int rq = 32 * wave + lr;
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int gq = 0; gq < 4; ++gq) {
        half4 hv = {(f16)o[u][4 * gq + 0], (f16)o[u][4 * gq + 1], (f16)o[u][4 * gq + 2], (f16)o[u][4 * gq + 3]};
        const int d = 32 * u + 8 * gq + 4 * lh;  // 16-B chunk d >> 3 of the row, half (d >> 2) & 1
        *reinterpret_cast<half4*>(so + aswz(rq, d >> 3) * 8 + (d & 7)) = hv;
      }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // wave-local rows: no barrier needed
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = 64 * i + lane, r = 32 * wave + (c >> 3), kc = c & 7;
    const uint4 v = *reinterpret_cast<const uint4*>(sQ + r * BDH + aswz(r, kc) * 8);
    if (NOUT == 32 || (c >> 3) < NOUT) *reinterpret_cast<uint4*>(ctx_row0 + (size_t)r * BH + kc * 8) = v;
  }
}

template <int PACK = 0>  // PACK: mask = the rows' segment ids (stage_mask)
__global__ __launch_bounds__(256) void bert_attention_kernel(const f16* __restrict__ qkv,
                                                             const int32_t* __restrict__ mask,
                                                             f16* __restrict__ ctx) {
  __shared__ __attribute__((aligned(16))) f16 sQ[ATT_L * BDH];
  __shared__ __attribute__((aligned(16))) f16 sK[ATT_L * BDH];
  __shared__ __attribute__((aligned(16))) f16 sV[ATT_L * BDH];
  __shared__ float sBias[ATT_L];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x / BHEADS, h = blockIdx.x - (blockIdx.x / BHEADS) * BHEADS;
  const f16* base = qkv + (size_t)b * ATT_L * (3 * BH) + h * BDH;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = tid + 256 * i;
    const int row = c >> 3, kc = c & 7;
    const f16* src = base + (size_t)row * (3 * BH) + kc * 8;
    const uint4 q = *reinterpret_cast<const uint4*>(src);
    const uint4 k = *reinterpret_cast<const uint4*>(src + BH);
    const uint4 v = *reinterpret_cast<const uint4*>(src + 2 * BH);
    *reinterpret_cast<uint4*>(sQ + row * BDH + aswz(row, kc) * 8) = q;
    *reinterpret_cast<uint4*>(sK + row * BDH + aswz(row, kc) * 8) = k;
    *reinterpret_cast<uint4*>(sV + row * BDH + vswz(row, kc) * 8) = v;
  }
  stage_mask<PACK>(sBias, mask, b, tid);
  __syncthreads();
  attn_head<32, PACK>(sQ, sK, sV, sBias, wave, lane, ctx + (size_t)b * ATT_L * BH + h * BDH);
}

// [CLS]-only attention of BERT's last layer (bert_cls_last): K | V of every token from the K / V
// GEMM ([B*128, 1536], kv), the [CLS] query row from qc ([B, 768]), the context written compact
// ([B, 768]). Wave 0 runs attn_head for queries 0..31 with Q rows 1..31 zero (an MFMA output column
// depends only on its own B column): the [CLS] row has bert_attention_kernel's bits.
// PACK: workgroup (b, h) serves sample b, whose [CLS] slot is cidx[b] = row * 128 + off: K / V and the
// segment ids are those of packed row `row`, the query's segment that of slot `off`.
template <int PACK = 0>
__global__ __launch_bounds__(256) void bert_attention_cls_kernel(const f16* __restrict__ kv,
                                                                 const int32_t* __restrict__ mask,
                                                                 const f16* __restrict__ qc,
                                                                 f16* __restrict__ ctx,
                                                                 const int32_t* __restrict__ cidx) {
  __shared__ __attribute__((aligned(16))) f16 sQ[32 * BDH];
  __shared__ __attribute__((aligned(16))) f16 sK[ATT_L * BDH];
  __shared__ __attribute__((aligned(16))) f16 sV[ATT_L * BDH];
  __shared__ float sBias[ATT_L];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x / BHEADS, h = blockIdx.x - (blockIdx.x / BHEADS) * BHEADS;
  const int cs = PACK ? cidx[b] : 0;
  const int bk = PACK ? cs >> 7 : b;  // the row whose K / V this sample reads
  const f16* base = kv + (size_t)bk * ATT_L * (2 * BH) + h * BDH;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = tid + 256 * i;
    const int row = c >> 3, kc = c & 7;
    const f16* src = base + (size_t)row * (2 * BH) + kc * 8;
    const uint4 k = *reinterpret_cast<const uint4*>(src);
    const uint4 v = *reinterpret_cast<const uint4*>(src + BH);
    *reinterpret_cast<uint4*>(sK + row * BDH + aswz(row, kc) * 8) = k;
    *reinterpret_cast<uint4*>(sV + row * BDH + vswz(row, kc) * 8) = v;
  }
  {
    const int row = tid >> 3, kc = tid & 7;  // 32 rows x 8 chunks
    const uint4 z = make_uint4(0u, 0u, 0u, 0u);
    const uint4 q = row == 0 ? *reinterpret_cast<const uint4*>(qc + (size_t)b * BH + h * BDH + kc * 8) : z;
    *reinterpret_cast<uint4*>(sQ + row * BDH + aswz(row, kc) * 8) = q;
  }
  stage_mask<PACK>(sBias, mask, bk, tid);
  __syncthreads();
  if (wave == 0) attn_head<1, PACK>(sQ, sK, sV, sBias, 0, lane, ctx + (size_t)b * BH + h * BDH, cs & 127);
}

// ----------------------------------------------------------------------------- fp32x3 attention
// The attention of one (sequence, head) on split operands, after K / V (aswz / vswz rows, hi and lo
// planes) and the mask bias are in LDS and this lane's Q fragments (row 32 wave + lr, k chunks
// 2 kk + lh; hi and lo) are in registers: S^T = K Q^T (three f16 products per fp32 product), fp32
// softmax, O^T = V^T P^T on split P / V, O -> hi / lo planes staged through this wave's own rows of
// sK and stored to ctx (row stride BH; lo plane at + clo; CLS: query 0 only). `wave` is the wave's
// index among the four serving this head; every wave of the workgroup reaches the barrier.
// PACK: sBias holds the row's segment ids (stage_mask<1>); the query's slot is 32 wave + lr (CLS: cls_slot).
template <int CLS, int PACK = 0>
__device__ __forceinline__ void attn_head_x3(f16* const (&sK)[2], const f16* const (&sV)[2], const float* sBias,
                                             const half8 (&qh)[4], const half8 (&ql)[4], int wave, int lane, f16* ctx,
                                             long long clo, int b, int h, float qks, int cls_slot = 0) {
  const int lr = lane & 31, lh = lane >> 5;
  const int qseg = mask_qseg<PACK>(sBias, CLS ? cls_slot : 32 * wave + lr);
  floatx16 s[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
#pragma unroll
    for (int e = 0; e < 16; ++e) s[t][e] = 0.f;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const int kc = 2 * kk + lh;
      const int rk = 32 * t + lr;
      const half8 ah = *reinterpret_cast<const half8*>(sK[0] + rk * BDH + aswz(rk, kc) * 8);
      const half8 al = *reinterpret_cast<const half8*>(sK[1] + rk * BDH + aswz(rk, kc) * 8);
      s[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, qh[kk], s[t], 0, 0, 0);
      s[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, ql[kk], s[t], 0, 0, 0);
      s[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, qh[kk], s[t], 0, 0, 0);
    }
  }
  if constexpr (!CLS) __syncthreads();  // every wave is done with sK: its rows stage the output below
  float mx = -INFINITY;
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int key = 32 * t + (e & 3) + 8 * (e >> 2) + 4 * lh;
      const float v = s[t][e] * qks + mask_term<PACK>(sBias, key, qseg);  // qks = 1/8 2^-(s_q + s_k) (Q, K planes at 2^s_q, 2^s_k): exact
      s[t][e] = v;
      mx = fmaxf(mx, v);
    }
  mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
  float sum = 0.f;
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const float p = expf(s[t][e] - mx);
      s[t][e] = p;
      sum += p;
    }
  sum += __shfl_xor(sum, 32, 64);
  const float inv = 1.0f / sum;

  floatx16 o[2];
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int e = 0; e < 16; ++e) o[u][e] = 0.f;
  const int tq = (lane >> 2) & 3, tp = lane & 3, tg = (lane >> 4) & 1;
#pragma unroll
  for (int st = 0; st < 8; ++st) {
    const int t = st >> 1, sp = st & 1;
    half8 ph, pl8;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float pv = (s[t][8 * sp + j] * inv) * 4096.f;
      ph[j] = (f16)pv;
      pl8[j] = (f16)(pv - (float)ph[j]);
    }
    const int kq = 32 * t + 16 * sp + 4 * lh + tq;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int dc = 32 * u + 16 * tg + 4 * tp;
      half8 vh, vl;
      {
        const half4 a = lds_tr16(sV[0] + kq * BDH + vswz(kq, dc >> 3) * 8 + (dc & 7));
        const half4 c = lds_tr16(sV[0] + (kq + 8) * BDH + vswz(kq + 8, dc >> 3) * 8 + (dc & 7));
        vh = half8{a[0], a[1], a[2], a[3], c[0], c[1], c[2], c[3]};
      }
      {
        const half4 a = lds_tr16(sV[1] + kq * BDH + vswz(kq, dc >> 3) * 8 + (dc & 7));
        const half4 c = lds_tr16(sV[1] + (kq + 8) * BDH + vswz(kq + 8, dc >> 3) * 8 + (dc & 7));
        vl = half8{a[0], a[1], a[2], a[3], c[0], c[1], c[2], c[3]};
      }
      o[u] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vl, ph, o[u], 0, 0, 0);
      o[u] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vh, pl8, o[u], 0, 0, 0);
      o[u] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vh, ph, o[u], 0, 0, 0);
    }
  }
  // O = o 2^-12 -> hi / lo planes, staged through this wave's own rows of sK[0] / sK[1]
  const int rq = 32 * wave + lr;
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int gq = 0; gq < 4; ++gq) {
      half4 hv, lv;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float x = o[u][4 * gq + e] * (1.0f / 4096.f);
        hv[e] = (f16)x;
        lv[e] = (f16)(x - (float)hv[e]);
      }
      const int d = 32 * u + 8 * gq + 4 * lh;
      *reinterpret_cast<half4*>(sK[0] + rq * BDH + aswz(rq, d >> 3) * 8 + (d & 7)) = hv;
      *reinterpret_cast<half4*>(sK[1] + rq * BDH + aswz(rq, d >> 3) * 8 + (d & 7)) = lv;
    }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // wave-local rows: no barrier needed
  const size_t row0 = (size_t)b * (CLS ? 1 : ATT_L);  // (clo = kX3Paired: the context planes are paired)
#pragma unroll
  for (int pl = 0; pl < 2; ++pl)
#pragma unroll
    for (int i = 0; i < (CLS ? 1 : 4); ++i) {
      const int c = 64 * i + lane, r = 32 * wave + (c >> 3), kc = c & 7;
      const uint4 v = *reinterpret_cast<const uint4*>(sK[pl] + r * BDH + aswz(r, kc) * 8);
      if (!CLS || r == 0) *reinterpret_cast<uint4*>(ctx + x3_at(clo, row0 + r, h * BDH + kc * 8, BH, pl)) = v;
    }
}

// The fp32 attention of one (sequence, head) on split-f16 operands (the MEC_PREC_FP32X3 path):
// Q, K, V arrive as f16 hi / lo planes (qkv, qkv + lo; the split QKV GEMM's output) and every
// product is hi.hi + hi.lo + lo.hi into an fp32 accumulator, as in the split GEMM:
//   S^T = K Q^T      3 v_mfma_f32_32x32x16_f16 per 16-deep k step (K_lo Q_hi, K_hi Q_lo, K_hi Q_hi)
//   P   = softmax(S / 8 + mask_bias) in fp32 with libm expf (the fp32 path's arithmetic)
//   O^T = V^T P^T    P (x 2^12, exact, so its small entries stay out of the f16 subnormals) split
//                    into hi / lo in registers, 3 MFMAs per step; O scaled back by 2^-12
// Layout and lane roles are attn_head's (keys in registers, one cross-half shuffle per row,
// transposed V reads); Q goes straight to registers (each wave reads only its own 32 query
// rows), so 64 KB of LDS (K, V planes) lets two workgroups share a CU and one's loads overlap
// the other's MFMAs. The output is staged per wave in K's rows (free after the score loop) and
// written as hi / lo planes (ctx, ctx + clo) for the split O-projection.
// CLS = 1 (BERT's last layer with bert_cls_last: only the [CLS] query's context is read): qkv holds
// K | V only ([B*128, 1536] planes, the K / V GEMM's output), the [CLS] query comes from qc ([B, 768]
// planes, lo at qc + qclo) and the context is written compact ([B, 768] planes). All four waves
// stage K and V; wave 0 then runs the full kernel's instruction sequence for queries 0..31 with Q
// zero for all but query 0 (an MFMA output column depends only on its own B column), so the [CLS]
// context has the full kernel's bits; waves 1-3 leave after staging.
// PACK: mask = the rows' segment ids (stage_mask); with CLS, workgroup (b, h) serves sample b, whose [CLS]
// slot is cidx[b] = row * 128 + off (K / V and segment ids of packed row `row`, the query's segment that of
// slot `off`).
template <int CLS = 0, int PACK = 0>
__global__ __launch_bounds__(256, 2) void bert_attention_x3_kernel(const f16* __restrict__ qkv, long long lo,
                                                                   const int32_t* __restrict__ mask,
                                                                   f16* __restrict__ ctx, long long clo,
                                                                   const f16* __restrict__ qc, long long qclo, float qks,
                                                                   const int32_t* __restrict__ cidx) {
  constexpr int LD = CLS ? 2 * BH : 3 * BH;  // row stride of qkv
  constexpr int KO = CLS ? 0 : BH;           // K column offset (V at KO + BH)
  __shared__ __attribute__((aligned(16))) f16 sK[2][ATT_L * BDH];
  __shared__ __attribute__((aligned(16))) f16 sV[2][ATT_L * BDH];
  __shared__ float sBias[ATT_L];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x / BHEADS, h = blockIdx.x - (blockIdx.x / BHEADS) * BHEADS;
  const int lr = lane & 31, lh = lane >> 5;
  const int cs = (CLS && PACK) ? cidx[b] : 0;
  const int bk = (CLS && PACK) ? cs >> 7 : b;  // the row whose K / V are staged
  half8 qh[4], ql[4];  // this lane's Q row 32 wave + lr, k chunks 2 kk + lh (the MFMA B operand)
  if constexpr (CLS) {
    const bool own = wave == 0 && lr == 0;
    // (lo / qclo / clo = kX3Paired: that tensor's planes are paired, x3_at)
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
#pragma unroll
      for (int j = 0; j < 8; ++j) { qh[kk][j] = (f16)0.f; ql[kk][j] = (f16)0.f; }
      if (own) {
        qh[kk] = *reinterpret_cast<const half8*>(qc + x3_at(qclo, b, h * BDH + (2 * kk + lh) * 8, BH, 0));
        ql[kk] = *reinterpret_cast<const half8*>(qc + x3_at(qclo, b, h * BDH + (2 * kk + lh) * 8, BH, 1));
      }
    }
  } else {
    const size_t qr = (size_t)b * ATT_L + 32 * wave + lr;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      qh[kk] = *reinterpret_cast<const half8*>(qkv + x3_at(lo, qr, h * BDH + (2 * kk + lh) * 8, LD, 0));
      ql[kk] = *reinterpret_cast<const half8*>(qkv + x3_at(lo, qr, h * BDH + (2 * kk + lh) * 8, LD, 1));
    }
  }
#pragma unroll
  for (int pl = 0; pl < 2; ++pl) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = tid + 256 * i;
      const int row = c >> 3, kc = c & 7;
      const size_t kr = (size_t)bk * ATT_L + row;
      const uint4 k = *reinterpret_cast<const uint4*>(qkv + x3_at(lo, kr, KO + h * BDH + kc * 8, LD, pl));
      const uint4 v = *reinterpret_cast<const uint4*>(qkv + x3_at(lo, kr, KO + BH + h * BDH + kc * 8, LD, pl));
      *reinterpret_cast<uint4*>(sK[pl] + row * BDH + aswz(row, kc) * 8) = k;
      *reinterpret_cast<uint4*>(sV[pl] + row * BDH + vswz(row, kc) * 8) = v;
    }
  }
  stage_mask<PACK>(sBias, mask, bk, tid);
  __syncthreads();
  if (CLS && wave != 0) return;
  f16* const sKp[2] = {sK[0], sK[1]};
  const f16* const sVp[2] = {sV[0], sV[1]};
  attn_head_x3<CLS, PACK>(sKp, sVp, sBias, qh, ql, wave, lane, ctx, clo, b, h, qks, cs & 127);
}

int launch_bert_attention_x3(const f16* qkv, long long lo, const int32_t* mask, f16* ctx, long long clo, int B,
                             float qks, hipStream_t s, bool packed) {
  if (packed)
    hipLaunchKernelGGL((bert_attention_x3_kernel<0, 1>), dim3(B * BHEADS), dim3(256), 0, s, qkv, lo, mask, ctx, clo,
                       nullptr, 0LL, qks, nullptr);
  else
    hipLaunchKernelGGL((bert_attention_x3_kernel<0, 0>), dim3(B * BHEADS), dim3(256), 0, s, qkv, lo, mask, ctx, clo,
                       nullptr, 0LL, qks, nullptr);
  MEC_LAUNCH_CHECK();
  return 0;
}

int launch_bert_attention_x3_cls(const f16* kv, long long lo, const int32_t* mask, const f16* qc, long long qclo,
                                 f16* ctx, long long clo, int B, float qks, hipStream_t s, const int32_t* cidx) {
  if (cidx)
    hipLaunchKernelGGL((bert_attention_x3_kernel<1, 1>), dim3(B * BHEADS), dim3(256), 0, s, kv, lo, mask, ctx, clo,
                       qc, qclo, qks, cidx);
  else
    hipLaunchKernelGGL((bert_attention_x3_kernel<1, 0>), dim3(B * BHEADS), dim3(256), 0, s, kv, lo, mask, ctx, clo,
                       qc, qclo, qks, nullptr);
  MEC_LAUNCH_CHECK();
  return 0;
}

// ----------------------------------------------------------------------------- QKV + attention
// The QKV projection and the attention of one (sequence, head pair) in one workgroup, so Q,
// K and V never go through HBM (unfused: a 151-MB write by the QKV GEMM and the same read by
// the attention kernel per layer at B = 256):
//   * a 128 (tokens) x 384 (Q | K | V of heads 2hp, 2hp+1) x 768 GEMM tile, 8 waves (2 x 4,
//     wave tile 64 x 96), v_mfma_f32_16x16x32_f16 computed transposed (out^T = W . X^T, so a
//     lane holds 4 consecutive features of one token), A and B staged HBM -> LDS by
//     global_load_lds_dwordx4 in two 64-KB stages (128-B rows, kc ^ ((row>>1)&7) swizzle);
//   * the epilogue adds the bias exactly as the GEMM epilogue does ((acc + b) + 0, f16) and
//     writes Q, K, V straight into the attention's LDS images (aswz / vswz rows);
//   * each 4-wave half then runs attn_head on one head.
// Same k order as the QKV GEMM tiles and the same attention code: ctx is bit-identical to
// the unfused pair (tests/test_gpu_parity.py::test_text_qkv_attn_bit_identical).
constexpr int QA_BM = 128, QA_BN = 384, QA_BK = 64, QA_NK = BH / QA_BK;
constexpr int QA_STAGE = (QA_BM + QA_BN) * QA_BK;  // halfs per stage (64 KB)

// HP heads per workgroup: HP = 2, 8 waves on the 128 x 384 tile, 64-KB stages, one workgroup per CU;
// HP = 1 (bert_qkv_attn_heads 1), 4 waves (2 x 2 of the same 64 x 96 wave tile) on a 128 x 192 tile,
// 40-KB stages and 80 KB of LDS in all (the mask bias inside it), so two workgroups share a CU and one's
// attention overlaps the other's GEMM. Same sums in the same order: the same bits.
// PACK: mask = the rows' segment ids (stage_mask), nseq the number of packed rows.
template <int DBG = 0, int HP = 2, int PACK = 0>  // probe builds (wrong results): DBG 1 = no attention, 2 = main loop only
__global__ __launch_bounds__(256 * HP, HP == 1 ? 2 : 1) void bert_qkv_attn_kernel(const f16* __restrict__ h16,
                                                                                  const f16* __restrict__ wqkv,
                                                                                  const float* __restrict__ bqkv,
                                                                                  const int32_t* __restrict__ mask,
                                                                                  f16* __restrict__ ctx, int nseq) {
  static_assert(HP == 1 || HP == 2, "heads per workgroup");
  constexpr int NW = 4 * HP, WNC = 2 * HP;        // waves; waves along N
  constexpr int STAGE = (QA_BM + 192 * HP) * QA_BK;  // halfs per stage (64 / 40 KB)
  constexpr int IT = (QA_BM + 192 * HP) / 8 / NW;  // 8-row wave-instructions per stage per wave
  constexpr int IMG = ATT_L * BDH;
  static_assert(IT * 8 * NW == QA_BM + 192 * HP, "loader");
  static_assert(HP == 2 || 3 * IMG + 2 * ATT_L <= 2 * STAGE, "mask bias past the Q / K / V images");
  __shared__ __attribute__((aligned(16))) f16 smem[2 * STAGE];  // 2 GEMM stages, then Q/K/V images
  __shared__ float sBias2[HP == 2 ? ATT_L : 1];
  float* const sBias = HP == 2 ? sBias2 : reinterpret_cast<float*>(smem + 3 * IMG);
  typedef __attribute__((address_space(3))) void* lds_p;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WNC, wn = wave % WNC;
  const int l16 = lane & 15, lq = lane >> 4;
  // XCD-aware bijective remap: the 12 / HP head groups of a sequence (which share its 192-KB token
  // rows) run on one XCD's L2
  constexpr int NG = BHEADS / HP;
  const int nwg = nseq * NG;
  int bid = blockIdx.x;
  {
    const int xcd = bid & 7, q = nwg >> 3, r = nwg & 7;
    bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
  }
  const int b = bid / NG, hp = bid - (bid / NG) * NG;

  // stage loader: LDS row R < 128 = token row R of the sequence; R >= 128 = W row
  // seg * 768 + (HP hp) * 64 + j for n = R - 128 = seg * 64 HP + j (the Q, K, V blocks of the heads)
  const int lrow = lane >> 3, pch = lane & 7;
  const f16* src0[IT];
#pragma unroll
  for (int it = 0; it < IT; ++it) {
    const int R = (it * NW + wave) * 8 + lrow;  // 8 NW rows per pass of the waves
    const int c = pch ^ ((R >> 1) & 7);
    if (R < QA_BM) {
      src0[it] = h16 + ((size_t)b * ATT_L + R) * BH + c * 8;
    } else {
      const int n = R - QA_BM, seg = n / (64 * HP), j = n - seg * (64 * HP);
      src0[it] = wqkv + ((size_t)seg * BH + hp * 64 * HP + j) * BH + c * 8;
    }
  }
  auto issue = [&](int kt, int st) {
    f16* base = smem + st * STAGE;
#pragma unroll
    for (int it = 0; it < IT; ++it)
      __builtin_amdgcn_global_load_lds((const void*)(src0[it] + kt * QA_BK), (lds_p)(base + (it * NW + wave) * 8 * QA_BK),
                                       16, 0, 0);
  };

  floatx4 acc[4][6];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 6; ++j) acc[i][j] = floatx4{0.f, 0.f, 0.f, 0.f};
  issue(0, 0);
  issue(1, 1);
#pragma unroll 1
  for (int kt = 0; kt < QA_NK; ++kt) {
    if (kt + 1 < QA_NK)
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(IT) : "memory");
    else
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // stage kt landed for every wave
    const f16* sA = smem + (kt & 1) * STAGE;
    const f16* sB = sA + QA_BM * QA_BK;
    half8 af[2][4], bf[2][6];
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      const int kc = 4 * s2 + lq;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int r = 64 * wm + 16 * i + l16;
        af[s2][i] = *reinterpret_cast<const half8*>(sA + r * QA_BK + (kc ^ ((r >> 1) & 7)) * 8);
      }
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        const int r = 96 * wn + 16 * j + l16;  // B row (feature); its LDS row is QA_BM + r
        const int rr = QA_BM + r;
        bf[s2][j] = *reinterpret_cast<const half8*>(sB + r * QA_BK + (kc ^ ((rr >> 1) & 7)) * 8);
      }
    }
    // the stage is free as soon as every wave holds its fragments: restage it for kt + 2
    // BEFORE the MFMAs, so the DMA has two K steps of MFMAs to land
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // every wave is done reading stage kt
    if (kt + 2 < QA_NK) issue(kt + 2, kt & 1);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 6; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bf[s2][j], af[s2][i], acc[i][j], 0, 0, 0);
  }

  if constexpr (DBG == 2) {
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 6; ++j) t += acc[i][j][0] + acc[i][j][1] + acc[i][j][2] + acc[i][j][3];
    if (t == 12345.678f) ctx[tid] = (f16)t;
    return;
  }
  // ---- epilogue: (acc + bias) + 0 -> f16 -> the attention's Q / K / V LDS images (every wave is past
  // its last stage read: the loop's second barrier)
  stage_mask<PACK>(sBias, mask, b, tid);
  f16* img = smem;  // [Q (HP heads) | K | V], each [128][64]
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    const int n = 96 * wn + 16 * j + 4 * lq;  // features n .. n+3 (one 64-column head block)
    const int seg = n / (64 * HP), hh = (n - seg * 64 * HP) >> 6, d = n & 63;
    const float4 bv = *reinterpret_cast<const float4*>(bqkv + seg * BH + (hp * HP + hh) * 64 + d);
    const float bb[4] = {bv.x, bv.y, bv.z, bv.w};
    f16* dst = img + (seg * HP + hh) * IMG;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = 64 * wm + 16 * i + l16;  // token
      half4 hv;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float v = acc[i][j][e] + bb[e];
        v += 0.f;
        hv[e] = (f16)v;
      }
      const int ch = seg == 2 ? vswz(m, d >> 3) : aswz(m, d >> 3);
      *reinterpret_cast<half4*>(dst + m * BDH + ch * 8 + (d & 7)) = hv;
    }
  }
  __syncthreads();
  if constexpr (DBG == 1) {
    if (img[tid] == (f16)12345.f) ctx[tid] = img[tid + 1];
    return;
  }
  const int hh = wave >> 2;
  attn_head<32, PACK>(img + hh * IMG, img + (HP + hh) * IMG, img + (2 * HP + hh) * IMG, sBias, wave & 3, lane,
                      ctx + (size_t)b * ATT_L * BH + (HP * hp + hh) * BDH);
}

// ----------------------------------------------------------------------------- fp32x3 QKV + attention
// The fp32x3 path's QKV projection and attention of one (sequence, head pair) in one workgroup, as
// bert_qkv_attn_kernel does on the f16 path, so the Q / K / V hi / lo planes (302 MB per layer at
// B = 256 written by the split QKV GEMM and read back by bert_attention_x3_kernel) never reach HBM:
//   * the 128 (tokens) x 384 (Q | K | V of heads 2 hp, 2 hp + 1) x 768 split GEMM tile: 8 waves
//     (2 x 4, wave tile 64 x 96) on v_mfma_f32_16x16x32_f16 computed transposed (out^T = W . X^T),
//     32-deep K stages holding the hi AND lo tiles of the token rows and the weight rows (64 KB;
//     two stages, restaged for k + 2 as soon as every wave holds its fragments), and per k chunk the
//     K-interleaved split engine's three terms in its order (X_lo W_hi, X_hi W_lo, X_hi W_hi);
//   * the epilogue computes (acc 2^-e + b) + 0 and its hi / lo planes exactly as the split GEMM's
//     epilogue, in two phases through the freed stages: the Q planes first, from which every
//     attention wave loads its query fragments into registers, then the K / V planes (aswz / vswz
//     rows: 128 KB for both heads);
//   * each 4-wave half runs attn_head_x3 (bert_attention_x3_kernel's body) on one head.
// Same products, term order and k order as the split QKV GEMM, the same attention code: the context
// planes are bit-identical to the unfused pair (tests/test_gpu_fp32x3.py).
constexpr int QX_BK = 32, QX_NK = BH / QX_BK;       // 24 K steps of 32

__device__ __forceinline__ int qx_sw(int row, int kc) { return kc ^ ((4 - ((row >> 2) & 3)) & 3); }  // sw<32>

// HP heads per workgroup: HP = 2, 8 waves (2 x 4, wave tile 64 x 96) on a 128 x 384 tile, 64-KB stages,
// one workgroup per CU; HP = 1, 4 waves (2 x 2, the same 64 x 96 wave tile) on a 128 x 192 tile, 40-KB
// stages and 80 KB of LDS in all, so two workgroups share a CU and one's attention phase overlaps the
// other's GEMM. Both sum every output in the same term and k order: the same bits.
// PACK: mask = the rows' segment ids (stage_mask), nseq the number of packed rows.
template <int HP, int PACK = 0, int PAIR = 0>
__global__ __launch_bounds__(256 * HP, HP == 1 ? 2 : 1) void bert_qkv_attn_x3_kernel(
    const f16* __restrict__ hs, long long hlo, const f16* __restrict__ wqkv, long long wlo, float oscale,
    const float* __restrict__ bqkv, const int32_t* __restrict__ mask, f16* __restrict__ ctx, long long clo, int nseq,
    float qks, unsigned* flag, int late_dma) {
  static_assert(HP == 1 || HP == 2, "heads per workgroup");
  constexpr int NW = 4 * HP, WNC = 2 * HP;             // waves; waves along N
  constexpr int QBN = 192 * HP;                        // Q | K | V columns of the HP heads
  constexpr int PLANE = (QA_BM + QBN) * QX_BK;         // halfs per plane of a stage
  constexpr int STAGE = 2 * PLANE;                     // hi + lo planes (64 / 40 KB)
  constexpr int IT = (QA_BM + QBN) / 16 / NW;          // 16-row wave-instructions per plane per wave
  constexpr int IMG = ATT_L * BDH;                     // halfs per [128][64] image plane
  static_assert(IT * 16 * NW == QA_BM + QBN, "loader");
  static_assert(2 * STAGE >= 4 * HP * IMG, "K / V images (and before them the Q images) fit in the stages");
  // 2 GEMM stages, then the Q, then the K / V images; HP = 1 keeps the mask bias in the stages too
  // (past the K / V images), so the workgroup's LDS is exactly 80 KB
  __shared__ __attribute__((aligned(16))) f16 smem[2 * STAGE];
  __shared__ float sBias2[HP == 2 ? ATT_L : 1];
  float* const sBias = HP == 2 ? sBias2 : reinterpret_cast<float*>(smem + 4 * IMG);
  static_assert(HP == 2 || 4 * IMG + 2 * ATT_L <= 2 * STAGE, "mask bias past the K / V images");
  typedef __attribute__((address_space(3))) void* lds_p;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WNC, wn = wave % WNC;
  const int l16 = lane & 15, lq = lane >> 4;
  // XCD-aware bijective remap: the 12 / HP head groups of a sequence (which share its token rows) on one XCD
  constexpr int NG = BHEADS / HP;
  const int nwg = nseq * NG;
  int bid = blockIdx.x;
  {
    const int xcd = bid & 7, q = nwg >> 3, r = nwg & 7;
    bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
  }
  const int b = bid / NG, hp = bid - (bid / NG) * NG;

  // stage loader: LDS row R < 128 = token row R of the sequence; R >= 128 = weight row
  // seg * 768 + (HP hp) * 64 + j for n = R - 128 = seg * 64 HP + j; 16 rows of 64 B per wave-instruction
  // PAIR (hs and wqkv paired, [rows][2 x 768]; hlo / wlo unused): a stage is 128 + QBN rows of 64 halfs, the
  // K chunk's hi halfs in 16-B chunks 0-3 and its lo halfs in 4-7 (swizzled as the GEMM engine's 128-B rows,
  // chunk c of row R at c ^ ((R >> 1) & 7)), filled by 8-row x 128-B pieces: whole cache lines, and as many
  // pieces per wave and stage as the planar form's 16-row x 64-B ones
  constexpr int NP = PAIR ? 2 * IT : IT;  // source pointers per lane
  const int lrow = PAIR ? lane >> 3 : lane >> 2, pch = PAIR ? lane & 7 : lane & 3;
  const f16* src[NP];
  long long lo_off[PAIR ? 1 : IT];
#pragma unroll
  for (int it = 0; it < NP; ++it) {
    const int R = (it * NW + wave) * (PAIR ? 8 : 16) + lrow;
    const int c = PAIR ? pch ^ ((R >> 1) & 7) : qx_sw(R, pch);
    constexpr int LD = PAIR ? 2 * BH : BH;
    if (R < QA_BM) {
      src[it] = hs + ((size_t)b * ATT_L + R) * LD + c * 8;
      if constexpr (!PAIR) lo_off[it] = hlo;
    } else {
      const int n = R - QA_BM, seg = n / (64 * HP), j = n - seg * (64 * HP);
      src[it] = wqkv + ((size_t)seg * BH + hp * 64 * HP + j) * LD + c * 8;
      if constexpr (!PAIR) lo_off[it] = wlo;
    }
  }
  auto issue = [&](int kt, int st) {
    f16* base = smem + st * STAGE;
    if constexpr (PAIR) {
#pragma unroll
      for (int it = 0; it < NP; ++it)
        __builtin_amdgcn_global_load_lds((const void*)(src[it] + kt * 64), (lds_p)(base + (it * NW + wave) * 8 * 64),
                                         16, 0, 0);
    } else {
#pragma unroll
      for (int pl = 0; pl < 2; ++pl)
#pragma unroll
        for (int it = 0; it < IT; ++it)
          __builtin_amdgcn_global_load_lds((const void*)(src[it] + (pl ? lo_off[it] : 0) + kt * QX_BK),
                                           (lds_p)(base + pl * PLANE + (it * NW + wave) * 16 * QX_BK), 16, 0, 0);
    }
  };
  // fragment of plane pl of stage row r, 16-B k chunk kc
  auto frag = [&](const f16* sA, int pl, int r, int kc) {
    if constexpr (PAIR) return *reinterpret_cast<const half8*>(sA + r * 64 + ((4 * pl + kc) ^ ((r >> 1) & 7)) * 8);
    else return *reinterpret_cast<const half8*>(sA + pl * PLANE + r * QX_BK + qx_sw(r, kc) * 8);
  };

  floatx4 acc[4][6];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 6; ++j) acc[i][j] = floatx4{0.f, 0.f, 0.f, 0.f};
  issue(0, 0);
  issue(1, 1);
#pragma unroll 1
  for (int kt = 0; kt < QX_NK; ++kt) {
    if (kt + 1 < QX_NK)
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * IT) : "memory");
    else
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // stage kt landed for every wave
    const f16* sA = smem + (kt & 1) * STAGE;
    half8 af[2][4], bf[2][6];  // [plane: 0 hi, 1 lo]
#pragma unroll
    for (int pl = 0; pl < 2; ++pl) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int r = 64 * wm + 16 * i + l16;
        af[pl][i] = frag(sA, pl, r, lq);
      }
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        const int rr = QA_BM + 96 * wn + 16 * j + l16;
        bf[pl][j] = frag(sA, pl, rr, lq);
      }
    }
    // the stage is free once every wave holds its fragments: restage it for kt + 2 before the MFMAs
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    // late_dma (opt().qkv_x3_late_dma, HP = 1): every other 256-block of workgroups -- the second resident
    // workgroup of a CU in the first dispatch pass -- issues the stage refill after its first MFMA term group
    // (1) or its second (2), so the two workgroups' waves on a SIMD do not both sit in DMA issue while the
    // matrix core idles; the refill still has the rest of this step and all of the next to land. Same bits
    const bool late = late_dma && ((blockIdx.x >> 8) & 1);
    if (kt + 2 < QX_NK && !late) issue(kt + 2, kt & 1);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 6; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bf[0][j], af[1][i], acc[i][j], 0, 0, 0);
    if (kt + 2 < QX_NK && late && late_dma == 1) {
      __builtin_amdgcn_sched_barrier(0);
      issue(kt + 2, kt & 1);
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 6; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bf[1][j], af[0][i], acc[i][j], 0, 0, 0);
    if (kt + 2 < QX_NK && late && late_dma == 2) {
      __builtin_amdgcn_sched_barrier(0);
      issue(kt + 2, kt & 1);
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 6; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bf[0][j], af[0][i], acc[i][j], 0, 0, 0);
  }
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __syncthreads();  // every wave is past its last stage read: the stages become the Q / K / V images

  // ---- epilogue: v = (acc 2^-e + b) + 0 (the split GEMM epilogue's expression), hi = f16(v),
  // lo = f16(v - hi). Images: [seg][head][plane] = [128][64] halfs, seg 0 Q / 1 K / 2 V
  stage_mask<PACK>(sBias, mask, b, tid);
  bool bad = false;
  auto write_seg = [&](int want, f16* img) {
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      const int n = 96 * wn + 16 * j + 4 * lq;  // features n .. n+3 (one 64-column head block)
      const int seg = n / (64 * HP), hh = (n - seg * 64 * HP) >> 6, d = n & 63;
      if (seg != want) continue;
      const float4 bv = *reinterpret_cast<const float4*>(bqkv + seg * BH + (hp * HP + hh) * 64 + d);
      const float bb[4] = {bv.x, bv.y, bv.z, bv.w};
      // hi plane of this (segment, head); its lo plane follows (Q: [head][plane]; K / V: [seg-1][head][plane])
      f16* dst = img + (want == 0 ? 2 * hh : 2 * (HP * (seg - 1) + hh)) * IMG;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int m = 64 * wm + 16 * i + l16;  // token
        half4 hv, lv;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float v = __builtin_fmaf(acc[i][j][e], oscale, bb[e]);
          v += 0.f;
          hv[e] = (f16)v;
          lv[e] = (f16)(v - (float)hv[e]);
          bad |= x3_out_of_range(v);
        }
        const int ch = seg == 2 ? vswz(m, d >> 3) : aswz(m, d >> 3);
        *reinterpret_cast<half4*>(dst + m * BDH + ch * 8 + (d & 7)) = hv;
        *reinterpret_cast<half4*>(dst + IMG + m * BDH + ch * 8 + (d & 7)) = lv;
      }
    }
  };
  // phase 1: Q planes of the heads ([head][plane] at smem), then every wave's query fragments
  write_seg(0, smem);
  __syncthreads();
  const int hh = wave >> 2, aw = wave & 3;  // this wave's head (of the group) and its index among that head's 4
  const int lr = lane & 31, lh = lane >> 5;
  half8 qh[4], ql[4];
  {
    const f16* qi = smem + hh * 2 * IMG;
    const int rq = 32 * aw + lr;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const int kc = 2 * kk + lh;
      qh[kk] = *reinterpret_cast<const half8*>(qi + rq * BDH + aswz(rq, kc) * 8);
      ql[kk] = *reinterpret_cast<const half8*>(qi + IMG + rq * BDH + aswz(rq, kc) * 8);
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __syncthreads();
  // phase 2: K and V planes ([K h0 hi, K h0 lo, (K h1 ..), V h0 hi, ..] at smem)
  write_seg(1, smem);
  write_seg(2, smem);
  x3_raise(flag, bad);
  __syncthreads();
  f16* const sK[2] = {smem + (0 * HP + hh) * 2 * IMG, smem + ((0 * HP + hh) * 2 + 1) * IMG};
  const f16* const sV[2] = {smem + (1 * HP + hh) * 2 * IMG, smem + ((1 * HP + hh) * 2 + 1) * IMG};
  attn_head_x3<0, PACK>(sK, sV, sBias, qh, ql, aw, lane, ctx, clo, b, HP * hp + hh, qks);
}

int launch_bert_qkv_attn_x3(const f16* hs, long long hlo, const f16* wqkv, long long wlo, float oscale,
                            const float* bqkv, const int32_t* mask, f16* ctx, long long clo, int B, float qks,
                            hipStream_t s, bool packed) {
  const int one = opt().bert_qkv_attn_x3_heads == 1;
  MEC_REQUIRE((hlo == kX3Paired) == (wlo == kX3Paired), "bert_qkv_attn_x3: hs and wqkv are paired together");
  if (hlo == kX3Paired) {  // paired operand planes (the context planes: clo says which)
    if (one && packed)
      hipLaunchKernelGGL((bert_qkv_attn_x3_kernel<1, 1, 1>), dim3(B * 12), dim3(256), 0, s, hs, hlo, wqkv, wlo, oscale,
                         bqkv, mask, ctx, clo, B, qks, range_flag(), opt().qkv_x3_late_dma);
    else if (packed)
      hipLaunchKernelGGL((bert_qkv_attn_x3_kernel<2, 1, 1>), dim3(B * 6), dim3(512), 0, s, hs, hlo, wqkv, wlo, oscale,
                         bqkv, mask, ctx, clo, B, qks, range_flag(), 0);
    else if (one)
      hipLaunchKernelGGL((bert_qkv_attn_x3_kernel<1, 0, 1>), dim3(B * 12), dim3(256), 0, s, hs, hlo, wqkv, wlo, oscale,
                         bqkv, mask, ctx, clo, B, qks, range_flag(), opt().qkv_x3_late_dma);
    else
      hipLaunchKernelGGL((bert_qkv_attn_x3_kernel<2, 0, 1>), dim3(B * 6), dim3(512), 0, s, hs, hlo, wqkv, wlo, oscale,
                         bqkv, mask, ctx, clo, B, qks, range_flag(), 0);
  } else if (one && packed)
    hipLaunchKernelGGL((bert_qkv_attn_x3_kernel<1, 1>), dim3(B * 12), dim3(256), 0, s, hs, hlo, wqkv, wlo, oscale, bqkv,
                       mask, ctx, clo, B, qks, range_flag(), opt().qkv_x3_late_dma);
  else if (packed)
    hipLaunchKernelGGL((bert_qkv_attn_x3_kernel<2, 1>), dim3(B * 6), dim3(512), 0, s, hs, hlo, wqkv, wlo, oscale, bqkv,
                       mask, ctx, clo, B, qks, range_flag(), 0);
  else if (one)
    hipLaunchKernelGGL((bert_qkv_attn_x3_kernel<1, 0>), dim3(B * 12), dim3(256), 0, s, hs, hlo, wqkv, wlo, oscale, bqkv,
                       mask, ctx, clo, B, qks, range_flag(), opt().qkv_x3_late_dma);
  else
    hipLaunchKernelGGL((bert_qkv_attn_x3_kernel<2, 0>), dim3(B * 6), dim3(512), 0, s, hs, hlo, wqkv, wlo, oscale, bqkv,
                       mask, ctx, clo, B, qks, range_flag(), 0);
  MEC_LAUNCH_CHECK();
  return 0;
}

// ----------------------------------------------------------------------------- f16 attention launchers
// kv: K | V of every token [rows * 128, 1536]; qc, ctx: the samples' [CLS] query / context rows [NS, 768];
// cidx (or null): the packed form (mask = segment ids, sample b's [CLS] slot cidx[b])
int launch_bert_attention_cls(const f16* kv, const int32_t* mask, const f16* qc, f16* ctx, int NS, hipStream_t s,
                              const int32_t* cidx) {
  if (cidx)
    hipLaunchKernelGGL(bert_attention_cls_kernel<1>, dim3(NS * BHEADS), dim3(256), 0, s, kv, mask, qc, ctx, cidx);
  else
    hipLaunchKernelGGL(bert_attention_cls_kernel<0>, dim3(NS * BHEADS), dim3(256), 0, s, kv, mask, qc, ctx, nullptr);
  MEC_LAUNCH_CHECK();
  return 0;
}

// packed: mask holds the rows' uint8 segment ids and B counts packed rows (both launchers below)
int launch_bert_qkv_attn(const f16* h16, const f16* wqkv, const float* bqkv, const int32_t* mask, f16* ctx, int B,
                         hipStream_t s, bool packed) {
#ifdef MEC_PROBES
  if (opt().bert_qkv_attn == 2)
    hipLaunchKernelGGL((bert_qkv_attn_kernel<1>), dim3(B * 6), dim3(512), 0, s, h16, wqkv, bqkv, mask, ctx, B);
  else if (opt().bert_qkv_attn == 3)
    hipLaunchKernelGGL((bert_qkv_attn_kernel<2>), dim3(B * 6), dim3(512), 0, s, h16, wqkv, bqkv, mask, ctx, B);
  else
#endif
  if (opt().bert_qkv_attn_heads == 1 && packed)
    hipLaunchKernelGGL((bert_qkv_attn_kernel<0, 1, 1>), dim3(B * 12), dim3(256), 0, s, h16, wqkv, bqkv, mask, ctx, B);
  else if (packed)
    hipLaunchKernelGGL((bert_qkv_attn_kernel<0, 2, 1>), dim3(B * 6), dim3(512), 0, s, h16, wqkv, bqkv, mask, ctx, B);
  else if (opt().bert_qkv_attn_heads == 1)
    hipLaunchKernelGGL((bert_qkv_attn_kernel<0, 1>), dim3(B * 12), dim3(256), 0, s, h16, wqkv, bqkv, mask, ctx, B);
  else
    hipLaunchKernelGGL((bert_qkv_attn_kernel<0>), dim3(B * 6), dim3(512), 0, s, h16, wqkv, bqkv, mask, ctx, B);
  MEC_LAUNCH_CHECK();
  return 0;
}

int launch_bert_attention(const f16* qkv, const int32_t* mask, f16* ctx, int B, hipStream_t s, bool packed) {
  if (packed)
    hipLaunchKernelGGL(bert_attention_kernel<1>, dim3(B * BHEADS), dim3(256), 0, s, qkv, mask, ctx);
  else
    hipLaunchKernelGGL(bert_attention_kernel<0>, dim3(B * BHEADS), dim3(256), 0, s, qkv, mask, ctx);
  MEC_LAUNCH_CHECK();
  return 0;
}

// ----------------------------------------------------------------------------- model
static void to_f16(std::vector<f16>& dst, size_t off, const float* src, size_t n) {
  for (size_t i = 0; i < n; ++i) dst[off + i] = (f16)src[i];
}

int TextModel::create(const float* blob, size_t n) {
  BlobReader rd(blob, n);
  std::vector<float> e;
  const float* word = rd.take((size_t)BVOCAB * BH);
  const float* pos = rd.take((size_t)BMAXPOS * BH);
  const float* type = rd.take(2 * BH);
  const float* lg = rd.take(BH);
  const float* lb = rd.take(BH);
  if (!rd.ok) { set_error("text blob too small"); return -1; }
  e.insert(e.end(), word, word + (size_t)BVOCAB * BH);
  e.insert(e.end(), pos, pos + (size_t)BMAXPOS * BH);
  e.insert(e.end(), type, type + 2 * BH);
  e.insert(e.end(), lg, lg + BH);
  e.insert(e.end(), lb, lb + BH);
  // f16 path: GEMM weights in f16 (wts); fp32 path: the same layout in f32 (wts32); fp32x3
  // path: built in f32, then split into f16 hi / lo planes (wts, below)
  const bool f32 = prec != PREC_F16;
  std::vector<f16> w(f32 ? 0 : WT_LAYER * BLAYERS);
  std::vector<float> w32(f32 ? WT_LAYER * BLAYERS : 0);
  // the next cnt blob floats -> matrix m of layer l (WT_OFF), from its element `off` on
  auto put = [&](int l, int m, size_t off, size_t cnt) {
    const float* src = rd.take(cnt);
    const size_t at = WT_LAYER * l + WT_OFF[m] + off;
    if (f32) std::copy(src, src + cnt, w32.begin() + at);
    else to_f16(w, at, src, cnt);
  };
  auto take_to = [&](float* dst, size_t cnt) {
    const float* x = rd.take(cnt);
    std::copy(x, x + cnt, dst);
  };
  std::vector<float> pr(PRM_FLOATS);
  for (int l = 0; l < BLAYERS; ++l) {
    const LayerParams<float> p = layer_params(pr.data(), l);
    // Wqkv rows: query | key | value (torch Linear weight [out,in] = GEMM B [N,K])
    for (int q = 0; q < 3; ++q) {
      put(l, 0, (size_t)q * BH * BH, (size_t)BH * BH);
      take_to(p.bqkv + q * BH, BH);
    }
    put(l, 1, 0, WT_SIZE[1]);
    take_to(p.bo, BH);
    take_to(p.g1, BH);
    take_to(p.b1, BH);
    put(l, 2, 0, WT_SIZE[2]);
    take_to(p.bi, BI);
    put(l, 3, 0, WT_SIZE[3]);
    take_to(p.bo2, BH);
    take_to(p.g2, BH);
    take_to(p.b2, BH);
  }
  float* head = pr.data() + PRM_LAYER * BLAYERS;
  const float* wp = rd.take((size_t)BH * BH);
  const float* bp = rd.take(BH);
  const float* wc = rd.take((size_t)BCLASSES * BH);
  const float* bc = rd.take(BCLASSES);
  MEC_REQUIRE(rd.ok && rd.off == n, "text blob size mismatch");
  for (int i = 0; i < BH; ++i)
    for (int j = 0; j < BH; ++j) head[HO_WPT + (size_t)i * BH + j] = wp[(size_t)j * BH + i];
  std::copy(bp, bp + BH, head + HO_BP);
  for (int i = 0; i < BH; ++i)
    for (int j = 0; j < BCLASSES; ++j) head[HO_WCT + (size_t)i * BCLASSES + j] = wc[(size_t)j * BH + i];
  std::copy(bc, bc + BCLASSES, head + HO_BC);
  MEC_TRY(upload(emb, e.data(), e.size() * sizeof(float)));
  if (prec == PREC_FP32X3) {
    // Activation-plane exponents from rigorous bounds (activation_exp, target 2^15, so no plane can
    // overflow): a LayerNorm output is at most sqrt(H - 1) max|gamma| + max|beta| (a zero-mean,
    // unit-variance row of H values has no entry above sqrt(H - 1)); a projection row j of such rows is
    // at most bound ||W_j||_1 + |b_j|, and GELU never grows it; the context is a convex combination of
    // V rows, so it shares V's exponent. Q, K and V get one exponent each: their weight rows and
    // biases are pre-scaled by 2^s_q | 2^s_k | 2^s_v before the split (exact), so one epilogue scale
    // serves the whole QKV GEMM; the scores carry 2^(s_q + s_k) (qks undoes it). Every consumer's
    // epilogue scale folds in 2^(s_out - s_in).
    auto ln_bound = [&](const float* g, const float* b) {
      double mg = 0.0, mb = 0.0;
      for (int i = 0; i < BH; ++i) {
        mg = std::max(mg, std::fabs((double)g[i]));
        mb = std::max(mb, std::fabs((double)b[i]));
      }
      return std::sqrt((double)BH - 1.0) * mg + mb;
    };
    auto proj_bound = [&](double in, const float* W, const float* b, int N, int K) {
      double mx = 0.0;
      for (int j = 0; j < N; ++j) {
        double l1 = 0.0;
        for (int k = 0; k < K; ++k) l1 += std::fabs((double)W[(size_t)j * K + k]);
        mx = std::max(mx, in * l1 + std::fabs((double)b[j]));
      }
      return mx;
    };
    double b_in = ln_bound(lg, lb);
    x3_s_emb = x3_exp(b_in, kX3BoundTarget);
    x3_note("emb_ln", x3_s_emb, b_in);
    x3_layers.assign(BLAYERS, X3Layer());
    std::vector<float> bq((size_t)BQKV * BLAYERS);
    const size_t total = WT_LAYER * BLAYERS;
    std::vector<f16> hl(2 * total);
    x3_lo = total;
    for (int l = 0; l < BLAYERS; ++l) {
      X3Layer& x = x3_layers[l];
      const LayerWeights<float> wl = layer_weights(w32.data(), l);
      const LayerParams<const float> pl = layer_params<const float>(pr.data(), l);
      const int s_in = l ? x3_layers[l - 1].s_ln2 : x3_s_emb;
      int sqkv[3];
      double bqkv3[3];
      for (int q = 0; q < 3; ++q) {
        bqkv3[q] = proj_bound(b_in, wl.wqkv + (size_t)q * BH * BH, pl.bqkv + q * BH, BH, BH);
        sqkv[q] = x3_exp(bqkv3[q], kX3BoundTarget);
      }
      const double b1 = ln_bound(pl.g1, pl.b1);
      x.s_ln1 = x3_exp(b1, kX3BoundTarget);
      const double bffn = proj_bound(b1, wl.wi, pl.bi, BI, BH);
      x.s_ffn = x3_exp(bffn, kX3BoundTarget);
      b_in = ln_bound(pl.g2, pl.b2);
      x.s_ln2 = x3_exp(b_in, kX3BoundTarget);
      const std::string ln = "layer" + std::to_string(l) + ".";
      x3_note(ln + "q", sqkv[0], bqkv3[0]);
      x3_note(ln + "k", sqkv[1], bqkv3[1]);
      x3_note(ln + "v", sqkv[2], bqkv3[2]);
      x3_note(ln + "ln1", x.s_ln1, b1);
      x3_note(ln + "ffn", x.s_ffn, bffn);
      x3_note(ln + "ln2", x.s_ln2, b_in);
      x.s_q = sqkv[0];
      x.s_k = sqkv[1];
      x.s_v = sqkv[2];
      for (int q = 0; q < 3; ++q) {
        float* wq = wl.wqkv + (size_t)q * BH * BH;
        for (size_t i = 0; i < (size_t)BH * BH; ++i) wq[i] = std::ldexp(wq[i], sqkv[q]);
        for (int j = 0; j < BH; ++j) bq[(size_t)BQKV * l + q * BH + j] = std::ldexp(pl.bqkv[q * BH + j], sqkv[q]);
      }
      // each GEMM's B matrix (Wqkv | Wo | Wi | Wo2 of a layer) scaled by 2^e (max |w| 2^e <= 2^14,
      // exact) and split into hi = f16(w 2^e) and lo = f16(w 2^e - hi) planes; the GEMM epilogue
      // multiplies the accumulator by 2^-e and the activation-plane factors (GemmParams::oscale)
      const int s_a[4] = {s_in, x.s_v, x.s_ln1, x.s_ffn};  // each GEMM's A operand planes' exponent
      for (int m = 0; m < 4; ++m) {
        const size_t off = WT_LAYER * l + WT_OFF[m];
        const float e2 = split_planes(w32.data() + off, WT_SIZE[m], hl.data() + off, hl.data() + total + off);
        x.scale[m] = std::ldexp(e2, -s_a[m]);
      }
    }
    MEC_TRY(upload(x3b, bq.data(), bq.size() * sizeof(float)));
    x3_paired = opts.x3_layout == 1 && opts.gemm_x3_order == 1;
    if (x3_paired) {  // the same planes, each matrix [N][K] paired at twice its planar offset
      std::vector<f16> pw(2 * total);
      for (int l = 0; l < BLAYERS; ++l)
        for (int m = 0; m < 4; ++m) {
          const size_t off = WT_LAYER * l + WT_OFF[m];
          const int K = m == 3 ? BI : BH;
          const size_t N = WT_SIZE[m] / K;
          for (size_t r = 0; r < N; ++r)
            for (int k = 0; k < K; ++k) {
              pw[2 * off + x3_pair_index(r, k, K, 0)] = hl[off + r * K + k];
              pw[2 * off + x3_pair_index(r, k, K, 1)] = hl[total + off + r * K + k];
            }
        }
      hl.swap(pw);
    }
    MEC_TRY(upload(wts, hl.data(), hl.size() * sizeof(f16)));
  } else if (f32) {
    MEC_TRY(upload(wts32, w32.data(), w32.size() * sizeof(float)));
  } else {
    MEC_TRY(upload(wts, w.data(), w.size() * sizeof(f16)));
  }
  MEC_TRY(upload(prm, pr.data(), pr.size() * sizeof(float)));
  return 0;
}

int TextModel::forward_packed(const int32_t* ids, const int32_t* row, const int32_t* off, const int32_t* len, int B,
                              int Bp, float* cls, float* logits, float* probs, hipStream_t s) {
  MEC_REQUIRE(B >= 0, "text: B < 0");
  if (B == 0) return 0;
  MEC_REQUIRE(ids && row && off && len && cls && logits && probs, "text: null pointer");
  MEC_REQUIRE(Bp >= 1 && Bp <= B, "text: a packed batch of B samples has 1 <= Bp <= B rows");
  const TextPack pk{row, off, len, B};
  return forward(ids, nullptr, Bp, ATT_L, cls, logits, probs, s, &pk);
}

// pk (or null): the packed form. B is then the number of packed rows, pk->ns the number of samples
// (bert_model.h TextBatch). Every buffer over token rows keeps M = B * 128; every compact [CLS]-row buffer
// has ns rows.
int TextModel::forward(const int32_t* ids, const int32_t* mask, int B, int L, float* cls, float* logits,
                       float* probs, hipStream_t s, const TextPack* pk) {
  MEC_REQUIRE(B >= 0, "text: B < 0");
  if (B == 0) return 0;
  MEC_REQUIRE(L == ATT_L, "text: L must be 128 (padding='max_length', MAX_TEXT_LENGTH=128)");
  MEC_REQUIRE(ids && (mask || pk) && cls && logits && probs, "text: null pointer");
  if (prec == PREC_FP32) return forward_f32(ids, mask, B, L, cls, logits, probs, s, pk);
  if (prec == PREC_FP32X3) return forward_x3(ids, mask, B, L, cls, logits, probs, s, pk);
  // workspace: h32 | t32 (f32 [M,768]) ; h16 | ctx16 (f16 [M,768]) ; qkv16 [M,2304] / i16 [M,3072]
  // + the [CLS]-row buffers of the last layer (bert_cls_last): h32c | t32c (f32 [NS,768]) ; h16c | qc |
  // ctxc (f16 [NS,768]) ; fc (f16 [NS,3072]) ; st1c | st2c ([NS] float2)
  float *h32, *t32, *pooled, *h32c, *t32c;
  f16 *h16, *ctx16, *big16, *h16c, *qc, *ctxc, *fc;
  float2 *st1, *st1c;
  TextBatch tb;
  MEC_TRY(text_prologue(tb, ws, ids, mask, B, pk, s, [&](Carver& c) {
    const size_t M = tb.M, NS = tb.NS;
    h32 = c.take<float>(M * BH);
    t32 = c.take<float>(M * BH);
    h16 = c.take<f16>(M * BH);
    ctx16 = c.take<f16>(M * BH);
    big16 = c.take<f16>(M * BI);  // qkv16 [M,2304] then i16 [M,3072]
    pooled = c.take<float>(NS * BH);
    st1 = c.take<float2>(M * 2);  // LN1 | LN2 row stats [M] each
    h32c = c.take<float>(NS * BH);
    t32c = c.take<float>(NS * BH);
    h16c = c.take<f16>(NS * BH);
    qc = c.take<f16>(NS * BH);
    ctxc = c.take<f16>(NS * BH);
    fc = c.take<f16>(NS * BI);
    st1c = c.take<float2>(NS * 2);
  }));
  const int M = tb.M, NS = tb.NS;
  float2* st2 = st1 + M;
  float2* st2c = st1c + NS;
  const bool cls_last = opt().bert_cls_last != 0;
  const f16* W = wts.as<f16>();
  const float* P = prm.as<float>();

  // Only the first LN (the embedding's) and the last write their f32 output. Every other residual add
  // re-derives it from the pre-LN sum and the row stats in its GEMM epilogue (r_stats). The f32 stream
  // ping-pongs, so no GEMM reads its own output (a launch stays idempotent: the tile autotuner re-runs
  // candidates on the same buffers).
  auto tail = [&](int l, const TailRows& r) -> int {
    const LayerWeights<const f16> w = layer_weights(W, l);
    const LayerParams<const float> p = layer_params(P, l);
    auto tag = [&](int t) { return r.tagged ? t : (int)TAG_NONE; };
    GemmParams g;
    g.A = r.ctx; g.B = w.wo; g.bias = p.bo; g.R = r.h32; g.r_f32 = 1; g.C32 = r.t32; g.M = r.n; g.N = BH; g.K = BH;
    if (r.deferred_in) { g.r_stats = r.st2; g.r_g = layer_params(P, l - 1).g2; g.r_b = layer_params(P, l - 1).b2; }
    MEC_TRY(launch_gemm(g, s, &prof, tag(TAG_BERT_OPROJ)));
    MEC_TRY(prof.begin(tag(TAG_BERT_LN), s));
    MEC_TRY(launch_bert_layernorm(r.t32, r.n, p.g1, p.b1, nullptr, r.op, r.st1, s));
    MEC_TRY(prof.end(tag(TAG_BERT_LN), s));
    g = GemmParams();
    g.A = r.op; g.B = w.wi; g.bias = p.bi; g.act = ACT_GELU; g.C16 = r.ffn; g.M = r.n; g.N = BI; g.K = BH;
    MEC_TRY(launch_gemm(g, s, &prof, tag(TAG_BERT_FFN1)));
    g = GemmParams();
    g.A = r.ffn; g.B = w.wo2; g.bias = p.bo2; g.R = r.t32; g.r_f32 = 1; g.r_stats = r.st1; g.r_g = p.g1; g.r_b = p.b1;
    g.C32 = r.h32; g.M = r.n; g.N = BH; g.K = BI;
    MEC_TRY(launch_gemm(g, s, &prof, tag(TAG_BERT_FFN2)));
    MEC_TRY(prof.begin(tag(TAG_BERT_LN), s));
    // in place: each wave holds its row in registers before writing it
    MEC_TRY(launch_bert_layernorm(r.h32, r.n, p.g2, p.b2, r.full_out ? r.h32 : nullptr, r.op, r.st2, s));
    MEC_TRY(prof.end(tag(TAG_BERT_LN), s));
    return 0;
  };

  MEC_TRY(launch_bert_embed_ln(tb.ids, M, L, emb.as<float>(), h32, h16, s, 0, 1.f, tb.posid));
  for (int l = 0; l < BLAYERS; ++l) {
    const LayerWeights<const f16> w = layer_weights(W, l);
    const LayerParams<const float> p = layer_params(P, l);
    const bool last = l == BLAYERS - 1;
    GemmParams g;
    if (cls_last && last) {
      // [CLS]-only last layer: K / V for every token, everything else on the NS [CLS] rows (the
      // pooler, logits and CLS feature read nothing else). Same kernels and expressions per row as
      // the full layer, so same bits.
      MEC_TRY(gather_cls_rows(tb, {{h32, h32c, BH * 4}, {h16, h16c, BH * 2}, {st2, st2c, 8}}, s));
      g.A = h16; g.B = w.wqkv + (size_t)BH * BH; g.bias = p.bqkv + BH; g.C16 = big16; g.M = M; g.N = 2 * BH; g.K = BH;
      MEC_TRY(launch_gemm(g, s, &prof, TAG_NONE));  // K | V [M, 1536]
      g = GemmParams();
      g.A = h16c; g.B = w.wqkv; g.bias = p.bqkv; g.C16 = qc; g.M = NS; g.N = BH; g.K = BH;
      MEC_TRY(launch_gemm(g, s, &prof, TAG_NONE));  // Q of the [CLS] rows
      MEC_TRY(launch_bert_attention_cls(big16, tb.mask, qc, ctxc, NS, s, tb.cidx));
      MEC_TRY(tail(l, {NS, h32c, t32c, ctxc, h16c, fc, st1c, st2c, /*deferred_in=*/true, /*full_out=*/true, /*tagged=*/false}));
      break;
    }
    if (opt().bert_qkv_attn) {
      MEC_TRY(prof.begin(TAG_BERT_ATTN, s));
      MEC_TRY(launch_bert_qkv_attn(h16, w.wqkv, p.bqkv, tb.mask, ctx16, B, s, pk != nullptr));
      MEC_TRY(prof.end(TAG_BERT_ATTN, s));
    } else {
      g.A = h16; g.B = w.wqkv; g.bias = p.bqkv; g.C16 = big16; g.M = M; g.N = BQKV; g.K = BH;
      MEC_TRY(launch_gemm(g, s, &prof, TAG_BERT_QKV));
      MEC_TRY(prof.begin(TAG_BERT_ATTN, s));
      MEC_TRY(launch_bert_attention(big16, tb.mask, ctx16, B, s, pk != nullptr));
      MEC_TRY(prof.end(TAG_BERT_ATTN, s));
    }
    MEC_TRY(tail(l, {M, h32, t32, ctx16, h16, big16, st1, st2, /*deferred_in=*/l != 0, /*full_out=*/last, /*tagged=*/true}));
  }
  return text_outputs(tb, P, h32, h32c, cls_last, pooled, cls, logits, probs, s);
}

}  // namespace mec
