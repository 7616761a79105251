// BERT-base's shape, the layout of TextModel's packed weights (wts / wts32 / prm), and the host steps the three
// text forwards (bert.hip: f16; bert_f32.hip: fp32, fp32x3) share: prologue, [CLS]-row gather, output tail.
#pragma once
#include "block_ops.h"
#include "models.h"

namespace mec {

constexpr int BH = 768, BI = 3072, BHEADS = 12, BDH = 64, BLAYERS = 12, BVOCAB = 30522, BMAXPOS = 512;
constexpr int ATT_L = 128;  // the sequence length every kernel here is built for
constexpr int BQKV = 3 * BH, BCLASSES = 7;

// ---------------------------------------------------------------- prm: per layer, then the head
// per layer (floats): bqkv 2304 | bo 768 | ln1g 768 | ln1b 768 | bi 3072 | bo2 768 | ln2g 768 | ln2b 768
constexpr size_t PO_BQKV = 0, PO_BO = PO_BQKV + BQKV, PO_G1 = PO_BO + BH, PO_B1 = PO_G1 + BH, PO_BI = PO_B1 + BH,
                 PO_BO2 = PO_BI + BI, PO_G2 = PO_BO2 + BH, PO_B2 = PO_G2 + BH, PRM_LAYER = PO_B2 + BH;
static_assert(PRM_LAYER == BQKV + 3 * BH + BI + 3 * BH, "per-layer parameter offsets sum to PRM_LAYER");
// head: WpT 768*768 | bp 768 | WcT 768*7 | bc 7 (the Linear weights transposed: [in][out])
constexpr size_t HO_WPT = 0, HO_BP = HO_WPT + (size_t)BH * BH, HO_WCT = HO_BP + BH,
                 HO_BC = HO_WCT + (size_t)BH * BCLASSES, HEAD_FLOATS = HO_BC + BCLASSES;
static_assert(HEAD_FLOATS == (size_t)BH * BH + BH + BH * BCLASSES + BCLASSES, "head block: WpT | bp | WcT | bc");
constexpr size_t PRM_FLOATS = PRM_LAYER * BLAYERS + HEAD_FLOATS;  // what TextModel::create allocates

template <class T>  // T = float (create fills it) or const float (the forwards)
struct LayerParams {
  T *bqkv, *bo, *g1, *b1, *bi, *bo2, *g2, *b2;
};
template <class T> inline LayerParams<T> layer_params(T* prm, int l) {
  T* p = prm + PRM_LAYER * l;
  return {p + PO_BQKV, p + PO_BO, p + PO_G1, p + PO_B1, p + PO_BI, p + PO_BO2, p + PO_G2, p + PO_B2};
}

// ---------------------------------------------------------------- wts / wts32: per layer Wqkv | Wo | Wi | Wo2
// each a torch Linear weight [out][in] = a GEMM B matrix [N][K]; Wqkv's rows: query | key | value
constexpr size_t WT_SIZE[4] = {(size_t)BQKV * BH, (size_t)BH * BH, (size_t)BI * BH, (size_t)BH * BI};
constexpr size_t WT_OFF[4] = {0, WT_SIZE[0], WT_SIZE[0] + WT_SIZE[1], WT_SIZE[0] + WT_SIZE[1] + WT_SIZE[2]};
constexpr size_t WT_LAYER = WT_OFF[3] + WT_SIZE[3];
static_assert(WT_LAYER == ((size_t)BQKV + BH + 2 * BI) * BH, "per-layer weight offsets sum to WT_LAYER");

template <class T>  // T = const f16 (f16 weights, fp32x3 hi planes), const float (fp32), float (create)
struct LayerWeights {
  T *wqkv, *wo, *wi, *wo2;
};
template <class T> inline LayerWeights<T> layer_weights(T* w, int l) {
  T* p = w + WT_LAYER * l;
  return {p + WT_OFF[0], p + WT_OFF[1], p + WT_OFF[2], p + WT_OFF[3]};
}

// ---------------------------------------------------------------- the batch a forward runs on
// M = B * 128 token rows (every buffer over token rows), NS samples (every compact [CLS]-row buffer and
// the outputs). Padded batch: NS = B, mask = the attention mask, sample b's [CLS] row is row b * 128.
// Packed batch (B packed rows): mask = the slots' uint8 segment ids, which take the mask's place in every
// attention kernel; posid = the slots' position ids; sample b's [CLS] row is slot cidx[b].
struct TextBatch {
  const int32_t *ids, *mask, *posid, *cidx;
  long long gs;  // token rows between gathered [CLS] rows (cidx counts slots: 1)
  int M, NS;
};
// Sets tb's extents and carves the forward's buffers (layout(Carver&), which may read tb.M / tb.NS). Packed
// batch: after them what the pack kernel writes (per slot the token id, position id and uint8 segment id, per
// sample its [CLS] slot row * 128 + off), then the pack kernel.
template <class F>
inline int text_prologue(TextBatch& tb, DevBuf& ws, const int32_t* ids, const int32_t* mask, int B,
                         const TextPack* pk, hipStream_t s, F&& layout) {
  tb = TextBatch{ids, mask, nullptr, nullptr, ATT_L, B * ATT_L, pk ? pk->ns : B};
  int32_t *pids = nullptr, *ppos = nullptr, *cidx = nullptr;
  uint8_t* seg = nullptr;
  MEC_TRY(carve(ws, [&](Carver& c) {
    layout(c);
    if (!pk) return;
    pids = c.take<int32_t>((size_t)tb.M);
    ppos = c.take<int32_t>((size_t)tb.M);
    seg = c.take<uint8_t>((size_t)tb.M);
    cidx = c.take<int32_t>((size_t)tb.NS);
  }));
  if (!pk) return 0;
  MEC_TRY(launch_bert_pack(ids, *pk, B, pids, ppos, seg, cidx, s));
  tb = TextBatch{pids, reinterpret_cast<const int32_t*>(seg), ppos, cidx, 1, tb.M, tb.NS};
  return 0;
}

// The samples' [CLS] rows of up to four arrays over token rows, gathered into dense [NS, .] arrays
struct ClsRows {
  const void* src;
  void* dst;
  int bytes;  // of one row
};
static inline int gather_cls_rows(const TextBatch& tb, std::initializer_list<ClsRows> arrays, hipStream_t s) {
  RowGather rg{};
  rg.idx = tb.cidx;
  for (const ClsRows& a : arrays) {
    MEC_REQUIRE(rg.n < 4, "gather_cls_rows: at most four arrays");
    rg.src[rg.n] = static_cast<const char*>(a.src); rg.dst[rg.n] = static_cast<char*>(a.dst);
    rg.sstride[rg.n] = tb.gs * a.bytes; rg.bytes[rg.n] = a.bytes;
    ++rg.n;
  }
  return launch_gather_rows(rg, tb.NS, s);
}

// Output tail: pooled = tanh(cls . Wp^T + bp) over the samples' [CLS] rows of the last LayerNorm's output
// (the launch also copies that CLS feature out), then logits and probs. compact: h32c already holds those
// rows (the [CLS]-only last layer); else they are rows of h32, which a packed batch gathers first.
static inline int text_outputs(const TextBatch& tb, const float* prm, const float* h32, float* h32c, bool compact,
                               float* pooled, float* cls, float* logits, float* probs, hipStream_t s) {
  if (tb.cidx && !compact) {
    MEC_TRY(gather_cls_rows(tb, {{h32, h32c, BH * 4}}, s));
    compact = true;
  }
  const float* head = prm + PRM_LAYER * BLAYERS;
  MEC_TRY(launch_linear_mfma<BACT_TANH>(compact ? h32c : h32, compact ? (size_t)BH : (size_t)ATT_L * BH, tb.NS, BH,
                                        head + HO_WPT, head + HO_BP, BH, pooled, BH, cls, BH, s));
  return launch_head7(pooled, tb.NS, BH, head + HO_WCT, head + HO_BC, logits, probs, s);
}

// The rows a layer's tail (O-projection -> LN1 -> FFN1 -> FFN2 -> LN2) runs on, f16 and fp32x3 forwards: every
// token row, or the samples' [CLS] rows in the last layer (bert_cls_last). fp32x3: the f16 buffers are hi | lo
// planes, the lo plane n * 768 (ctx, op) or n * 3072 (ffn) halfs after the hi plane.
struct TailRows {
  int n;
  float *h32, *t32;     // the f32 stream pair: O-proj reads h32 and writes t32, FFN2 reads t32 and writes h32
  f16 *ctx, *op, *ffn;  // the context (in), the LayerNorm outputs (the GEMMs' operand), the FFN intermediate
  float2 *st1, *st2;    // LN1's and LN2's row (mean, rstd)
  bool deferred_in;     // h32 holds the previous layer's pre-LN2 sum and st2 its stats (else: an LN output)
  bool full_out;        // LN2 also writes its f32 output (in place in h32): the pooler's input
  bool tagged;          // launches carry their profiling tags. [CLS] rows: TAG_NONE, so the per-tag timings and
                        // the per-tag GEMM tile pins keep meaning the token-row launches
};

}  // namespace mec
