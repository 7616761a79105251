// The host steps the six image forwards share (ResNet50: resnet.hip f16, resnet_f32.hip fp32 / fp32x3; MobileNetV2:
// mobilenet.hip, mobilenet_f32.hip, mobilenet_x3.hip): argument check, resize, the walk over the backbone's blocks,
// output tail. A precision contributes a small policy struct: how an operand is addressed in GemmParams, which
// packed fields feed a conv, the launch function, and what may take over a block's end. Host code only.
#pragma once
#include <algorithm>
#include <string>

#include "block_ops.h"
#include "models.h"

namespace mec {

// ---------------------------------------------------------------- prologue and output tail
// 0: run the forward; 1: an empty batch, nothing to do; -1: error
static inline int image_args(const uint8_t* img, int B, int H, int W, int C, const float* feat, const float* logits,
                             const float* probs) {
  MEC_REQUIRE(B >= 0, "image: B < 0");
  if (B == 0) return 1;
  MEC_REQUIRE(img && feat && logits && probs, "image: null pointer");
  MEC_REQUIRE((H == 48 && W == 48 && C == 1) || (H == 224 && W == 224 && (C == 1 || C == 3)),
              "image: input must be u8 [B,48,48,1] (GPU resize) or [B,224,224,{1,3}] (already resized)");
  return 0;
}

constexpr size_t kImgPixels = (size_t)224 * 224;  // of the resized image (the `resized` buffer: B of them, u8)

// The stem's input: u8 [B,224,224,C], the caller's image or the 48 x 48 gray one resized into `resized`
struct StemIn {
  const uint8_t* img;
  int C;
};
static inline int image_stem_input(const uint8_t* img, int B, int H, int W, int C, uint8_t* resized, hipStream_t s,
                                   StemIn& si) {
  si = StemIn{img, C};
  if (H == 48 && W == 48 && C == 1) {
    MEC_TRY(resize_u8(img, B, 48, 48, resized, 224, 224, s));
    si.img = resized;
  }
  return 0;
}

// pooled [B,F] -> fc[1] Linear(F,512) + fc[2] ReLU = the 512-d feature (extract_features), then fc[4] + softmax
template <class M>
int image_outputs(const M& m, const float* pooled, int B, int F, float* feat, float* logits, float* probs,
                  hipStream_t s) {
  const float* P = m.prm.template as<float>();
  MEC_TRY(launch_linear_mfma<BACT_RELU>(pooled, F, B, F, P + m.fc1_off, P + m.fc1b_off, 512, feat, 512, nullptr, 0, s));
  return launch_head7(feat, B, 512, P + m.fc2_off, P + m.fc2b_off, logits, probs, s);
}

// ---------------------------------------------------------------- ResNet50
// per-image elements: the largest NHWC activation (layer1's output, X / Y / DS), conv1's output at its largest
// (layer2 block 0, T1), conv2's (T2) = the stem output, and the pooled features
constexpr size_t kRnBig = (size_t)56 * 56 * 256, kRnT1 = (size_t)56 * 56 * 128, kRnT2 = (size_t)56 * 56 * 64;
constexpr size_t kRnStem = (size_t)56 * 56 * 64;
constexpr int kRnFeat = 2048;
constexpr size_t kRnL12 = 7;  // layer1 (3 blocks) + layer2 (4 blocks)

// The stem output [B,56,56,64] sits in the last quarter of X: a chunk's layer-1 outputs (4x the per-image stride)
// then never reach the stem output of a later chunk's images (resnet_chunk)
template <class T> T* resnet_stem_slot(T* X, int B) { return X + 3 * B * kRnStem; }

static inline void conv_geometry(GemmParams& g, int H, int C, int OH, int ks, int stride, int pad) {
  g.H = H; g.W = H; g.C = C; g.OH = OH; g.OW = OH; g.ks = ks; g.stride = stride; g.pad = pad;
}

// The tensors with an fp32x3 plane exponent (models.h X3Tensors): the stem output, then per stage (a block with a
// downsample opens one) the residual stream "layerN.out", shared by the stage's block outputs, and each block's
// conv1 / conv2 outputs. The fp32x3 creation names its exponents from this list and an observing fp32 forward
// fills one slot per entry (RnTap).
static inline X3Tensors resnet_x3_tensors(const std::vector<Bottleneck>& blocks) {
  X3Tensors t;
  t.names.push_back("stem");
  int stage = 1;
  for (size_t b0 = 0; b0 < blocks.size(); ++stage) {
    size_t b1 = b0 + 1;
    while (b1 < blocks.size() && !blocks[b1].has_ds) ++b1;  // [b0, b1): one stage
    const std::string st = "layer" + std::to_string(stage);
    const int out = (int)t.names.size();
    t.names.push_back(st + ".out");
    for (size_t bi = b0; bi < b1; ++bi) {
      const std::string bn = st + "." + std::to_string(bi - b0);
      t.out.push_back(out);
      t.c1.push_back((int)t.names.size());
      t.names.push_back(bn + ".conv1");
      t.c2.push_back((int)t.names.size());
      t.names.push_back(bn + ".conv2");
    }
    b0 = b1;
  }
  return t;
}
enum RnTap : int { TAP_CONV1, TAP_CONV2, TAP_OUT };

// What a policy's block_end sees once conv2 has run: it may run conv3 (+ downsample | + identity) + ReLU and the
// next block's conv1 in one seam kernel (returns 1; 0: not taken, the walk runs the GEMMs; -1: error).
struct RnBlockEnd {
  const Bottleneck& bk;
  const Bottleneck* nx;   // the walk's next block, or null at its last one
  const Bottleneck* nxc;  // the same, but past the walk's end too when the walk covers the whole batch (`cross`)
  int wd, cin, st, OH, M;  // M = nb OH OH output rows
  size_t pix0;             // i0 OH OH: the image range's first row (the next conv1's output starts at T1 + pix0 N)
};

// A policy Pol (one per precision) has: T (activation element), buffers X, Y, Xs (the stem output), T1, T2 (and DS
// without kDualDs), prof, s, and
//   a(g, p) / a2(g, p) / c(g, p) / r(g, p)   operand A / second source of a dual GEMM / output / residual at p
//   w(g, conv) / w_dual(g, block)            weights, bias (and scales) of a conv / of [conv3 | downsample]
//   launch(g, prof, tag)                     the GEMM engine
//   kDualDs                                  the downsample rides in conv3's GEMM (A_DUAL), else its own GEMM into DS
//   kChunked                                 opt().resnet_chunk applies
//   block_end(e, t2, in, out)                see RnBlockEnd
//   kTap, tap(which, bi, x, n)               fp32: block bi's finished conv1 / conv2 / output tensor x of n elements
//                                            (RnTap) is offered to the observation (a no-op unless armed)
//
// Bottleneck blocks [b0, b1) over images [i0, i0 + nb) of the batch (NHWC buffers are image-major, so an image
// range is a pointer offset; fp32x3 lo planes stay L elements after their hi planes). cur/other swap once per
// block. conv1_done: this block's conv1 already ran in the previous block's seam kernel (carried across walks).
template <class Pol>
int resnet_walk(const std::vector<Bottleneck>& blocks, Pol& p, size_t b0, size_t b1, int i0, int nb, int Hin,
                bool cross, typename Pol::T*& cur, typename Pol::T*& other, bool& conv1_done) {
  using T = typename Pol::T;
  int H = Hin;
  for (size_t bi = b0; bi < b1; ++bi) {
    const Bottleneck& bk = blocks[bi];
    const int wd = bk.c1.cout, cin = bk.c1.cin, st = bk.c2.stride;
    const int OH = (H + 2 - 3) / st + 1, M = nb * OH * OH;
    T* in = (bi == 0 ? p.Xs : cur) + (size_t)i0 * H * H * cin;
    T* out = other + (size_t)i0 * OH * OH * 4 * wd;
    T* t1 = p.T1 + (size_t)i0 * H * H * wd;
    T* t2 = p.T2 + (size_t)i0 * OH * OH * wd;
    GemmParams g;
    if (!conv1_done) {
      p.a(g, in); p.w(g, bk.c1); p.c(g, t1); g.act = ACT_RELU;
      g.M = nb * H * H; g.N = wd; g.K = cin;
      MEC_TRY(p.launch(g, &p.prof, TAG_RESNET_CONV1X1));
      if constexpr (Pol::kTap) MEC_TRY(p.tap(TAP_CONV1, bi, t1, (size_t)nb * H * H * wd));
    }
    conv1_done = false;
    g = GemmParams();
    g.amode = A_CONV; p.a(g, t1); p.w(g, bk.c2); p.c(g, t2); g.act = ACT_RELU;
    g.M = M; g.N = wd; g.K = 9 * wd;
    conv_geometry(g, H, wd, OH, 3, st, 1);
    MEC_TRY(p.launch(g, &p.prof, TAG_RESNET_CONV3X3));
    if constexpr (Pol::kTap) MEC_TRY(p.tap(TAP_CONV2, bi, t2, (size_t)M * wd));
    const Bottleneck* nx = bi + 1 < b1 ? &blocks[bi + 1] : nullptr;
    const Bottleneck* nxc = nx ? nx : (cross && bi + 1 < blocks.size() ? &blocks[bi + 1] : nullptr);
    const int fused = p.block_end(RnBlockEnd{bk, nx, nxc, wd, cin, st, OH, M, (size_t)i0 * OH * OH}, t2, in, out);
    if (fused < 0) return -1;
    conv1_done = fused > 0;
    if (!fused) {
      g = GemmParams();
      const T* idn = in;
      bool dual = false;
      if constexpr (Pol::kDualDs) {
        if (bk.has_ds) {  // relu(bn3(conv3(t2)) + bn_ds(conv_ds/s(x))) as one GEMM over K = [w | cin]
          g.amode = A_DUAL; p.a(g, t2); g.K1 = wd; p.a2(g, in); p.w_dual(g, bk); g.K = wd + cin;
          conv_geometry(g, H, cin, OH, 1, st, 0);
          dual = true;
        }
      } else if (bk.has_ds) {  // downsample = BN(conv1x1/s(x)), no activation
        T* ds = p.DS + (size_t)i0 * OH * OH * 4 * wd;
        g.amode = A_CONV; p.a(g, in); p.w(g, bk.ds); p.c(g, ds);
        g.M = M; g.N = 4 * wd; g.K = cin;
        conv_geometry(g, H, cin, OH, 1, st, 0);
        MEC_TRY(p.launch(g, &p.prof, TAG_RESNET_CONV1X1));
        idn = ds;
        g = GemmParams();
      }
      if (!dual) {  // relu(bn3(conv3(t2)) + identity)
        p.a(g, t2); p.w(g, bk.c3); p.r(g, idn); g.K = wd;
      }
      p.c(g, out); g.act = ACT_RELU; g.M = M; g.N = 4 * wd;
      MEC_TRY(p.launch(g, &p.prof, TAG_RESNET_CONV1X1));
    }
    if constexpr (Pol::kTap) MEC_TRY(p.tap(TAP_OUT, bi, out, (size_t)M * 4 * wd));
    std::swap(cur, other);
    H = OH;
  }
  return 0;
}

// All blocks; last = the final [B,7,7,2048] activation. Layers 1-2 can run over chunks of opt().resnet_chunk
// images (f16 and fp32x3), so that a chunk's activations stay in the 256-MB Infinity Cache between a block's
// producer and consumer kernels (off by default: measured slower, see Options::resnet_chunk). Every GEMM row and
// conv pixel is computed the same way at any batch split (every interleaved split tile sums in one k order), so
// the outputs do not depend on the chunk size.
template <class Pol>
int resnet_blocks(const std::vector<Bottleneck>& blocks, Pol& p, int B, typename Pol::T*& last) {
  using T = typename Pol::T;
  T* other = p.Y;
  last = p.X;
  bool conv1_done = false;
  const int chunk = Pol::kChunked && opt().resnet_chunk > 0 ? std::min(opt().resnet_chunk, B) : B;
  for (int i0 = 0; i0 < B; i0 += chunk) {
    T* c = p.X;
    T* o = p.Y;
    MEC_TRY(resnet_walk(blocks, p, 0, kRnL12, i0, std::min(chunk, B - i0), 56, chunk == B, c, o, conv1_done));
    last = c;
    other = o;
  }
  return resnet_walk(blocks, p, kRnL12, blocks.size(), 0, B, 28, false, last, other, conv1_done);
}

// ---------------------------------------------------------------- MobileNetV2
constexpr size_t kMbBig = (size_t)112 * 112 * 16;  // per image: the largest fused block output (features[1])
constexpr size_t kMbLast = (size_t)49 * 1280;      // features[18]'s output
constexpr int kMbFeat = 1280;

static inline int mb_out_side(const MbBlock& b, int h) { return b.stride == 2 ? h / 2 : h; }
static inline bool mb_residual(const MbBlock& b) { return b.stride == 1 && b.cin == b.cout; }

// The tensors with an fp32x3 plane exponent (models.h X3Tensors): one per stage, "featuresA-B.out", shared by the
// outputs of blocks[A - 1 .. B - 1] (features[A .. B]); a stage runs from a block without a residual to the next one
static inline X3Tensors mb_x3_tensors(const std::vector<MbBlock>& blocks) {
  X3Tensors t;
  for (size_t b0 = 0; b0 < blocks.size();) {
    size_t b1 = b0 + 1;
    while (b1 < blocks.size() && mb_residual(blocks[b1])) ++b1;
    for (size_t i = b0; i < b1; ++i) t.out.push_back((int)t.names.size());
    t.names.push_back("features" + std::to_string(b0 + 1) + "-" + std::to_string(b1) + ".out");
    b0 = b1;
  }
  return t;
}

// Layered tail: blocks[l0 ..] (features[l0 + 1 ..]) run as expand GEMM -> depthwise -> project GEMM. knob names
// features[k] (0: none); last_always: the last block has no fused form and is layered at every setting.
static inline int mb_layered_from(const std::vector<MbBlock>& blocks, int knob, bool last_always, const char* err,
                                  size_t& l0) {
  l0 = blocks.size() - (last_always ? 1 : 0);
  if (knob) l0 = std::min(l0, (size_t)knob - 1);
  for (size_t i = l0; i < blocks.size(); ++i) MEC_REQUIRE(blocks[i].lwe_off, err);
  return 0;
}
// A block's row widths (padded channel counts) in the GEMM form: the layered copies' (f16, fp32x3: lcinp / lcoutp,
// multiples of 64 from one block to the next) or the fp32 path's own (cinp / coutp)
template <bool LAYERED> int mb_kin(const MbBlock& b) { return LAYERED ? b.lcinp : b.cinp; }
template <bool LAYERED> int mb_nout(const MbBlock& b) { return LAYERED ? b.lcoutp : b.coutp; }
// per-image elements of E (expanded), D (depthwise output) and the block I/O rows of blocks[l0 ..] in the GEMM form
template <bool LAYERED>
void mb_tail_sizes(const std::vector<MbBlock>& blocks, size_t l0, size_t& pe, size_t& pd, size_t& pp) {
  pe = pd = pp = 0;
  int h = 112;
  for (size_t i = 0; i < blocks.size(); ++i) {
    const MbBlock& b = blocks[i];
    const int oh = mb_out_side(b, h);
    if (i >= l0) {
      pe = std::max(pe, (size_t)h * h * b.hidp);
      pd = std::max(pd, (size_t)oh * oh * b.hidp);
      pp = std::max(pp, std::max((size_t)h * h * mb_kin<LAYERED>(b), (size_t)oh * oh * mb_nout<LAYERED>(b)));
    }
    h = oh;
  }
}

// What the fused-block kernels' argument structs (MbArgs, MbX3Args) share
template <class Args, class Y>
void mb_fused_args(Args& a, const MobileNetModel& m, const MbBlock& b, const void* x, Y* y, int h, int C) {
  const f16* Wt = m.wts.as<f16>();
  const float* P = m.prm.as<float>();
  a.x = static_cast<decltype(a.x)>(x); a.y = y; a.H = h; a.OH = mb_out_side(b, h);
  a.cin = b.cin; a.cout = b.cout;
  a.We = Wt + b.we_off; a.be = P + b.be_off; a.Wd = P + b.wd_off; a.bd = P + b.bd_off;
  a.Wp = Wt + b.wp_off; a.bp = P + b.bp_off;
  a.stem_w = P + (C == 3 ? m.stem_rgb_off : m.stem_w_off);
  a.stem_corr = P + m.stem_corr_off;
}

// A policy Pol has: IO (element of a block's input / output rows), kLayered (their widths: mb_kin / mb_nout),
// prof, s, and
//   expand(g, b, i, in)         operands, weights and bias of block i's expand GEMM (in -> E)
//   depthwise(b, B, h, oh, in)  E (or, t == 1, the block input) -> D
//   project(g, b, i, res, out)  the same for the project GEMM (D -> out, + res when not null)
//   last(g, in)                 and for features[18]
//   launch(g, prof, tag)        the GEMM engine
//   kTap, tap(i, x, n)          fp32: block i's finished output x of n elements is offered to the observation
// One block: [expand 1x1 + BN + ReLU6] -> depthwise 3x3/s + BN + ReLU6 -> project 1x1 + BN (+ the block input).
// Untagged launches: inside the TAG_MBV2_BLOCK window.
template <class Pol>
int mb_block(Pol& p, const MbBlock& b, size_t i, int B, int h, const typename Pol::IO* in, typename Pol::IO* out) {
  const int oh = mb_out_side(b, h);
  GemmParams g;
  if (b.t != 1) {
    p.expand(g, b, i, in); g.act = ACT_RELU6;
    g.M = B * h * h; g.N = b.hidp; g.K = mb_kin<Pol::kLayered>(b);
    MEC_TRY(p.launch(g, nullptr, TAG_NONE));
    g = GemmParams();
  }
  MEC_TRY(p.depthwise(b, B, h, oh, in));
  p.project(g, b, i, mb_residual(b) ? in : nullptr, out);
  g.M = B * oh * oh; g.N = mb_nout<Pol::kLayered>(b); g.K = b.hidp;
  MEC_TRY(p.launch(g, nullptr, TAG_NONE));
  if constexpr (Pol::kTap) MEC_TRY(p.tap(i, out, (size_t)g.M * g.N));
  return 0;
}

// features[18] 1x1 320 -> 1280 + BN + ReLU6
template <class Pol>
int mb_last(Pol& p, int B, int h, const typename Pol::IO* in) {
  GemmParams g;
  p.last(g, in); g.act = ACT_RELU6;
  g.M = B * h * h; g.N = kMbFeat; g.K = 320;
  return p.launch(g, &p.prof, TAG_MBV2_LAST);
}

// f16 and fp32x3: blocks [0, l0) as one fused kernel each (fused(i, b, x, y, h): x the u8 image for block 0, then
// X / Y in turn), blocks [l0, ..) layered on the P0 / P1 row buffers; p.enter(b, B, h, x, P0, P1, in) first turns
// the fused blocks' output x into the layered row stride (in = where block l0 reads). last / h: features[18]'s input.
template <class Pol, class F, class Fused>
int mb_walk(const std::vector<MbBlock>& blocks, size_t l0, Pol& p, int B, const uint8_t* img, F* X, F* Y,
            typename Pol::IO* P0, typename Pol::IO* P1, Fused&& fused, const typename Pol::IO*& last, int& h) {
  const void* cur = img;
  F* out = X;
  last = nullptr;
  h = 112;
  for (size_t i = 0; i < blocks.size(); ++i) {
    const MbBlock& b = blocks[i];
    if (i < l0) {
      MEC_TRY(fused(i, b, cur, out, h));
      cur = out;
      out = (out == X) ? Y : X;
    } else {
      if (i == l0) MEC_TRY(p.enter(b, B, h, cur, P0, P1, last));
      typename Pol::IO* pout = (last == P0) ? P1 : P0;
      MEC_TRY(mb_block(p, b, i, B, h, last, pout));
      last = pout;
    }
    h = mb_out_side(b, h);
  }
  if (!last) last = static_cast<const typename Pol::IO*>(cur);
  return 0;
}

}  // namespace mec
