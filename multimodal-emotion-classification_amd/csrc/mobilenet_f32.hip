// MobileNetV2 image path in fp32 (mec_create_ex(MEC_IMAGE_MBV2, ..., MEC_PREC_FP32)): the
// same head and transform as the ResNet50 path (inference/image_inference.py:28-32, :59-65) on
// torchvision's mobilenet_v2 backbone (README.md:13; oracle/image_mbv2.py restates it), every
// operand and product in fp32:
//   stem        explicit im2col of ToTensor + Normalize (torchvision's order), k = c*9 + kh*3
//               + kw (the torch weight order) padded 27 -> 32, then one fp32 GEMM to 32 channels
//               (stored 64 wide: the GEMM engine's N granularity) + BN + ReLU6
//   blocks      expand 1x1 (gemm_f32) + BN + ReLU6 -> depthwise 3x3/s + BN + ReLU6
//               (mbv2_dw_f32_kernel, fp32 FMA in torch's tap order) -> project 1x1 (gemm_f32)
//               + BN (+ the block input when stride 1 and cin == cout)
//   features[18] 1x1 320 -> 1280 + BN + ReLU6 (gemm_f32), average pool, fc head (block_ops.h)
// Activations are NHWC f32 with channels zero-padded to multiples of 64 (the engine's N
// granularity and a multiple of its 32-float K tiles): the padded channels stay exactly zero
// through every layer (zero weights and zero biases), so they never touch a real output.
#include <algorithm>
#include <cmath>

#include "block_ops.h"
#include "image_model.h"
#include "image_pack.h"
#include "models.h"

namespace mec {

namespace {
constexpr int MB_STEM_K = 32;  // 27 taps padded to a 32-float K tile
}  // namespace

// stem im2col: one thread per 4 consecutive k of one 112 x 112 output pixel's row
__global__ __launch_bounds__(256) void mbv2_stem_im2col_f32_kernel(const uint8_t* __restrict__ img, int B, int C,
                                                                   float* __restrict__ A) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t total = (size_t)B * 112 * 112 * (MB_STEM_K / 4);
  if (idx >= total) return;
  const int q = (int)(idx % (MB_STEM_K / 4));
  const size_t m = idx / (MB_STEM_K / 4);
  const int ow = (int)(m % 112), oh = (int)((m / 112) % 112);
  const size_t b = m / (112 * 112);
  const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};
  float v[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int k = 4 * q + j;
    float x = 0.f;
    if (k < 27) {
      const int c = k / 9, tap = k - c * 9, kh = tap / 3, kw = tap - kh * 3;
      const int ih = 2 * oh - 1 + kh, iw = 2 * ow - 1 + kw;
      if (ih >= 0 && ih < 224 && iw >= 0 && iw < 224) {
        const uint8_t px = img[((b * 224 + ih) * 224 + iw) * C + (C == 3 ? c : 0)];
        x = ((float)px / 255.0f - mean[c]) / stdv[c];
      }
    }
    v[j] = x;
  }
  *reinterpret_cast<float4*>(A + m * MB_STEM_K + 4 * q) = make_float4(v[0], v[1], v[2], v[3]);
}

// Depthwise 3x3 / stride S, padding 1, + BN shift + ReLU6 on NHWC f32 [B,H,H,Cp]: one thread
// per (output pixel, 4 channels); the taps accumulate in torch's (kh, kw) order from 0.
// Weights [9][Cp] (BN scale folded), bias [Cp].
__global__ __launch_bounds__(256) void mbv2_dw_f32_kernel(const float* __restrict__ x, int B, int H, int Cp, int S,
                                                          int OH, const float* __restrict__ w,
                                                          const float* __restrict__ bias, float* __restrict__ y) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  const int C4 = Cp / 4;
  const size_t total = (size_t)B * OH * OH * C4;
  if (idx >= total) return;
  const int c4 = (int)(idx % C4);
  const size_t pix = idx / C4;
  const int ow = (int)(pix % OH), oh = (int)((pix / OH) % OH);
  const size_t b = pix / ((size_t)OH * OH);
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int kh = 0; kh < 3; ++kh) {
    const int ih = S * oh - 1 + kh;
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) {
      const int iw = S * ow - 1 + kw;
      if (ih < 0 || ih >= H || iw < 0 || iw >= H) continue;
      const float4 v = *reinterpret_cast<const float4*>(x + ((b * H + ih) * H + iw) * Cp + 4 * c4);
      const float4 k = *reinterpret_cast<const float4*>(w + (kh * 3 + kw) * Cp + 4 * c4);
      acc.x = fmaf(v.x, k.x, acc.x); acc.y = fmaf(v.y, k.y, acc.y);
      acc.z = fmaf(v.z, k.z, acc.z); acc.w = fmaf(v.w, k.w, acc.w);
    }
  }
  const float4 bb = *reinterpret_cast<const float4*>(bias + 4 * c4);
  float4 o;
  o.x = fminf(fmaxf(acc.x + bb.x, 0.f), 6.f); o.y = fminf(fmaxf(acc.y + bb.y, 0.f), 6.f);
  o.z = fminf(fmaxf(acc.z + bb.z, 0.f), 6.f); o.w = fminf(fmaxf(acc.w + bb.w, 0.f), 6.f);
  *reinterpret_cast<float4*>(y + idx * 4) = o;
}

int MobileNetModel::create_f32(const float* blob, size_t n) {
  BlobReader rd(blob, n);
  std::vector<float> w, pr;
  {  // stem [64][32] (32 real output channels, k = c*9 + kh*3 + kw), bias [64] (at stem_corr_off)
    const float* src = rd.take((size_t)32 * 27);
    const BnFold bn = bn_fold(rd, 32);
    stem_w_off = w.size();
    w.resize(w.size() + (size_t)64 * MB_STEM_K, 0.f);
    align4(pr);
    stem_corr_off = pr.size();
    pr.resize(pr.size() + 64, 0.f);
    if (rd.ok)
      for (int o = 0; o < 32; ++o) {
        for (int k = 0; k < 27; ++k) w[stem_w_off + (size_t)o * MB_STEM_K + k] = (float)((double)src[o * 27 + k] * bn.scale[o]);
        pr[stem_corr_off + o] = (float)bn.shift[o];
      }
  }
  pack_mbv2_body(rd, kMbF32, w, pr, blocks, last_w_off, last_b_off);  // image_pack.h
  MEC_REQUIRE(pack_head(rd, 1280, pr, fc1_off, fc1b_off, fc2_off, fc2b_off), "image_mbv2 blob size mismatch");
  MEC_TRY(upload(wts32, w.data(), w.size() * sizeof(float)));
  MEC_TRY(upload(prm, pr.data(), pr.size() * sizeof(float)));
  return 0;
}

// fp32 policy of a block (image_model.h): f32 rows of cinp / coutp channels (padded to 64), f32 weights on gemm_f32
// obs (null: disarmed, no launch): the observation's slots, one per tensor of xt (mec_model_x3_observe)
struct MbF32 {
  using IO = float;
  static constexpr bool kLayered = false, kTap = true;
  const MobileNetModel& m;
  const float *Wt, *P;
  Prof& prof;
  hipStream_t s;
  float *E, *D, *L;
  unsigned* obs;
  const X3Tensors& xt;
  int tap(size_t i, const float* x, size_t n) const { return obs ? launch_absmax_f32(x, n, obs + xt.out[i], s) : 0; }
  void expand(GemmParams& g, const MbBlock& b, size_t, const float* in) const {
    g.A = in; g.B32 = Wt + b.we_off; g.bias = P + b.be_off; g.C32 = E;
  }
  int depthwise(const MbBlock& b, int B, int h, int oh, const float* in) const {
    const size_t total = (size_t)B * oh * oh * (b.hidp / 4);
    hipLaunchKernelGGL(mbv2_dw_f32_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, b.t != 1 ? E : in, B, h,
                       b.hidp, b.stride, oh, P + b.wd_off, P + b.bd_off, D);
    MEC_LAUNCH_CHECK();
    return 0;
  }
  void project(GemmParams& g, const MbBlock& b, size_t, const float* res, float* out) const {
    g.A = D; g.B32 = Wt + b.wp_off; g.bias = P + b.bp_off; g.C32 = out;
    if (res) { g.R = res; g.r_f32 = 1; }
  }
  void last(GemmParams& g, const float* in) const { g.A = in; g.B32 = Wt + m.last_w_off; g.bias = P + m.last_b_off; g.C32 = L; }
  int launch(const GemmParams& g, Prof* pr, int tag) const { return launch_gemm_f32(g, s, pr, tag); }
};

X3Tensors MobileNetModel::x3_tensors() const { return mb_x3_tensors(blocks); }

int MobileNetModel::forward_f32(const uint8_t* img, int B, int H, int W, int C, float* feat, float* logits,
                                float* probs, hipStream_t s) {
  MEC_REQUIRE(wts32.p, "image_mbv2: fp32 weights missing (handle created at f16 precision)");
  // per image (floats): the largest expanded and depthwise tensors and block input/output (block 0's input, the
  // 112*112*64 stem output, included: a block's cinp is the previous one's coutp)
  size_t big_io, big_e, big_d;
  mb_tail_sizes<false>(blocks, 0, big_e, big_d, big_io);
  uint8_t* resized;
  float *A0, *X, *Y, *E, *D, *Lst, *pooled;
  MEC_TRY(carve(ws, [&](Carver& c) {
    resized = c.take<uint8_t>(B * kImgPixels);
    A0 = c.take<float>((size_t)B * 12544 * MB_STEM_K);
    X = c.take<float>(B * big_io);
    Y = c.take<float>(B * big_io);
    E = c.take<float>(B * big_e);
    D = c.take<float>(B * big_d);
    Lst = c.take<float>(B * kMbLast);
    pooled = c.take<float>((size_t)B * kMbFeat);
  }));
  const X3Tensors xt = obs_on ? x3_tensors() : X3Tensors();
  MbF32 p{*this, wts32.as<float>(), prm.as<float>(), prof, s, E, D, Lst, obs_on ? obs.as<unsigned>() : nullptr, xt};
  StemIn in;
  MEC_TRY(image_stem_input(img, B, H, W, C, resized, s, in));
  MEC_TRY(prof.begin(TAG_MBV2_BLOCK, s));
  {
    const size_t total = (size_t)B * 112 * 112 * (MB_STEM_K / 4);
    hipLaunchKernelGGL(mbv2_stem_im2col_f32_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, in.img,
                       B, in.C, A0);
    MEC_LAUNCH_CHECK();
  }
  GemmParams g;
  g.A = A0; g.B32 = p.Wt + stem_w_off; g.bias = p.P + stem_corr_off; g.act = ACT_RELU6; g.C32 = X;
  g.M = B * 112 * 112; g.N = 64; g.K = MB_STEM_K;
  MEC_TRY(launch_gemm_f32(g, s, nullptr, TAG_NONE));
  float* cur = X;
  float* other = Y;
  int h = 112;
  for (size_t i = 0; i < blocks.size(); ++i) {
    MEC_TRY(mb_block(p, blocks[i], i, B, h, cur, other));
    std::swap(cur, other);
    h = mb_out_side(blocks[i], h);
  }
  MEC_TRY(prof.end(TAG_MBV2_BLOCK, s));
  MEC_TRY(mb_last(p, B, h, cur));
  hipLaunchKernelGGL(avgpool_f32_kernel, dim3(B, kMbFeat / 256), dim3(256), 0, s, Lst, h * h, kMbFeat, pooled);
  MEC_LAUNCH_CHECK();
  return image_outputs(*this, pooled, B, kMbFeat, feat, logits, probs, s);
}

}  // namespace mec
