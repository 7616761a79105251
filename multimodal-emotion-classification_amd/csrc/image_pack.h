// The image checkpoints' walk and weight packing, stated once for the three precisions (host code only).
// MobileNetModel::create / create_f32 / create_x3 and ImageModel::create / create_f32 read the canonical
// blob (mec/synthetic.py: spec()) through these and keep only what is theirs: the stems that exist once
// (MobileNet's fp32 im2col stem, ResNet's two), the f16 [conv3 | downsample] concatenation, and the fp32x3
// exponents and plane splitting.
//
// Rounding, which the precisions must not share: a weight is the double product (checkpoint weight) x (BN
// scale) rounded ONCE to the stored type T -- straight to f16 on the f16 path, to float on the fp32 and
// fp32x3 paths (fp32x3 splits that float later). MobileNet multiplies by the double BN scale; ResNet rounds
// the scale to float first and multiplies by (double)(float)scale.
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

#include "models.h"

namespace mec {

inline int pad_to(int v, int m) { return (v + m - 1) / m * m; }
inline void align4(std::vector<float>& v) { while (v.size() % 4) v.push_back(0.f); }  // 16-B aligned float4 reads

// BatchNorm (gamma, beta, running mean, running var) of c channels folded to y = x scale + shift, and the
// fp32x3 output estimate max_c |beta_c| + 6 |gamma_c| (activation_exp). All zeros after a short read.
struct BnFold {
  std::vector<double> scale, shift;
  double est = 0.0;
};
inline BnFold bn_fold(BlobReader& rd, int c) {
  const float* g = rd.take(c);
  const float* b = rd.take(c);
  const float* rm = rd.take(c);
  const float* rv = rd.take(c);
  BnFold f;
  f.scale.assign(c, 0.0);
  f.shift.assign(c, 0.0);
  if (!rd.ok) return f;
  for (int i = 0; i < c; ++i) {
    f.scale[i] = (double)g[i] / std::sqrt((double)rv[i] + 1e-5);
    f.shift[i] = (double)b[i] - (double)rm[i] * f.scale[i];
    f.est = std::max(f.est, std::fabs((double)b[i]) + 6.0 * std::fabs((double)g[i]));
  }
  return f;
}
// the BN shift as an unaligned f32 run at the end of pr (the ResNet biases) -> its offset
inline size_t append_shift(std::vector<float>& pr, const BnFold& bn) {
  const size_t off = pr.size();
  for (double s : bn.shift) pr.push_back((float)s);
  return off;
}

// The fc head that ends both blobs: Linear(K, 512) and Linear(512, 7) transposed to fp32 [K][N], each
// followed by its bias. False, with pr untouched, unless the head's end is exactly the blob's.
inline bool pack_head(BlobReader& rd, int K, std::vector<float>& pr, size_t& fc1, size_t& fc1b, size_t& fc2,
                      size_t& fc2b) {
  const float* f1w = rd.take((size_t)512 * K);
  const float* f1b = rd.take(512);
  const float* f2w = rd.take((size_t)7 * 512);
  const float* f2b = rd.take(7);
  if (!rd.ok || rd.off != rd.n) return false;
  align4(pr);
  fc1 = pr.size();
  pr.resize(pr.size() + (size_t)K * 512);
  for (int i = 0; i < K; ++i)
    for (int j = 0; j < 512; ++j) pr[fc1 + (size_t)i * 512 + j] = f1w[(size_t)j * K + i];
  fc1b = pr.size();
  pr.insert(pr.end(), f1b, f1b + 512);
  fc2 = pr.size();
  pr.resize(pr.size() + 512 * 7);
  for (int i = 0; i < 512; ++i)
    for (int j = 0; j < 7; ++j) pr[fc2 + (size_t)i * 7 + j] = f2w[(size_t)j * 512 + i];
  fc2b = pr.size();
  pr.insert(pr.end(), f2b, f2b + 7);
  return true;
}

// ---------------------------------------------------------------- MobileNetV2
// torchvision's inverted-residual settings (t, c, n, s) of features[1..17]
constexpr int kMbv2Stages[7][4] = {{1, 16, 1, 1}, {6, 24, 2, 2}, {6, 32, 3, 2}, {6, 64, 4, 2},
                                   {6, 96, 3, 1}, {6, 160, 3, 2}, {6, 320, 1, 1}};

// How a precision pads a block's channels (with zero weights and biases) and lays its depthwise taps out.
struct MbLayout {
  int cin_pad, hid_pad, cout_pad;
  bool dw_tap_major;  // depthwise f32 [9][hidp], else [hidp/8][9][8]
  bool layered;       // also the layered copies (MbBlock lwe / lwp / lbp) of the blocks with hidp % 64 == 0
};
constexpr MbLayout kMbFused = {32, 32, 16, false, true};  // f16 and fp32x3: the fused block kernels' tiles
constexpr MbLayout kMbF32 = {64, 64, 64, true, false};    // fp32: the GEMM engine's N granularity

// features[0] for the fused block kernels (f16, fp32x3): conv 3x3/2 (3 -> 32) + BN. ToTensor (/255) and
// Normalize fold into per-pixel weights, f32 [9][32] for gray input (the three replicated channels summed)
// and [3*9][32] for RGB; the -mean/std term of the in-image taps becomes a bias per border class, [4][32],
// cls = 2 * (row 0) + (col 0): stem row 0 / col 0 lose their top / left taps, and 224 = 2 * 112, so the
// bottom / right taps are always inside.
inline void pack_mbv2_stem_folded(BlobReader& rd, std::vector<float>& pr, size_t& stem_w, size_t& stem_rgb,
                                  size_t& stem_corr) {
  const float* src = rd.take((size_t)32 * 3 * 9);
  const BnFold bn = bn_fold(rd, 32);
  align4(pr);
  stem_w = pr.size();
  pr.resize(pr.size() + 9 * 32, 0.f);
  stem_rgb = pr.size();
  pr.resize(pr.size() + 27 * 32, 0.f);
  stem_corr = pr.size();
  pr.resize(pr.size() + 4 * 32, 0.f);
  const double mean[3] = {0.485, 0.456, 0.406}, stdv[3] = {0.229, 0.224, 0.225};
  if (!rd.ok) return;
  for (int o = 0; o < 32; ++o) {
    double cterm[9] = {};
    for (int t = 0; t < 9; ++t) {
      double gsum = 0.0;
      for (int c = 0; c < 3; ++c) {
        const double wv = src[((size_t)o * 3 + c) * 9 + t];
        const double mf = (double)(float)mean[c], sf = (double)(float)stdv[c];
        gsum += wv / (255.0 * sf);
        cterm[t] -= wv * mf / sf;
        pr[stem_rgb + (size_t)(c * 9 + t) * 32 + o] = (float)(wv / (255.0 * sf) * bn.scale[o]);
      }
      pr[stem_w + (size_t)t * 32 + o] = (float)(gsum * bn.scale[o]);
    }
    for (int cls = 0; cls < 4; ++cls) {
      double sum = bn.shift[o];
      for (int t = 0; t < 9; ++t) {
        const int ky = t / 3, kx = t % 3;
        if (((cls & 2) && ky == 0) || ((cls & 1) && kx == 0)) continue;
        sum += cterm[t] * bn.scale[o];
      }
      pr[stem_corr + (size_t)cls * 32 + o] = (float)sum;
    }
  }
}

// One 1x1 conv [n][k] + BN: weights T [np][kp] appended to w (allocated first), bias f32 [np] to pr after
// an align4. Returns the BN estimate.
template <class T>
double pack_mbv2_pw(BlobReader& rd, std::vector<T>& w, std::vector<float>& pr, int n, int k, int np, int kp,
                    size_t& w_off, size_t& b_off) {
  const float* src = rd.take((size_t)n * k);
  const BnFold bn = bn_fold(rd, n);
  w_off = w.size();
  w.resize(w.size() + (size_t)np * kp, (T)0.f);
  align4(pr);
  b_off = pr.size();
  pr.resize(pr.size() + np, 0.f);
  if (rd.ok)
    for (int o = 0; o < n; ++o) {
      for (int c = 0; c < k; ++c) w[w_off + (size_t)o * kp + c] = (T)((double)src[(size_t)o * k + c] * bn.scale[o]);
      pr[b_off + o] = (float)bn.shift[o];
    }
  return bn.est;
}

// features[1..18]: per block the expand 1x1 (t != 1), the depthwise 3x3 (f32, in pr) and the project 1x1,
// each with its BN folded, then the layered copies; last the 1x1 320 -> 1280 of features[18] (unpadded).
template <class T>
void pack_mbv2_body(BlobReader& rd, const MbLayout& lay, std::vector<T>& w, std::vector<float>& pr,
                    std::vector<MbBlock>& blocks, size_t& last_w, size_t& last_b) {
  blocks.clear();
  int cin = 32, prev_lcoutp = 32;
  for (const auto& st : kMbv2Stages)
    for (int r = 0; r < st[2]; ++r) {
      MbBlock b;
      b.t = st[0]; b.cin = cin; b.hid = cin * b.t; b.cout = st[1]; b.stride = r == 0 ? st[3] : 1;
      b.cinp = pad_to(cin, lay.cin_pad); b.hidp = pad_to(b.hid, lay.hid_pad); b.coutp = pad_to(b.cout, lay.cout_pad);
      if (b.t != 1) pack_mbv2_pw(rd, w, pr, b.hid, cin, b.hidp, b.cinp, b.we_off, b.be_off);  // (+ ReLU6)
      {  // depthwise 3x3 + BN (+ ReLU6)
        const float* wd = rd.take((size_t)b.hid * 9);
        const BnFold bn = bn_fold(rd, b.hid);
        align4(pr);
        b.wd_off = pr.size();
        pr.resize(pr.size() + (size_t)b.hidp * 9, 0.f);
        b.bd_off = pr.size();
        pr.resize(pr.size() + b.hidp, 0.f);
        if (rd.ok)
          for (int h = 0; h < b.hid; ++h) {
            for (int t = 0; t < 9; ++t) {
              const size_t i = lay.dw_tap_major ? (size_t)t * b.hidp + h : (size_t)(h / 8) * 72 + t * 8 + (h % 8);
              pr[b.wd_off + i] = (float)((double)wd[(size_t)h * 9 + t] * bn.scale[h]);
            }
            pr[b.bd_off + h] = (float)bn.shift[h];
          }
      }
      b.x3_est = pack_mbv2_pw(rd, w, pr, b.cout, b.hid, b.coutp, b.hidp, b.wp_off, b.bp_off);  // linear bottleneck
      b.lcinp = prev_lcoutp;
      b.lcoutp = pad_to(b.cout, 64);
      prev_lcoutp = b.lcoutp;
      if (lay.layered && b.t != 1 && b.hidp % 64 == 0) {  // the same matrices, K / N padded with zeros
        b.lwe_off = w.size();
        w.resize(w.size() + (size_t)b.hidp * b.lcinp, (T)0.f);
        for (int h = 0; h < b.hidp; ++h)
          for (int c = 0; c < b.cinp && c < b.lcinp; ++c)
            w[b.lwe_off + (size_t)h * b.lcinp + c] = w[b.we_off + (size_t)h * b.cinp + c];
        b.lwp_off = w.size();
        w.resize(w.size() + (size_t)b.lcoutp * b.hidp, (T)0.f);
        std::copy(w.begin() + b.wp_off, w.begin() + b.wp_off + (size_t)b.coutp * b.hidp, w.begin() + b.lwp_off);
        align4(pr);
        b.lbp_off = pr.size();
        pr.resize(pr.size() + b.lcoutp, 0.f);
        std::copy(pr.begin() + b.bp_off, pr.begin() + b.bp_off + b.coutp, pr.begin() + b.lbp_off);
      }
      blocks.push_back(b);
      cin = b.cout;
    }
  pack_mbv2_pw(rd, w, pr, 1280, 320, 1280, 320, last_w, last_b);  // (+ ReLU6; GEMM engine)
}

// ---------------------------------------------------------------- ResNet50
// torchvision's stages (width, blocks, stride of the first block's 3x3: v1.5)
constexpr int kResnetStages[4][3] = {{64, 3, 1}, {128, 4, 2}, {256, 6, 2}, {512, 3, 2}};

// One conv + BN: OIHW -> T [Cout][kh][kw][Cin] with the float-rounded BN scale folded, appended to w; the BN
// shift appended to pr.
template <class T>
ConvLayer pack_conv(BlobReader& rd, std::vector<T>& w, std::vector<float>& pr, int cout, int cin, int ks, int stride,
                    int pad) {
  ConvLayer L;
  L.cin = cin; L.cout = cout; L.ks = ks; L.stride = stride; L.pad = pad;
  const float* src = rd.take((size_t)cout * cin * ks * ks);
  const BnFold bn = bn_fold(rd, cout);
  L.b_off = append_shift(pr, bn);
  L.x3_est = bn.est;
  L.w_off = w.size();
  w.resize(w.size() + (size_t)cout * cin * ks * ks, (T)0.f);
  if (!rd.ok) return L;
  for (int o = 0; o < cout; ++o) {
    const double s = (double)(float)bn.scale[o];
    for (int kh = 0; kh < ks; ++kh)
      for (int kw = 0; kw < ks; ++kw)
        for (int c = 0; c < cin; ++c)
          w[L.w_off + (((size_t)o * ks + kh) * ks + kw) * cin + c] =
              (T)((double)src[(((size_t)o * cin + c) * ks + kh) * ks + kw] * s);
  }
  return L;
}

// layer1..4 after the stem: per bottleneck conv1 1x1, conv2 3x3 (carrying the stride), conv3 1x1, and for a
// stage's first block the downsample 1x1, after which after(block, width, cin) runs.
template <class T, class AfterBlock>
void pack_resnet_blocks(BlobReader& rd, std::vector<T>& w, std::vector<float>& pr, std::vector<Bottleneck>& blocks,
                        AfterBlock&& after) {
  blocks.clear();
  int cin = 64;
  for (const auto& st : kResnetStages) {
    const int wd = st[0];
    for (int b = 0; b < st[1]; ++b) {
      Bottleneck bk;
      const int s = b == 0 ? st[2] : 1;
      bk.c1 = pack_conv(rd, w, pr, wd, cin, 1, 1, 0);
      bk.c2 = pack_conv(rd, w, pr, wd, wd, 3, s, 1);
      bk.c3 = pack_conv(rd, w, pr, 4 * wd, wd, 1, 1, 0);
      if (b == 0) {
        bk.has_ds = true;
        bk.ds = pack_conv(rd, w, pr, 4 * wd, cin, 1, s, 0);
        after(bk, wd, cin);
      }
      blocks.push_back(bk);
      cin = 4 * wd;
    }
  }
}

}  // namespace mec
