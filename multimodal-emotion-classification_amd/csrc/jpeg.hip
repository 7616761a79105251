// Baseline JPEG decoding of a ragged batch (include/mec.h mec_jpeg_probe, mec_jpeg_decode_ragged): what Pillow on
// libjpeg-turbo gives for the files of mec_jpeg_probe's domain, byte for byte. Everything libjpeg does to such a
// file is integer arithmetic and is restated here: Huffman decoding, the slow-integer IDCT (jidctint), fancy
// h2v1 / h2v2 upsampling and the 16-bit fixed-point YCbCr -> RGB. Three kernels:
//   entropy  one wave per restart segment: serial Huffman decoding, its state kept wave-uniform (scalar), the
//            lanes used for staging input bytes and for storing each block's 64 coefficients as one 128-byte line
//   idct     8 threads per block: dequantize, column pass, row pass, u8 planes padded to whole blocks
//   colour   4 pixels per thread: upsample, convert, crop, packed [H, W, C] out
// The parser is jpeg_probe.h. The host side of the call (staging) is ragged_stage.h's. tests/jpeg_ref.py is the
// numpy restatement the kernels are tested against.
#include <algorithm>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "jpeg_probe.h"
#include "mec.h"
#include "mec_common.h"
#include "ragged_stage.h"

namespace mec {
namespace jp {

constexpr int kChunk = 1024;    // input bytes staged per refill: 16 per lane
constexpr int kLook = 9;        // bits of the short-code lookup
constexpr int kIdctBlocks = 32; // blocks per IDCT workgroup (8 threads each)
constexpr int kTilePix = 1024;  // pixels per colour workgroup (4 per thread)

// A Huffman table as the entropy kernel reads it (1424 bytes, a multiple of 16).
struct HuffDev {
  uint16_t look[1 << kLook];  // the next 9 bits -> length << 8 | symbol for a code of at most 9 bits, else 0
  int32_t maxcode[17];        // [l]: the largest code of l bits, -1 where there is none
  int32_t valoff[17];         // [l]: index of the first value of l bits minus its code
  uint8_t vals[256];
  uint8_t pad[8];
};
static_assert(sizeof(HuffDev) % 16 == 0, "HuffDev is copied in words");

struct Image {
  long long coef_off[3], plane_off[3];  // bytes into the workspace
  long long dst_off;
  int H, W, ncomp, hmax, vmax;
  int bw[3], bh[3];  // each component's plane in blocks, padded to whole MCUs
  int ch[3], cv[3];  // its blocks per MCU
  int mcux;
  int dc[3], ac[3], qt[3];  // its tables' indices
};
struct Segment {
  long long off;  // bytes into src
  int len, img, mcu0, nmcu;
};
struct BlockTile {
  int img, comp, blk0, nblk;
};
struct PixTile {
  int img, pix0, npix;
};

__device__ const uint8_t kNatural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                         41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                         30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
const uint8_t kNaturalHost[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                  41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                  30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

__device__ inline int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }

__device__ inline void raise(int* status, int img, int code) {
  if (threadIdx.x == 0) atomicCAS(status + img, 0, code);
}

// One wave per segment. The decoder's state (bit buffer, cursors, DC predictions) is the same in every lane and is
// kept scalar through readfirstlane on what it reads from LDS, so its branches are scalar too. The bounds do not
// depend on the data: the byte cursor stops at the segment's length (nothing outside [off, off + len) is loaded,
// the ends of the staged range byte by byte), the MCU loop runs the host's nmcu MCUs of the image's own grid, a
// coefficient index above 63 ends the decoding, and every table index is masked to its table.
__global__ __launch_bounds__(64) void entropy_kernel(const uint8_t* src, const Image* __restrict__ imgs,
                                                     const Segment* __restrict__ segs, const HuffDev* __restrict__ tabs,
                                                     uint8_t* ws, int* status) {
  __shared__ __attribute__((aligned(16))) uint8_t s_in[kChunk];
  __shared__ __attribute__((aligned(16))) HuffDev s_tab[6];
  __shared__ __attribute__((aligned(16))) int16_t s_blk[64];
  __shared__ uint8_t s_nat[64];
  const int lane = threadIdx.x;
  const Segment seg = segs[blockIdx.x];
  const Image& im = imgs[seg.img];
  const int ncomp = im.ncomp;
  for (int c = 0; c < ncomp; ++c) {
    const uint32_t* d = reinterpret_cast<const uint32_t*>(tabs + im.dc[c]);
    const uint32_t* a = reinterpret_cast<const uint32_t*>(tabs + im.ac[c]);
    uint32_t* sd = reinterpret_cast<uint32_t*>(&s_tab[c]);
    uint32_t* sa = reinterpret_cast<uint32_t*>(&s_tab[3 + c]);
    for (int i = lane; i < (int)(sizeof(HuffDev) / 4); i += 64) {
      sd[i] = d[i];
      sa[i] = a[i];
    }
  }
  s_nat[lane] = kNatural[lane];

  const uint8_t* g0 = src + seg.off;
  const int len = seg.len;
  const int phase = (int)(reinterpret_cast<uintptr_t>(g0) & 15);  // s_in[phase + pos - cbase] = g0[pos]
  int cbase = -kChunk;  // the staged chunk holds positions [cbase - phase, cbase - phase + kChunk)
  int pos = 0, cnt = 0;
  uint64_t acc = 0;  // the next cnt bits, from the top

  auto stage = [&]() {  // the next chunk
    cbase += kChunk;
    __syncthreads();
    const int lo = cbase - phase + 16 * lane;
    if (lo >= 0 && lo + 16 <= len) {
      *reinterpret_cast<uint4*>(s_in + 16 * lane) = *reinterpret_cast<const uint4*>(g0 + lo);
    } else {
      for (int b = max(lo, 0); b < min(lo + 16, len); ++b) s_in[b - (cbase - phase)] = g0[b];
    }
    __syncthreads();
  };
  auto refill = [&]() {
    while (cnt <= 56 && pos < len) {
      while (pos + phase - cbase >= kChunk) stage();
      const int b = uni(s_in[pos + phase - cbase]);
      ++pos;
      if (b == 0xFF) {
        if (pos >= len) break;  // an 0xFF without its stuffed byte: the segment ends here
        ++pos;                  // the stuffed byte
      }
      acc |= (uint64_t)b << (56 - cnt);
      cnt += 8;
    }
  };
  // One Huffman symbol -> 0 and sym, or the status.
  auto symbol = [&](const HuffDev& t, int& sym) -> int {
    refill();
    const int top = (int)(acc >> 48);
    const int e = uni(t.look[top >> (16 - kLook)]);
    int l = 0;
    if (e) {
      l = e >> 8;
      sym = e & 255;
    } else {
      for (int k = kLook + 1; k <= 16; ++k) {
        const int c = top >> (16 - k);
        if (c <= uni(t.maxcode[k])) {
          l = k;
          sym = uni(t.vals[(c + uni(t.valoff[k])) & 255]);
          break;
        }
      }
      if (!l) return cnt < 16 ? MEC_JPEG_ST_SEGMENT_END : MEC_JPEG_ST_BAD_CODE;
    }
    if (l > cnt) return MEC_JPEG_ST_SEGMENT_END;
    acc <<= l;
    cnt -= l;
    return 0;
  };
  // s >= 1 further bits, sign-extended as a JPEG magnitude -> 0 and v, or the status.
  auto receive = [&](int s, int& v) -> int {
    refill();
    if (s > cnt) return MEC_JPEG_ST_SEGMENT_END;
    const int raw = (int)(acc >> (64 - s));
    acc <<= s;
    cnt -= s;
    v = raw < (1 << (s - 1)) ? raw - (1 << s) + 1 : raw;
    return 0;
  };

  stage();
  int pred[3] = {0, 0, 0};
  for (int m = 0; m < seg.nmcu; ++m) {
    const int mcu = seg.mcu0 + m;
    const int yy = mcu / im.mcux, xx = mcu - yy * im.mcux;
    for (int c = 0; c < ncomp; ++c) {
      const int nb = im.ch[c] * im.cv[c];
      for (int b = 0; b < nb; ++b) {
        const int v = b / im.ch[c], h = b - v * im.ch[c];
        const int blk = (yy * im.cv[c] + v) * im.bw[c] + xx * im.ch[c] + h;
        if (lane < 32) reinterpret_cast<uint32_t*>(s_blk)[lane] = 0;
        __syncthreads();
        int st, s = 0, val = 0;
        if ((st = symbol(s_tab[c], s))) return raise(status, seg.img, st);
        if (s > 11) return raise(status, seg.img, MEC_JPEG_ST_DC_CATEGORY);
        if (s) {
          if ((st = receive(s, val))) return raise(status, seg.img, st);
          pred[c] += val;
        }
        if (pred[c] < -32768 || pred[c] > 32767) return raise(status, seg.img, MEC_JPEG_ST_COEF_RANGE);
        if (lane == 0) s_blk[0] = (int16_t)pred[c];
        int k = 1;
        while (k < 64) {
          int rs = 0;
          if ((st = symbol(s_tab[3 + c], rs))) return raise(status, seg.img, st);
          const int r = rs >> 4;
          s = rs & 15;
          if (s == 0) {
            if (r != 15) break;  // end of block
            k += 16;
            continue;
          }
          if (s > 10) return raise(status, seg.img, MEC_JPEG_ST_AC_SIZE);
          k += r;
          if (k > 63) return raise(status, seg.img, MEC_JPEG_ST_COEF_INDEX);
          if ((st = receive(s, val))) return raise(status, seg.img, st);
          if (lane == 0) s_blk[s_nat[k]] = (int16_t)val;
          ++k;
        }
        __syncthreads();
        if (lane < 32)
          reinterpret_cast<uint32_t*>(ws + im.coef_off[c] + (size_t)blk * 128)[lane] = reinterpret_cast<uint32_t*>(s_blk)[lane];
      }
    }
  }
}

__host__ __device__ constexpr int fix13(double x) { return (int)(x * 8192 + 0.5); }

// jidctint's 1-D pass (CONST_BITS 13), in 64 bits so that no input overflows it; out = descale(., shift).
__device__ inline void idct_pass(const long long* x, int shift, long long* out) {
  constexpr long long F0298 = fix13(0.298631336), F0390 = fix13(0.390180644), F0541 = fix13(0.541196100),
                      F0765 = fix13(0.765366865), F0899 = fix13(0.899976223), F1175 = fix13(1.175875602),
                      F1501 = fix13(1.501321110), F1847 = fix13(1.847759065), F1961 = fix13(1.961570560),
                      F2053 = fix13(2.053119869), F2562 = fix13(2.562915447), F3072 = fix13(3.072711026);
  long long z2 = x[2], z3 = x[6];
  long long z1 = (z2 + z3) * F0541;
  long long tmp2 = z1 - z3 * F1847;
  long long tmp3 = z1 + z2 * F0765;
  long long tmp0 = (x[0] + x[4]) * 8192;
  long long tmp1 = (x[0] - x[4]) * 8192;
  const long long tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  tmp0 = x[7];
  tmp1 = x[5];
  tmp2 = x[3];
  tmp3 = x[1];
  z1 = tmp0 + tmp3;
  z2 = tmp1 + tmp2;
  z3 = tmp0 + tmp2;
  long long z4 = tmp1 + tmp3;
  const long long z5 = (z3 + z4) * F1175;
  tmp0 *= F0298;
  tmp1 *= F2053;
  tmp2 *= F3072;
  tmp3 *= F1501;
  z1 *= -F0899;
  z2 *= -F2562;
  z3 = z3 * -F1961 + z5;
  z4 = z4 * -F0390 + z5;
  tmp0 += z1 + z3;
  tmp1 += z2 + z4;
  tmp2 += z2 + z3;
  tmp3 += z1 + z4;
  const long long half = 1LL << (shift - 1);
  out[0] = (tmp10 + tmp3 + half) >> shift;
  out[7] = (tmp10 - tmp3 + half) >> shift;
  out[1] = (tmp11 + tmp2 + half) >> shift;
  out[6] = (tmp11 - tmp2 + half) >> shift;
  out[2] = (tmp12 + tmp1 + half) >> shift;
  out[5] = (tmp12 - tmp1 + half) >> shift;
  out[3] = (tmp13 + tmp0 + half) >> shift;
  out[4] = (tmp13 - tmp0 + half) >> shift;
}

// 8 threads per block: thread j dequantizes and transforms column j into LDS, then transforms row j and stores its
// 8 bytes of the component's plane ([bh * 8][bw * 8], so the store is 8-byte aligned). The values that libjpeg's
// SIMD code would saturate or wrap (a dequantized coefficient or a column result outside int16, a result outside
// [-512, 511]) raise the image's status.
__global__ __launch_bounds__(256) void idct_kernel(const Image* __restrict__ imgs, const BlockTile* __restrict__ tiles,
                                                   const uint16_t* __restrict__ qts, uint8_t* ws, int* status) {
  __shared__ int s_ws[kIdctBlocks][65];
  const BlockTile tile = tiles[blockIdx.x];
  const Image& im = imgs[tile.img];
  const int b = threadIdx.x >> 3, j = threadIdx.x & 7;
  const bool active = b < tile.nblk;
  int bad = 0;
  long long x[8], o[8];
  if (active) {
    const int16_t* cf = reinterpret_cast<const int16_t*>(ws + im.coef_off[tile.comp]) + (size_t)(tile.blk0 + b) * 64;
    const uint16_t* q = qts + im.qt[tile.comp] * 64;
    for (int r = 0; r < 8; ++r) {
      const int v = (int)cf[r * 8 + j] * (int)q[r * 8 + j];
      if (v < -32768 || v > 32767) bad = MEC_JPEG_ST_COEF_RANGE;
      x[r] = v;
    }
    idct_pass(x, 11, o);
    for (int r = 0; r < 8; ++r) {
      if ((o[r] < -32768 || o[r] > 32767) && !bad) bad = MEC_JPEG_ST_IDCT_RANGE;
      s_ws[b][r * 8 + j] = (int)o[r];
    }
  }
  __syncthreads();
  if (active) {
    for (int c = 0; c < 8; ++c) x[c] = s_ws[b][j * 8 + c];
    idct_pass(x, 18, o);
    uint32_t w[2] = {0, 0};
    for (int c = 0; c < 8; ++c) {
      if ((o[c] < -512 || o[c] > 511) && !bad) bad = MEC_JPEG_ST_IDCT_RANGE;
      const int v = (int)o[c] + 128;
      const uint32_t u = (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v)) & 255u;
      w[c >> 2] |= u << (8 * (c & 3));
    }
    const int blk = tile.blk0 + b, bw = im.bw[tile.comp];
    const int by = blk / bw, bx = blk - by * bw;
    uint8_t* p = ws + im.plane_off[tile.comp] + ((size_t)(by * 8 + j) * bw + bx) * 8;
    *reinterpret_cast<uint2*>(p) = make_uint2(w[0], w[1]);
  }
  if (bad) atomicCAS(status + tile.img, 0, bad);
}

// Component c's sample at output pixel (y, x): the plane itself, or libjpeg's fancy (triangle) upsampling of its
// dw x dh real samples (edge replication uses that extent, not the padded blocks).
__device__ inline int sample(const uint8_t* p, int stride, int dw, int dh, int hmax, int vmax, int y, int x) {
  if (hmax == 1) return p[(size_t)y * stride + x];
  const int i = x >> 1;
  if (vmax == 1) {
    const uint8_t* r = p + (size_t)y * stride;
    const int c = r[i];
    if (x & 1) return i == dw - 1 ? c : (3 * c + r[i + 1] + 2) >> 2;
    return i == 0 ? c : (3 * c + r[i - 1] + 1) >> 2;
  }
  const int rn = y >> 1;
  const int rf = (y & 1) ? min(rn + 1, dh - 1) : max(rn - 1, 0);
  const uint8_t* nr = p + (size_t)rn * stride;
  const uint8_t* fr = p + (size_t)rf * stride;
  const int s = 3 * nr[i] + fr[i];
  if (x & 1) return i == dw - 1 ? (4 * s + 7) >> 4 : (3 * s + 3 * nr[i + 1] + fr[i + 1] + 7) >> 4;
  return i == 0 ? (4 * s + 8) >> 4 : (3 * s + 3 * nr[i - 1] + fr[i - 1] + 8) >> 4;
}

__device__ inline int clamp8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }
__host__ __device__ constexpr int fix16(double x) { return (int)(x * 65536 + 0.5); }

// Pixel p of image im -> its gray byte, or R | G << 8 | B << 16.
__device__ inline uint32_t pixel(const Image& im, const uint8_t* ws, int p) {
  const int y = p / im.W, x = p - y * im.W;
  const int yv = ws[im.plane_off[0] + (size_t)y * (im.bw[0] * 8) + x];
  if (im.ncomp == 1) return (uint32_t)yv;
  const int dw = (im.W + im.hmax - 1) / im.hmax, dh = (im.H + im.vmax - 1) / im.vmax;
  const int cb = sample(ws + im.plane_off[1], im.bw[1] * 8, dw, dh, im.hmax, im.vmax, y, x) - 128;
  const int cr = sample(ws + im.plane_off[2], im.bw[2] * 8, dw, dh, im.hmax, im.vmax, y, x) - 128;
  const uint32_t r = (uint32_t)clamp8(yv + ((fix16(1.402) * cr + 32768) >> 16));
  const uint32_t g = (uint32_t)clamp8(yv + ((-fix16(0.34414) * cb - fix16(0.71414) * cr + 32768) >> 16));
  const uint32_t b = (uint32_t)clamp8(yv + ((fix16(1.772) * cb + 32768) >> 16));
  return r | (g << 8) | (b << 16);
}

// One workgroup per tile of 1024 pixels, 4 adjacent pixels per thread: their 4 or 12 output bytes start on a word
// of the (16-byte aligned) image and are stored as words; the image's last 1 to 3 pixels are byte stores. ws and
// dst may lie in one allocation with src, so they are not __restrict__.
__global__ __launch_bounds__(256) void colour_kernel(const Image* __restrict__ imgs, const PixTile* __restrict__ tiles,
                                                     const uint8_t* ws, uint8_t* dst) {
  const PixTile tile = tiles[blockIdx.x];
  const Image& im = imgs[tile.img];
  const int C = im.ncomp;
  const int p0 = 4 * threadIdx.x;
  if (p0 >= tile.npix) return;
  const int n = min(4, tile.npix - p0);
  uint8_t* o = dst + im.dst_off + (size_t)(tile.pix0 + p0) * C;
  if (n == 4) {
    const uint32_t a = pixel(im, ws, tile.pix0 + p0), b = pixel(im, ws, tile.pix0 + p0 + 1);
    const uint32_t c = pixel(im, ws, tile.pix0 + p0 + 2), d = pixel(im, ws, tile.pix0 + p0 + 3);
    uint32_t* w = reinterpret_cast<uint32_t*>(o);
    if (C == 1) {
      w[0] = a | (b << 8) | (c << 16) | (d << 24);
    } else {
      w[0] = a | (b << 24);
      w[1] = (b >> 8) | (c << 16);
      w[2] = (c >> 16) | (d << 8);
    }
  } else {
    for (int i = 0; i < n; ++i) {
      const uint32_t v = pixel(im, ws, tile.pix0 + p0 + i);
      for (int k = 0; k < C; ++k) o[i * C + k] = (uint8_t)(v >> (8 * k));
    }
  }
}

// ---- host

// The decoding table of one Huffman table (counts validated by huff_ok).
HuffDev build_table(const mec_jpeg_huff& h) {
  HuffDev t;
  std::memset(&t, 0, sizeof t);
  std::memcpy(t.vals, h.vals, 256);
  int code = 0, p = 0;
  t.maxcode[0] = -1;
  for (int l = 1; l <= 16; ++l) {
    const int n = h.counts[l - 1];
    t.valoff[l] = p - code;
    for (int i = 0; i < n; ++i, ++p, ++code) {
      if (l <= kLook) {
        const int lo = code << (kLook - l);
        for (int f = 0; f < (1 << (kLook - l)); ++f) t.look[lo + f] = (uint16_t)((l << 8) | h.vals[p]);
      }
    }
    t.maxcode[l] = n ? code - 1 : -1;
    code <<= 1;
  }
  return t;
}

// What a descriptor must be; "" or what is wrong with it.
std::string check_desc(const mec_jpeg_desc& d) {
  if (d.ncomp != 1 && d.ncomp != 3) return "has ncomp " + std::to_string(d.ncomp) + ", which is not 1 or 3";
  if (!size_on_gpu(d.H, d.W))
    return "is " + std::to_string(d.H) + " x " + std::to_string(d.W) + ", outside 1 <= H, W <= 4096 with H <= 100 W";
  for (int c = 0; c < d.ncomp; ++c) {
    const bool luma3 = d.ncomp == 3 && c == 0;
    const bool ok = luma3 ? ((d.hs[0] == 1 && d.vs[0] == 1) || (d.hs[0] == 2 && d.vs[0] == 1) || (d.hs[0] == 2 && d.vs[0] == 2))
                          : (d.hs[c] == 1 && d.vs[c] == 1);
    if (!ok) return "has a sampling that is not 1 x 1, or 2 x 1 or 2 x 2 luma over 1 x 1 chroma";
    if (!huff_ok(d.dc[c].counts) || !huff_ok(d.ac[c].counts)) return "has a Huffman table whose counts give no canonical code";
    for (int k = 0; k < 64; ++k)
      if (d.qt[c][k] > 255) return "has a quantization value above 255";
  }
  if (d.ncomp == 3 && d.hs[0] == 2 && d.W < 5) return "is horizontally subsampled and narrower than 5";
  if (d.restart < 0 || d.restart > 65535) return "has a restart interval outside 0..65535";
  int mx, my;
  mcu_grid(d, &mx, &my);
  const long long mcus = (long long)mx * my;
  const long long want = d.restart ? (mcus + d.restart - 1) / d.restart : 1;
  if (d.nseg != want) return "has " + std::to_string(d.nseg) + " segments where its MCUs and restart interval give " + std::to_string(want);
  return "";
}

// Blocks of every component, padded to whole MCUs.
long long blocks_of(const mec_jpeg_desc& d) {
  int mx, my;
  mcu_grid(d, &mx, &my);
  long long n = 0;
  for (int c = 0; c < d.ncomp; ++c) n += (long long)mx * my * (d.ncomp == 1 ? 1 : d.hs[c] * d.vs[c]);
  return n;
}

using State = StageBuf;
std::mutex g_mu;
std::map<int, State> g_state;
// mec_jpeg_prof_*. Never destroyed (events must not outlive the HIP runtime's shutdown).
Prof& g_prof_e = *new Prof;
Prof& g_prof_i = *new Prof;
Prof& g_prof_c = *new Prof;

int decode_ragged(const uint8_t* src, size_t src_bytes, const mec_jpeg_desc* descs, const int64_t* segs, int B, uint8_t* dst,
                  const int64_t* dst_offs, size_t dst_bytes, void* ws, size_t ws_bytes, int32_t* status, hipStream_t s) {
  const char* call = "mec_jpeg_decode_ragged";
  MEC_REQUIRE(B >= 0, "mec_jpeg_decode_ragged: B < 0");
  if (B == 0) return 0;
  MEC_REQUIRE(src && descs && segs && dst && dst_offs && ws && status,
              "mec_jpeg_decode_ragged: src, descs, segs, dst, dst_offs, ws or status is null");
  MEC_REQUIRE(B <= 65535, "mec_jpeg_decode_ragged: B must be at most 65535");
  MEC_REQUIRE(reinterpret_cast<uintptr_t>(dst) % 16 == 0, "mec_jpeg_decode_ragged: dst must be 16-byte aligned");
  MEC_REQUIRE(reinterpret_cast<uintptr_t>(ws) % 16 == 0, "mec_jpeg_decode_ragged: ws must be 16-byte aligned");
  // ---- host: every descriptor is checked before anything is launched
  std::vector<Image> imgs((size_t)B);
  std::vector<Segment> dsegs;
  std::vector<BlockTile> btiles;
  std::vector<PixTile> ptiles;
  std::vector<HuffDev> tabs;
  std::vector<uint16_t> qts;
  std::map<std::string, int> tab_at, qt_at;
  struct Range {
    uintptr_t lo, hi;
    int written, img;
  };
  std::vector<Range> ranges;
  const uintptr_t s0 = reinterpret_cast<uintptr_t>(src), d0 = reinterpret_cast<uintptr_t>(dst);
  size_t need = 0, seg_at = 0;
  for (int i = 0; i < B; ++i) {
    const mec_jpeg_desc& d = descs[i];
    const std::string what = check_desc(d);
    if (!what.empty()) return mec::fail(call, i, what);
    Image& im = imgs[i];
    std::memset(&im, 0, sizeof im);
    int mx, my;
    mcu_grid(d, &mx, &my);
    im.H = d.H;
    im.W = d.W;
    im.ncomp = d.ncomp;
    im.hmax = d.ncomp == 1 ? 1 : d.hs[0];
    im.vmax = d.ncomp == 1 ? 1 : d.vs[0];
    im.mcux = mx;
    for (int c = 0; c < d.ncomp; ++c) {
      im.ch[c] = d.ncomp == 1 ? 1 : d.hs[c];
      im.cv[c] = d.ncomp == 1 ? 1 : d.vs[c];
      im.bw[c] = mx * im.ch[c];
      im.bh[c] = my * im.cv[c];
    }
    const long long nblk = blocks_of(d);
    long long at = (long long)need;
    for (int c = 0; c < d.ncomp; ++c) {
      im.coef_off[c] = at;
      at += (long long)im.bw[c] * im.bh[c] * 128;
    }
    for (int c = 0; c < d.ncomp; ++c) {
      im.plane_off[c] = at;
      at += (long long)im.bw[c] * im.bh[c] * 64;
    }
    need += (size_t)nblk * 192;
    // tables, each distinct one once per call
    for (int c = 0; c < d.ncomp; ++c) {
      for (int k = 0; k < 2; ++k) {
        const mec_jpeg_huff& h = k ? d.ac[c] : d.dc[c];
        const std::string key(reinterpret_cast<const char*>(&h), sizeof h);
        auto it = tab_at.find(key);
        if (it == tab_at.end()) {
          it = tab_at.emplace(key, (int)tabs.size()).first;
          tabs.push_back(build_table(h));
        }
        (k ? im.ac : im.dc)[c] = it->second;
      }
      const std::string key(reinterpret_cast<const char*>(d.qt[c]), sizeof d.qt[c]);
      auto it = qt_at.find(key);
      if (it == qt_at.end()) {
        it = qt_at.emplace(key, (int)(qts.size() / 64)).first;
        qts.resize(qts.size() + 64);
        for (int k = 0; k < 64; ++k) qts[qts.size() - 64 + kNaturalHost[k]] = d.qt[c][k];
      }
      im.qt[c] = it->second;
    }
    // segments
    const long long mcus = (long long)mx * my, per = d.restart ? d.restart : mcus;
    for (int k = 0; k < d.nseg; ++k, ++seg_at) {
      const int64_t off = segs[2 * seg_at], len = segs[2 * seg_at + 1];
      if (off < 0 || len < 0 || len > 0x7fffffff || (uint64_t)off > src_bytes || (uint64_t)len > src_bytes - (uint64_t)off)
        return mec::fail(call, i, "has a segment that does not lie inside src_bytes");
      dsegs.push_back(Segment{off, (int)len, i, (int)(k * per), (int)std::min<long long>(per, mcus - k * per)});
      if (len) ranges.push_back(Range{s0 + (size_t)off, s0 + (size_t)off + (size_t)len, 0, i});
    }
    // the output
    const size_t out_bytes = (size_t)d.H * d.W * d.ncomp;
    if (dst_offs[i] < 0 || dst_offs[i] % 16 != 0) return mec::fail(call, i, "has a dst_off that is negative or not a multiple of 16 bytes");
    if ((uint64_t)dst_offs[i] > dst_bytes || out_bytes > dst_bytes - (size_t)dst_offs[i])
      return mec::fail(call, i, "has an output that does not lie inside dst_bytes");
    im.dst_off = dst_offs[i];
    ranges.push_back(Range{d0 + (size_t)dst_offs[i], d0 + (size_t)dst_offs[i] + out_bytes, 1, i});
    for (int c = 0; c < d.ncomp; ++c) {
      const int n = im.bw[c] * im.bh[c];
      for (int b = 0; b < n; b += kIdctBlocks) btiles.push_back(BlockTile{i, c, b, std::min(kIdctBlocks, n - b)});
    }
    const int npix = d.H * d.W;
    for (int p = 0; p < npix; p += kTilePix) ptiles.push_back(PixTile{i, p, std::min(kTilePix, npix - p)});
  }
  MEC_REQUIRE(ws_bytes >= need, "mec_jpeg_decode_ragged: ws_bytes is less than mec_jpeg_workspace_bytes");
  ranges.push_back(Range{reinterpret_cast<uintptr_t>(ws), reinterpret_cast<uintptr_t>(ws) + need, 1, -1});
  std::sort(ranges.begin(), ranges.end(), [](const Range& a, const Range& b) { return a.lo < b.lo; });
  uintptr_t read_end = 0, write_end = 0;  // the furthest ends of the ranges that start no later
  for (const Range& r : ranges) {
    if (r.lo < write_end || (r.written && r.lo < read_end)) {
      MEC_REQUIRE(r.img >= 0, "mec_jpeg_decode_ragged: the workspace overlaps a segment or an output");
      return mec::fail(call, r.img, "has a segment or an output that overlaps an output or the workspace");
    }
    (r.written ? write_end : read_end) = std::max(r.written ? write_end : read_end, r.hi);
  }
  MEC_REQUIRE(dsegs.size() < ((size_t)1 << 30) && btiles.size() < ((size_t)1 << 30) && ptiles.size() < ((size_t)1 << 30),
              "mec_jpeg_decode_ragged: too many segments or tiles for one launch");
  // ---- device
  int dev = 0;
  MEC_HIP(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(g_mu);
  const Section sec[] = {section(imgs), section(dsegs), section(btiles), section(ptiles), section(tabs), section(qts)};
  return staged_call(g_state[dev], sec, s, [&](const void* const* d) -> int {
    const Image* d_imgs = static_cast<const Image*>(d[0]);
    uint8_t* w = static_cast<uint8_t*>(ws);
    MEC_HIP(hipMemsetAsync(status, 0, (size_t)B * sizeof(int32_t), s));
    MEC_TRY(g_prof_e.begin(TAG_JPEG_ENTROPY, s));
    hipLaunchKernelGGL(entropy_kernel, dim3((unsigned)dsegs.size()), dim3(64), 0, s, src, d_imgs,
                       static_cast<const Segment*>(d[1]), static_cast<const HuffDev*>(d[4]), w, status);
    MEC_LAUNCH_CHECK();
    MEC_TRY(g_prof_e.end(TAG_JPEG_ENTROPY, s));
    MEC_TRY(g_prof_i.begin(TAG_JPEG_IDCT, s));
    hipLaunchKernelGGL(idct_kernel, dim3((unsigned)btiles.size()), dim3(256), 0, s, d_imgs,
                       static_cast<const BlockTile*>(d[2]), static_cast<const uint16_t*>(d[5]), w, status);
    MEC_LAUNCH_CHECK();
    MEC_TRY(g_prof_i.end(TAG_JPEG_IDCT, s));
    MEC_TRY(g_prof_c.begin(TAG_JPEG_COLOUR, s));
    hipLaunchKernelGGL(colour_kernel, dim3((unsigned)ptiles.size()), dim3(256), 0, s, d_imgs,
                       static_cast<const PixTile*>(d[3]), w, dst);
    MEC_LAUNCH_CHECK();
    MEC_TRY(g_prof_c.end(TAG_JPEG_COLOUR, s));
    return 0;
  });
}

}  // namespace jp
}  // namespace mec

using namespace mec;

extern "C" {

int mec_jpeg_probe(const uint8_t* data, size_t n, mec_jpeg_desc* desc, int64_t* segs, int seg_cap) {
  API_GUARD({
    MEC_REQUIRE(data && desc, "mec_jpeg_probe: data or desc is null");
    MEC_REQUIRE(seg_cap >= 0 && (segs || seg_cap == 0), "mec_jpeg_probe: seg_cap < 0, or segs is null with seg_cap > 0");
    return jp::probe(data, n, desc, segs, seg_cap);
  })
}

long long mec_jpeg_workspace_bytes(const mec_jpeg_desc* descs, int B) {
  API_GUARD({
    MEC_REQUIRE(B >= 0 && (descs || B == 0), "mec_jpeg_workspace_bytes: B < 0 or descs is null");
    long long n = 0;
    for (int i = 0; i < B; ++i) {
      const std::string what = jp::check_desc(descs[i]);
      if (!what.empty()) return mec::fail("mec_jpeg_workspace_bytes", i, what);
      n += jp::blocks_of(descs[i]) * 192;
    }
    return n;
  })
}

int mec_jpeg_decode_ragged(const uint8_t* src, size_t src_bytes, const mec_jpeg_desc* descs, const int64_t* segs, int B,
                           uint8_t* dst, const int64_t* dst_offs, size_t dst_bytes, void* ws, size_t ws_bytes,
                           int32_t* status, void* stream) {
  API_GUARD({
    return jp::decode_ragged(src, src_bytes, descs, segs, B, dst, dst_offs, dst_bytes, ws, ws_bytes, status,
                             reinterpret_cast<hipStream_t>(stream));
  })
}

int mec_jpeg_prof_enable(int on) {
  std::lock_guard<std::mutex> lk(jp::g_mu);
  jp::g_prof_e.tag = on ? TAG_JPEG_ENTROPY : TAG_NONE;
  jp::g_prof_i.tag = on ? TAG_JPEG_IDCT : TAG_NONE;
  jp::g_prof_c.tag = on ? TAG_JPEG_COLOUR : TAG_NONE;
  jp::g_prof_e.reset();
  jp::g_prof_i.reset();
  jp::g_prof_c.reset();
  return 0;
}

int mec_jpeg_prof_read(double* entropy_ms, double* idct_ms, double* colour_ms, int* count) {
  if (!entropy_ms || !idct_ms || !colour_ms || !count) { set_error("mec_jpeg_prof_read: bad args"); return -1; }
  std::lock_guard<std::mutex> lk(jp::g_mu);
  int n = 0;
  MEC_TRY(jp::g_prof_e.read(entropy_ms, count));
  MEC_TRY(jp::g_prof_i.read(idct_ms, &n));
  MEC_TRY(jp::g_prof_c.read(colour_ms, &n));
  jp::g_prof_e.reset();
  jp::g_prof_i.reset();
  jp::g_prof_c.reset();
  return 0;
}

}  // extern "C"
