// PIL-exact bilinear resize of a ragged batch of u8 images to 224 x 224 (include/mec.h mec_resize_ragged_u8,
// mec_resize_taps). Pillow's ImagingResample at 8 bits per channel is integer arithmetic on 22-bit fixed-point
// taps: a horizontal pass into a u8 intermediate, then a vertical pass, each clip8((2^21 + sum px * k) >> 22).
// The taps are made on the host in double, as Pillow makes them (precompute_coeffs, normalize_coeffs_8bpc),
// and only integers reach the device, so the kernels give Pillow's bytes. The 48 x 48 gray fast path
// (resnet.hip resize_u8) is a kernel of its own and stays as it is.
#include <algorithm>
#include <cmath>

#include "mec.h"
#include "mec_common.h"
#include "ragged_stage.h"

namespace mec {
namespace rr {

constexpr int kOut = 224;       // IMAGE_SIZE
constexpr int kMaxSide = 4096;  // of a source image: ksize <= 2 * ceil(4096 / 224) + 1 = 39
constexpr int kPrec = 22;       // Pillow's PRECISION_BITS = 32 - 8 - 2
constexpr int kLds = 32768;     // the horizontal pass' source tile (two workgroups' tiles per 64 KB)
constexpr int kTileRows = 32;   // at most this many source rows per tile

int ksize_of(int in_size, int out_size) {
  const double scale = (double)in_size / out_size;
  return (int)std::ceil(scale < 1.0 ? 1.0 : scale) * 2 + 1;
}

// One extent's table as the kernels read it: xmin[out] | n[out] | k[out][ksize], taps past n are 0.
#pragma clang fp contract(off)
void build_taps(int in_size, int out_size, int* xmins, int* ns, int* kk, int kstride) {
  const double scale = (double)in_size / out_size;
  const double filterscale = scale < 1.0 ? 1.0 : scale;
  const double support = 1.0 * filterscale;  // the bilinear filter's support is 1
  const double ss = 1.0 / filterscale;
  std::vector<double> w((size_t)ksize_of(in_size, out_size));
  for (int xx = 0; xx < out_size; ++xx) {
    const double center = (xx + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    xmax -= xmin;
    double ww = 0.0;
    for (int x = 0; x < xmax; ++x) {
      double t = (x + xmin - center + 0.5) * ss;
      if (t < 0) t = -t;
      w[x] = t < 1.0 ? 1.0 - t : 0.0;
      ww += w[x];
    }
    int* k = kk + (size_t)xx * kstride;
    for (int x = 0; x < kstride; ++x) k[x] = 0;
    for (int x = 0; x < xmax; ++x) {
      const double v = ww != 0.0 ? w[x] / ww : w[x];
      k[x] = v < 0 ? (int)(-0.5 + v * (1 << kPrec)) : (int)(0.5 + v * (1 << kPrec));
    }
    xmins[xx] = xmin;
    ns[xx] = xmax;
  }
}

// Tables by source extent (-> 224), process-wide. An extent is one of 4096 values and a table at most
// (2 + 39) * 224 ints, but a process that sees every extent would hold 80 MB of them: the cache keeps at most
// kCacheMax extents (under 10 MB) and is emptied when a new extent finds it full; a table costs microseconds.
constexpr size_t kCacheMax = 256;
std::mutex g_cache_mu;
std::map<int, std::vector<int>> g_cache;

std::vector<int> taps_for(int extent) {
  std::lock_guard<std::mutex> lk(g_cache_mu);
  auto it = g_cache.find(extent);
  if (it != g_cache.end()) return it->second;
  const int ks = ksize_of(extent, kOut);
  std::vector<int> t((size_t)kOut * (2 + ks));
  build_taps(extent, kOut, t.data(), t.data() + kOut, t.data() + 2 * kOut, ks);
  if (g_cache.size() >= kCacheMax) g_cache.clear();
  g_cache[extent] = t;
  return t;
}

struct Image {
  long long src_off, tmp_off;  // bytes into src / tmp
  int H, W;
  int xtab, ytab;  // the width's and the height's table, in ints from the tables' start
  int kx, ky;      // their ksize
};
struct Tile {
  int img, row0, rows;
};

__device__ inline int clip8(int acc) {
  const int v = acc >> kPrec;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// Horizontal pass: one workgroup per tile of whole source rows, which are one contiguous byte range. The range
// is staged in LDS at its own 16-byte phase (aligned 16-byte loads for the chunks inside it, byte loads for the
// two ends, so nothing outside the tile is read), then lane o of a row's 224 * C outputs sums its n taps from
// LDS and stores one byte: a wave writes 64 contiguous bytes of tmp. Four rows share one read of the taps.
template <int C>
__global__ __launch_bounds__(256) void horizontal_kernel(const uint8_t* __restrict__ src, const Image* __restrict__ imgs,
                                                         const Tile* __restrict__ tiles, const int* __restrict__ taps,
                                                         uint8_t* __restrict__ tmp) {
  __shared__ __attribute__((aligned(16))) uint8_t s[kLds];
  const Tile tile = tiles[blockIdx.x];
  const Image im = imgs[tile.img];
  const int tid = threadIdx.x, rowbytes = im.W * C, nbytes = tile.rows * rowbytes;
  const uint8_t* g0 = src + im.src_off + (size_t)tile.row0 * rowbytes;
  const int phase = (int)(reinterpret_cast<uintptr_t>(g0) & 15);  // s[phase + i] = g0[i]
  const int nchunks = (phase + nbytes + 15) >> 4;
  for (int q = tid; q < nchunks; q += 256) {
    const int lo = 16 * q - phase;
    if (lo >= 0 && lo + 16 <= nbytes) {
      *reinterpret_cast<uint4*>(s + 16 * q) = *reinterpret_cast<const uint4*>(g0 + lo);
    } else {
      for (int b = max(lo, 0); b < min(lo + 16, nbytes); ++b) s[phase + b] = g0[b];
    }
  }
  __syncthreads();
  const int* xmin = taps + im.xtab;
  const int* xn = xmin + kOut;
  const int* xk = xn + kOut;
  constexpr int nout = kOut * C;
  uint8_t* t0 = tmp + im.tmp_off + (size_t)tile.row0 * nout;
  for (int o = tid; o < nout; o += 256) {
    const int xx = o / C, c = o - xx * C;
    const int n = xn[xx];
    const int* k = xk + xx * im.kx;
    const uint8_t* p = s + phase + xmin[xx] * C + c;
    int r = 0;
    for (; r + 4 <= tile.rows; r += 4) {
      int a0 = 1 << (kPrec - 1), a1 = a0, a2 = a0, a3 = a0;
      const uint8_t* q = p + r * rowbytes;
      for (int j = 0; j < n; ++j) {
        const int kj = k[j];
        a0 += (int)q[j * C] * kj;
        a1 += (int)q[j * C + rowbytes] * kj;
        a2 += (int)q[j * C + 2 * rowbytes] * kj;
        a3 += (int)q[j * C + 3 * rowbytes] * kj;
      }
      uint8_t* t = t0 + (size_t)r * nout + o;
      t[0] = (uint8_t)clip8(a0);
      t[nout] = (uint8_t)clip8(a1);
      t[2 * nout] = (uint8_t)clip8(a2);
      t[3 * nout] = (uint8_t)clip8(a3);
    }
    for (; r < tile.rows; ++r) {
      int a0 = 1 << (kPrec - 1);
      const uint8_t* q = p + r * rowbytes;
      for (int j = 0; j < n; ++j) a0 += (int)q[j * C] * k[j];
      t0[(size_t)r * nout + o] = (uint8_t)clip8(a0);
    }
  }
}

// Vertical pass: grid (224 * G / 256, B), G = 224 * C / 4. A thread makes 4 adjacent bytes of one output row
// from one aligned word of each of its n tmp rows, so a wave reads and writes 256 contiguous bytes. The four
// results are stored as four bytes: a word assembled from them would have to mask each one (the compiler may
// pair the shift and the clamp of two results into v_ashr_pk_u8_i32, whose upper result bits are not zero).
template <int C>
__global__ __launch_bounds__(256) void vertical_kernel(const uint8_t* __restrict__ tmp, const Image* __restrict__ imgs,
                                                       const int* __restrict__ taps, uint8_t* __restrict__ out) {
  constexpr int G = kOut * C / 4;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= kOut * G) return;
  const Image im = imgs[blockIdx.y];
  const int yy = idx / G, g = idx - yy * G;
  const int* ymin = taps + im.ytab;
  const int n = ymin[kOut + yy];
  const int* k = ymin + 2 * kOut + yy * im.ky;
  const uint32_t* t = reinterpret_cast<const uint32_t*>(tmp + im.tmp_off) + (size_t)ymin[yy] * G + g;
  int a0 = 1 << (kPrec - 1), a1 = a0, a2 = a0, a3 = a0;
  for (int j = 0; j < n; ++j) {
    const uint32_t w = t[(size_t)j * G];
    const int kj = k[j];
    a0 += (int)(w & 0xFF) * kj;
    a1 += (int)((w >> 8) & 0xFF) * kj;
    a2 += (int)((w >> 16) & 0xFF) * kj;
    a3 += (int)(w >> 24) * kj;
  }
  uint8_t* o = out + ((size_t)blockIdx.y * kOut * G + idx) * 4;
  o[0] = (uint8_t)clip8(a0);
  o[1] = (uint8_t)clip8(a1);
  o[2] = (uint8_t)clip8(a2);
  o[3] = (uint8_t)clip8(a3);
}

// The batch's descriptors and tables (ragged_stage.h), per device.
using State = StageBuf;
std::mutex g_mu;
std::map<int, State> g_state;
// mec_resize_prof_*: TAG_RESIZE_H / TAG_RESIZE_V. Never destroyed: a static's destructor would destroy events
// after the HIP runtime has shut down.
Prof& g_prof_h = *new Prof;
Prof& g_prof_v = *new Prof;

bool on_gpu(long long H, long long W) {
  return H >= 1 && H <= kMaxSide && W >= 1 && W <= kMaxSide && H <= 100 * W;
}

int resize_ragged(const uint8_t* src, const int64_t* offs, const int32_t* hw, int B, int C, size_t src_bytes,
                  uint8_t* tmp, size_t tmp_bytes, uint8_t* out, hipStream_t s) {
  MEC_REQUIRE(B >= 0, "mec_resize_ragged_u8: B < 0");
  MEC_REQUIRE(C == 1 || C == 3, "mec_resize_ragged_u8: C must be 1 or 3");
  if (B == 0) return 0;
  MEC_REQUIRE(src && offs && hw && tmp && out, "mec_resize_ragged_u8: src, offs, hw, tmp or out is null");
  MEC_REQUIRE(reinterpret_cast<uintptr_t>(tmp) % 4 == 0, "mec_resize_ragged_u8: tmp must be 4-byte aligned");
  // ---- host: every descriptor is checked before anything is launched
  std::vector<Image> imgs((size_t)B);
  std::vector<Tile> tiles;
  std::map<int, int> tab;  // extent -> its table's offset in ints
  std::vector<int> taps;
  auto table = [&](int extent) {
    auto it = tab.find(extent);
    if (it != tab.end()) return it->second;
    const std::vector<int> t = taps_for(extent);
    const int at = (int)taps.size();
    taps.insert(taps.end(), t.begin(), t.end());
    tab[extent] = at;
    return at;
  };
  size_t need = 0;
  for (int i = 0; i < B; ++i) {
    const int H = hw[2 * i], W = hw[2 * i + 1];
    MEC_TRY(check_source("mec_resize_ragged_u8", i, H, W, C, offs[i], src_bytes));
    Image& im = imgs[i];
    im.src_off = offs[i];
    im.tmp_off = (long long)need;
    im.H = H;
    im.W = W;
    need += (size_t)H * kOut * C;
  }
  MEC_REQUIRE(tmp_bytes >= need, "mec_resize_ragged_u8: tmp_bytes is less than the sum of H_i * 224 * C");
  for (int i = 0; i < B; ++i) {
    Image& im = imgs[i];
    im.xtab = table(im.W);
    im.ytab = table(im.H);
    im.kx = ksize_of(im.W, kOut);
    im.ky = ksize_of(im.H, kOut);
    const int rows = std::max(1, std::min({im.H, kTileRows, (kLds - 16) / (im.W * C)}));
    for (int r = 0; r < im.H; r += rows) tiles.push_back(Tile{i, r, std::min(rows, im.H - r)});
  }
  MEC_REQUIRE(tiles.size() < ((size_t)1 << 30), "mec_resize_ragged_u8: too many row tiles for one launch");
  MEC_REQUIRE(B <= 65535, "mec_resize_ragged_u8: B must be at most 65535");
  // ---- device
  int dev = 0;
  MEC_HIP(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(g_mu);
  const Section sec[] = {section(imgs), section(tiles), section(taps)};
  return staged_call(g_state[dev], sec, s, [&](const void* const* d) -> int {
    const Image* d_imgs = static_cast<const Image*>(d[0]);
    const Tile* d_tiles = static_cast<const Tile*>(d[1]);
    const int* d_taps = static_cast<const int*>(d[2]);
    MEC_TRY(g_prof_h.begin(TAG_RESIZE_H, s));
    if (C == 1)
      hipLaunchKernelGGL(horizontal_kernel<1>, dim3((unsigned)tiles.size()), dim3(256), 0, s, src, d_imgs, d_tiles, d_taps, tmp);
    else
      hipLaunchKernelGGL(horizontal_kernel<3>, dim3((unsigned)tiles.size()), dim3(256), 0, s, src, d_imgs, d_tiles, d_taps, tmp);
    MEC_LAUNCH_CHECK();
    MEC_TRY(g_prof_h.end(TAG_RESIZE_H, s));
    MEC_TRY(g_prof_v.begin(TAG_RESIZE_V, s));
    const unsigned gx = (unsigned)((kOut * (kOut * C / 4) + 255) / 256);
    if (C == 1)
      hipLaunchKernelGGL(vertical_kernel<1>, dim3(gx, (unsigned)B), dim3(256), 0, s, tmp, d_imgs, d_taps, out);
    else
      hipLaunchKernelGGL(vertical_kernel<3>, dim3(gx, (unsigned)B), dim3(256), 0, s, tmp, d_imgs, d_taps, out);
    MEC_LAUNCH_CHECK();
    MEC_TRY(g_prof_v.end(TAG_RESIZE_V, s));
    return 0;
  });
}

}  // namespace rr
}  // namespace mec

using namespace mec;

extern "C" {

int mec_resize_on_gpu(int H, int W) { return rr::on_gpu(H, W) ? 1 : 0; }

int mec_resize_taps(int in_size, int out_size, int32_t* xmin, int32_t* n, int32_t* k, int kmax) {
  API_GUARD({
    MEC_REQUIRE(in_size >= 1 && out_size >= 1, "mec_resize_taps: in_size and out_size must be at least 1");
    MEC_REQUIRE(xmin && n && k, "mec_resize_taps: xmin, n or k is null");
    MEC_REQUIRE(kmax >= rr::ksize_of(in_size, out_size), "mec_resize_taps: kmax is less than 2 * ceil(max(in / out, 1)) + 1");
    rr::build_taps(in_size, out_size, xmin, n, k, kmax);
    return 0;
  })
}

int mec_resize_ragged_u8(const uint8_t* src, const int64_t* offs, const int32_t* hw, int B, int C, size_t src_bytes,
                         uint8_t* tmp, size_t tmp_bytes, uint8_t* out, void* stream) {
  API_GUARD({
    return rr::resize_ragged(src, offs, hw, B, C, src_bytes, tmp, tmp_bytes, out, reinterpret_cast<hipStream_t>(stream));
  })
}

int mec_resize_prof_enable(int on) {
  std::lock_guard<std::mutex> lk(rr::g_mu);
  rr::g_prof_h.tag = on ? TAG_RESIZE_H : TAG_NONE;
  rr::g_prof_v.tag = on ? TAG_RESIZE_V : TAG_NONE;
  rr::g_prof_h.reset();
  rr::g_prof_v.reset();
  return 0;
}

int mec_resize_prof_read(double* h_ms, double* v_ms, int* count) {
  if (!h_ms || !v_ms || !count) { set_error("mec_resize_prof_read: bad args"); return -1; }
  std::lock_guard<std::mutex> lk(rr::g_mu);
  int nv = 0;
  MEC_TRY(rr::g_prof_h.read(h_ms, count));
  MEC_TRY(rr::g_prof_v.read(v_ms, &nv));
  rr::g_prof_h.reset();
  rr::g_prof_v.reset();
  return 0;
}

}  // extern "C"
