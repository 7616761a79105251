// Mode conversion and the gray test of a ragged batch of u8 images in their native pixel formats (include/mec.h
// mec_image_gray_ragged_u8, mec_image_canon_ragged_u8, MEC_PIX_*): what Pillow's convert('RGB') and the host's
// R == G == B comparison give, for L, LA, RGB, RGBA and P. The conversion is a byte selection (L and LA replicate
// L, RGBA drops alpha, P looks its index up in a 256-entry RGB palette), so the bytes are Pillow's. The images
// are packed as mec_resize_ragged_u8 takes them, and the converted ones are written where that call can read
// them through the same src pointer. The host side of a call (staging, the source check) is ragged_stage.h's.
#include <algorithm>

#include "mec.h"
#include "mec_common.h"
#include "ragged_stage.h"

namespace mec {
namespace ic {

constexpr int kTilePix = 4096;  // pixels per tile: at most 16 KB of source; a multiple of 4, so a tile's output
                                // starts on a word of the (16-byte aligned) destination image
constexpr int kMaxBpp = 4;
constexpr int kPalBytes = 768;  // 256 RGB entries

__host__ __device__ inline int bpp_of(int fmt) {
  return fmt == MEC_PIX_LA ? 2 : fmt == MEC_PIX_RGB ? 3 : fmt == MEC_PIX_RGBA ? 4 : 1;
}

struct Image {
  long long src_off, pal_off;  // bytes into src (pal_off -1: no palette)
  long long dst_off;           // bytes into dst (the canon call)
  int fmt, c_out;
};
struct Tile {
  int img, pix0, npix;
};

// A tile's source bytes, one contiguous range of whole pixels, into LDS at its own 16-byte phase:
// s[phase + i] = g0[i]. Aligned 16-byte loads for the chunks inside the range and byte loads for its two ends,
// so no byte outside the tile is read (csrc/resize.hip stages its row tiles the same way).
__device__ inline int stage(const uint8_t* g0, int nbytes, uint8_t* s, int tid) {
  const int phase = (int)(reinterpret_cast<uintptr_t>(g0) & 15);
  const int nchunks = (phase + nbytes + 15) >> 4;
  for (int q = tid; q < nchunks; q += 256) {
    const int lo = 16 * q - phase;
    if (lo >= 0 && lo + 16 <= nbytes) {
      *reinterpret_cast<uint4*>(s + 16 * q) = *reinterpret_cast<const uint4*>(g0 + lo);
    } else {
      for (int b = max(lo, 0); b < min(lo + 16, nbytes); ++b) s[phase + b] = g0[b];
    }
  }
  return phase;
}

// One workgroup per tile of an RGB, RGBA or P image. colour[img] becomes non-zero when a pixel of the tile has
// R != G or R != B after conversion; only staged bytes (the tile's own) enter the test. For P the palette's
// "entry is coloured" table is derived here, per tile, from the 768 palette bytes: an entry counts only where an
// index byte of the image selects it. Every tile reads all its bytes: returning early where the image's word is
// already set was measured and is slower (the loads of a word under atomics cost more than the tile).
__global__ __launch_bounds__(256) void gray_kernel(const uint8_t* __restrict__ src, const Image* __restrict__ imgs,
                                                   const Tile* __restrict__ tiles, int* colour) {
  __shared__ __attribute__((aligned(16))) uint8_t s[kTilePix * kMaxBpp + 16];
  __shared__ uint8_t ctab[256];
  __shared__ int flags[4];  // the waves' results
  const Tile tile = tiles[blockIdx.x];
  const Image im = imgs[tile.img];
  const int tid = threadIdx.x;
  const int bpp = bpp_of(im.fmt);
  const int phase = stage(src + im.src_off + (size_t)tile.pix0 * bpp, tile.npix * bpp, s, tid);
  if (im.fmt == MEC_PIX_P) {
    const uint8_t* pal = src + im.pal_off + 3 * tid;
    ctab[tid] = (uint8_t)((pal[0] != pal[1]) | (pal[0] != pal[2]));
  }
  __syncthreads();
  int c = 0;
  const uint8_t* p0 = s + phase;
  if (im.fmt == MEC_PIX_P) {
    for (int p = tid; p < tile.npix; p += 256) c |= ctab[p0[p]];
  } else {
    for (int p = tid; p < tile.npix; p += 256) {
      const uint8_t* q = p0 + p * bpp;
      c |= (q[0] ^ q[1]) | (q[0] ^ q[2]);
    }
  }
  const int w = __any(c != 0);
  if ((tid & 63) == 0) flags[tid >> 6] = w;
  __syncthreads();
  if (tid == 0 && (flags[0] | flags[1] | flags[2] | flags[3])) atomicOr(colour + tile.img, 1);
}

// gray[i] = 1 where no tile found colour (L and LA have no tiles).
__global__ void flags_kernel(int* gray, int B) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < B) gray[i] = gray[i] ? 0 : 1;
}

// One workgroup per tile of an image with c_out 1 or 3: the tile's npix * c_out output bytes are contiguous
// and start on a word. A thread assembles one aligned word from four converted bytes (a wave stores 256
// contiguous bytes); the up to three bytes behind the last whole word are byte stores. src and dst may lie in
// one allocation (the host has rejected every overlap), so neither is __restrict__.
__global__ __launch_bounds__(256) void canon_kernel(const uint8_t* src, const Image* __restrict__ imgs,
                                                    const Tile* __restrict__ tiles, uint8_t* dst) {
  __shared__ __attribute__((aligned(16))) uint8_t s[kTilePix * kMaxBpp + 16];
  __shared__ uint8_t pal[kPalBytes];
  const Tile tile = tiles[blockIdx.x];
  const Image im = imgs[tile.img];
  const int tid = threadIdx.x;
  const int bpp = bpp_of(im.fmt), C = im.c_out;
  const int phase = stage(src + im.src_off + (size_t)tile.pix0 * bpp, tile.npix * bpp, s, tid);
  if (im.fmt == MEC_PIX_P)
    for (int i = tid; i < kPalBytes; i += 256) pal[i] = src[im.pal_off + i];
  __syncthreads();
  const uint8_t* p0 = s + phase;
  const bool grayfmt = im.fmt == MEC_PIX_L || im.fmt == MEC_PIX_LA, isp = im.fmt == MEC_PIX_P;
  auto byte_at = [&](int j) -> uint32_t {  // output byte j of the tile
    const int p = C == 1 ? j : j / 3, ch = j - p * C;
    const uint8_t v = p0[p * bpp + (grayfmt || isp ? 0 : ch)];
    return isp ? pal[3 * v + ch] : v;
  };
  const int nout = tile.npix * C, nwords = nout >> 2;
  uint8_t* o = dst + im.dst_off + (size_t)tile.pix0 * C;
  for (int w = tid; w < nwords; w += 256) {
    const int j = 4 * w;
    reinterpret_cast<uint32_t*>(o)[w] = byte_at(j) | (byte_at(j + 1) << 8) | (byte_at(j + 2) << 16) | (byte_at(j + 3) << 24);
  }
  for (int j = 4 * nwords + tid; j < nout; j += 256) o[j] = (uint8_t)byte_at(j);
}

// A call's descriptors (ragged_stage.h), per entry point and per device.
using State = StageBuf;
std::mutex g_mu;
std::map<int, State> g_state[2];  // [0] the gray call, [1] the canon call
// mec_image_canon_prof_*. Never destroyed (events must not outlive the HIP runtime's shutdown).
Prof& g_prof_gray = *new Prof;
Prof& g_prof_canon = *new Prof;

// What both calls require of the source side, checked before anything else happens.
int check_sources(const char* call, const int64_t* offs, const int32_t* hw, const int32_t* fmt, const int64_t* pal_off,
                  int B, size_t src_bytes, std::vector<Image>& imgs) {
  imgs.resize((size_t)B);
  for (int i = 0; i < B; ++i) {
    const int H = hw[2 * i], W = hw[2 * i + 1], f = fmt[i];
    if (f != MEC_PIX_L && f != MEC_PIX_LA && f != MEC_PIX_RGB && f != MEC_PIX_RGBA && f != MEC_PIX_P)
      return fail(call, i, "has the unknown fmt " + std::to_string(f));
    MEC_TRY(check_source(call, i, H, W, bpp_of(f), offs[i], src_bytes));
    if (f == MEC_PIX_P) {
      if (pal_off[i] < 0) return fail(call, i, "is MEC_PIX_P and has no palette");
      if ((uint64_t)pal_off[i] > src_bytes || (size_t)kPalBytes > src_bytes - (size_t)pal_off[i])
        return fail(call, i, "has a palette that does not lie inside src_bytes");
    } else if (pal_off[i] != -1) {
      return fail(call, i, "is not MEC_PIX_P and names a palette (pal_off must be -1)");
    }
    imgs[i] = Image{offs[i], f == MEC_PIX_P ? pal_off[i] : -1, 0, f, 0};
  }
  return 0;
}

void add_tiles(std::vector<Tile>& tiles, int img, long long npix) {
  for (long long p = 0; p < npix; p += kTilePix) tiles.push_back(Tile{img, (int)p, (int)std::min<long long>(kTilePix, npix - p)});
}

int gray_ragged(const uint8_t* src, const int64_t* offs, const int32_t* hw, const int32_t* fmt, const int64_t* pal_off,
                int B, size_t src_bytes, int32_t* gray, hipStream_t s) {
  const char* call = "mec_image_gray_ragged_u8";
  MEC_REQUIRE(B >= 0, "mec_image_gray_ragged_u8: B < 0");
  if (B == 0) return 0;
  MEC_REQUIRE(src && offs && hw && fmt && pal_off && gray, "mec_image_gray_ragged_u8: src, offs, hw, fmt, pal_off or gray is null");
  MEC_REQUIRE(B <= 65535, "mec_image_gray_ragged_u8: B must be at most 65535");
  std::vector<Image> imgs;
  MEC_TRY(check_sources(call, offs, hw, fmt, pal_off, B, src_bytes, imgs));
  std::vector<Tile> tiles;
  for (int i = 0; i < B; ++i)
    if (fmt[i] != MEC_PIX_L && fmt[i] != MEC_PIX_LA) add_tiles(tiles, i, (long long)hw[2 * i] * hw[2 * i + 1]);
  MEC_REQUIRE(tiles.size() < ((size_t)1 << 30), "mec_image_gray_ragged_u8: too many tiles for one launch");
  // ---- device
  int dev = 0;
  MEC_HIP(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(g_mu);
  const Section sec[] = {section(imgs), section(tiles)};
  return staged_call(g_state[0][dev], sec, s, [&](const void* const* d) -> int {
    const Image* d_imgs = static_cast<const Image*>(d[0]);
    const Tile* d_tiles = static_cast<const Tile*>(d[1]);
    MEC_HIP(hipMemsetAsync(gray, 0, (size_t)B * sizeof(int32_t), s));  // the per-image "colour found" words
    if (!tiles.empty()) {
      MEC_TRY(g_prof_gray.begin(TAG_CANON_GRAY, s));
      hipLaunchKernelGGL(gray_kernel, dim3((unsigned)tiles.size()), dim3(256), 0, s, src, d_imgs, d_tiles, gray);
      MEC_LAUNCH_CHECK();
      MEC_TRY(g_prof_gray.end(TAG_CANON_GRAY, s));
    }
    hipLaunchKernelGGL(flags_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, s, gray, B);
    MEC_LAUNCH_CHECK();
    return 0;
  });
}

int canon_ragged(const uint8_t* src, const int64_t* offs, const int32_t* hw, const int32_t* fmt, const int64_t* pal_off,
                 const int32_t* c_out, const int64_t* dst_offs, int B, size_t src_bytes, uint8_t* dst, size_t dst_bytes,
                 hipStream_t s) {
  const char* call = "mec_image_canon_ragged_u8";
  MEC_REQUIRE(B >= 0, "mec_image_canon_ragged_u8: B < 0");
  if (B == 0) return 0;
  MEC_REQUIRE(src && offs && hw && fmt && pal_off && c_out && dst_offs && dst,
              "mec_image_canon_ragged_u8: src, offs, hw, fmt, pal_off, c_out, dst_offs or dst is null");
  MEC_REQUIRE(reinterpret_cast<uintptr_t>(dst) % 16 == 0, "mec_image_canon_ragged_u8: dst must be 16-byte aligned");
  MEC_REQUIRE(B <= 65535, "mec_image_canon_ragged_u8: B must be at most 65535");
  std::vector<Image> imgs;
  MEC_TRY(check_sources(call, offs, hw, fmt, pal_off, B, src_bytes, imgs));
  // every byte range the kernels of this call or a resize behind it read (0) or write (1), by address
  struct Range {
    uintptr_t lo, hi;
    int written, img;
  };
  std::vector<Range> ranges;
  std::vector<Tile> tiles;
  const uintptr_t s0 = reinterpret_cast<uintptr_t>(src), d0 = reinterpret_cast<uintptr_t>(dst);
  for (int i = 0; i < B; ++i) {
    const size_t npix = (size_t)hw[2 * i] * hw[2 * i + 1];
    ranges.push_back(Range{s0 + (size_t)offs[i], s0 + (size_t)offs[i] + npix * bpp_of(fmt[i]), 0, i});
    if (fmt[i] == MEC_PIX_P) ranges.push_back(Range{s0 + (size_t)pal_off[i], s0 + (size_t)pal_off[i] + kPalBytes, 0, i});
    const int C = c_out[i];
    if (C != 0 && C != 1 && C != 3) return fail(call, i, "has c_out " + std::to_string(C) + ", which is not 0, 1 or 3");
    if (C == 0) continue;
    if (dst_offs[i] < 0 || dst_offs[i] % 16 != 0) return fail(call, i, "has a dst_off that is negative or not a multiple of 16 bytes");
    if ((uint64_t)dst_offs[i] > dst_bytes || npix * C > dst_bytes - (size_t)dst_offs[i])
      return fail(call, i, "has an output that does not lie inside dst_bytes");
    ranges.push_back(Range{d0 + (size_t)dst_offs[i], d0 + (size_t)dst_offs[i] + npix * C, 1, i});
    imgs[i].dst_off = dst_offs[i];
    imgs[i].c_out = C;
    add_tiles(tiles, i, (long long)npix);
  }
  std::sort(ranges.begin(), ranges.end(), [](const Range& a, const Range& b) { return a.lo < b.lo; });
  uintptr_t read_end = 0, write_end = 0;  // the furthest ends of the ranges that start no later
  for (const Range& r : ranges) {
    if (r.lo < write_end || (r.written && r.lo < read_end))
      return fail(call, r.img, "has an output that overlaps an input, a palette or another output");
    (r.written ? write_end : read_end) = std::max(r.written ? write_end : read_end, r.hi);
  }
  MEC_REQUIRE(tiles.size() < ((size_t)1 << 30), "mec_image_canon_ragged_u8: too many tiles for one launch");
  if (tiles.empty()) return 0;  // every c_out is 0
  // ---- device
  int dev = 0;
  MEC_HIP(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(g_mu);
  const Section sec[] = {section(imgs), section(tiles)};
  return staged_call(g_state[1][dev], sec, s, [&](const void* const* d) -> int {
    MEC_TRY(g_prof_canon.begin(TAG_CANON_PIX, s));
    hipLaunchKernelGGL(canon_kernel, dim3((unsigned)tiles.size()), dim3(256), 0, s, src, static_cast<const Image*>(d[0]),
                       static_cast<const Tile*>(d[1]), dst);
    MEC_LAUNCH_CHECK();
    MEC_TRY(g_prof_canon.end(TAG_CANON_PIX, s));
    return 0;
  });
}

}  // namespace ic
}  // namespace mec

using namespace mec;

extern "C" {

int mec_image_gray_ragged_u8(const uint8_t* src, const int64_t* offs, const int32_t* hw, const int32_t* fmt,
                             const int64_t* pal_off, int B, size_t src_bytes, int32_t* gray, void* stream) {
  API_GUARD({
    return ic::gray_ragged(src, offs, hw, fmt, pal_off, B, src_bytes, gray, reinterpret_cast<hipStream_t>(stream));
  })
}

int mec_image_canon_ragged_u8(const uint8_t* src, const int64_t* offs, const int32_t* hw, const int32_t* fmt,
                              const int64_t* pal_off, const int32_t* c_out, const int64_t* dst_offs, int B,
                              size_t src_bytes, uint8_t* dst, size_t dst_bytes, void* stream) {
  API_GUARD({
    return ic::canon_ragged(src, offs, hw, fmt, pal_off, c_out, dst_offs, B, src_bytes, dst, dst_bytes,
                            reinterpret_cast<hipStream_t>(stream));
  })
}

int mec_image_canon_prof_enable(int on) {
  std::lock_guard<std::mutex> lk(ic::g_mu);
  ic::g_prof_gray.tag = on ? TAG_CANON_GRAY : TAG_NONE;
  ic::g_prof_canon.tag = on ? TAG_CANON_PIX : TAG_NONE;
  ic::g_prof_gray.reset();
  ic::g_prof_canon.reset();
  return 0;
}

int mec_image_canon_prof_read(double* gray_ms, int* gray_count, double* canon_ms, int* canon_count) {
  if (!gray_ms || !gray_count || !canon_ms || !canon_count) { set_error("mec_image_canon_prof_read: bad args"); return -1; }
  std::lock_guard<std::mutex> lk(ic::g_mu);
  MEC_TRY(ic::g_prof_gray.read(gray_ms, gray_count));
  MEC_TRY(ic::g_prof_canon.read(canon_ms, canon_count));
  ic::g_prof_gray.reset();
  ic::g_prof_canon.reset();
  return 0;
}

}  // extern "C"
