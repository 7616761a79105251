// max |x| of an f32 tensor (mec_absmax_f32, and the observation taps of the fp32 image forwards:
// mec_model_x3_observe). |x| is taken on the bits: a non-negative float orders as its unsigned bit pattern, so
// max over (bits & 0x7fffffff) is the maximum magnitude, +inf (0x7f800000) sorts above every finite value and a
// NaN above that. The integer maximum does not depend on the order it is taken in: the result is the same bits
// at any grid size and across runs.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <limits>

#include "models.h"

namespace mec {

namespace {
constexpr unsigned kAbsMask = 0x7fffffffu, kInfBits = 0x7f800000u;
}  // namespace

// Grid-stride over the 16-byte groups of x's aligned middle; workgroup 0 also takes the (at most 3 + 3) floats
// before the first and after the last whole group. Lanes by shuffles, the four waves through LDS, then one
// atomicMax per workgroup on *slot: the slot keeps the running maximum of every launch since it was zeroed.
__global__ __launch_bounds__(256) void absmax_f32_kernel(const float* __restrict__ x, size_t n,
                                                         unsigned* __restrict__ slot) {
  __shared__ unsigned part[4];
  const unsigned* u = reinterpret_cast<const unsigned*>(x);
  const size_t to16 = ((16 - (reinterpret_cast<uintptr_t>(x) & 15)) & 15) / 4;  // floats before a 16-byte boundary
  const size_t head = to16 < n ? to16 : n;
  const size_t n4 = (n - head) / 4, tail0 = head + 4 * n4;
  const uint4* v = reinterpret_cast<const uint4*>(u + head);
  unsigned m = 0;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
    const uint4 q = v[i];
    m = max(m, max(max(q.x & kAbsMask, q.y & kAbsMask), max(q.z & kAbsMask, q.w & kAbsMask)));
  }
  if (blockIdx.x == 0) {
    if (threadIdx.x < head) m = max(m, u[threadIdx.x] & kAbsMask);
    if (tail0 + threadIdx.x < n) m = max(m, u[tail0 + threadIdx.x] & kAbsMask);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, off));
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) atomicMax(slot, max(max(part[0], part[1]), max(part[2], part[3])));
}

// At most four workgroups per CU: these are small, HBM-bound launches that run only while calibrating.
int launch_absmax_f32(const float* x, size_t n, unsigned* slot, hipStream_t s) {
  if (n == 0) return 0;
  MEC_REQUIRE(x && slot, "absmax_f32: null pointer");
  MEC_REQUIRE((reinterpret_cast<uintptr_t>(x) & 3) == 0, "absmax_f32: x must be 4-byte aligned");
  const int ncu = cu_count();
  if (ncu < 0) return -1;
  const size_t groups = (n / 4 + 255) / 256;
  const unsigned grid = (unsigned)std::min<size_t>(std::max<size_t>(groups, 1), (size_t)4 * ncu);
  hipLaunchKernelGGL(absmax_f32_kernel, dim3(grid), dim3(256), 0, s, x, n, slot);
  MEC_LAUNCH_CHECK();
  return 0;
}

float absmax_from_bits(unsigned bits) {
  if (bits >= kInfBits) return std::numeric_limits<float>::infinity();
  float f;
  std::memcpy(&f, &bits, sizeof f);
  return f;
}

int absmax_f32(const float* x_dev, long long n, float* out_host, hipStream_t s) {
  MEC_REQUIRE(out_host, "mec_absmax_f32: out_host is null");
  MEC_REQUIRE(n >= 0, "mec_absmax_f32: n < 0");
  *out_host = 0.f;
  if (n == 0) return 0;
  MEC_REQUIRE(x_dev, "mec_absmax_f32: x_dev is null");
  DevBuf slot;
  MEC_TRY(slot.ensure(sizeof(unsigned)));
  MEC_HIP(hipMemsetAsync(slot.p, 0, sizeof(unsigned), s));
  MEC_TRY(launch_absmax_f32(x_dev, (size_t)n, slot.as<unsigned>(), s));
  unsigned bits = 0;
  MEC_HIP(hipMemcpyAsync(&bits, slot.p, sizeof bits, hipMemcpyDeviceToHost, s));
  MEC_HIP(hipStreamSynchronize(s));
  *out_host = absmax_from_bits(bits);
  return 0;
}

}  // namespace mec
