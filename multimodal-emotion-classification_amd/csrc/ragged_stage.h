// The descriptors of a ragged-batch call (resize.hip, image_canon.hip): one pinned host image and one device copy,
// per device and per entry point. A call waits for the previous call's kernels on that device (the event) before it
// overwrites either, so calls on any streams are safe; the kernels are short. Never freed (process lifetime).
// Also what those calls share on the host: the staged call itself and the check of an image's source.
#pragma once
#include <algorithm>
#include <cstring>

#include "mec.h"
#include "mec_common.h"

namespace mec {

struct StageBuf {
  void* host = nullptr;
  void* dev = nullptr;
  size_t bytes = 0;
  hipEvent_t done = nullptr;
  bool pending = false;
};

inline int ensure(StageBuf& st, size_t bytes) {
  if (!st.done) MEC_HIP(hipEventCreateWithFlags(&st.done, hipEventDisableTiming));
  if (st.pending) {
    MEC_HIP(hipEventSynchronize(st.done));
    st.pending = false;
  }
  if (bytes <= st.bytes) return 0;
  if (st.host) (void)hipHostFree(st.host);
  if (st.dev) (void)hipFree(st.dev);
  st.host = st.dev = nullptr;
  st.bytes = 0;
  const size_t cap = std::max(bytes * 2, (size_t)1 << 16);
  MEC_HIP(hipHostMalloc(&st.host, cap, hipHostMallocDefault));
  MEC_HIP(hipMalloc(&st.dev, cap));
  st.bytes = cap;
  return 0;
}

inline size_t pad16(size_t n) { return (n + 15) & ~(size_t)15; }

// One host array of a call's descriptors.
struct Section {
  const void* p;
  size_t bytes;
};
template <class T> Section section(const std::vector<T>& v) { return Section{v.data(), v.size() * sizeof(T)}; }

// A staged call: the sections are laid out in st's pinned image, each at a 16-byte boundary, uploaded in one copy
// on s, and launch(d) runs with d[i] the device address of section i. From the copy on the buffers are in use until
// `done`, which is recorded whatever launch returned. The caller holds its file's mutex and has validated everything.
template <size_t N, class F> int staged_call(StageBuf& st, const Section (&sec)[N], hipStream_t s, F&& launch) {
  size_t at[N], total = 0;
  for (size_t i = 0; i < N; ++i) {
    at[i] = pad16(total);
    total = at[i] + sec[i].bytes;
  }
  MEC_TRY(ensure(st, total));
  const void* d[N];
  for (size_t i = 0; i < N; ++i) {
    if (sec[i].bytes) std::memcpy(static_cast<char*>(st.host) + at[i], sec[i].p, sec[i].bytes);
    d[i] = static_cast<const char*>(st.dev) + at[i];
  }
  MEC_HIP(hipMemcpyAsync(st.dev, st.host, total, hipMemcpyHostToDevice, s));
  st.pending = true;
  const int rc = launch(d);
  MEC_HIP(hipEventRecord(st.done, s));
  return rc;
}

// "requirement failed: <call>: image <i> <what>", the form of every per-image rejection.
inline int fail(const char* call, int i, const std::string& what) {
  set_error(std::string("requirement failed: ") + call + ": image " + std::to_string(i) + " " + what);
  return -1;
}

// What every ragged call requires of image i's source: H x W in the resize's domain (mec_resize_on_gpu, resize.hip
// rr::on_gpu) and its H * W * bpp bytes at off inside src_bytes.
inline int check_source(const char* call, int i, int H, int W, int bpp, int64_t off, size_t src_bytes) {
  if (!mec_resize_on_gpu(H, W))
    return fail(call, i, "is " + std::to_string(H) + " x " + std::to_string(W) + ", outside 1 <= H, W <= 4096 with H <= 100 W");
  const size_t bytes = (size_t)H * W * bpp;
  if (off < 0 || (uint64_t)off > src_bytes || bytes > src_bytes - (size_t)off) return fail(call, i, "does not lie inside src_bytes");
  return 0;
}

}  // namespace mec
