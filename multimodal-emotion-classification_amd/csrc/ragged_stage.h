// The descriptors of a ragged-batch call (resize.hip, image_canon.hip): one pinned host image and one device copy,
// per device and per entry point. A call waits for the previous call's kernels on that device (the event) before it
// overwrites either, so calls on any streams are safe; the kernels are short. Never freed (process lifetime).
#pragma once
#include <algorithm>

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

}  // namespace mec
