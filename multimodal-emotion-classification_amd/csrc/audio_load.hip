// The audio front end on the GPU (include/mec.h mec_audio_load_ragged): a ragged batch of PCM clips, each with
// its own sample format, channel count, rate and length, becomes the f32 [B, n_out] block mec_audio_fwd reads.
// One kernel decodes, mixes to mono ((a + b) / 2 in float32), resamples to the handle's rate with the
// polyphase filter of resample_design.h (float64 taps and accumulation, one rounding to float32) and pads or
// trims to n_out. The decoded signal exists only in LDS.
//
// Schedule. A workgroup owns a run of G * U consecutive outputs of one clip, U = cycles * up. Output m has
// phase p = (m * down) mod up and reads x[q + L - jj], q = (m * down) / up, against the phase's J contiguous
// taps; outputs m, m + U, ... share a phase, so a lane keeps G of them in registers and loads each tap once
// for G FMAs. The run's input window, G * cycles * down + J - 1 samples, is staged once in LDS as float32.
// G and cycles depend on the rate alone, and a run's start on the clip alone, so a row's result depends on
// neither B nor its place in the batch.
#include <cmath>

#include "models.h"
#include "resample_design.h"

namespace mec {
namespace al {

constexpr int kThreads = 256;
constexpr int kCopyRun = 1024;  // outputs of one identity-plan workgroup

struct Clip {
  long long src_off;
  const double* tab;  // the phase-major table of the clip's rate (null for the identity plan)
  int fmt, ch, frames;
  int n;  // outputs before the zero padding, min(librosa's length, n_out)
  int up, down, J, L;
  int cycles, G;  // G == 0: the identity plan
};

struct Run {
  int clip, r;
};

__device__ __forceinline__ float decode(const uint8_t* p, int fmt) {
  switch (fmt) {
    case MEC_PCM_U8: return (float)((int)p[0] - 128) * (1.0f / 128.0f);
    case MEC_PCM_S16: return (float)(int16_t)(uint16_t)(p[0] | (p[1] << 8)) * (1.0f / 32768.0f);
    case MEC_PCM_S24: {
      const uint32_t u = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
      return (float)((int32_t)(u << 8) >> 8) * (1.0f / 8388608.0f);
    }
    case MEC_PCM_S32: {
      const uint32_t u = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
      return (float)(int32_t)u * (1.0f / 2147483648.0f);
    }
    default: {
      const uint32_t u = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
      return __uint_as_float(u);
    }
  }
}

__device__ __forceinline__ int bytes_of(int fmt) { return fmt == MEC_PCM_U8 ? 1 : fmt == MEC_PCM_S16 ? 2 : fmt == MEC_PCM_S24 ? 3 : 4; }

// frame k of the clip as mono float32; the caller has 0 <= k < frames
__device__ __forceinline__ float frame(const uint8_t* src, const Clip& c, int bps, long long k) {
  const uint8_t* p = src + c.src_off + k * (long long)(c.ch * bps);
  const float a = decode(p, c.fmt);
  if (c.ch == 1) return a;
  return (a + decode(p + bps, c.fmt)) * 0.5f;
}

template <int G>
__device__ __forceinline__ void run_outputs(const Clip& c, const float* win, int m0,
                                            float* __restrict__ row, int n_out) {
  const int U = c.cycles * c.up, nd = c.cycles * c.down;
  for (int col = threadIdx.x; col < U; col += kThreads) {
    if (m0 + col >= c.n) break;  // the columns' first outputs ascend: nothing left in this run
    const long long t = (long long)col * c.down;
    const int p = (int)(t % c.up), qc = (int)(t / c.up);
    const double2* g = reinterpret_cast<const double2*>(c.tab + (long long)p * c.J);
    const float* x = win + qc + c.J - 1;
    double acc[G];
#pragma unroll
    for (int i = 0; i < G; ++i) acc[i] = 0.0;
    for (int jj = 0; jj < c.J; jj += 2) {
      const double2 h = g[jj >> 1];
#pragma unroll
      for (int i = 0; i < G; ++i) {
        acc[i] = fma(h.x, (double)x[i * nd - jj], acc[i]);
        acc[i] = fma(h.y, (double)x[i * nd - jj - 1], acc[i]);
      }
    }
#pragma unroll
    for (int i = 0; i < G; ++i) {
      const int m = m0 + col + i * U;
      if (m < c.n) row[m] = (float)acc[i];
    }
  }
}

// One workgroup per run. Dynamic LDS: the largest window of the launch, in floats.
__global__ __launch_bounds__(kThreads) void load_kernel(const uint8_t* __restrict__ src, const Clip* __restrict__ clips,
                                                        const Run* __restrict__ runs, float* __restrict__ wave,
                                                        int n_out) {
  extern __shared__ float win[];
  const Run run = runs[blockIdx.x];
  const Clip c = clips[run.clip];
  float* row = wave + (long long)run.clip * n_out;
  const int bps = bytes_of(c.fmt);
  const int R = c.G ? c.G * c.cycles * c.up : kCopyRun;
  const int m0 = run.r * R, m1 = min(m0 + R, n_out);
  // the zero padding of this run
  for (int m = max(m0, c.n) + threadIdx.x; m < m1; m += kThreads) row[m] = 0.0f;
  if (m0 >= c.n) return;
  if (c.G == 0) {  // identity plan: decode, mix, copy (c.n <= frames)
    for (int m = m0 + threadIdx.x; m < min(m1, c.n); m += kThreads) row[m] = frame(src, c, bps, m);
    return;
  }
  // x[ks + i] -> win[i], from J - 1 samples before the first output's x[q0 + L]
  const int nd = c.cycles * c.down;
  const long long ks = (long long)run.r * c.G * nd + c.L - (c.J - 1);
  const int wn = c.G * nd + c.J - 1;
  for (int i = threadIdx.x; i < wn; i += kThreads) {
    const long long k = ks + i;
    win[i] = k >= 0 && k < c.frames ? frame(src, c, bps, k) : 0.0f;
  }
  __syncthreads();
  switch (c.G) {
    case 8: run_outputs<8>(c, win, m0, row, n_out); break;
    case 4: run_outputs<4>(c, win, m0, row, n_out); break;
    case 2: run_outputs<2>(c, win, m0, row, n_out); break;
    default: run_outputs<1>(c, win, m0, row, n_out); break;
  }
}

// mec_audio_load_prof_*: process-wide, as mec_resize_prof_*. Never destroyed (see resize.hip).
std::mutex g_prof_mu;
Prof& g_prof = *new Prof;

int fail(int i, const std::string& what) {
  set_error("requirement failed: mec_audio_load_ragged: clip " + std::to_string(i) + " " + what);
  return -1;
}

}  // namespace al

AudioModel::~AudioModel() {
  for (auto& t : load_tabs) {
    if (t.last) {
      (void)hipEventSynchronize(t.last);
      (void)hipEventDestroy(t.last);
    }
    if (t.dev) (void)hipFree(t.dev);
  }
  if (load_stage.done) {
    (void)hipEventSynchronize(load_stage.done);
    (void)hipEventDestroy(load_stage.done);
  }
  if (load_stage.host) (void)hipHostFree(load_stage.host);
  if (load_stage.dev) (void)hipFree(load_stage.dev);
}

// The cached phase-major table of rate_in -> sr, built and uploaded on first use. At most kMaxTables are
// kept; the least recently used one that this call does not need goes, after the event of the last call that
// read it. The caller holds load_mu.
int AudioModel::load_table(int rate_in, const std::vector<int>& keep, ResampleTable** out) {
  for (auto& t : load_tabs)
    if (t.rate_in == rate_in) {
      t.stamp = ++load_stamp;
      *out = &t;
      return 0;
    }
  rs::Plan p;
  MEC_REQUIRE(rs::plan(rate_in, sr, &p) && p.half > 0, "mec_audio_load_ragged: no resampling plan for the rate");
  if ((int)load_tabs.size() >= kMaxTables) {
    int lru = -1, i = 0;
    uint64_t oldest = 0;
    for (auto& t : load_tabs) {
      if (std::find(keep.begin(), keep.end(), t.rate_in) == keep.end() && (lru < 0 || t.stamp < oldest)) {
        lru = i;
        oldest = t.stamp;
      }
      ++i;
    }
    MEC_REQUIRE(lru >= 0, "mec_audio_load_ragged: more than 16 distinct rates in one call");
    ResampleTable& t = *std::next(load_tabs.begin(), lru);
    MEC_HIP(hipEventSynchronize(t.last));
    (void)hipEventDestroy(t.last);
    (void)hipFree(t.dev);
    load_tabs.erase(std::next(load_tabs.begin(), lru));
  }
  std::vector<double> h((size_t)p.taps()), g((size_t)p.up * p.J());
  rs::taps(p, h.data());
  rs::phase_major(p, h.data(), g.data());
  ResampleTable t;
  t.rate_in = rate_in;
  t.plan = p;
  MEC_HIP(hipMalloc(reinterpret_cast<void**>(&t.dev), g.size() * sizeof(double)));
  if (hipMemcpy(t.dev, g.data(), g.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
      hipEventCreateWithFlags(&t.last, hipEventDisableTiming) != hipSuccess) {
    (void)hipFree(t.dev);
    set_error("mec_audio_load_ragged: uploading a tap table failed");
    return -1;
  }
  t.stamp = ++load_stamp;
  load_tabs.push_back(t);
  *out = &load_tabs.back();
  return 0;
}

int AudioModel::load_ragged(const uint8_t* src, const int64_t* offs, const int32_t* desc, int B, size_t src_bytes,
                            float* wave, int n_out, hipStream_t s) {
  using namespace al;
  MEC_REQUIRE(B >= 0, "mec_audio_load_ragged: B < 0");
  MEC_REQUIRE(n_out >= 1, "mec_audio_load_ragged: n_out must be at least 1");
  if (B == 0) return 0;
  MEC_REQUIRE(offs && desc && wave, "mec_audio_load_ragged: offs, desc or wave is null");
  MEC_REQUIRE(src || src_bytes == 0, "mec_audio_load_ragged: src is null");
  MEC_REQUIRE(B <= 65535, "mec_audio_load_ragged: B must be at most 65535");
  // ---- host: every descriptor is checked before anything is launched
  std::vector<Clip> clips((size_t)B);
  std::vector<rs::Plan> plans((size_t)B);
  std::vector<int> rates;  // the distinct rates that need a table
  for (int i = 0; i < B; ++i) {
    const int fmt = desc[4 * i], ch = desc[4 * i + 1], rate = desc[4 * i + 2], frames = desc[4 * i + 3];
    if (fmt < MEC_PCM_U8 || fmt > MEC_PCM_F32) return fail(i, "has the unknown format " + std::to_string(fmt));
    if (ch < 1 || ch > 2) return fail(i, "has " + std::to_string(ch) + " channels, outside 1..2");
    if (!rs::plan(rate, sr, &plans[i]))
      return fail(i, "has the rate " + std::to_string(rate) + ", outside mec_resample_on_gpu for " + std::to_string(sr));
    if (frames < 0) return fail(i, "has frames < 0");
    const int bps = fmt == MEC_PCM_U8 ? 1 : fmt == MEC_PCM_S16 ? 2 : fmt == MEC_PCM_S24 ? 3 : 4;
    const uint64_t bytes = (uint64_t)frames * ch * bps;
    if (offs[i] < 0 || (uint64_t)offs[i] > src_bytes || bytes > src_bytes - (uint64_t)offs[i])
      return fail(i, "does not lie inside src_bytes");
    Clip& c = clips[i];
    c = Clip{};
    c.src_off = offs[i];
    c.fmt = fmt;
    c.ch = ch;
    c.frames = frames;
    c.n = (int)std::min<long long>(rs::out_len(frames, rate, sr), n_out);
    if (plans[i].half && std::find(rates.begin(), rates.end(), rate) == rates.end()) rates.push_back(rate);
  }
  MEC_REQUIRE((int)rates.size() <= kMaxTables, "mec_audio_load_ragged: more than 16 distinct rates in one call");
  // ---- device
  std::lock_guard<std::mutex> lk(load_mu);
  std::vector<ResampleTable*> tabs(rates.size());
  for (size_t r = 0; r < rates.size(); ++r) MEC_TRY(load_table(rates[r], rates, &tabs[r]));
  std::vector<Run> runs;
  size_t lds = 0;
  for (int i = 0; i < B; ++i) {
    Clip& c = clips[i];
    int R = kCopyRun;
    if (plans[i].half) {
      const rs::Plan& p = plans[i];
      const size_t r = std::find(rates.begin(), rates.end(), desc[4 * i + 2]) - rates.begin();
      c.tab = tabs[r]->dev;
      c.up = p.up;
      c.down = p.down;
      c.J = p.J();
      c.L = p.L();
      rs::schedule(p, kThreads, &c.cycles, &c.G);
      R = c.G * c.cycles * c.up;
      lds = std::max(lds, ((size_t)c.G * c.cycles * c.down + c.J - 1) * sizeof(float));
    }
    for (int r = 0; r * (long long)R < n_out; ++r) runs.push_back(Run{i, r});
  }
  MEC_REQUIRE(runs.size() < ((size_t)1 << 30), "mec_audio_load_ragged: too many runs for one launch");
  MEC_REQUIRE(lds <= (size_t)rs::kWindow * sizeof(float), "mec_audio_load_ragged: a window exceeds LDS");
  const Section sec[] = {section(clips), section(runs)};
  const int rc = staged_call(load_stage, sec, s, [&](const void* const* d) -> int {
    std::lock_guard<std::mutex> pl(g_prof_mu);
    MEC_TRY(g_prof.begin(TAG_AUDIO_LOAD, s));
    hipLaunchKernelGGL(load_kernel, dim3((unsigned)runs.size()), dim3(kThreads), lds, s, src,
                       static_cast<const Clip*>(d[0]), static_cast<const Run*>(d[1]), wave, n_out);
    MEC_LAUNCH_CHECK();
    MEC_TRY(g_prof.end(TAG_AUDIO_LOAD, s));
    return 0;
  });
  for (auto* t : tabs) MEC_HIP(hipEventRecord(t->last, s));
  return rc;
}

}  // namespace mec

using namespace mec;

extern "C" {

int mec_resample_on_gpu(int rate_in, int rate_out) { return rs::plan(rate_in, rate_out, nullptr) ? 1 : 0; }

int mec_resample_plan(int rate_in, int rate_out, int* up, int* down, int* half) {
  API_GUARD({
    MEC_REQUIRE(up && down && half, "mec_resample_plan: up, down or half is null");
    rs::Plan p;
    MEC_REQUIRE(rs::plan(rate_in, rate_out, &p), "mec_resample_plan: the rates are outside mec_resample_on_gpu");
    *up = p.up;
    *down = p.down;
    *half = p.half;
    return 0;
  })
}

int mec_resample_taps(int rate_in, int rate_out, double* h, size_t n) {
  API_GUARD({
    rs::Plan p;
    MEC_REQUIRE(rs::plan(rate_in, rate_out, &p), "mec_resample_taps: the rates are outside mec_resample_on_gpu");
    MEC_REQUIRE(h || p.taps() == 0, "mec_resample_taps: h is null");
    MEC_REQUIRE(n == (size_t)p.taps(), "mec_resample_taps: n is not the plan's tap count, 2 * half + 1 (0 for the identity)");
    if (p.half) rs::taps(p, h);
    return 0;
  })
}

int mec_audio_load_prof_enable(int on) {
  std::lock_guard<std::mutex> lk(al::g_prof_mu);
  al::g_prof.tag = on ? TAG_AUDIO_LOAD : TAG_NONE;
  al::g_prof.reset();
  return 0;
}

int mec_audio_load_prof_read(double* ms, int* count) {
  if (!ms || !count) { set_error("mec_audio_load_prof_read: bad args"); return -1; }
  std::lock_guard<std::mutex> lk(al::g_prof_mu);
  MEC_TRY(al::g_prof.read(ms, count));
  al::g_prof.reset();
  return 0;
}

}  // extern "C"
