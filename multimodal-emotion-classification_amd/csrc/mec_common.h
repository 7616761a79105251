// Shared definitions for the MI355X (gfx950) emotion-inference HIP library.
#pragma once
#include <hip/hip_runtime.h>
#include <array>
#include <cstddef>
#include <cstdint>
#include <map>
#include <mutex>
#include <new>
#include <stdexcept>
#include <string>
#include <vector>

typedef _Float16 f16;
typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef float floatx4 __attribute__((ext_vector_type(4)));

namespace mec {

void set_error(const std::string& msg);

#define MEC_HIP(x)                                                                        \
  do {                                                                                    \
    hipError_t e_ = (x);                                                                  \
    if (e_ != hipSuccess) {                                                               \
      ::mec::set_error(std::string(#x) + " failed: " + hipGetErrorString(e_) + " @" +     \
                       __FILE__ + ":" + std::to_string(__LINE__));                        \
      return -1;                                                                          \
    }                                                                                     \
  } while (0)

#define MEC_REQUIRE(cond, msg)                                                            \
  do {                                                                                    \
    if (!(cond)) {                                                                        \
      ::mec::set_error(std::string("requirement failed: ") + (msg));                     \
      return -1;                                                                          \
    }                                                                                     \
  } while (0)

#define MEC_TRY(x)                                                                        \
  do {                                                                                    \
    if ((x) != 0) return -1;                                                              \
  } while (0)

#define MEC_LAUNCH_CHECK() MEC_HIP(hipGetLastError())

// The body of an extern "C" entry point: no exception crosses the C ABI, it becomes -1 and the error text.
#define API_GUARD(body)                                  \
  try {                                                  \
    body                                                 \
  } catch (const std::bad_alloc&) {                      \
    ::mec::set_error("host allocation failed");          \
    return -1;                                           \
  } catch (const std::exception& e) {                    \
    ::mec::set_error(e.what());                          \
    return -1;                                           \
  }

// Kernel tags for the hipEvent timing hook (mec_prof_enable); see DESIGN.md §Measurement.
enum KernelTag : int {
  TAG_NONE = 0,
  TAG_BERT_QKV = 1,
  TAG_BERT_ATTN = 2,
  TAG_BERT_OPROJ = 3,
  TAG_BERT_FFN1 = 4,
  TAG_BERT_FFN2 = 5,
  TAG_BERT_LN = 6,
  TAG_RESNET_CONV3X3 = 7,
  TAG_RESNET_CONV1X1 = 8,
  TAG_RESNET_STEM = 9,
  TAG_SPEECH = 10,
  TAG_FUSION = 11,
  TAG_MBV2_BLOCK = 12,
  TAG_MBV2_LAST = 13,
  TAG_AUDIO = 14,
  TAG_COUNT = 15,  // bound of the per-tag option arrays (gemm_bn_tag ...); the tags below are timing-only
  TAG_LSTM_PROJ = 16,
  TAG_LSTM_REC1 = 17,
  TAG_LSTM_REC2 = 18,
  TAG_LSTM_HEAD = 19,
  TAG_RESIZE_H = 20,  // resize.hip: the ragged resize's two passes (mec_resize_prof_*)
  TAG_RESIZE_V = 21,
  TAG_CANON_GRAY = 22,  // image_canon.hip: the gray test and the conversion (mec_image_canon_prof_*)
  TAG_CANON_PIX = 23,
  TAG_AUDIO_LOAD = 24,  // audio_load.hip: decode + resample (mec_audio_load_prof_*)
  TAG_JPEG_ENTROPY = 25,  // jpeg.hip: the three kernels of the JPEG decode (mec_jpeg_prof_*)
  TAG_JPEG_IDCT = 26,
  TAG_JPEG_COLOUR = 27,
};

// Tuning knobs (mec_set_option / mec_model_set_option, include/mec.h). Every model handle
// owns a copy, taken from the process defaults when it is created, and kernels read the
// options of the handle whose call they serve (opt()), so handles never perturb each other.
// Every setting of a knob gives the same results bit for bit, with these exceptions:
//   * conv3x3_halo 0 vs 1, fusion_r 4 vs 1|2 and gemm_x3_order 0 vs 1 sum in other fp32 orders,
//     gelu_x3 0 vs 1 evaluates erf another way (same values to rounding, not the same bits;
//     include/mec.h);
//   * the probe-build values (compiled only with -DMEC_PROBES: they skip work to time a
//     kernel's parts and return wrong results).
struct Options {
  int gemm_bn = 0;          // forced f16 GEMM tile id (0 = autotune)
  int gemm_autotune = 1;
  int gemm_prefetch_r = 1;  // f16 (and split hi / lo) residual prefetch in short-K GEMMs
  int gemm_f32_tile = 0;    // forced fp32 GEMM tile id (0 = autotune)
  // fp32 autotune family: 0 both, 16 = 16x16x4 tiles only, 32 = 32x32x2 only. 16 (default): one k
  // order for every shape, so the fp32 path is batch-invariant bit for bit, at no measured cost
  // (ResNet50 20.73 vs 20.77 ms, BERT 45.95 vs 45.85 ms at B = 256; tools/ab_f32_family.py)
  int gemm_f32_family = 16;
  // fp32 engine, per launch class: BERT FFN1 pinned to 256x256 on 16x16x4 (it and the 32x32x2
  // form time within 0.3%, so the autotune flipped between them run to run)
  int gemm_f32_tag[TAG_COUNT] = {0, 0, 0, 0, /*TAG_BERT_FFN1*/ 8};
  // per launch class (profiling tag): forced tile, 0 = autotune. The BERT O-projection is
  // pinned to 128 x 128 (its candidates time within 2% alone; in the encoder 128 x 128 wins)
  int gemm_bn_tag[TAG_COUNT] = {0, 0, 0, /*TAG_BERT_OPROJ*/ 11128};
  int conv3x3_direct = 1;   // ResNet layer1 conv2 on the halo-tile kernel (conv3x3.hip)
  int conv3x3_halo = 1;     // layers 2-3 stride-1 conv2 on the halo kernel (conv3x3_halo.hip)
  int stem_gray_f32 = 1;    // fp32 gray stem as one conv + pool kernel (else im2col + GEMM + pool)
  // Images per ResNet50 layer1-2 pass, f16 and fp32x3 (0 = whole batch; image_model.h resnet_blocks). Measured
  // at B = 256 (tools/encoder_profile.py --opt resnet_chunk=N): 0 -> 4.23-4.25 ms, 128 -> 4.38, 64 -> 4.44-4.49,
  // 32 -> 5.08: the smaller GEMMs lose more than the cache residency gains, so chunking is off.
  int resnet_chunk = 0;
  // layer1 seam kernels (pw_chain.hip): 0 off, 1 the 256 -> 64 seams (block 1 -> 2, 2 -> 3), 2 also the
  // 256 -> 128 seam into layer2 (block 3 -> layer2 block 1). Image encoder at B = 256 (tools/ab_option.py, one
  // process): 4.03 / 3.83 / 3.75 ms for 0 / 1 / 2.
  int pw_chain = 2;
  int pw_chain_form = 0;
  // fp32x3 layer1 seam kernels (pw_chain_x3.hip): 0 off, 1 the 256 -> 64 seams (block 1 -> 2 with
  // the downsample, 2 -> 3), 2 also the 256 -> 128 seam into layer2
  int pw_chain_x3 = 2;
  // fp32x3 layer-2 seam kernels (pw_seam_x3.hip): 0 off, 1 the 512 -> 128 seams (blocks 2 -> 3, 3 -> 4),
  // 2 also the 512 -> 256 seam into layer3's first conv1 (whole-batch runs only: resnet_chunk 0). Same bits
  // at every setting. Per seam at B = 256: 512 -> 128 356-364 us against 379 for the two split GEMMs,
  // 512 -> 256 477 against 451 (profiles/r06l_seam_*.txt): 1 by default
  int pw_seam_x3 = 1;
  int bert_qkv_attn = 1;    // fused BERT QKV projection + attention
  // fp32x3 fused QKV + attention: heads per workgroup (2: 8 waves, 128 KB of LDS, one per CU; 1: 4 waves,
  // 80 KB, two per CU so one's attention overlaps the other's GEMM); same bits
  int bert_qkv_attn_x3_heads = 1;
  int bert_qkv_attn_heads = 1;  // the same for the f16 fused kernel (bert_qkv_attn_kernel)
  int bert_ln_rows = 2;     // BERT LayerNorm rows per wave (1 | 2 | 4): 27.0 / 25.7 / 26.3 us at B = 256
  // BERT's last layer on the [CLS] rows only (the outputs -- pooler, logits, CLS feature -- read
  // nothing else of it): K / V for every token, Q, attention, O-projection, LayerNorms and FFN for
  // the B [CLS] rows. Same bits as the full layer (every kernel is row-independent; the attention
  // computes the [CLS] query with the full kernel's instruction sequence). 0 = the full layer
  int bert_cls_last = 1;
  int mbv2_impl = 0;
  // fp32x3 MobileNetV2, stride-2 blocks at 56 / 28 outputs: 4 = 4x4 output tiles (9x9 inputs, four
  // workgroups per CU), 0 = 8x8 / 7x7 (17x17 / 15x15 inputs, one per CU); same bits. 4: 2.99 -> 2.92 ms
  // at B = 256 (profiles/r04_ab_mbv2x3_tile.txt)
  int mbv2_x3_tile = 4;
  int mbv2_x3_tpw = 2;  // fp32x3 MobileNetV2 fused blocks: output tiles per workgroup (next tile's input prefetched)
  // fp32x3 MobileNetV2 4x4-tile (stride-2) fused blocks: workgroups per CU their registers are allocated for
  // (4: 128 VGPRs and an 84-B spill per lane; 3: 168 VGPRs, no spill); same bits
  int mbv2_x3_occ = 3;
  // fp32x3 activation-plane scales (models.h activation_exp), read when a handle is created: 1 = per-tensor
  // exponents from bounds / BN estimates, 0 = every exponent 0 (round 4's unscaled planes; A/B only: small
  // activations then lose bits to the f16 subnormals, large ones overflow)
  int x3_plane_scale = 1;
  // fp32x3 extra headroom, read when a handle is created: every activation-plane exponent is chosen for a
  // target 2^-x3_headroom times the default (models.h activation_exp), so the planes take values that many
  // binades above the bound / BN estimate before the range flag trips. engine.HipModel re-creates a handle
  // with more headroom after a trip (the batch itself is re-run on the fp32 engine)
  int x3_headroom = 0;
  // fp32x3 text model, read when a handle is created: 1 = weight and activation planes paired (GemmParams::a_pair:
  // [rows][2K], each 32-element K chunk's hi halfs then its lo halfs, so every operand DMA takes whole 128-B
  // lines), 0 = planar (hi plane, then lo plane). Same bits. Paired needs the K-interleaved term order: a handle
  // created with gemm_x3_order 0 is planar
  int x3_layout = 1;
  // fp32x3 MobileNetV2 fused blocks: the expanded chunk's f32 rows with a per-tile-shape 16-B chunk swizzle
  // (1; fewer LDS bank conflicts on the depthwise reads) or unswizzled 36-float rows (0); same bits
  int mbv2_x3_sesw = 1;
  // fp32x3 MobileNetV2: features[k..17] as expand GEMM -> depthwise kernel -> project GEMM on hi / lo
  // planes (the "layered" form; k = 7..17, 0 = every block fused but features[17], which is always layered)
  int mbv2_layered = 8;
  int mbv2_layered16 = 8;  // the same on the f16 path (features[k..17] on f16 GEMMs; 0 = every block fused)
  // ping-pong GEMM tile order inside each XCD's contiguous tile range: 0 = row-major (all N
  // panels of one M panel in turn), G = groups of G M panels walked M-fastest, so the 32
  // tiles an XCD runs at once share G A panels and 32/G weight panels
  // (8: FFN1 reads 290 -> 227 MB per launch at B = 256, time unchanged; profiles/ffn1_traffic_gm*.json)
  int gemm_group_m = 8;
  // the same tile order for the multi-stage (glds) engine, every tile and A mode; 0 = row-major
  // (8: the fp32x3 FFN1 reads 911 -> 663 MB per launch at B = 256, time unchanged;
  // profiles/ffn1_x3_traffic*.json)
  int gemm_glds_group_m = 8;
  // split-f16 (fp32x3) GEMM term order: 0 = pass-major (all of K for lo.hi, then hi.lo, then
  // hi.hi), 1 = K-interleaved (each 32-deep k chunk's three terms back to back; tiles 7xxxx). Both
  // are fp32-accurate; they sum in different orders (not the same bits). 1: every operand byte is
  // fetched and staged once (not 1.5x) and 4 fragment reads feed 3 MFMAs (not 6): less energy per
  // MFMA, a higher held clock: text 18.84 -> 17.96 ms, ResNet50 10.06 -> 9.00, fused step 28.05 ->
  // 26.19 ms at B = 256 (profiles/r03_ab_x3order_*.txt)
  int gemm_x3_order = 1;
  // fp32x3 fused QKV + attention (one head per workgroup): every other 256-block of workgroups issues its stage
  // refill after its first (1) or second (2) MFMA term group instead of right after the barrier (0); same bits
  int qkv_x3_late_dma = 0;
  // K-interleaved split engine, tile 70256 on paired planes (GemmParams::a_pair): the ping-pong schedule
  // (gemm_pp_kernel SP = 3: four phases per 32-deep K tile, tile t + 2 in flight under a counted vmcnt)
  // instead of the two-stage ring (gemm_glds_kernel SP = 3). 0 = ring; 1 = ping-pong for the launches without
  // an activation (BERT's FFN2, O-projection and last-layer K|V: faster by the median at B = 256, though of
  // the three only the O-projection is `clear` by tools/bench_x3_pp.py's rule in both runs),
  // the ring for FFN1 (slower by the median); 2 = ping-pong for every launch (tests, A/B). The activation
  // stands in for the launch class: a new paired launch class should be measured before it relies on it. Any batch size; same bits. Planar
  // operands and every other tile stay on the ring
  int gemm_x3_pp = 1;
  // K-interleaved split engine, per launch class: forced tile (7xxxx), 0 = autotune. BERT FFN1 is
  // pinned to 70256 by default: it and the other tiles time within a few % of each other alone, so an
  // autotune would flip between them run to run, and the bench's roofline kernel (and its PMC traffic
  // file) must be one kernel. BERT FFN2 is pinned to the one-stage 72128 (two workgroups per CU: BERT
  // alone 17.44 -> 17.12 ms, profiles/r05l_ab_tile72128_text_fp32x3.txt), a tile the autotuner does not
  // offer: where the autotuner took it for a ResNet50 1x1 conv, and the one-stage 128-row tiles for most of
  // them, the image leg ran faster alone but the fused step slower (profiles/r05s_ab_tile73xxx_*.txt). The
  // fused step (FusedPipeline) pins FFN2 back to 70256 (profiles/r05m_ab_x3tag_ffn2.txt). A pin applies only
  // where its grid fills at least half the chip (kX3PinMinTiles tiles: FFN1 from B = 22; the one-stage 72128 from 512
  // tiles, two workgroups on every CU: FFN2 from B = 171, gemm.hip): a small batch
  // (latency-mode text inference) autotunes among the 7xxxx tiles instead, which give the same bits
  int gemm_x3_tag[TAG_COUNT] = {0, 0, 0, 0, /*TAG_BERT_FFN1*/ 70256, /*TAG_BERT_FFN2*/ 72128};
  // fp32x3 BERT FFN1 GELU: 1 = ACT_GELU_F32 (branch-free erf, one-instruction exp; max |error| /
  // max(|x|, 1) 1.21e-7 against float64, the correctly rounded erf's 1.06e-7), 0 = libm erff
  int gelu_x3 = 1;
  int fusion_r = 4;         // samples per fusion workgroup
  // BiLSTM recurrent kernel (text_lstm.hip): rows of one direction per workgroup (1 | 2 | 4), which share
  // the workgroup's register-resident recurrent weights; same bits at every value
  int lstm_rows = 2;
  int fusion_split = 1;     // fusion as 3 launches
  int gemm_debug = 0, conv3x3_debug = 0, stem_debug = 0, audio_debug = 0, speech_debug = 0;  // probe builds only
  int speech_spin_limit = -1;  // probe builds only: speech_flow_kernel wait limit (forces expired waits)
};

constexpr long kX3PinMinTiles = 128;  // gemm_x3_tag pins apply from this many tiles (half of 256 CUs)

// Engine slot of a tune-cache key: which engine tuned the shape, and on which operands. The fp32 engine
// adds the MFMA family its tiles were held to (ENGINE_F32 + gemm_f32_family: 1, 17, 33).
enum TuneEngine {
  ENGINE_F16 = 0,         // gemm_glds.hip, f16 operands
  ENGINE_F32 = 1,         // gemm_f32.hip (+ family)
  ENGINE_X3_PASS = 2,     // gemm_glds.hip, split operands, pass-major terms (gemm_x3_order 0)
  ENGINE_X3I = 3,         // gemm_glds.hip, split operands, K-interleaved terms
  ENGINE_X3I_PAIRED = 4,  // the same on paired hi / lo planes
};

// GEMM autotuner results: tile id per (engine, shape), per handle.
struct TuneCache {
  std::map<std::array<int, 11>, int> m;
  std::mutex mu;
  int find(const std::array<int, 11>& k) {
    std::lock_guard<std::mutex> lk(mu);
    auto it = m.find(k);
    return it == m.end() ? 0 : it->second;
  }
  void put(const std::array<int, 11>& k, int v) {
    std::lock_guard<std::mutex> lk(mu);
    m[k] = v;
  }
  int find_shape(int engine, int amode, int M, int N, int K) {  // any geometry
    std::lock_guard<std::mutex> lk(mu);
    for (const auto& kv : m)
      if (kv.first[0] == engine && kv.first[1] == amode && kv.first[2] == M && kv.first[3] == N && kv.first[4] == K)
        return kv.second;
    return 0;
  }
};

Options& default_options();      // process defaults (mec_set_option), copied into new handles
TuneCache& default_tune_cache(); // for the handle-less kernel entry points
const Options& opt();            // options of the handle the calling thread is serving
TuneCache& tune_cache();         // its autotune cache
// its fp32x3 range flag (device view of a host-mapped word; null on other precisions): raised by
// every kernel that writes an activation as f16 hi / lo planes when a value leaves the f16 range,
// reported by mec_model_check
unsigned* range_flag();
struct OptScope {                // set for the duration of one C-ABI call on a handle
  const Options* po;
  TuneCache* pt;
  unsigned* pf;
  OptScope(const Options* o, TuneCache* t, unsigned* flag = nullptr);
  ~OptScope();
};

// fp32x3 range guard. An activation x is carried as hi = f16(x), lo = f16(x - hi): |x| >= 65520
// rounds hi to inf (hi + lo = NaN downstream), and a NaN / inf input is no fp32 value either. Any
// such value raises the handle's flag (a vector store of 1; only on that rare path), so the
// forward fails loudly at mec_model_check instead of returning NaN probabilities.
__device__ __forceinline__ bool x3_out_of_range(float v) { return !(__builtin_fabsf(v) < 65520.f); }
__device__ __forceinline__ bool x3_out_of_range4(float4 v) {
  return x3_out_of_range(v.x) || x3_out_of_range(v.y) || x3_out_of_range(v.z) || x3_out_of_range(v.w);
}
__device__ __forceinline__ void x3_raise(unsigned* flag, bool bad) {
  if (bad && flag) __hip_atomic_store(flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
int set_option(Options& o, const std::string& key, int value);  // 0 = ok, -1 = unknown key / bad value
constexpr bool kProbes =
#ifdef MEC_PROBES
    true;
#else
    false;
#endif

// hipEvent pairs recorded around every launch whose tag matches `tag`.
struct Prof {
  int tag = TAG_NONE;
  std::vector<hipEvent_t> ev;
  size_t used = 0;
  int begin(int t, hipStream_t s);
  int end(int t, hipStream_t s);
  int read(double* total_ms, int* count);
  void reset() { used = 0; }
  ~Prof();
};

// Device buffer owned by a model handle (grow-only).
struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  int ensure(size_t n);
  void release();
  template <class T> T* as() const { return reinterpret_cast<T*>(p); }
  ~DevBuf() { release(); }
};

int upload(DevBuf& b, const void* host, size_t bytes);

// Workspace layout, stated once: a forward passes carve() a function that takes its buffers in order.
// carve() runs it with a null base to measure, grows ws to that size, then runs it on ws (the pointers it
// assigned are then real). Every buffer starts on a 256-byte boundary.
struct Carver {
  char* base;  // null: measuring
  size_t off = 0;
  template <class T> T* take(size_t count) {
    off = (off + 255) & ~size_t(255);
    T* r = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off += count * sizeof(T);
    return r;
  }
};
template <class F> int carve(DevBuf& ws, F&& layout) {
  Carver m{nullptr};
  layout(m);
  MEC_TRY(ws.ensure(m.off));
  Carver c{ws.as<char>()};
  layout(c);
  MEC_REQUIRE(c.off == m.off && c.off <= ws.bytes, "carve: the two passes of a workspace layout differ");
  return 0;
}

int cu_count();  // compute units of the current device (cached per device); -1 with the error set on failure

// Sequential reader over the canonical fp32 host blob (mec/synthetic.py: spec()).
struct BlobReader {
  const float* p;
  size_t n, off = 0;
  bool ok = true;
  BlobReader(const float* p_, size_t n_) : p(p_), n(n_) {}
  const float* take(size_t count) {
    if (off + count > n) { ok = false; return p; }
    const float* r = p + off;
    off += count;
    return r;
  }
};

// fp16 MFMA GEMM / implicit-GEMM convolution ------------------------------------------
// C[M,N] = epilogue( A'[M,K] . B[N,K]^T ), A' = A (plain) or the im2col view of an NHWC
// tensor (conv).
enum AMode : int { A_PLAIN = 0, A_CONV = 1, A_DUAL = 2 };
// ACT_GELU: a (4, 3) rational Phi (f16 path, gemm_common.h gelu_rat); ACT_GELU_EXACT: libm erff,
// x * 0.5 * (1 + erf(x / sqrt2)) as torch's CPU gelu kernel orders it (fp32 path); ACT_GELU_F32:
// the same expression with the library's erf polynomials evaluated branch-free and a one-instruction
// exp (gemm_common.h gelu_f32; fp32x3 path)
enum Act : int { ACT_NONE = 0, ACT_RELU = 1, ACT_GELU = 2, ACT_RELU6 = 3, ACT_GELU_EXACT = 4, ACT_GELU_F32 = 5 };

struct GemmParams {
  const void* A = nullptr;   // f16 [M,K] | f16 NHWC [n,H,W,C]
  const f16* B = nullptr;    // f16 [N,K], K contiguous
  const float* B32 = nullptr;   // f32 [N,K] (fp32 engine, gemm_f32.hip; A is then f32 too)
  const float* bias = nullptr;  // [N]
  const void* R = nullptr;      // residual [M,N] (f16 or f32) or null
  int r_f32 = 0;
  // deferred LayerNorm of an f32 residual: R' = fma((R - mean[row]) * rstd[row], r_g, r_b),
  // the exact expression bert_layernorm_kernel evaluates (so R' is that kernel's output)
  const float2* r_stats = nullptr;  // [M] (mean, rstd) or null
  const float* r_g = nullptr;       // [N]
  const float* r_b = nullptr;       // [N]
  f16* C16 = nullptr;           // [M,N] f16 out or null
  float* C32 = nullptr;         // [M,N] f32 out or null
  int M = 0, N = 0, K = 0;
  int act = ACT_NONE;
  int amode = A_PLAIN;
  const void* A2 = nullptr;  // A_DUAL second source (NHWC, geometry below), K1 = columns of A
  int K1 = 0;
  // conv geometry (NHWC input)
  int H = 1, W = 1, C = 0, OH = 1, OW = 1, ks = 1, stride = 1, pad = 0;
  int group_m = 0;  // ping-pong tile order inside an XCD's range: 0 row-major, G = G-row groups
  // Split-f16 operands (the MEC_PREC_FP32X3 path, f16 engine only): A and B are each an f16
  // hi plane and an f16 lo plane (x = hi + lo exactly, |lo| <= 2^-11 |hi|), the lo planes at
  // element offsets a_lo / b_lo from A / B (A_DUAL: from A and from A2 alike). The K loop makes three passes over K, A_lo.B_hi,
  // A_hi.B_lo, A_hi.B_hi, into one fp32 accumulator (the dropped A_lo.B_lo term is below
  // 2^-22 |A B|). oscale (a power of two: undoes the weights' pre-scale, exact) multiplies the
  // accumulator before the bias; it is 1 (an exact no-op) everywhere else.
  int split = 0;
  long long a_lo = 0, b_lo = 0;
  float oscale = 1.f;
  long long c_lo = 0;  // != 0: C16 is written as a hi plane and a lo plane (C16 + c_lo): f16(v), f16(v - hi)
  // split output's activation-plane scale (a power of two, exact): the planes carry v * cscale, v the
  // value after the activation (C32, when also written, carries v). Chosen per tensor at handle
  // creation so the planes' magnitudes sit where the lo plane is a normal f16 (activation_exp below)
  float cscale = 1.f;
  unsigned* ovf = nullptr;  // split output's range flag (x3_raise); launch_gemm fills in range_flag()
  long long r_lo = 0;  // != 0: the f16 residual R is a hi plane + a lo plane at R + r_lo (R = hi + lo)
  // Paired split planes (K-interleaved engine, plain A): a split tensor X[rows][K], K % 32 == 0, stored as
  // one f16 array [rows][2K] holding, per 32-element K chunk, the chunk's hi halfs then its lo halfs
  // (x3_pair_index below), so one row's operands of one 32-deep K step are one aligned 128-B line. Same
  // values and scales as the planar form, only the addresses move; a_lo / b_lo / c_lo are then unused.
  // a_pair and b_pair go together (one stage layout); c_pair lays the c_lo-style output out the same way.
  int a_pair = 0, b_pair = 0, c_pair = 0;
};

// Paired split planes: index of element (r, k) of plane p (0 hi, 1 lo) of a [rows][K] tensor.
__host__ __device__ inline size_t x3_pair_index(size_t r, int k, int K, int p) {
  return r * 2 * (size_t)K + (size_t)(k >> 5) * 64 + p * 32 + (k & 31);
}
// The text kernels locate a split tensor's lo plane by an element offset `lo` > 0 from its hi plane; kX3Paired
// in that place says the tensor is paired. x3_at: index of element (r, k) of plane p either way.
constexpr long long kX3Paired = -1;
__host__ __device__ inline size_t x3_at(long long lo, size_t r, int k, int K, int p) {
  return lo < 0 ? x3_pair_index(r, k, K, p) : (size_t)(p ? lo : 0) + r * (size_t)K + k;
}

// conv / dual geometry (gemm.hip): what both engines require of ks, stride, pad and the extents before a
// launch; and the C-ABI entries' form, which validates n and the rest before dividing by stride and sets
// OH, OW and M = n OH OW
int check_conv_geometry(const GemmParams& p);
int set_conv_geometry(GemmParams& g, int n);
int launch_gemm(const GemmParams& p, hipStream_t s, Prof* prof, int tag);
int launch_gemm_glds(const GemmParams& p, hipStream_t s, int force_bn);
// 3x3/1 conv 64 -> 64 on 56x56 (+ BN shift + ReLU) as a halo-tile kernel (conv3x3.hip);
// launch_gemm routes matching A_CONV shapes to it while opt().conv3x3_direct is set
int launch_conv3x3_c64(const f16* x, const f16* w, const float* bias, f16* y, int B, int H, int C, int Cout,
                       hipStream_t s);
// 3x3/1 convs C -> C on 28x28x128 and 14x14x256 (+ BN shift + ReLU): halo kernel
// (conv3x3_halo.hip), routed from launch_gemm while opt().conv3x3_halo is set. Same fp32
// accumulation as the GEMM path in another summation order (not bit-identical to it).
bool conv3x3_halo_supported(int H, int C, int N);
int launch_conv3x3_halo(const f16* x, const f16* w, const float* bias, f16* y, int B, int H, int C, hipStream_t s);
int gemm_tuned_bn(int amode, int M, int N, int K);
// fp32 engine (gemm_f32.hip): f32 A (plain or NHWC conv) and B32, v_mfma_f32_32x32x2_f32
int launch_gemm_f32(const GemmParams& p, hipStream_t s, Prof* prof, int tag);
int gemm_f32_tuned(int amode, int M, int N, int K);

}  // namespace mec
