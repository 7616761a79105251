// Model handles behind the C-ABI (include/mec.h). Each handle owns its packed device
// weights and a grow-only activation workspace; forwards are asynchronous on the caller's
// stream. One handle is used by one host thread at a time (the Python wrapper locks).
#pragma once
#include "../../include/mec.h"
#include <list>

#include "mec_common.h"
#include "ragged_stage.h"
#include "resample_design.h"

namespace mec {

enum ModelKind : int { KIND_SPEECH = 0, KIND_TEXT = 1, KIND_IMAGE = 2, KIND_FUSION = 3, KIND_IMAGE_MBV2 = 4, KIND_AUDIO = 5, KIND_TEXT_LSTM = 6 };

size_t blob_floats(int kind);

// Arithmetic of a handle (mec_create_ex): PREC_F16 = f16 MFMA operands with fp32
// accumulation / LayerNorm / softmax / residual stream (the fast path); PREC_FP32 = every
// operand and product in fp32 (v_mfma_f32_32x32x2_f32), the reference's own precision.
// PREC_FP32X3 = fp32 arithmetic on the f16 MFMA: every fp32 GEMM operand x is carried as an
// exact pair of f16 planes x = hi + lo, and each product as hi.hi + hi.lo + lo.hi in one fp32
// accumulator (gemm_glds.hip split mode; 22 significant bits per operand against fp32's 24,
// the dropped lo.lo term below 2^-22 of the product); LayerNorm, softmax, attention, GELU, the
// residual stream and the heads are fp32 exactly as on the fp32 path.
enum Precision : int { PREC_F16 = 0, PREC_FP32 = 1, PREC_FP32X3 = 2 };

struct Model {
  int kind = -1;
  int device = 0;
  int prec = PREC_F16;
  Options opts = default_options();  // this handle's knobs (mec_model_set_option)
  TuneCache tune;                    // this handle's GEMM autotune results
  Prof prof;
  // fp32x3 handles: host-mapped pinned word (range_host) and its device view (range_dev), raised by
  // the kernels that write activation planes when a value leaves the f16 range (x3_raise)
  unsigned* range_host = nullptr;
  unsigned* range_dev = nullptr;
  int alloc_range_flag();
  // fp32x3 handles: one line per activation tensor (group) written at creation, "name s=<exponent>
  // bound=<bound or BN estimate>" plus the headroom the exponents were chosen with (mec_model_x3_report)
  std::string x3_report;
  void x3_note(const std::string& name, int s, double bound);
  // the exponent this handle gives an activation tensor: activation_exp (below) against 2^-x3_headroom of
  // the target (a handle re-created after a range trip), or 0 with x3_plane_scale off (unscaled planes, A/B only)
  int x3_exp(double bound, double target) const;
  // Calibrated creation (mec_create_x3_calibrated; the image kinds): x3_cal holds one observed max |x| per
  // tensor in report order, and x3_tensor -- the exponent of the next tensor of that order, noted under `name`
  // -- takes a finite x3_cal[i] > 0 in place of the BN estimate `est` (0, a dead tensor: the estimate stays)
  std::vector<double> x3_cal;
  size_t x3_noted = 0;
  int x3_tensor(const std::string& name, double est, double target);
  virtual ~Model();
  // errors a kernel could only report after the fact (mec_model_check): 0 = none since the last
  // check. Call after the stream that ran the handle's forwards has been synchronized.
  virtual int check();
};

// ---------------------------------------------------------------- speech DNN
struct SpeechModel : Model {
  DevBuf w;  // fp32: mean, scale, {W,b,inv,shift} x5, W6, b6
  size_t off_mean = 0, off_scale = 0, off_W[6] = {}, off_b[6] = {}, off_inv[5] = {}, off_shift[5] = {};
  // speech_flow_kernel: hand-off buffers of layers 0-3 (f32 [16 * chunks, N_l]) and the
  // per-chunk arrival counters + the launch's error word (zeroed on the stream before every
  // launch); host_err: host-mapped pinned flag a launch with an expired wait raises
  DevBuf flow_act, flow_sync;
  int flow_chunks = 0;
  unsigned* host_err = nullptr;
  ~SpeechModel() override;
  int create(const float* blob, size_t n);
  int forward(const float* x, int B, float* feat, float* logits, float* probs, hipStream_t s);
  int check() override;
};

// ---------------------------------------------------------------- speech features (audio.hip)
// blob = [sample_rate, n_fft, hop, n_mels, n_mfcc] (config.py:57-59 + librosa defaults); the
// handle owns the filterbank / window / twiddle tables and a grow-only workspace.
// One cached tap table of the audio front end (audio_load.hip): rate_in -> the handle's rate, phase-major on
// the device; `last` is recorded after every call that read it.
struct ResampleTable {
  int rate_in = 0;
  rs::Plan plan;
  double* dev = nullptr;
  hipEvent_t last = nullptr;
  uint64_t stamp = 0;
};

struct AudioModel : Model {
  int sr = 22050, n_mfcc = 40, lo_bin = 0, hi_bin = 0, mel_nnz = 0, mel_ch = 0;
  DevBuf tables, ws;
  size_t off_hann = 0, off_tw = 0, off_post = 0, off_freq = 0, off_dct = 0, off_chroma = 0, off_meloff = 0,
         off_melbin = 0, off_melw = 0, off_melseg = 0;
  int create(const float* blob, size_t n);
  // wave f32 [B, L] -> feat f32 [B, n_mfcc + 16]; tuning f32 [B] (estimate_tuning) or null
  int forward(const float* wave, int B, int L, float* feat, float* tuning, hipStream_t s);
  // mec_audio_load_ragged (audio_load.hip): the descriptors' staging and the tap tables, under load_mu
  static constexpr int kMaxTables = 16;
  std::mutex load_mu;
  StageBuf load_stage;
  std::list<ResampleTable> load_tabs;
  uint64_t load_stamp = 0;
  ~AudioModel() override;
  int load_table(int rate_in, const std::vector<int>& keep, ResampleTable** out);
  int load_ragged(const uint8_t* src, const int64_t* offs, const int32_t* desc, int B, size_t src_bytes, float* wave,
                  int n_out, hipStream_t s);
};

// ---------------------------------------------------------------- fusion model
struct FusionRows;  // speech_fusion.hip: which rows a fusion workgroup reads and writes
struct FusionModel : Model {
  DevBuf w;  // fp32, transposed Linear weights ([in][out]) + biases + LN params
  std::vector<size_t> off;  // offsets by FusionParam index
  DevBuf ws;  // split form: projected (P) and fusion-projected (T) features, f32 [B, 768] each
  int create(const float* blob, size_t n);
  int forward(const float* sf, const float* tf, const float* imf, const float* sp, const float* tp,
              const float* ip, int B, float* logits, float* probs, float* attn_w, float* dec_w,
              hipStream_t s);
  // the attention model's launches over B group rows (dense, or the rows x lists)
  int launch(const float* sf, const float* tf, const float* imf, const float* sp, const float* tp, const float* ip,
             int B, const FusionRows& x, float* logits, float* probs, float* attn_w, float* dec_w, hipStream_t s);
};
// mec_fusion_fwd_mixed: the argument checks (no handle, no device), then the call (p null: no model)
int fusion_mixed_check(const mec_fusion_mixed_args* a, bool have_model);
int fusion_fwd_mixed(FusionModel* p, const mec_fusion_mixed_args& a, hipStream_t s);

int fuse_weighted(const float* s, const float* t, const float* i, int B, double* out, hipStream_t st);
int fuse_weighted_f64(const double* s, const double* t, const double* i, int B, double* out, hipStream_t st);

// ---------------------------------------------------------------- BERT-base
// A packed batch (mec_text_fwd_packed): sample i of ns occupies slots off[i] .. off[i] + len[i] - 1 of the
// 128-slot row row[i] (device arrays, a plan of mec_text_pack_plan).
struct TextPack {
  const int32_t *row, *off, *len;
  int ns;
};
struct TextModel : Model {
  DevBuf emb;      // fp32 word | pos | type | ln_g | ln_b
  DevBuf wts;      // f16 per layer: Wqkv Wo Wi Wo2 (bert_model.h LayerWeights)
  DevBuf prm;      // fp32 per layer: bqkv bo ln1g ln1b bi bo2 ln2g ln2b ; head: WpT bp WcT bc (bert_model.h)
  DevBuf wts32;    // fp32 path: the same GEMM weights in f32
  DevBuf ws;       // workspace
  int create(const float* blob, size_t n);
  // The three forwards (f16: bert.hip; fp32, fp32x3: bert_f32.hip) share one shape (bert_model.h): the
  // prologue (workspace, and for a packed batch the pack kernel), the embedding LayerNorm, then per layer
  // the attention and the layer tail (O-projection, LN1, FFN1, FFN2, LN2). With bert_cls_last the last
  // layer computes K | V for every token and runs its attention and that same tail on the samples' [CLS]
  // rows only. Then the output tail (pooler, logits, probs).
  // pk (or null): the packed form -- B packed rows holding pk->ns samples, mask unused; outputs [ns, .]
  int forward(const int32_t* ids, const int32_t* mask, int B, int L, float* cls, float* logits,
              float* probs, hipStream_t s, const TextPack* pk = nullptr);
  // ids int32 [B, 128] (padded layout), plan row / off / len [B] over Bp rows -> outputs in sample order
  int forward_packed(const int32_t* ids, const int32_t* row, const int32_t* off, const int32_t* len, int B, int Bp,
                     float* cls, float* logits, float* probs, hipStream_t s);
  int forward_f32(const int32_t* ids, const int32_t* mask, int B, int L, float* cls, float* logits,
                  float* probs, hipStream_t s, const TextPack* pk = nullptr);  // bert_f32.hip
  // fp32x3 path: wts holds the hi planes, then the lo planes (at x3_lo halfs). Per layer: the
  // activation-plane exponents (activation_exp, rigorous bounds) of LN1's and LN2's outputs, Q, K, V (= the
  // context's) and the FFN intermediate, and per GEMM B matrix (Wqkv, Wo, Wi, Wo2) the epilogue scale
  // 2^-e 2^(s_out - s_in): its planes' pre-scale with the activation exponents folded in. x3_s_emb: the
  // embedding LN's exponent. x3b: bq 2^s_q | bk 2^s_k | bv 2^s_v per layer (the Wqkv planes carry the same
  // factors)
  struct X3Layer {
    int s_ln1 = 0, s_ln2 = 0, s_q = 0, s_k = 0, s_v = 0, s_ffn = 0;
    float scale[4] = {1.f, 1.f, 1.f, 1.f};
  };
  size_t x3_lo = 0;
  // x3_layout 1 (with the K-interleaved term order): wts holds every matrix [N][K] paired, [N][2K] at twice its
  // planar offset (mec_common.h x3_pair_index), and every activation tensor of the forward is paired too
  bool x3_paired = false;
  int x3_s_emb = 0;
  std::vector<X3Layer> x3_layers;
  DevBuf x3b;
  int forward_x3(const int32_t* ids, const int32_t* mask, int B, int L, float* cls, float* logits,
                 float* probs, hipStream_t s, const TextPack* pk = nullptr);  // bert_f32.hip
};
// The pack kernel (bert.hip): the slots' ids / position ids / segment ids over Bp rows and the samples'
// [CLS] slots, from the padded ids [ns, 128] and the plan
int launch_bert_pack(const int32_t* ids, const TextPack& pk, int Bp, int32_t* pids, int32_t* ppos, uint8_t* seg,
                     int32_t* cidx, hipStream_t s);
// lo != 0 (fp32x3 path): h16 is written as a hi plane and h16 + lo as the lo plane f16(y - hi)
// (planes of y up: up = 2^s, the planes' activation scale, activation_exp)
// posid (or null): per-row position ids in place of row % L (the packed path)
int launch_bert_embed_ln(const int32_t* ids, int M, int L, const float* emb, float* h32, f16* h16, hipStream_t s,
                         long long lo = 0, float up = 1.f, const int32_t* posid = nullptr);
int launch_bert_layernorm(const float* x, int M, const float* g, const float* b, float* h32, f16* h16, float2* stats,
                          hipStream_t s, long long lo = 0, float up = 1.f);
// f16 attention (bert.hip): Q|K|V [B*128, 2304] -> ctx [B*128, 768]; its [CLS]-only form (K | V [rows*128,
// 1536], the [CLS] queries qc and contexts ctx [NS, 768]; cidx or null as below); and the fused QKV
// projection + attention (h16 [B*128, 768], wqkv [2304, 768]). fp32 attention (bert_f32.hip): the same two
// unfused forms on f32 tensors. packed: mask holds the rows' uint8 segment ids and B counts packed rows
int launch_bert_attention(const f16* qkv, const int32_t* mask, f16* ctx, int B, hipStream_t s, bool packed);
int launch_bert_attention_cls(const f16* kv, const int32_t* mask, const f16* qc, f16* ctx, int NS, hipStream_t s,
                              const int32_t* cidx);
int launch_bert_qkv_attn(const f16* h16, const f16* wqkv, const float* bqkv, const int32_t* mask, f16* ctx, int B,
                         hipStream_t s, bool packed);
int launch_bert_attention_f32(const float* qkv, const int32_t* mask, float* ctx, int B, hipStream_t s, bool packed);
int launch_bert_attention_f32_cls(const float* kv, const int32_t* mask, const float* qc, float* ctx, int NS,
                                  hipStream_t s, const int32_t* cidx);
// fp32x3 attention (bert.hip): Q|K|V as f16 hi / lo planes [B*128, 2304] (lo at qkv + lo) of q 2^s_q,
// k 2^s_k, v 2^s_v; ctx 2^s_v written as hi / lo planes [B*128, 768] (lo at ctx + clo); qks = 1/8
// 2^-(s_q + s_k) (the scores' scale)
// packed: mask holds the rows' uint8 segment ids (block_ops.h stage_mask) and B counts packed rows
int launch_bert_attention_x3(const f16* qkv, long long lo, const int32_t* mask, f16* ctx, long long clo, int B,
                             float qks, hipStream_t s, bool packed = false);
// its [CLS]-only form (bert_cls_last): K | V planes [B*128, 1536] (lo at kv + lo), the [CLS] query
// planes [B, 768] (lo at qc + qclo), the [CLS] context planes [B, 768] (lo at ctx + clo)
// cidx (or null): the packed form -- B samples, sample b's [CLS] slot cidx[b], mask = segment ids
int launch_bert_attention_x3_cls(const f16* kv, long long lo, const int32_t* mask, const f16* qc, long long qclo,
                                 f16* ctx, long long clo, int B, float qks, hipStream_t s,
                                 const int32_t* cidx = nullptr);

// fp32x3 QKV projection + attention of one (sequence, head pair) per workgroup (bert.hip, L = 128):
// h planes [B*128, 768] (lo at hs + hlo), Wqkv planes (lo at wqkv + wlo, epilogue scale oscale) ->
// ctx planes [B*128, 768] (lo at ctx + clo); Q / K / V never reach HBM
int launch_bert_qkv_attn_x3(const f16* hs, long long hlo, const f16* wqkv, long long wlo, float oscale,
                            const float* bqkv, const int32_t* mask, f16* ctx, long long clo, int B, float qks,
                            hipStream_t s, bool packed = false);

// Split n fp32 weights into f16 planes for the fp32x3 path: hi = f16(w 2^e), lo = f16(w 2^e - hi)
// with e the largest power of two keeping max |w| 2^e <= 2^14 (so hi never overflows and lo
// stays out of the f16 subnormals for all but the smallest weights); returns 2^-e, the GEMM
// epilogue's oscale. Host code (runtime.hip).
float split_planes(const float* w, size_t n, f16* hi, f16* lo);

// fp32x3 activation planes. An activation x is carried as hi = f16(x 2^s), lo = f16(x 2^s - hi)
// with s fixed per tensor at handle creation; its consumer folds 2^-s into its epilogue scale (exact).
// The lo plane is a normal f16 -- 22 significant bits -- while |x 2^s| >= 2^-3, and hi stays finite
// while |x 2^s| < 65520. activation_exp(bound, target) = the largest s with bound 2^s <= target:
//   * a rigorous bound (BERT: LayerNorm outputs, |y| <= sqrt(H - 1) max|gamma| + max|beta|, and the
//     projections of such rows, max_j (bound ||W_j||_1 + |b_j|)) with target 2^15: never overflows;
//   * a BatchNorm estimate (ResNet50 / MobileNetV2: max_c |beta_c| + 6 |gamma_c| per BN output, summed
//     along residual paths) with target 2^10: 64x headroom to the f16 range over that estimate, and
//     the estimate's typical values near 2^7, far above the 2^-3 floor.
// Clamped to [-40, 40]; 0 for a zero or non-finite bound. Host code (runtime.hip).
int activation_exp(double bound, double target);
constexpr double kX3BoundTarget = 32768.0, kX3EstimateTarget = 1024.0;

// ---------------------------------------------------------------- BiLSTM text model (text_lstm.hip)
// fp32 at every precision setting. w: layer 1's projected table Emb.W + b [10000][1024] (forward | backward
// gates, built at creation), the recurrent kernels of both layers, layer 2's input projection as the fp32
// GEMM's B operand, the dense head (Keras kernels [in][out]).
struct LstmTextModel : Model {
  static constexpr int kVocab = 10000;  // train_lstm_text_model.py:171 caps vocab_size here; loaders zero-pad
  DevBuf w, ws;
  size_t off_table = 0, off_u1[2] = {}, off_w2 = 0, off_b2 = 0, off_u2[2] = {}, off_dw[3] = {}, off_db[3] = {};
  int create(const float* blob, size_t n);
  // ids int32 [B, L = 128] (post-padded with 0; pads run through the LSTMs like any token) -> feat f32 [B, 64]
  // (Dense-64 ReLU) or null, logits f32 [B, 7] or null, probs f32 [B, 7]
  int forward(const int32_t* ids, int B, int L, float* feat, float* logits, float* probs, hipStream_t s);
};
// One LSTM direction over precomputed gate pre-activations (mec_lstm_seq_f32)
int lstm_seq_f32(const float* xz, const float* U, int B, int L, int units, int reverse, float* y_seq, float* h_last,
                 hipStream_t s);

// ---------------------------------------------------------------- image encoders
// Both backbones take the same u8 inputs and produce the same (512-d feature, logits, probs).
// Their six forwards (f16: forward_u8 in resnet.hip / mobilenet.hip; fp32, fp32x3: forward_f32, forward_x3 in
// resnet_f32.hip / mobilenet_f32.hip / mobilenet_x3.hip) share one shape (image_model.h): the argument check, the
// workspace carve, the optional 48 -> 224 resize, the precision's own stem, the walk over the backbone's blocks
// under that precision's policy, the precision's average pool, then the output tail (fc1 + ReLU = the feature,
// logits, probs).
// The activation tensors the fp32x3 creation of an image kind gives a plane exponent, in mec_model_x3_report's
// order (image_model.h resnet_x3_tensors / mb_x3_tensors), and where block i's tensors stand in that list: its
// output (a stage's blocks share one entry, "layerN.out" / "featuresA-B.out") and, ResNet50, its conv1 / conv2
struct X3Tensors {
  std::vector<std::string> names;
  std::vector<int> out, c1, c2;
};

struct ImageNet : Model {
  // Observation (mec_model_x3_observe; fp32 handles): while obs_on, forward_f32 reduces every tensor of
  // x3_tensors() to max |x| (absmax.hip) on its stream, into that tensor's slot of obs (float bits, unsigned
  // [obs_n]); a slot keeps the running maximum across forwards until observation is armed again
  DevBuf obs;
  int obs_n = 0;
  bool obs_on = false;
  virtual X3Tensors x3_tensors() const = 0;
  std::string x3_names;  // its names, one per line (mec_model_x3_names; built on first use)
  // img u8 [B,H,W,C]: (48,48,1) gray FER2013 (GPU resize), (224,224,1) gray, (224,224,3) RGB
  virtual int forward_u8(const uint8_t* img, int B, int H, int W, int C, float* feat, float* logits, float* probs,
                         hipStream_t s) = 0;
  int forward(const uint8_t* gray, int B, float* feat, float* logits, float* probs, hipStream_t s) {
    return forward_u8(gray, B, 48, 48, 1, feat, logits, probs, s);
  }
};

// ---------------------------------------------------------------- ResNet50 + head
struct ConvLayer {
  size_t w_off = 0;   // [Cout][kh][kw][Cin] (BN scale folded; image_pack.h pack_conv)
  size_t b_off = 0;   // f32 [Cout] (BN shift)
  int cin = 0, cout = 0, ks = 1, stride = 1, pad = 0;
  // fp32x3 path: the epilogue scale 2^-e 2^(x3_s - s_in) (weight planes' pre-scale, activation-plane
  // scales of output and input), the BN output estimate, the output planes' exponent x3_s, and the BN
  // shift times 2^x3_s (at x3b_off in prm)
  float x3_scale = 1.f;
  double x3_est = 0.0;
  int x3_s = 0;
  size_t x3b_off = 0;
};
struct Bottleneck {
  ConvLayer c1, c2, c3, ds;  // fp32x3: c3.x3_s = the stage's residual-stream exponent (the block output)
  int x3_s_in = 0;           // fp32x3: the block input planes' exponent
  bool has_ds = false;
  size_t c3ds_w_off = 0, c3ds_b_off = 0;  // block 0: [conv3 | downsample] weights [4w][w+cin], summed bias
  float c3ds_x3_scale = 1.f;              // fp32x3 path: its planes' scale (in wts_dual) and lo offset
  size_t c3ds_x3_lo = 0;
};
// The walk (image_model.h resnet_blocks / resnet_walk): per bottleneck conv1 (unless the previous block's seam
// kernel ran it), conv2, then conv3 + downsample-or-identity + ReLU as GEMMs or, where the policy's block_end
// takes over, as a seam kernel that also runs the next conv1; layers 1-2 per resnet_chunk images (f16, fp32x3).
struct ImageModel : ImageNet {
  DevBuf wts;   // f16 conv weights
  DevBuf prm;   // fp32 biases, stem weights, head
  DevBuf ws;    // workspace
  ConvLayer stem;      // gray input (channels folded): f16 [64][64] pixel taps
  ConvLayer stem_rgb;  // RGB input: f16 [64][3*64]
  size_t stem_corr_off = 0;  // f32 [16 border classes][64] -mean/std term
  std::vector<Bottleneck> blocks;
  size_t fc1_off = 0, fc1b_off = 0, fc2_off = 0, fc2b_off = 0;
  // fp32 path (resnet_f32.hip): f32 weights, same [Cout][kh][kw][Cin] layout; the stem is a
  // [64][160] GEMM over an explicit im2col of the normalized image (k = c*49 + kh*7 + kw)
  DevBuf wts32;
  size_t stem_gray32_off = 0;  // f32 [49][2][64]: gray-input stem folded to (pixel, inside) taps
  int create(const float* blob, size_t n);
  int create_f32(const float* blob, size_t n);
  int forward_u8(const uint8_t* img, int B, int H, int W, int C, float* feat, float* logits, float* probs,
                 hipStream_t s) override;
  int forward_f32(const uint8_t* img, int B, int H, int W, int C, float* feat, float* logits, float* probs,
                  hipStream_t s);
  // fp32x3 path (resnet_f32.hip): wts holds every bottleneck conv's f16 hi planes, then the lo
  // planes at x3_lo halfs (w_off indexes both); the stem, pooling and head run as on the fp32 path
  size_t x3_lo = 0;
  float stem_x3_up = 1.f;  // 2^e: the gray stem's weight pre-scale (stem.x3_scale = 2^-e)
  int x3_s_out = 0;        // the last stage's activation-plane exponent (undone by the average pool)
  DevBuf wts_dual;  // fp32x3: block 0's [conv3 | downsample] hi / lo planes (c3ds_w_off, c3ds_x3_lo)
  int forward_x3(const uint8_t* img, int B, int H, int W, int C, float* feat, float* logits, float* probs,
                 hipStream_t s);
  X3Tensors x3_tensors() const override;
};

// ---------------------------------------------------------------- MobileNetV2 + head
// One inverted-residual block (features[1..17]) as image_pack.h packs it (pack_mbv2_body): channel counts
// padded with zero weights per precision (MbLayout: 32 / 32 / 16 for the fused kernels, 64 on the fp32 path).
struct MbBlock {
  int t = 1, cin = 0, hid = 0, cout = 0, stride = 1;
  int cinp = 0, hidp = 0, coutp = 0;
  size_t we_off = 0, wp_off = 0;          // f16: expand [hidp][cinp], project [coutp][hidp]
  size_t be_off = 0, wd_off = 0, bd_off = 0, bp_off = 0;  // f32: expand bias, dw (MbLayout), dw bias, project bias
  // fp32x3 layered form (hidp % 64 == 0): expand [hidp][lcinp], project [lcoutp][hidp] (lcoutp = cout padded
  // to 64, lcinp = the previous block's lcoutp), project bias [lcoutp]
  int lcinp = 0, lcoutp = 0;
  size_t lwe_off = 0, lwp_off = 0, lbp_off = 0;
  // fp32x3 activation planes (activation_exp, BN estimates): the block input's and output's exponents
  // (a stage's outputs share one, as a residual block's output and input must), the project BN
  // estimate, and the layered project bias times 2^x3_s_out (lbp_x3_off)
  int x3_s_in = 0, x3_s_out = 0;
  double x3_est = 0.0;
  size_t lbp_x3_off = 0;
};
// The walk (image_model.h mb_walk / mb_block): f16 and fp32x3 run blocks [0, l0) as one fused kernel each and
// blocks [l0, ..) layered (expand GEMM -> depthwise -> project GEMM); fp32 runs every block layered.
struct MobileNetModel : ImageNet {
  DevBuf wts;   // f16 1x1 weights
  DevBuf prm;   // fp32 stem, depthwise weights, biases, head
  DevBuf ws;    // workspace
  // f32 [9][32], [3*9][32], [4 border classes][32] (image_pack.h pack_mbv2_stem_folded); fp32 path: stem_w_off
  // in wts32, [64][32] im2col weights, and stem_corr_off the stem bias [64]
  size_t stem_w_off = 0, stem_rgb_off = 0, stem_corr_off = 0;
  std::vector<MbBlock> blocks;
  size_t last_w_off = 0, last_b_off = 0;  // features[18]: f16 [1280][320], f32 [1280]
  size_t fc1_off = 0, fc1b_off = 0, fc2_off = 0, fc2b_off = 0;
  DevBuf wts32;  // fp32 path (mobilenet_f32.hip): f32 weights, channels padded to 64
  int create(const float* blob, size_t n);
  int create_f32(const float* blob, size_t n);
  int forward_u8(const uint8_t* img, int B, int H, int W, int C, float* feat, float* logits, float* probs,
                 hipStream_t s) override;
  int forward_f32(const uint8_t* img, int B, int H, int W, int C, float* feat, float* logits, float* probs,
                  hipStream_t s);
  // fp32x3 path (mobilenet_x3.hip): wts holds every 1x1 matrix's f16 hi planes (f16 path layouts), then
  // the lo planes at x3_lo halfs; x3_scale: per block (expand, project) epilogue scales, then features[18]
  size_t x3_lo = 0;
  std::vector<float> x3_scale;
  std::vector<float> lx3_scale;  // layered form: per block (expand, project) epilogue scales
  int create_x3(const float* blob, size_t n);
  int forward_x3(const uint8_t* img, int B, int H, int W, int C, float* feat, float* logits, float* probs,
                 hipStream_t s);
  X3Tensors x3_tensors() const override;
};

// max |x| of n floats into *slot as float bits, by atomicMax: the running maximum since the slot was zeroed
// (absmax.hip); absmax_from_bits: a slot's value, +inf for an inf or a NaN; absmax_f32: mec_absmax_f32
int launch_absmax_f32(const float* x, size_t n, unsigned* slot, hipStream_t s);
float absmax_from_bits(unsigned bits);
int absmax_f32(const float* x_dev, long long n, float* out_host, hipStream_t s);

int resize_u8(const uint8_t* in, int B, int H, int W, uint8_t* out, int OH, int OW, hipStream_t s);
// layer1 seam: conv3 (64 -> 256) + residual + ReLU, then the next block's conv1 (256 -> N2)
int launch_pw_chain(const f16* t2, const f16* xin, const f16* w3, const float* b3, const f16* w1, const float* b1,
                    f16* xout, f16* t1, int M, int N2, hipStream_t s);
// layer1 block 1 -> 2 seam: conv3 + downsample (K = [T2 | X0]) + ReLU, then block 2's conv1
int launch_pw_chain_dual(const f16* t2, const f16* x0, const f16* w3ds, const float* b3ds, const f16* w1,
                         const float* b1, f16* xout, f16* t1, int M, hipStream_t s);
// fp32x3 layer1 seam (pw_chain_x3.hip): the same two products on hi / lo planes (lo planes L
// elements after their hi planes; weight lo planes at w*_lo, pre-scales undone by os*); dual =
// conv3 + downsample over K = [T2 | X0] (xin = X0), else conv3 + identity residual (xin)
int launch_pw_chain_x3(const f16* t2, const f16* xin, long long L, const f16* w3, long long w3_lo, float os3,
                       const float* b3, const f16* w1, long long w1_lo, float os1, const float* b1, f16* xout, f16* t1,
                       int M, int N2, bool dual, hipStream_t s);
// fp32x3 layer-2 seam (pw_seam_x3.hip): conv3 (K3 = 128 -> 512) + identity residual + ReLU, then the next
// conv1 (512 -> N1 = 128 | 256), the block output walked in 32-channel chunks; any M (row tails masked)
int launch_pw_seam_x3(const f16* t2, const f16* xin, long long L, const f16* w3, long long w3_lo, float os3,
                      const float* b3, const f16* w1, long long w1_lo, float os1, const float* b1, f16* xout, f16* t1,
                      int M, int K3, int N1, hipStream_t s);


}  // namespace mec
