// extern "C" boundary (include/mec.h).
#include "../../include/mec.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <exception>
#include <new>

#include "gemm_tiles.h"
#include "models.h"

namespace mec {
const char* last_error();

size_t blob_floats(int kind) {
  switch (kind) {
    case KIND_SPEECH: {
      const int d[6] = {56, 512, 512, 256, 128, 64};
      size_t s = 112;
      for (int i = 0; i < 5; ++i) s += (size_t)d[i] * d[i + 1] + 5 * d[i + 1];
      return s + 64 * 7 + 7;
    }
    case KIND_TEXT: {
      size_t s = (size_t)30522 * 768 + 512 * 768 + 2 * 768 + 2 * 768;
      const size_t layer = 4 * ((size_t)768 * 768 + 768) + 2 * 768 + ((size_t)3072 * 768 + 3072) +
                           ((size_t)768 * 3072 + 768) + 2 * 768;
      return s + 12 * layer + (size_t)768 * 768 + 768 + 7 * 768 + 7;
    }
    case KIND_IMAGE: {
      size_t s = 64 * 3 * 49 + 4 * 64;
      const int L[4][3] = {{64, 3, 1}, {128, 4, 2}, {256, 6, 2}, {512, 3, 2}};
      int cin = 64;
      for (int l = 0; l < 4; ++l)
        for (int b = 0; b < L[l][1]; ++b) {
          const int w = L[l][0];
          s += (size_t)w * cin + 4 * w + (size_t)w * w * 9 + 4 * w + (size_t)4 * w * w + 16 * w;
          if (b == 0) s += (size_t)4 * w * cin + 16 * w;
          cin = 4 * w;
        }
      return s + (size_t)512 * 2048 + 512 + 7 * 512 + 7;
    }
    case KIND_IMAGE_MBV2: {
      size_t s = 32 * 27 + 4 * 32;
      const int set[7][4] = {{1, 16, 1, 1}, {6, 24, 2, 2}, {6, 32, 3, 2}, {6, 64, 4, 2}, {6, 96, 3, 1}, {6, 160, 3, 2}, {6, 320, 1, 1}};
      int cin = 32;
      for (int i = 0; i < 7; ++i)
        for (int r = 0; r < set[i][2]; ++r) {
          const size_t t = set[i][0], hid = cin * t, cout = set[i][1];
          if (t != 1) s += hid * cin + 4 * hid;
          s += hid * 9 + 4 * hid + cout * hid + 4 * cout;
          cin = (int)cout;
        }
      return s + (size_t)1280 * 320 + 4 * 1280 + (size_t)512 * 1280 + 512 + 7 * 512 + 7;
    }
    case KIND_FUSION: {
      size_t s = 0;
      const int d[3] = {64, 768, 512};
      for (int m = 0; m < 3; ++m) s += (size_t)256 * d[m] + 256 + 512;
      s += 3 * ((size_t)768 * 256 + 768 + 256 * 256 + 256 + 512);
      s += 3 * ((size_t)256 * 256 + 256 + 512);
      s += (size_t)256 * 768 + 256 + 3 * 256 + 3 + 64 * 21 + 64 + 3 * 64 + 3;
      s += (size_t)256 * 263 + 256 + 512 + 128 * 256 + 128 + 7 * 128 + 7;
      return s;
    }
    case KIND_AUDIO: return 5;  // [sample_rate, n_fft, hop, n_mels, n_mfcc]
    case KIND_TEXT_LSTM: {
      size_t s = (size_t)LstmTextModel::kVocab * 128;
      s += 2 * ((size_t)128 * 512 + 128 * 512 + 512);  // Bidirectional(LSTM 128): kernel, recurrent_kernel, bias
      s += 2 * ((size_t)256 * 256 + 64 * 256 + 256);   // Bidirectional(LSTM 64)
      return s + 128 * 128 + 128 + 128 * 64 + 64 + 64 * 7 + 7;
    }
    default: return 0;
  }
}

// Tensors with an fp32x3 plane exponent taken from a BN estimate (image_model.h resnet_x3_tensors /
// mb_x3_tensors), known before a handle exists; 0: the kind has none
static int x3_tensor_count(int kind) {
  if (kind == KIND_IMAGE) return 1 + 4 + 2 * (3 + 4 + 6 + 3);  // stem, layerN.out, conv1 + conv2 per block
  if (kind == KIND_IMAGE_MBV2) return 7;                      // one per (t, c, n, s) setting
  return 0;
}
}  // namespace mec

using namespace mec;

struct mec_model {
  Model* impl;
};

static hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }

// Image entry points take either backbone (ResNet50 or MobileNetV2).
static ImageNet* image_net(mec_model* m) {
  if (!m || !m->impl) { set_error("null model handle"); return nullptr; }
  if (m->impl->kind != KIND_IMAGE && m->impl->kind != KIND_IMAGE_MBV2) {
    set_error("model handle has the wrong kind for this call");
    return nullptr;
  }
  if (hipSetDevice(m->impl->device) != hipSuccess) { set_error("hipSetDevice failed"); return nullptr; }
  return static_cast<ImageNet*>(m->impl);
}

// The observation entry points take an exact-fp32 handle of either backbone: its forward is what is observed.
static ImageNet* observed_net(mec_model* m, const char* who) {
  if (!m || !m->impl || (m->impl->kind != KIND_IMAGE && m->impl->kind != KIND_IMAGE_MBV2) || m->impl->prec != PREC_FP32) {
    set_error(std::string(who) + ": needs an MEC_PREC_FP32 handle of kind MEC_IMAGE or MEC_IMAGE_MBV2");
    return nullptr;
  }
  return image_net(m);
}

template <class T>
static T* as(mec_model* m, int kind) {
  if (!m || !m->impl) { set_error("null model handle"); return nullptr; }
  if (m->impl->kind != kind) { set_error("model handle has the wrong kind for this call"); return nullptr; }
  if (hipSetDevice(m->impl->device) != hipSuccess) { set_error("hipSetDevice failed"); return nullptr; }
  return static_cast<T*>(m->impl);
}

// mec_create_opt's body; cal (or null): the observed maxima of a calibrated creation, already checked
static int create_model(int kind, const float* host_blob, size_t n, int device, int precision, const char* opts,
                        const std::vector<double>* cal, mec_model** out) {
  if (!out) { set_error("mec_create: out is null"); return -1; }
  if (precision != MEC_PREC_F16 && precision != MEC_PREC_FP32 && precision != MEC_PREC_FP32X3) {
    set_error("mec_create: precision must be MEC_PREC_F16, MEC_PREC_FP32 or MEC_PREC_FP32X3");
    return -1;
  }
  *out = nullptr;
  const size_t want = blob_floats(kind);
  if (!want) { set_error("mec_create: unknown kind"); return -1; }
  if (!host_blob || n != want) {
    set_error("mec_create: blob has " + std::to_string(n) + " floats, expected " + std::to_string(want));
    return -1;
  }
  // "key=value,key=value": this handle's knobs, applied over the process defaults before its weights are
  // packed (so creation-time knobs such as x3_headroom take effect)
  Options o = default_options();
  if (opts && *opts) {
    std::string all(opts);
    size_t pos = 0;
    while (pos <= all.size()) {
      const size_t end = std::min(all.find(',', pos), all.size());
      const std::string kv = all.substr(pos, end - pos);
      const size_t eq = kv.find('=');
      if (eq == std::string::npos || eq == 0) { set_error("mec_create_opt: bad option \"" + kv + "\" (key=value)"); return -1; }
      char* tail = nullptr;
      const long v = std::strtol(kv.c_str() + eq + 1, &tail, 10);
      if (!tail || *tail || tail == kv.c_str() + eq + 1) { set_error("mec_create_opt: bad value in \"" + kv + "\""); return -1; }
      if (set_option(o, kv.substr(0, eq), (int)v) != 0) return -1;
      pos = end + 1;
    }
  }
  MEC_HIP(hipSetDevice(device));
  Model* impl = nullptr;
  int rc = -1;
  switch (kind) {
    // speech, fusion, audio and the BiLSTM are fp32 at every precision
    case KIND_SPEECH: { auto* p = new SpeechModel(); impl = p; p->opts = o; rc = p->create(host_blob, n); break; }
    case KIND_TEXT: { auto* p = new TextModel(); p->prec = precision; impl = p; p->opts = o; rc = p->create(host_blob, n); break; }
    case KIND_IMAGE: { auto* p = new ImageModel(); p->prec = precision; impl = p; p->opts = o; if (cal) p->x3_cal = *cal; rc = p->create(host_blob, n); break; }
    case KIND_FUSION: { auto* p = new FusionModel(); impl = p; p->opts = o; rc = p->create(host_blob, n); break; }
    case KIND_IMAGE_MBV2: { auto* p = new MobileNetModel(); p->prec = precision; impl = p; p->opts = o; if (cal) p->x3_cal = *cal; rc = p->create(host_blob, n); break; }
    case KIND_AUDIO: { auto* p = new AudioModel(); impl = p; p->opts = o; rc = p->create(host_blob, n); break; }
    case KIND_TEXT_LSTM: { auto* p = new LstmTextModel(); impl = p; p->opts = o; rc = p->create(host_blob, n); break; }
  }
  if (rc != 0) { delete impl; return -1; }
  if (cal && impl->x3_noted != cal->size()) {  // x3_tensor_count and the creation disagree
    set_error("mec_create_x3_calibrated: the creation named " + std::to_string(impl->x3_noted) + " tensors");
    delete impl;
    return -1;
  }
  impl->kind = kind;
  impl->device = device;
  impl->prec = (kind == KIND_SPEECH || kind == KIND_FUSION || kind == KIND_AUDIO || kind == KIND_TEXT_LSTM) ? MEC_PREC_FP32 : precision;
  if (impl->prec == PREC_FP32X3 && impl->alloc_range_flag() != 0) { delete impl; return -1; }
  if (impl->prec == PREC_FP32X3)
    impl->x3_report = "x3_headroom=" + std::to_string(o.x3_headroom) + " x3_plane_scale=" +
                      std::to_string(o.x3_plane_scale) + (cal ? " x3_calibrated=1" : "") + "\n" + impl->x3_report;
  *out = new mec_model{impl};
  return 0;
}

extern "C" {

const char* mec_version(void) { return "mec-hip 0.1 (gfx950)"; }
const char* mec_last_error(void) { return last_error(); }

long long mec_blob_size(int kind) {
  const size_t n = blob_floats(kind);
  return n ? (long long)n : -1;
}

int mec_create(int kind, const float* host_blob, size_t n, int device, mec_model** out) {
  return mec_create_ex(kind, host_blob, n, device, MEC_PREC_F16, out);
}

int mec_create_ex(int kind, const float* host_blob, size_t n, int device, int precision, mec_model** out) {
  return mec_create_opt(kind, host_blob, n, device, precision, nullptr, out);
}

int mec_create_opt(int kind, const float* host_blob, size_t n, int device, int precision, const char* opts,
                   mec_model** out) {
  API_GUARD({ return create_model(kind, host_blob, n, device, precision, opts, nullptr, out); })
}

int mec_create_x3_calibrated(int kind, const float* host_blob, size_t n, int device, const char* opts,
                             const float* absmax, int count, mec_model** out) {
  API_GUARD({
    if (!out) { set_error("mec_create_x3_calibrated: out is null"); return -1; }
    *out = nullptr;
    const int want = x3_tensor_count(kind);
    if (!want) {
      set_error("mec_create_x3_calibrated: kind must be MEC_IMAGE or MEC_IMAGE_MBV2 (the plane exponents of the "
                "other kinds come from rigorous bounds, or the kind has no fp32x3 path)");
      return -1;
    }
    if (!absmax) { set_error("mec_create_x3_calibrated: absmax is null"); return -1; }
    if (count != want) {
      set_error("mec_create_x3_calibrated: count is " + std::to_string(count) + ", this kind has " +
                std::to_string(want) + " tensors (mec_model_x3_names)");
      return -1;
    }
    std::vector<double> cal(absmax, absmax + count);
    for (int i = 0; i < count; ++i)
      if (!(cal[i] >= 0.0) || !std::isfinite(cal[i])) {
        set_error("mec_create_x3_calibrated: absmax[" + std::to_string(i) + "] is negative, NaN or inf (an observed "
                  "maximum is finite and >= 0; 0 keeps the tensor's estimate)");
        return -1;
      }
    return create_model(kind, host_blob, n, device, MEC_PREC_FP32X3, opts, &cal, out);
  })
}

const char* mec_model_x3_report(mec_model* m) {
  if (!m || !m->impl) { set_error("mec_model_x3_report: null handle"); return nullptr; }
  return m->impl->x3_report.c_str();
}

const char* mec_model_x3_names(mec_model* m) {
  try {
    ImageNet* p = image_net(m);
    if (!p) return nullptr;
    if (p->x3_names.empty())
      for (const std::string& name : p->x3_tensors().names) p->x3_names += name + "\n";
    return p->x3_names.c_str();
  } catch (const std::exception& e) {
    set_error(e.what());
    return nullptr;
  }
}

int mec_model_x3_observe(mec_model* m, int on) {
  API_GUARD({
    ImageNet* p = observed_net(m, "mec_model_x3_observe");
    if (!p) return -1;
    MEC_REQUIRE(on == 0 || on == 1, "mec_model_x3_observe: on is 0 or 1");
    if (on) {
      const int n = (int)p->x3_tensors().names.size();
      MEC_HIP(hipDeviceSynchronize());  // no forward of the handle may still fill the slots
      MEC_TRY(p->obs.ensure(n * sizeof(unsigned)));
      MEC_HIP(hipMemset(p->obs.p, 0, n * sizeof(unsigned)));
      MEC_HIP(hipDeviceSynchronize());
      p->obs_n = n;
    }
    p->obs_on = on != 0;
    return p->obs_n;
  })
}

int mec_model_x3_observed(mec_model* m, float* absmax_host, int cap) {
  API_GUARD({
    ImageNet* p = observed_net(m, "mec_model_x3_observed");
    if (!p) return -1;
    MEC_REQUIRE(p->obs_n > 0, "mec_model_x3_observed: the handle was never armed (mec_model_x3_observe(m, 1))");
    MEC_REQUIRE(absmax_host && cap >= p->obs_n, "mec_model_x3_observed: absmax_host must hold the handle's tensor "
                                                "count (what mec_model_x3_observe returned)");
    MEC_HIP(hipDeviceSynchronize());
    std::vector<unsigned> bits(p->obs_n);
    MEC_HIP(hipMemcpy(bits.data(), p->obs.p, bits.size() * sizeof(unsigned), hipMemcpyDeviceToHost));
    for (int i = 0; i < p->obs_n; ++i) absmax_host[i] = absmax_from_bits(bits[i]);
    return p->obs_n;
  })
}

int mec_absmax_f32(const float* x_dev, long long n, float* out_host, void* stream) {
  API_GUARD({ return absmax_f32(x_dev, n, out_host, S(stream)); })
}

int mec_destroy(mec_model* m) {
  if (!m) return 0;
  if (m->impl) (void)hipSetDevice(m->impl->device);
  delete m->impl;
  delete m;
  return 0;
}

int mec_speech_fwd(mec_model* m, const float* x, int B, float* feat, float* logits, float* probs, void* stream) {
  API_GUARD({
    auto* p = as<SpeechModel>(m, KIND_SPEECH);
    if (!p) return -1;
    OptScope sc(&p->opts, &p->tune, p->range_dev);
    return p->forward(x, B, feat, logits, probs, S(stream));
  })
}

int mec_text_fwd(mec_model* m, const int32_t* ids, const int32_t* mask, int B, int L, float* cls, float* logits,
                 float* probs, void* stream) {
  API_GUARD({
    auto* p = as<TextModel>(m, KIND_TEXT);
    if (!p) return -1;
    OptScope sc(&p->opts, &p->tune, p->range_dev);
    return p->forward(ids, mask, B, L, cls, logits, probs, S(stream));
  })
}

int mec_image_fwd(mec_model* m, const uint8_t* gray, int B, float* feat, float* logits, float* probs,
                  void* stream) {
  API_GUARD({
    auto* p = image_net(m);
    if (!p) return -1;
    OptScope sc(&p->opts, &p->tune, p->range_dev);
    return p->forward(gray, B, feat, logits, probs, S(stream));
  })
}

int mec_image_fwd_u8(mec_model* m, const uint8_t* img, int B, int H, int W, int C, float* feat, float* logits,
                     float* probs, void* stream) {
  API_GUARD({
    auto* p = image_net(m);
    if (!p) return -1;
    OptScope sc(&p->opts, &p->tune, p->range_dev);
    return p->forward_u8(img, B, H, W, C, feat, logits, probs, S(stream));
  })
}

int mec_fusion_fwd(mec_model* m, const float* s_feat, const float* t_feat, const float* i_feat, const float* s_pred,
                   const float* t_pred, const float* i_pred, int B, float* logits, float* probs, float* attn_w,
                   float* dec_w, void* stream) {
  API_GUARD({
    auto* p = as<FusionModel>(m, KIND_FUSION);
    if (!p) return -1;
    OptScope sc(&p->opts, &p->tune, p->range_dev);
    return p->forward(s_feat, t_feat, i_feat, s_pred, t_pred, i_pred, B, logits, probs, attn_w, dec_w, S(stream));
  })
}

}  // extern "C"

// mec_fusion_mixed_plan's body (include/mec.h states it): one pass in ascending sample order. Host only.
static int fusion_mixed_plan(const uint8_t* present, int B, int have_model, int32_t* s_idx, int32_t* t_idx,
                             int32_t* i_idx, int32_t* route, int32_t* att, int32_t* counts) {
  MEC_REQUIRE(B >= 0, "mec_fusion_mixed_plan: B < 0");
  if (B == 0) {
    if (counts) counts[0] = counts[1] = counts[2] = 0;
    return 0;
  }
  MEC_REQUIRE(present && s_idx && t_idx && i_idx && route && att && counts,
              "mec_fusion_mixed_plan: null pointer (present, the three index arrays, route and att hold B entries, counts 3)");
  for (int b = 0; b < B; ++b)
    MEC_REQUIRE(present[b] <= 7, "mec_fusion_mixed_plan: every present value must be an or of the MEC_MOD_* bits (0..7)");
  int32_t* idx[3] = {s_idx, t_idx, i_idx};
  int n[3] = {0, 0, 0}, n_att = 0;
  for (int b = 0; b < B; ++b) {
    int bits = 0;
    for (int m = 0; m < 3; ++m) {
      const bool has = (present[b] >> m) & 1;
      idx[m][b] = has ? n[m]++ : -1;
      bits += has;
    }
    route[b] = bits == 3 ? (have_model ? MEC_ROUTE_ATTENTION : MEC_ROUTE_AVERAGE) : bits;  // 0 none, 1 single, 2 average
    if (route[b] == MEC_ROUTE_ATTENTION) att[n_att++] = b;
  }
  for (int k = n_att; k < B; ++k) att[k] = -1;
  for (int m = 0; m < 3; ++m) counts[m] = n[m];
  return n_att;
}

extern "C" {

int mec_fusion_mixed_plan(const uint8_t* present, int B, int have_model, int32_t* s_idx, int32_t* t_idx, int32_t* i_idx,
                          int32_t* route, int32_t* att, int32_t counts[3]) {
  API_GUARD({ return fusion_mixed_plan(present, B, have_model, s_idx, t_idx, i_idx, route, att, counts); })
}

int mec_fusion_fwd_mixed(mec_model* m, const mec_fusion_mixed_args* a, void* stream) {
  API_GUARD({
    MEC_TRY(fusion_mixed_check(a, m != nullptr));
    if (m && !m->impl) { set_error("null model handle"); return -1; }
    if (m && m->impl->kind != KIND_FUSION) { set_error("model handle has the wrong kind for this call"); return -1; }
    if (a->B == 0) return 0;
    if (!m) return fusion_fwd_mixed(nullptr, *a, S(stream));
    auto* p = as<FusionModel>(m, KIND_FUSION);
    if (!p) return -1;
    OptScope sc(&p->opts, &p->tune, p->range_dev);
    return fusion_fwd_mixed(p, *a, S(stream));
  })
}

int mec_audio_fwd(mec_model* m, const float* wave, int B, int n_samples, float* feat, float* tuning, void* stream) {
  API_GUARD({
    auto* p = as<AudioModel>(m, KIND_AUDIO);
    if (!p) return -1;
    OptScope sc(&p->opts, &p->tune, p->range_dev);
    return p->forward(wave, B, n_samples, feat, tuning, S(stream));
  })
}

int mec_audio_load_ragged(mec_model* m, const uint8_t* src, const int64_t* offs, const int32_t* desc, int B,
                          size_t src_bytes, float* wave, int n_out, void* stream) {
  API_GUARD({
    auto* p = as<AudioModel>(m, KIND_AUDIO);
    if (!p) return -1;
    return p->load_ragged(src, offs, desc, B, src_bytes, wave, n_out, S(stream));
  })
}

// First-fit decreasing over 128-slot rows: samples by length descending (ties: ascending index), each into
// the lowest-numbered row with room, at that row's fill; a new row when none has room. Host only.
int mec_text_pack_plan(const int32_t* lens, int B, int32_t* row, int32_t* off) {
  API_GUARD({
    MEC_REQUIRE(B >= 0, "mec_text_pack_plan: B < 0");
    if (B == 0) return 0;
    MEC_REQUIRE(lens && row && off, "mec_text_pack_plan: null pointer (lens, row and off hold B entries; lengths in [1,128])");
    for (int i = 0; i < B; ++i)
      MEC_REQUIRE(lens[i] >= 1 && lens[i] <= 128, "mec_text_pack_plan: every length must be in [1,128]");
    std::vector<int> order(B);
    for (int i = 0; i < B; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return lens[a] > lens[b]; });
    std::vector<int> fill;
    for (int i : order) {
      size_t r = 0;
      while (r < fill.size() && 128 - fill[r] < lens[i]) ++r;
      if (r == fill.size()) fill.push_back(0);
      row[i] = (int32_t)r;
      off[i] = fill[r];
      fill[r] += lens[i];
    }
    return (int)fill.size();
  })
}

int mec_text_fwd_packed(mec_model* m, const int32_t* ids, const int32_t* row, const int32_t* off, const int32_t* len,
                        int B, int Bp, float* cls, float* logits, float* probs, void* stream) {
  API_GUARD({
    auto* p = as<TextModel>(m, KIND_TEXT);
    if (!p) return -1;
    OptScope sc(&p->opts, &p->tune, p->range_dev);
    return p->forward_packed(ids, row, off, len, B, Bp, cls, logits, probs, S(stream));
  })
}

int mec_text_lstm_fwd(mec_model* m, const int32_t* ids, int B, int L, float* feat, float* logits, float* probs,
                      void* stream) {
  API_GUARD({
    auto* p = as<LstmTextModel>(m, KIND_TEXT_LSTM);
    if (!p) return -1;
    OptScope sc(&p->opts, &p->tune, p->range_dev);
    return p->forward(ids, B, L, feat, logits, probs, S(stream));
  })
}

int mec_lstm_seq_f32(const float* xz, const float* U, int B, int L, int units, int reverse, float* y_seq,
                     float* h_last, void* stream) {
  API_GUARD({ return lstm_seq_f32(xz, U, B, L, units, reverse, y_seq, h_last, S(stream)); })
}

int mec_fuse_weighted(const float* s, const float* t, const float* i, int B, double* out, void* stream) {
  API_GUARD({ return fuse_weighted(s, t, i, B, out, S(stream)); })
}

int mec_fuse_weighted_f64(const double* s, const double* t, const double* i, int B, double* out, void* stream) {
  API_GUARD({ return fuse_weighted_f64(s, t, i, B, out, S(stream)); })
}

int mec_resize_u8(const uint8_t* in, int B, int H, int W, uint8_t* out, int OH, int OW, void* stream) {
  API_GUARD({ return resize_u8(in, B, H, W, out, OH, OW, S(stream)); })
}

int mec_gemm_f16(const void* A, const void* B, const float* bias, const void* R, int r_is_f32, void* C16,
                 float* C32, int M, int N, int K, int act, void* stream) {
  API_GUARD({
    GemmParams g;
    g.A = A; g.B = reinterpret_cast<const f16*>(B); g.bias = bias; g.R = R; g.r_f32 = r_is_f32;
    g.C16 = reinterpret_cast<f16*>(C16); g.C32 = C32; g.M = M; g.N = N; g.K = K; g.act = act;
    return launch_gemm(g, S(stream), nullptr, TAG_NONE);
  })
}

int mec_gemm_f16x3(const void* A, long long a_lo, const void* B, long long b_lo, float oscale, const float* bias,
                   const float* R, void* C16, long long c_lo, float* C32, int M, int N, int K, int act,
                   void* stream) {
  API_GUARD({
    MEC_REQUIRE(a_lo != 0 && b_lo != 0, "mec_gemm_f16x3: a_lo / b_lo must locate the lo planes");
    GemmParams g;
    g.split = 1; g.A = A; g.a_lo = a_lo; g.B = reinterpret_cast<const f16*>(B); g.b_lo = b_lo; g.oscale = oscale;
    g.bias = bias; g.R = R; g.r_f32 = R != nullptr; g.C16 = reinterpret_cast<f16*>(C16); g.c_lo = C16 ? c_lo : 0;
    g.C32 = C32; g.M = M; g.N = N; g.K = K; g.act = act;
    return launch_gemm(g, S(stream), nullptr, TAG_NONE);
  })
}

// The paired-operand split GEMM behind both C entries below.
static int gemm_f16x3_paired(const void* A, const void* B, float oscale, const float* bias, const float* R,
                             const float* r_stats, const float* r_gamma, const float* r_beta, void* C16, int c_paired,
                             long long c_lo, float cscale, float* C32, int M, int N, int K, int act, unsigned* flag,
                             void* stream) {
  GemmParams g;
  g.split = 1; g.a_pair = g.b_pair = 1; g.A = A; g.B = reinterpret_cast<const f16*>(B); g.oscale = oscale;
  g.bias = bias; g.R = R; g.r_f32 = R != nullptr;
  g.r_stats = reinterpret_cast<const float2*>(r_stats); g.r_g = r_gamma; g.r_b = r_beta;
  g.C16 = reinterpret_cast<f16*>(C16); g.c_pair = C16 && c_paired; g.c_lo = C16 && !c_paired ? c_lo : 0;
  g.cscale = cscale; g.C32 = C32; g.M = M; g.N = N; g.K = K; g.act = act; g.ovf = flag;
  return launch_gemm(g, S(stream), nullptr, TAG_NONE);
}

int mec_gemm_f16x3_paired(const void* A, const void* B, float oscale, const float* bias, const float* R, void* C16,
                          int c_paired, long long c_lo, float* C32, int M, int N, int K, int act, void* stream) {
  API_GUARD({
    MEC_REQUIRE(!C16 || c_paired || c_lo != 0, "mec_gemm_f16x3_paired: a planar C16 needs c_lo");
    return gemm_f16x3_paired(A, B, oscale, bias, R, nullptr, nullptr, nullptr, C16, c_paired, c_lo, 1.f, C32, M, N, K,
                             act, nullptr, stream);
  })
}

int mec_gemm_f16x3_paired_ln(const void* A, const void* B, float oscale, const float* bias, const float* R,
                             const float* r_stats, const float* r_gamma, const float* r_beta, void* C16, int c_paired,
                             long long c_lo, float cscale, float* C32, int M, int N, int K, int act,
                             unsigned* range_flag, void* stream) {
  API_GUARD({
    MEC_REQUIRE(!C16 || c_paired || c_lo != 0, "mec_gemm_f16x3_paired_ln: a planar C16 needs c_lo");
    MEC_REQUIRE(oscale != 0.f && cscale != 0.f, "mec_gemm_f16x3_paired_ln: oscale and cscale must be set (1 = none)");
    return gemm_f16x3_paired(A, B, oscale, bias, R, r_stats, r_gamma, r_beta, C16, c_paired, c_lo, cscale, C32, M, N, K,
                             act, range_flag, stream);
  })
}

int mec_conv_f16(const void* x, const void* w, const float* bias, const void* R, void* y, int n, int H, int W,
                 int C, int Cout, int ks, int stride, int pad, int act, void* stream) {
  API_GUARD({
    GemmParams g;
    g.amode = A_CONV; g.A = x; g.B = reinterpret_cast<const f16*>(w); g.bias = bias; g.R = R;
    g.C16 = reinterpret_cast<f16*>(y); g.act = act;
    g.H = H; g.W = W; g.C = C; g.ks = ks; g.stride = stride; g.pad = pad;
    MEC_TRY(set_conv_geometry(g, n));
    g.N = Cout; g.K = ks * ks * C;
    return launch_gemm(g, S(stream), nullptr, TAG_NONE);
  })
}

int mec_gemm_ex(const mec_gemm_args* a, void* stream) {
  API_GUARD({
    MEC_REQUIRE(a, "mec_gemm_ex: null descriptor");
    MEC_REQUIRE(a->amode == MEC_A_PLAIN || a->amode == MEC_A_CONV || a->amode == MEC_A_DUAL,
                "mec_gemm_ex: amode must be MEC_A_PLAIN, MEC_A_CONV or MEC_A_DUAL");
    MEC_REQUIRE((a->a_lo != 0) == (a->b_lo != 0), "mec_gemm_ex: a_lo and b_lo locate the lo planes together (both or neither)");
    MEC_REQUIRE(a->oscale != 0.f && a->cscale != 0.f, "mec_gemm_ex: oscale and cscale must be set (1 = none)");
    GemmParams g;
    g.amode = a->amode; g.split = a->a_lo != 0;
    g.A = a->A; g.a_lo = a->a_lo; g.A2 = a->A2; g.K1 = a->K1;
    g.B = reinterpret_cast<const f16*>(a->B); g.b_lo = a->b_lo; g.oscale = a->oscale;
    g.bias = a->bias; g.R = a->R; g.r_f32 = a->r_is_f32; g.r_lo = a->r_lo;
    g.r_stats = reinterpret_cast<const float2*>(a->r_stats); g.r_g = a->r_gamma; g.r_b = a->r_beta;
    g.C16 = reinterpret_cast<f16*>(a->C16); g.c_lo = a->C16 ? a->c_lo : 0; g.cscale = a->cscale; g.C32 = a->C32;
    g.M = a->M; g.N = a->N; g.K = a->K; g.act = a->act;
    if (a->amode != MEC_A_PLAIN) {  // conv / dual: M and K follow from the geometry
      g.H = a->H; g.W = a->W; g.C = a->C; g.ks = a->ks; g.stride = a->stride; g.pad = a->pad;
      MEC_TRY(set_conv_geometry(g, a->n));
      g.K = a->amode == MEC_A_CONV ? a->ks * a->ks * a->C : a->K1 + a->C;
    }
    return launch_gemm(g, S(stream), nullptr, TAG_NONE);
  })
}

int mec_bert_attn(const mec_attn_args* a, void* stream) {
  API_GUARD({
    MEC_REQUIRE(a, "mec_bert_attn: null descriptor");
    const bool x3 = a->precision == MEC_PREC_FP32X3;
    MEC_REQUIRE(a->precision == MEC_PREC_F16 || a->precision == MEC_PREC_FP32 || x3,
                "mec_bert_attn: precision must be MEC_PREC_F16, MEC_PREC_FP32 or MEC_PREC_FP32X3");
    MEC_REQUIRE((a->form == 0 || a->form == 1) && (a->fused == 0 || a->fused == 1) && (a->packed == 0 || a->packed == 1),
                "mec_bert_attn: form, fused and packed are 0 or 1");
    MEC_REQUIRE(a->rows >= 0 && a->rows <= (1 << 20), "mec_bert_attn: rows out of range");
    MEC_REQUIRE(a->mask && a->ctx, "mec_bert_attn: null mask or ctx");
    // a split tensor's lo plane: a positive element offset (16-B loads: a multiple of 8), or kX3Paired
    auto lo_ok = [](long long lo) { return lo == kX3Paired || (lo > 0 && lo % 8 == 0); };
    if (x3) {
      MEC_REQUIRE(lo_ok(a->ctx_lo), "mec_bert_attn: ctx_lo must locate the lo plane (a multiple of 8) or be -1 (paired)");
      MEC_REQUIRE(a->qks > 0.f && a->qks < 1e30f, "mec_bert_attn: qks must be set (1/8 2^-(s_q + s_k))");
    } else {
      MEC_REQUIRE(a->qks == 0.125f, "mec_bert_attn: the f16 and fp32 kernels scale the scores by 1/8 (qks = 0.125)");
    }
    const int32_t* mask = reinterpret_cast<const int32_t*>(a->mask);
    if (a->fused) {
      MEC_REQUIRE(a->precision != MEC_PREC_FP32, "mec_bert_attn: the fp32 path has no fused QKV + attention kernel");
      MEC_REQUIRE(a->form == 0, "mec_bert_attn: the fused kernels serve all 128 queries only (form 0)");
      MEC_REQUIRE(a->hs && a->wqkv && a->bqkv, "mec_bert_attn: fused needs hs, wqkv and bqkv");
      if (a->rows == 0) return 0;
      if (!x3) {
        MEC_REQUIRE(a->oscale == 1.f, "mec_bert_attn: the f16 fused kernel has no output scale (oscale = 1)");
        return launch_bert_qkv_attn(reinterpret_cast<const f16*>(a->hs), reinterpret_cast<const f16*>(a->wqkv), a->bqkv,
                                    mask, reinterpret_cast<f16*>(a->ctx), a->rows, S(stream), a->packed != 0);
      }
      MEC_REQUIRE(lo_ok(a->hs_lo) && lo_ok(a->w_lo), "mec_bert_attn: hs_lo and w_lo must locate the lo planes or be -1");
      MEC_REQUIRE(a->oscale > 0.f && a->oscale < 1e30f, "mec_bert_attn: oscale must be set (1 = none)");
      MEC_REQUIRE(opt().gemm_x3_order == 1, "mec_bert_attn: the fused fp32x3 kernel has the K-interleaved term order (gemm_x3_order 1)");
      return launch_bert_qkv_attn_x3(reinterpret_cast<const f16*>(a->hs), a->hs_lo, reinterpret_cast<const f16*>(a->wqkv),
                                     a->w_lo, a->oscale, a->bqkv, mask, reinterpret_cast<f16*>(a->ctx), a->ctx_lo, a->rows,
                                     a->qks, S(stream), a->packed != 0);
    }
    MEC_REQUIRE(a->qkv, "mec_bert_attn: null qkv");
    MEC_REQUIRE(!x3 || lo_ok(a->qkv_lo), "mec_bert_attn: qkv_lo must locate the lo plane (a multiple of 8) or be -1 (paired)");
    if (a->form == 0) {
      if (a->rows == 0) return 0;
      if (x3)
        return launch_bert_attention_x3(reinterpret_cast<const f16*>(a->qkv), a->qkv_lo, mask, reinterpret_cast<f16*>(a->ctx),
                                        a->ctx_lo, a->rows, a->qks, S(stream), a->packed != 0);
      if (a->precision == MEC_PREC_FP32)
        return launch_bert_attention_f32(reinterpret_cast<const float*>(a->qkv), mask, reinterpret_cast<float*>(a->ctx),
                                         a->rows, S(stream), a->packed != 0);
      return launch_bert_attention(reinterpret_cast<const f16*>(a->qkv), mask, reinterpret_cast<f16*>(a->ctx), a->rows,
                                   S(stream), a->packed != 0);
    }
    // the [CLS]-only form: ns samples over `rows` rows of K | V
    MEC_REQUIRE(a->qc, "mec_bert_attn: the [CLS]-only form needs qc");
    MEC_REQUIRE(!x3 || lo_ok(a->qc_lo), "mec_bert_attn: qc_lo must locate the lo plane (a multiple of 8) or be -1 (paired)");
    MEC_REQUIRE(a->ns >= 0 && a->ns <= (1 << 20), "mec_bert_attn: ns out of range");
    if (a->packed) {
      MEC_REQUIRE(a->cidx, "mec_bert_attn: the packed [CLS]-only form needs cidx");
      MEC_REQUIRE(a->ns == 0 || a->rows >= 1, "mec_bert_attn: samples without a row");
    } else {
      MEC_REQUIRE(!a->cidx, "mec_bert_attn: cidx goes with packed");
      MEC_REQUIRE(a->ns == a->rows, "mec_bert_attn: unpacked, sample b reads row b (ns == rows)");
    }
    if (a->ns == 0) return 0;
    if (x3)
      return launch_bert_attention_x3_cls(reinterpret_cast<const f16*>(a->qkv), a->qkv_lo, mask,
                                          reinterpret_cast<const f16*>(a->qc), a->qc_lo, reinterpret_cast<f16*>(a->ctx),
                                          a->ctx_lo, a->ns, a->qks, S(stream), a->cidx);
    if (a->precision == MEC_PREC_FP32)
      return launch_bert_attention_f32_cls(reinterpret_cast<const float*>(a->qkv), mask, reinterpret_cast<const float*>(a->qc),
                                           reinterpret_cast<float*>(a->ctx), a->ns, S(stream), a->cidx);
    return launch_bert_attention_cls(reinterpret_cast<const f16*>(a->qkv), mask, reinterpret_cast<const f16*>(a->qc),
                                     reinterpret_cast<f16*>(a->ctx), a->ns, S(stream), a->cidx);
  })
}

}  // extern "C"

namespace mec {
// One knob of `o` (include/mec.h lists them). The probe-build values (*_debug, bert_qkv_attn
// 2 | 3, speech_spin_limit >= 0) return wrong results and exist only in -DMEC_PROBES builds.
int set_option(Options& o, const std::string& k, int value) {
  const bool probe = kProbes;
  if (k == "fusion_r" && (value == 1 || value == 2 || value == 4)) { o.fusion_r = value; return 0; }
  if (k == "gemm_f32_family" && (value == 0 || value == 16 || value == 32)) {
    o.gemm_f32_family = value;
    return 0;
  }
  if (k == "bert_cls_last" && (value == 0 || value == 1)) { o.bert_cls_last = value; return 0; }
  if (k == "gemm_x3_order" && (value == 0 || value == 1)) { o.gemm_x3_order = value; return 0; }
  if (k == "gelu_x3" && (value == 0 || value == 1)) { o.gelu_x3 = value; return 0; }
  if (k == "bert_ln_rows" && (value == 1 || value == 2 || value == 4)) {
    o.bert_ln_rows = value;
    return 0;
  }
  if (k == "gemm_group_m" && (value == 0 || value == 2 || value == 4 || value == 8 || value == 16)) {
    o.gemm_group_m = value;
    return 0;
  }
  if (k == "gemm_glds_group_m" && (value == 0 || value == 2 || value == 4 || value == 8 || value == 16)) {
    o.gemm_glds_group_m = value;
    return 0;
  }
  if (k == "lstm_rows" && (value == 1 || value == 2 || value == 4)) { o.lstm_rows = value; return 0; }
  if (k == "fusion_split" && (value == 0 || value == 1)) { o.fusion_split = value; return 0; }
  if (k == "speech_spin_limit" && (value == -1 || (probe && value >= 0))) { o.speech_spin_limit = value; return 0; }
  if (k == "gemm_debug" && (value == 0 || (probe && value >= 1 && value <= 6))) { o.gemm_debug = value; return 0; }
  if (k == "gemm_autotune" && (value == 0 || value == 1)) { o.gemm_autotune = value; return 0; }
  auto f32_tile_ok = [](int id) { return id == 0 || f32_tile(id); };  // 0 = autotune, else a catalogued tile
  if (k == "gemm_f32_tile" && f32_tile_ok(value)) { o.gemm_f32_tile = value; return 0; }
  if (k == "gemm_f32_tag" && value >= 0 && value / 100000 > 0 && value / 100000 < TAG_COUNT && f32_tile_ok(value % 100000)) {
    o.gemm_f32_tag[value / 100000] = value % 100000;
    return 0;
  }
  if (k == "gemm_prefetch_r" && (value == 0 || value == 1)) { o.gemm_prefetch_r = value; return 0; }
  if (k == "mbv2_impl" && value >= 0 && value <= 2) { o.mbv2_impl = value; return 0; }
  if (k == "mbv2_x3_tile" && (value == 0 || value == 4)) { o.mbv2_x3_tile = value; return 0; }
  if (k == "mbv2_x3_tpw" && value >= 1 && value <= 16) { o.mbv2_x3_tpw = value; return 0; }
  if (k == "mbv2_x3_occ" && (value == 3 || value == 4)) { o.mbv2_x3_occ = value; return 0; }
  if (k == "mbv2_x3_sesw" && (value == 0 || value == 1)) { o.mbv2_x3_sesw = value; return 0; }
  if (k == "x3_plane_scale" && (value == 0 || value == 1)) { o.x3_plane_scale = value; return 0; }
  if (k == "x3_headroom" && value >= 0 && value <= 24) { o.x3_headroom = value; return 0; }
  if (k == "x3_layout" && (value == 0 || value == 1)) { o.x3_layout = value; return 0; }
  if (k == "qkv_x3_late_dma" && value >= 0 && value <= 2) { o.qkv_x3_late_dma = value; return 0; }
  if (k == "gemm_x3_pp" && value >= 0 && value <= 2) { o.gemm_x3_pp = value; return 0; }
  if (k == "mbv2_layered" && (value == 0 || (value >= 7 && value <= 17))) { o.mbv2_layered = value; return 0; }
  if (k == "mbv2_layered16" && (value == 0 || (value >= 7 && value <= 17))) { o.mbv2_layered16 = value; return 0; }
  if (k == "conv3x3_direct" && (value == 0 || value == 1)) { o.conv3x3_direct = value; return 0; }
  if (k == "conv3x3_halo" && (value == 0 || value == 1)) { o.conv3x3_halo = value; return 0; }
  if (k == "stem_gray_f32" && (value == 0 || value == 1)) { o.stem_gray_f32 = value; return 0; }
  if (k == "resnet_chunk" && value >= 0) { o.resnet_chunk = value; return 0; }
  if (k == "bert_qkv_attn" && (value == 0 || value == 1 || (probe && (value == 2 || value == 3)))) {
    o.bert_qkv_attn = value;
    return 0;
  }
  if (k == "stem_debug" && (value == 0 || (probe && (value == 1 || value == 2 || value == 4 || value == 7)))) {
    o.stem_debug = value;
    return 0;
  }
  if (k == "pw_chain" && (value >= 0 && value <= 2)) { o.pw_chain = value; return 0; }
  if (k == "pw_chain_form" && (value >= 0 && value <= 2)) { o.pw_chain_form = value; return 0; }
  if (k == "pw_chain_x3" && (value >= 0 && value <= 2)) { o.pw_chain_x3 = value; return 0; }
  if (k == "pw_seam_x3" && (value >= 0 && value <= 2)) { o.pw_seam_x3 = value; return 0; }
  if (k == "bert_qkv_attn_x3_heads" && (value == 1 || value == 2)) { o.bert_qkv_attn_x3_heads = value; return 0; }
  if (k == "bert_qkv_attn_heads" && (value == 1 || value == 2)) { o.bert_qkv_attn_heads = value; return 0; }
  if (k == "conv3x3_debug" && (value == 0 || (probe && (value == 1 || value == 2 || value == 4 || value == 7)))) {
    o.conv3x3_debug = value;
    return 0;
  }
  if (k == "speech_debug" && (value == 0 || (probe && value == 1))) {
    o.speech_debug = value;
    return 0;
  }
  if (k == "audio_debug" && (value == 0 || (probe && (value == 1 || value == 2 || value == 4 || value == 8 || value == 15 ||
                                                       value == 32 || value == 64 || value == 96 || value == 128)))) {
    o.audio_debug = value;
    return 0;
  }
  auto tile_ok = [](int id) { return id == 0 || gemm_tile(id); };  // 0 = autotune, else a catalogued tile (gemm_tiles.h)
  if (k == "gemm_bn" && tile_ok(value)) {
    o.gemm_bn = value;
    return 0;
  }
  // one launch class only: value = tag * 100000 + tile id (tags: mec_common.h KernelTag)
  if (k == "gemm_bn_tag" && value >= 0 && value / 100000 > 0 && value / 100000 < TAG_COUNT && tile_ok(value % 100000)) {
    o.gemm_bn_tag[value / 100000] = value % 100000;
    return 0;
  }
  if (k == "gemm_x3_tag" && value >= 0 && value / 100000 > 0 && value / 100000 < TAG_COUNT &&
      (value % 100000 == 0 || gemm_tile_x3i(value % 100000))) {
    o.gemm_x3_tag[value / 100000] = value % 100000;
    return 0;
  }
  set_error("mec_set_option: unknown key or bad value: " + k + " = " + std::to_string(value) +
            (probe ? "" : " (probe values need a -DMEC_PROBES build)"));
  return -1;
}
}  // namespace mec

extern "C" {

int mec_set_option(const char* key, int value) { return set_option(default_options(), key ? key : "", value); }

int mec_model_set_option(mec_model* m, const char* key, int value) {
  if (!m || !m->impl) { set_error("null model handle"); return -1; }
  const std::string k = key ? key : "";
  if (k == "gemm_x3_order" && value == 0 && m->impl->kind == KIND_TEXT &&
      static_cast<TextModel*>(m->impl)->x3_paired) {
    set_error("mec_model_set_option: this text handle's planes are paired (x3_layout 1), which the pass-major term "
              "order does not read; create it with x3_layout=0 or gemm_x3_order=0");
    return -1;
  }
  if (k == "x3_plane_scale" || k == "x3_headroom" || k == "x3_layout") {  // read while the weights are packed: too late here
    set_error("mec_model_set_option: \"" + k + "\" is a creation-time option (pass it to mec_create_opt, or set "
              "the process default with mec_set_option before mec_create_ex)");
    return -1;
  }
  return set_option(m->impl->opts, k, value);
}

int mec_build_flags(void) { return kProbes ? MEC_BUILD_PROBES : 0; }

int mec_model_gemm_query(mec_model* m, int amode, int M, int N, int K) {
  if (!m || !m->impl) { set_error("null model handle"); return -1; }
  OptScope sc(&m->impl->opts, &m->impl->tune);
  return m->impl->prec == PREC_FP32 ? gemm_f32_tuned(amode, M, N, K) : gemm_tuned_bn(amode, M, N, K);
}

int mec_gemm_query(int amode, int M, int N, int K) { return gemm_tuned_bn(amode, M, N, K); }

int mec_gemm_f32_query(int amode, int M, int N, int K) { return gemm_f32_tuned(amode, M, N, K); }

int mec_precision(const mec_model* m) {
  if (!m || !m->impl) { set_error("null model handle"); return -1; }
  return m->impl->prec;
}

int mec_gemm_f32(const float* A, const float* B, const float* bias, const float* R, float* C, int M, int N, int K,
                 int act, void* stream) {
  API_GUARD({
    GemmParams g;
    g.A = A; g.B32 = B; g.bias = bias; g.R = R; g.r_f32 = 1; g.C32 = C; g.M = M; g.N = N; g.K = K; g.act = act;
    return launch_gemm_f32(g, S(stream), nullptr, TAG_NONE);
  })
}

int mec_conv_f32(const float* x, const float* w, const float* bias, const float* R, float* y, int n, int H, int W,
                 int C, int Cout, int ks, int stride, int pad, int act, void* stream) {
  API_GUARD({
    GemmParams g;
    g.amode = A_CONV; g.A = x; g.B32 = w; g.bias = bias; g.R = R; g.r_f32 = 1; g.C32 = y; g.act = act;
    g.H = H; g.W = W; g.C = C; g.ks = ks; g.stride = stride; g.pad = pad;
    MEC_TRY(set_conv_geometry(g, n));
    g.N = Cout; g.K = ks * ks * C;
    return launch_gemm_f32(g, S(stream), nullptr, TAG_NONE);
  })
}

int mec_prof_enable(mec_model* m, int tag) {
  if (!m || !m->impl) { set_error("null model handle"); return -1; }
  m->impl->prof.tag = tag;
  m->impl->prof.reset();
  return 0;
}

int mec_model_check(mec_model* m) {
  if (!m || !m->impl) { set_error("mec_model_check: null handle"); return -1; }
  return m->impl->check();
}

int mec_prof_read(mec_model* m, double* total_ms, int* count) {
  if (!m || !m->impl || !total_ms || !count) { set_error("mec_prof_read: bad args"); return -1; }
  return m->impl->prof.read(total_ms, count);
}

}  // extern "C"
