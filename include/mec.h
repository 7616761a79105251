/*
 * mec.h — C ABI of libmec_hip.so, the MI355X (gfx950) batched tri-modal emotion
 * inference path. Drop-in boundary for the reference's inference/ classes
 * (RachaCodez/multimodal-emotion-classification); see INTEGRATION.md for the Python
 * (ctypes) binding the reference-side classes use.
 *
 * Conventions
 *   - Every data pointer is a DEVICE pointer owned by the caller; row-major, contiguous.
 *   - Calls are asynchronous on `stream` (a hipStream_t; NULL = default stream).
 *   - Return 0 on success, -1 on failure; mec_last_error() (thread-local) says why.
 *   - A model handle owns its packed device weights and a grow-only workspace; it may be
 *     used by one host thread at a time.
 *   - Host weight blobs are fp32, in the canonical order of mec/synthetic.py:spec(kind),
 *     i.e. the reference's own state_dict / Keras layer order.
 */
#ifndef MEC_H_
#define MEC_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mec_model mec_model;

enum { MEC_SPEECH = 0, MEC_TEXT = 1, MEC_IMAGE = 2, MEC_FUSION = 3, MEC_IMAGE_MBV2 = 4, MEC_AUDIO = 5, MEC_TEXT_LSTM = 6 };
/* MEC_IMAGE is the reference's ResNet50 image model (inference/image_inference.py:55-65);
 * MEC_IMAGE_MBV2 the same head on a torchvision mobilenet_v2 backbone (README.md:13 names
 * MobileNetV2; blob = state_dict order of mec/synthetic.py:image_mbv2_spec). Both kinds are
 * accepted by mec_image_fwd / mec_image_fwd_u8.
 * MEC_TEXT_LSTM is the reference's second text model, the Keras BiLSTM of
 * model_training/train_lstm_text_model.py:96-120 (blob = Keras layer order of
 * mec/synthetic.py:text_lstm_spec; the embedding has 10000 rows, smaller trained vocabularies zero-padded). */

/* Version / diagnostics. */
const char* mec_version(void);
const char* mec_last_error(void);

/* Number of fp32 values the host blob for `kind` must hold (-1 if kind is unknown). */
long long mec_blob_size(int kind);

/* Create a model of `kind` on `device` from a host fp32 blob of `n` floats.
 * Replaces the per-request model loads of the reference:
 *   speech  tf.keras.models.load_model + joblib scaler   inference/speech_inference.py:21-28
 *   text    BertForSequenceClassification.from_pretrained inference/text_inference.py:40-43
 *   image   _build_model + load_state_dict               inference/image_inference.py:35-40
 *           (MEC_IMAGE_MBV2: the same with base = mobilenet_v2, base.classifier = the head)
 *   fusion  _build_fusion_model + load_state_dict        inference/multimodal_fusion.py:43-56
 *   text (BiLSTM)  tf.keras load_model                   inference/text_lstm_inference.py:35-36 */
int mec_create(int kind, const float* host_blob, size_t n, int device, mec_model** out);

/* Arithmetic of a handle. MEC_PREC_F16 (mec_create's default, the fast path): BERT and the
 * image backbones on f16 MFMA operands with fp32 accumulation, LayerNorm, softmax, GELU,
 * residual stream and heads; outside the north_star's 1e-3 / argmax-exact contract margin (text
 * probs within 8.2e-4 of the oracle on the bench batch, rows with a smaller top-2 margin can flip:
 * INTEGRATION.md). MEC_PREC_FP32: every operand and product in fp32
 * (v_mfma_f32_32x32x2_f32, an exact fmaf chain), the precision the reference computes in
 * (inference/text_inference.py:91-93, inference/image_inference.py:116-118).
 * MEC_PREC_FP32X3 (BERT, ResNet50, MobileNetV2): the fp32 path's arithmetic with every GEMM / conv
 * operand carried as a pair of f16 planes (x = hi + lo) and each product as hi.hi + hi.lo + lo.hi
 * on the f16 MFMA into one fp32 accumulator; LayerNorm, softmax, attention, GELU, depthwise convs,
 * residual stream and heads fp32. Envelope: weights are split after a per-matrix power-of-two
 * pre-scale (22 significant bits each); each activation tensor is split at a power-of-two plane
 * scale 2^s fixed at creation (hi = f16(x 2^s), lo = f16(x 2^s - hi); the consumer's epilogue folds
 * in 2^-s, exactly): from rigorous bounds for BERT (LayerNorm outputs and their projections: no
 * plane can overflow) and from the BatchNorm parameters for ResNet50 / MobileNetV2 (64x headroom
 * over a 6-sigma estimate), so the planes hold 22 significant bits for the tensor's whole working
 * range (INTEGRATION.md "fp32x3 envelope"). A plane value at |x 2^s| >= 65520 (activations far above
 * what the BN parameters predict) or a NaN / inf raises the handle's range flag and mec_model_check
 * fails. Speech, fusion, audio and BiLSTM text handles are fp32 at every setting. */
enum { MEC_PREC_F16 = 0, MEC_PREC_FP32 = 1, MEC_PREC_FP32X3 = 2 };
int mec_create_ex(int kind, const float* host_blob, size_t n, int device, int precision, mec_model** out);
/* mec_create_ex with this handle's own knobs, "key=value[,key=value...]" (the keys of mec_set_option),
 * applied over the process defaults BEFORE the weights are packed; NULL or "" = the defaults. The
 * creation-time knobs live here: "x3_headroom" 0..24 [0] (fp32x3: every activation-plane exponent chosen
 * for 2^-x3_headroom of the default target, i.e. that many binades more room above the bound / BN
 * estimate before the range flag trips; the Python engine re-creates a handle with +8 after a trip, once
 * the batch has been re-run on an MEC_PREC_FP32 handle) and "x3_plane_scale". Same semantics as the
 * reference's model loads (see mec_create). */
int mec_create_opt(int kind, const float* host_blob, size_t n, int device, int precision, const char* opts,
                   mec_model** out);
/* fp32x3 handles: the activation-plane exponents chosen at creation, one line per tensor (group),
 * "name s=<exponent> bound=<rigorous bound or BN estimate>", after a first line with the creation knobs;
 * "" for other precisions, NULL on a null handle. Owned by the handle (valid until mec_destroy). For
 * diagnosing a range-flag failure (mec_model_check returning MEC_ERR_X3_RANGE). */
const char* mec_model_x3_report(mec_model* m);

/* Calibration of the image kinds' fp32x3 plane exponents (MEC_IMAGE, MEC_IMAGE_MBV2) from observed data. By
 * default those exponents come from a BatchNorm estimate (above); a checkpoint whose activations do not follow
 * it either trips the range flag or sits far below the planes' 2^-3 floor unnoticed. The tensors concerned are
 * the lines of mec_model_x3_report, in its order: ResNet50's 37 ("stem", then per stage "layerN.out" and per
 * block "layerN.k.conv1", "layerN.k.conv2"), MobileNetV2's 7 ("featuresA-B.out"); "layerN.out" and
 * "featuresA-B.out" stand for every block output of the stage, which share one exponent.
 *   1. mec_model_x3_observe(m32, 1) on an MEC_PREC_FP32 handle m32 of the same kind and weights: allocates and
 *      zeroes one slot per tensor and arms the forward's taps (synchronizes the device). Returns the tensor
 *      count n. While armed, every forward of m32 reduces each of those tensors to max |x| on its stream (one
 *      small HBM-bound launch per tensor) into the tensor's slot; a slot keeps the running maximum over all
 *      forwards since it was armed. The forward's outputs are the same bits armed or not.
 *      mec_model_x3_observe(m32, 0) disarms (no launch is added to a forward; the slots stay readable) and
 *      returns n as well. -1 for any other handle.
 *   2. mec_model_x3_observed(m32, absmax, cap): synchronizes the device and copies the n maxima in report order
 *      to the host array absmax (cap >= n entries); returns n, -1 if the handle was never armed or cap < n. A
 *      tensor that held an inf or a NaN reads +inf. mec_model_x3_names(m): the n names, one per line, for any
 *      handle of the two kinds (owned by the handle; NULL on error).
 *   3. mec_create_x3_calibrated(kind, blob, n, device, opts, absmax, count, &m): an MEC_PREC_FP32X3 handle
 *      exactly as mec_create_opt creates it, except that a tensor with absmax[i] > 0 takes its exponent from
 *      that observed maximum in place of the estimate, against the same target (2^10: 64x headroom to the f16
 *      range, kept because a calibration batch is a sample of the data; "x3_headroom" applies on top).
 *      absmax[i] == 0 (a dead tensor) keeps the estimate. Epilogue scales, scaled biases and the dual GEMM's
 *      pre-scale follow from the exponents as always. Its mec_model_x3_report has "x3_calibrated=1" on the
 *      first line and the observed value as the line's bound=. Returns -1 before any device call for a kind
 *      other than the two, count != n, a null absmax or out, and a negative, NaN or inf value. */
int mec_model_x3_observe(mec_model* m, int on);
int mec_model_x3_observed(mec_model* m, float* absmax_host, int cap);
const char* mec_model_x3_names(mec_model* m);
int mec_create_x3_calibrated(int kind, const float* host_blob, size_t n, int device, const char* opts,
                             const float* absmax, int count, mec_model** out);
/* The taps' reduction on its own: max |x| over n floats at x_dev (device, 4-byte aligned) -> *out_host, +inf
 * if any is an inf or a NaN; synchronizes `stream`. n == 0 gives 0.0 without a launch. The maximum is taken
 * on the bit patterns, so it is exact and the same at any launch geometry. */
int mec_absmax_f32(const float* x_dev, long long n, float* out_host, void* stream);
/* The handle's precision (MEC_PREC_*), -1 on a null handle. */
int mec_precision(const mec_model* m);
int mec_destroy(mec_model* m);

/* Speech DNN. x: raw (pre-scaler) features f32[B,56]. Outputs feat f32[B,64] (block-5
 * ReLU = layers[-3]), logits f32[B,7], probs f32[B,7].
 * Replaces SpeechInference.predict / extract_features model arithmetic
 *   inference/speech_inference.py:66-69, :86-103. */
int mec_speech_fwd(mec_model* m, const float* x, int B, float* feat, float* logits, float* probs,
                   void* stream);

/* BERT-base text encoder + classifier. ids/mask int32[B,L] with L == 128
 * (padding='max_length'). Outputs cls f32[B,768] (last_hidden_state[:,0]), logits,
 * probs f32[B,7]. Replaces TextInference.predict / extract_features model arithmetic
 *   inference/text_inference.py:87-94, :119-128. */
int mec_text_fwd(mec_model* m, const int32_t* ids, const int32_t* mask, int B, int L, float* cls,
                 float* logits, float* probs, void* stream);

/* Sentence packing for the BERT text path: short sentences share 128-slot rows, so a batch of B
 * sentences runs the encoder over Bp <= B rows. The plan is made on the host (where the tokenizer's
 * lengths are) by first-fit decreasing: samples are visited by length descending, ties by ascending
 * index; each goes to the lowest-numbered row whose free space is at least its length, at that row's
 * fill at that moment (its off); a new row is opened when none has room.
 * lens int32[B] on the HOST, each in [1,128]. Writes row[B], off[B] (host) and returns the number of
 * packed rows Bp (0 for B == 0), -1 on error (null pointer, B < 0, a length outside [1,128]). Uses no
 * GPU. No reference counterpart (the reference pads every sentence to 128, text_inference.py:81-83). */
int mec_text_pack_plan(const int32_t* lens, int B, int32_t* row, int32_t* off);

/* mec_text_fwd on a packed batch. ids int32[B,128] (device, the padded layout mec_text_fwd takes: a
 * sentence's len tokens first); row/off/len int32[B] (device), a plan as above with Bp rows. Sample i's
 * tokens occupy slots off[i] .. off[i]+len[i]-1 of row row[i]; position ids restart at 0 in every
 * sentence and a key counts only for the queries of its own sentence (a block-diagonal attention
 * mask), so every sample's outputs are those of mec_text_fwd with a prefix mask of len[i] ones, to the
 * precision's rounding (the key's slot changes the MFMA summation grouping, not the terms; a plan with
 * Bp == B and every off == 0 gives the same bits). Unused slots form a segment of their own and no
 * output reads them. Outputs in the caller's sample order, as mec_text_fwd: cls f32[B,768], logits,
 * probs f32[B,7]. B == 0 returns 0 without a launch. Returns -1 before any launch for a null pointer,
 * a handle of another kind, Bp < 1 with B > 0, or Bp > B. The library TRUSTS the contents of the
 * device-side plan (it cannot read them without a synchronization): indices are clamped to the
 * workspace, so a plan that overlaps sentences or leaves gaps yields wrong outputs, not an error.
 * Honours bert_qkv_attn, bert_qkv_attn_heads / bert_qkv_attn_x3_heads and bert_cls_last like
 * mec_text_fwd; the GEMM shapes (and so the autotuned tiles) follow Bp, not B. */
int mec_text_fwd_packed(mec_model* m, const int32_t* ids, const int32_t* row, const int32_t* off,
                        const int32_t* len, int B, int Bp, float* cls, float* logits, float* probs, void* stream);

/* BiLSTM text model (MEC_TEXT_LSTM handle). ids int32[B,L] with L == 128, post-padded and
 * post-truncated with id 0 (pad_sequences(padding='post', truncating='post')); the embedding has no
 * mask_zero, so pad positions run through the LSTMs like any token. ids outside [0, 10000) are clamped.
 * Outputs feat f32[B,64] (the Dense-64 ReLU) or NULL, logits f32[B,7] or NULL, probs f32[B,7].
 * B == 0 returns 0 and launches nothing; a null handle, a handle of another kind or L != 128 returns -1
 * before any launch. fp32 throughout (no f16 anywhere), a row's bits independent of B and of its
 * position in the batch. Replaces FastTextEmotionPredictor.predict / predict_batch model arithmetic
 *   inference/text_lstm_inference.py:66, :106. */
int mec_text_lstm_fwd(mec_model* m, const int32_t* ids, int B, int L, float* feat, float* logits, float* probs,
                      void* stream);

/* Tokenization on the GPU for both text paths: UTF-8 bytes in, ids / mask / len on the device. A
 * tokenizer is an object of its own (not a mec_model): its creation data is a vocabulary, not an fp32 blob.
 * The vocabulary is given on the HOST as n entries, entry e = the bytes pool[off[e] .. off[e+1]) -> id[e];
 * creation builds an open-addressing hash table over them (load factor <= 1/2) and uploads it with the
 * byte pool. A hash hit is always confirmed by comparing the bytes, so a collision never yields a wrong id.
 *
 * MEC_TOK_KERAS restates keras Tokenizer.texts_to_sequences + pad_sequences(padding='post',
 * truncating='post') as the BiLSTM path calls them (inference/text_lstm_inference.py:61-62), on the bytes
 * of the already lower-cased text: words are the maximal runs of bytes b with delim[b] == 0; each word in
 * order writes its id when it is in the table, else oov_id when oov_id >= 0, else nothing; stop after L
 * ids, fill the row with 0; len = ids written, mask[j] = j < len.
 *
 * MEC_TOK_WORDPIECE restates transformers 4.30's BertTokenizer (BasicTokenizer + WordpieceTokenizer,
 * text_inference.py:78-85) for 7-BIT input (the caller keeps other texts on the host): bytes 0x00,
 * 0x01-0x1F other than \t \n \r, and 0x7F are dropped; \t \n \r and space separate words; A-Z folds to a-z
 * when `lower`; every punctuation byte (33-47, 58-64, 91-96, 123-126) is a word of its own; a word longer
 * than max_word is unk_id, else greedy longest-match-first, plain entries at word position 0 and, later in
 * the word, entries whose pool form starts with "##" (the prefix is stripped into a flag at creation); a
 * word with an unmatched position is one unk_id. The row is cls_id, the first L-2 pieces, sep_id, then
 * pad_id; len counts cls_id and sep_id, mask[j] = j < len.
 *
 * MEC_TOK_WORDPIECE_UTF8 (mec_tok_create_utf8) is MEC_TOK_WORDPIECE for any well-formed UTF-8 text, for a
 * lower-casing, accent-stripping BERT tokenizer, whose Unicode handling is one table look-up per code point
 * (mec_tok_cpmap below). The text is decoded code point by code point. A code point below 0x80 follows the
 * 7-bit rules above (`lower` included), so a 7-bit text gets the row MEC_TOK_WORDPIECE gives it. Any other
 * code point acts by its class: DROP vanishes (its neighbours join); SPACE ends the word; CHAR appends the
 * code point's own UTF-8 bytes to the word; PUNCT ends the word and is a word of its own; MAPPED stands for
 * its 0 to 3 output code points in order, each of which is appended to the word or, when its own class is
 * PUNCT (below 0x80: when it is a punctuation byte), ends the word and is a word of its own. With the
 * ISOLATE flag the word ends before and after the code point, so that its output is a word of its own. A
 * word that ends up empty emits nothing. max_word counts the word's output CHARACTERS, not bytes: a word of
 * more is unk_id. Matching, cls_id, the first L-2 pieces, sep_id, pad_id, mask and len are as for
 * MEC_TOK_WORDPIECE, on the word's bytes. The table holds every entry, which must be well-formed UTF-8.
 * Byte-level matching never splits a character: a piece starts on a character boundary (the word's start,
 * or the end of the piece before it), and from a boundary a well-formed entry can only equal whole
 * characters, since each lead byte fixes its character's length; so it ends on a boundary too.
 * A row whose text holds an UNCOVERED code point or ill-formed UTF-8 anywhere (an overlong form, a
 * surrogate, a value above 0x10FFFF, a sequence cut off by the text's end, a stray continuation byte, a
 * byte that no sequence holds) is pad_id throughout with mask 0 and len = -1: never a guess, and never an
 * access outside the text. */
typedef struct mec_tokenizer mec_tokenizer;
enum { MEC_TOK_KERAS = 0, MEC_TOK_WORDPIECE = 1, MEC_TOK_WORDPIECE_UTF8 = 2 };
typedef struct mec_tok_desc {
  int kind;             /* MEC_TOK_KERAS, MEC_TOK_WORDPIECE or MEC_TOK_WORDPIECE_UTF8 */
  const uint8_t* pool;  /* HOST: the entries' bytes, back to back */
  const int64_t* off;   /* HOST: n + 1 monotone offsets into pool, off[0] >= 0 */
  const int32_t* id;    /* HOST: n ids, each >= 0 */
  int n;
  uint8_t delim[256];   /* KERAS: 1 = this byte separates words */
  int oov_id;           /* KERAS: id written for a word not in the table; -1 = such words are dropped */
  int lower;            /* WORDPIECE (both kinds from here on): fold A-Z to a-z */
  int unk_id, cls_id, sep_id, pad_id; /* WORDPIECE */
  int max_word;         /* WORDPIECE: 1..128 (transformers: 100) */
} mec_tok_desc;
/* Returns -1 (mec_last_error says why) for a null pointer, an unknown kind, n < 0, non-monotone off, an
 * entry longer than 65535 bytes, a duplicate entry, an id < 0, oov_id < -1 and, WORDPIECE only, an entry
 * holding a byte >= 0x80, a special id < 0 or max_word outside 1..128. Nothing of the descriptor is
 * referenced after the call returns. */
int mec_tok_create(const mec_tok_desc* d, int device, mec_tokenizer** out);
/* The code-point table of MEC_TOK_WORDPIECE_UTF8, HOST arrays. cls[cp] = a class in the low 3 bits, or'ed
 * with MEC_CP_ISOLATE; entries 0..127 are ignored (the 7-bit rules hold there). The MAPPED code points are
 * listed in map_cp, ascending, with the outputs of map_cp[i] at map_out[map_off[i] .. map_off[i+1]). */
enum { MEC_CP_UNCOVERED = 0, MEC_CP_DROP = 1, MEC_CP_SPACE = 2, MEC_CP_CHAR = 3, MEC_CP_PUNCT = 4, MEC_CP_MAPPED = 5,
       MEC_CP_ISOLATE = 8 };
typedef struct mec_tok_cpmap {
  const uint8_t* cls;     /* HOST: 0x110000 entries */
  const int32_t* map_cp;  /* HOST: n_map code points >= 0x80, strictly ascending, exactly those of class MAPPED */
  const int32_t* map_off; /* HOST: n_map + 1 offsets into map_out, map_off[0] = 0, 0..3 outputs each */
  const int32_t* map_out; /* HOST: the outputs; each of class CHAR or PUNCT, or a 7-bit word character or
                             punctuation byte (A-Z is folded when the descriptor's `lower` is set) */
  int n_map;
} mec_tok_cpmap;
/* d->kind must be MEC_TOK_WORDPIECE_UTF8. Returns -1 for everything mec_tok_create rejects (an entry with a
 * byte >= 0x80 is fine here, an entry that is not well-formed UTF-8 is not) and for a null pointer in m, a
 * class above MAPPED, a surrogate or a value >= 0x110000 that is not UNCOVERED, a map_cp that is not
 * strictly ascending, below 0x80 or not of class MAPPED, a MAPPED code point that map_cp lacks, more than 3
 * outputs, and an output that is not of class CHAR or PUNCT (below 0x80: that the 7-bit rules drop or treat
 * as whitespace). Creation folds cls and the map into a two-stage table (an index by cp >> 7 into shared
 * 128-entry blocks, the outputs as UTF-8 bytes with their punctuation flags) and uploads it with the
 * vocabulary table as one allocation. mec_tok_encode and mec_tok_destroy serve the tokenizer as any other. */
int mec_tok_create_utf8(const mec_tok_desc* d, const mec_tok_cpmap* m, int device, mec_tokenizer** out);
/* text u8 and text_off int64[B+1] are DEVICE pointers: text i is the bytes text[text_off[i] ..
 * text_off[i+1]), and text_off[B] is the blob's size. Outputs (device) ids int32[B,L], mask int32[B,L] or
 * NULL, len int32[B] or NULL; 1 <= L <= 512 (both WORDPIECE kinds: 2 <= L). B == 0 returns 0 without a launch; a null
 * tokenizer, text, text_off or ids, B < 0 or L out of range return -1 before any launch. Asynchronous on
 * `stream`; allocates nothing, never synchronizes, can be captured into a hipGraph. The library TRUSTS the
 * offsets (it cannot read them without a synchronization) and clamps them: every offset into
 * [0, text_off[B]] and a text's end to at least its start, so wrong offsets give wrong ids for that row,
 * never an access outside text[0 .. text_off[B]). One wave per text; a row's output depends on neither B
 * nor the row's position. Cost: linear in the text's bytes (DESIGN.md §4.12 states the bound). */
int mec_tok_encode(mec_tokenizer* t, const uint8_t* text, const int64_t* text_off, int B, int L, int32_t* ids,
                   int32_t* mask, int32_t* len, void* stream);
int mec_tok_destroy(mec_tokenizer* t);

/* ResNet50 image encoder + head. gray: u8[B,48,48]; the PIL RGB/resize/ToTensor/Normalize
 * transform runs on the GPU. Outputs feat f32[B,512] (fc[2]), logits, probs f32[B,7].
 * Replaces ImageInference.predict / extract_features (after Image.open)
 *   inference/image_inference.py:112-119, :137-144. */
int mec_image_fwd(mec_model* m, const uint8_t* gray, int B, float* feat, float* logits, float* probs,
                  void* stream);

/* Generic image entry: img u8[B,H,W,C] in one of
 *   (48,48,1)    FER2013 gray, resized on the GPU (same as mec_image_fwd),
 *   (224,224,1)  gray already resized by PIL on the host (any input size),
 *   (224,224,3)  RGB already resized by PIL on the host (colour inputs).
 * Replaces ImageInference.predict for arbitrary image files (image_inference.py:112-113). */
int mec_image_fwd_u8(mec_model* m, const uint8_t* img, int B, int H, int W, int C, float* feat, float* logits,
                     float* probs, void* stream);

/* Attention-MLP fusion. Outputs logits/probs f32[B,7], attn_w/dec_w f32[B,3].
 * Replaces MultimodalFusion.fuse_with_attention  inference/multimodal_fusion.py:201-239. */
int mec_fusion_fwd(mec_model* m, const float* s_feat, const float* t_feat, const float* i_feat,
                   const float* s_pred, const float* t_pred, const float* i_pred, int B, float* logits,
                   float* probs, float* attn_w, float* dec_w, void* stream);

/* Mixed-modality batches: B requests, each with any subset of {speech, text, image}, fused in one call
 * that routes every row as MultimodalFusion.predict_multimodal routes one request
 * (inference/multimodal_fusion.py:244-283). Each encoder runs once over the compact rows that have its
 * modality; the fusion call reads them through index arrays (no gather or scatter copies).
 *
 * The plan is made on the host. present[b] is an or of the MEC_MOD_* bits of sample b. Compact order is
 * ascending sample index: x_idx[b] (x = s, t, i) is the number of samples before b that have modality x,
 * or -1 when sample b lacks it; counts = {ns, nt, ni}, the samples that have each modality. route[b] is
 * MEC_ROUTE_NONE for no bit, MEC_ROUTE_SINGLE for one, MEC_ROUTE_AVERAGE for two and, when have_model == 0,
 * for three, MEC_ROUTE_ATTENTION for three when have_model != 0. att holds the MEC_ROUTE_ATTENTION samples in
 * ascending order, then -1 up to B. All arrays are on the HOST with B entries (counts 3). Returns n_att, the
 * number of attention samples (0 for B == 0, which touches no array but counts, zeroed when given); -1 on
 * error: B < 0, a null pointer with B > 0, a present value above 7. Uses no GPU. */
enum { MEC_MOD_SPEECH = 1, MEC_MOD_TEXT = 2, MEC_MOD_IMAGE = 4 };
enum { MEC_ROUTE_NONE = 0, MEC_ROUTE_SINGLE = 1, MEC_ROUTE_AVERAGE = 2, MEC_ROUTE_ATTENTION = 3 };
int mec_fusion_mixed_plan(const uint8_t* present, int B, int have_model, int32_t* s_idx, int32_t* t_idx,
                          int32_t* i_idx, int32_t* route, int32_t* att, int32_t counts[3]);

/* The fusion step of a mixed batch. m: a MEC_FUSION handle, or NULL (no attention model: the plan was made
 * with have_model == 0). Per sample b, with "present" meaning x_idx[b] >= 0:
 *   attention  all three present and m != NULL (the samples att lists): the fusion model on
 *              s_feat[s_idx[b]], t_feat[t_idx[b]], ... writes logits, attn_w, dec_w at row b and its float32
 *              probs, widened to double (exact), at fused[b]. Bit-identical to mec_fusion_fwd on the same
 *              rows gathered densely at the same "fusion_r" / "fusion_split": the kernels keep one
 *              accumulator set per row, so a row's bits depend on neither its group-mates nor its slot.
 *   average    two present, or three with m == NULL: fused[b] = fuse_predictions of the row in float64, a
 *              missing modality as zeros (mec_fuse_weighted's arithmetic, one device function).
 *   single     fused[b] = that modality's probs widened to double.
 *   none       fused[b] = zeros.
 * Every row off the attention route gets zeros in logits, attn_w and dec_w: the call writes every element
 * of its four outputs, so callers need not clear them.
 * The index arrays and att are on the DEVICE. The library trusts them (as mec_text_fwd_packed trusts its
 * plan) but clamps every index into its array, x_idx to [-1, n_x - 1] and att entries to [0, B - 1]: a wrong
 * plan gives wrong rows, never an access outside the arrays.
 * B == 0 returns 0 without a launch. Returns -1 before any launch for: a null descriptor; with B > 0 a null
 * index array or output; a negative count or one above B; n_att > 0 with m == NULL or with att NULL;
 * n_att > min(ns, nt, ni); a handle of another kind; a compact array that is NULL while its count is > 0
 * (the three feature arrays may be NULL when m == NULL). Asynchronous on `stream`, no synchronization; its
 * only allocation is the handle's workspace. At most one launch beyond the attention model's own. */
typedef struct mec_fusion_mixed_args {
  const float *s_feat, *t_feat, *i_feat; /* compact f32 [ns,64] [nt,768] [ni,512] */
  const float *s_pred, *t_pred, *i_pred; /* compact f32 [ns,7] [nt,7] [ni,7] */
  int ns, nt, ni;
  const int32_t *s_idx, *t_idx, *i_idx; /* device int32[B], a plan as above */
  const int32_t* att;                   /* device int32[>= n_att] */
  int n_att;
  int B;
  double* fused;                 /* [B,7] the row's answer */
  float *logits, *attn_w, *dec_w; /* [B,7] [B,3] [B,3] */
} mec_fusion_mixed_args;
int mec_fusion_fwd_mixed(mec_model* m, const mec_fusion_mixed_args* a, void* stream);

/* Speech features on the GPU (MEC_AUDIO handle; blob = {sample_rate, 2048, 512, 128, n_mfcc},
 * i.e. config.py's SAMPLE_RATE / N_MFCC and librosa's n_fft / hop / n_mels). wave: f32[B, n]
 * fixed-length waveforms (load_audio's pad/trim applied). feat: f32[B, n_mfcc + 16] =
 * [mean MFCC | mean chroma (12) | mean zcr, centroid, rolloff, rms]; tuning: f32[B] (the
 * estimate_tuning value chroma used) or NULL. Replaces preprocess_audio's feature arithmetic
 *   preprocessing/audio_preprocessing.py:22-46 (librosa 0.10.0 mfcc / chroma_stft /
 *   zero_crossing_rate / spectral_centroid / spectral_rolloff / rms). */
int mec_audio_fwd(mec_model* m, const float* wave, int B, int n_samples, float* feat, float* tuning, void* stream);

/* Decode and resample a ragged batch of PCM clips into the waveforms mec_audio_fwd takes (csrc/audio_load.hip;
 * MEC_AUDIO handle, whose blob gives the target rate sr). What load_audio does per file on the host,
 *   librosa.load(path, sr=22050, duration=3) + pad/trim   preprocessing/audio_preprocessing.py:12-19
 * for audio that is already PCM: decode to float32 as libsndfile normalises it (U8 (x - 128) / 128, S16 x / 2^15,
 * S24 x / 2^23, S32 (float)x * 2^-31, F32 as stored), mean of two channels in float32, resample, and zeros up to
 * n_out or a cut at it. Clip i gives min(n_out, ceil(frames_i * (sr / rate_i))) samples (float64, as librosa
 * 0.10.0 resample computes it). A clip at the rate sr is copied: bit for bit the host's waveform.
 *
 * The resampler is this library's own (csrc/resample_design.h): a polyphase Kaiser-windowed sinc, passband to
 * 0.913 of the lower Nyquist, 125 dB design attenuation, float64 taps and accumulation and one rounding to
 * float32. It is held to that float64 definition; parity with librosa's soxr_hq is NOT pinned.
 *
 * mec_resample_on_gpu: 1 when rate_in -> rate_out is in the domain: both in 1 .. 192000, max(up, down) <= 8192
 * for the reduced ratio up / down, at most 2^21 taps, and one output cycle's input window within LDS (always so
 * for rate_out = 22050). mec_resample_plan: up, down and half (taps = 2 * half + 1; half = 0 is the identity
 * plan, rate_in == rate_out). mec_resample_taps: the n = 2 * half + 1 taps, unit sum. These three need no GPU.
 *
 * mec_audio_load_ragged: clip i is little-endian interleaved frames at byte offs[i] of the device buffer src
 * (src_bytes long), any byte alignment; desc (HOST, [B, 4]) = fmt, channels (1 or 2), rate, frames. wave: device
 * f32 [B, n_out]. Everything is checked on the host before any launch ("requirement failed:
 * mec_audio_load_ragged: clip <i> ..."). B == 0 returns 0 without a launch; frames == 0 gives a zero row. Tap
 * tables are built per rate on first use and cached on the handle (16 at most, least recently used dropped; a
 * call may name at most 16 distinct rates). Asynchronous on `stream`; not graph-capturable.
 * mec_audio_load_prof_*: hipEvent timing of the kernel, process-wide, as mec_resize_prof_*. */
enum { MEC_PCM_U8 = 0, MEC_PCM_S16 = 1, MEC_PCM_S24 = 2, MEC_PCM_S32 = 3, MEC_PCM_F32 = 4 };
int mec_resample_on_gpu(int rate_in, int rate_out);
int mec_resample_plan(int rate_in, int rate_out, int* up, int* down, int* half);
int mec_resample_taps(int rate_in, int rate_out, double* h, size_t n);
int mec_audio_load_ragged(mec_model* m, const uint8_t* src, const int64_t* offs, const int32_t* desc, int B,
                          size_t src_bytes, float* wave, int n_out, void* stream);
int mec_audio_load_prof_enable(int on);
int mec_audio_load_prof_read(double* ms, int* count);

/* Weighted-average fallback (float64, like numpy); any of s/t/i may be NULL (= zeros).
 * Replaces MultimodalFusion.fuse_predictions  inference/multimodal_fusion.py:184-199. */
int mec_fuse_weighted(const float* s_probs, const float* t_probs, const float* i_probs, int B,
                      double* out, void* stream);

/* Same with float64 inputs (per-request dicts carry Python floats, e.g. heuristic 0.1/6). */
int mec_fuse_weighted_f64(const double* s_probs, const double* t_probs, const double* i_probs, int B,
                          double* out, void* stream);

/* Kernel-level entry points (parity tests / microbenchmarks). */
int mec_resize_u8(const uint8_t* in, int B, int H, int W, uint8_t* out, int OH, int OW, void* stream);

/* PIL-exact bilinear resize of a ragged batch to 224 x 224 (csrc/resize.hip): what
 *   rgb.resize((224, 224), Image.BILINEAR)   inference/image_inference.py (the reference's Resize((224,224)))
 * gives, byte for byte, for every image of the domain
 *   1 <= H <= 4096, 1 <= W <= 4096, H <= 100 W          (mec_resize_on_gpu(H, W) != 0)
 * Pillow 12.2 resamples horizontally into a u8 intermediate, then vertically, and these kernels do the same;
 * for H > 100 W (and H > 224) Pillow's bytes are those of the other order, which is not restated: such an
 * image stays with the host.
 *
 * mec_resize_taps: Pillow's taps for one extent (precompute_coeffs + normalize_coeffs_8bpc, bilinear, in
 * double on the host): output i sums n[i] source samples from xmin[i] on, times k[i * kmax + j] / 2^22; the
 * taps past n[i] are 0. kmax >= 2 * ceil(max(in_size / out_size, 1)) + 1 (39 for 4096 -> 224). Host only: it
 * needs no GPU.
 *
 * mec_resize_ragged_u8: image i is u8 [H_i, W_i, C] (hw[2 i], hw[2 i + 1]) at byte offs[i] of the device
 * buffer src (src_bytes long); C is 1 or 3 for the whole batch. tmp (device, 4-byte aligned, tmp_bytes >= the
 * sum of H_i * 224 * C) takes the horizontal pass' result; out (device) is u8 [B, 224, 224, C]. offs and hw
 * are HOST arrays. Everything is checked on the host before any launch: a null pointer, B < 0, C, an image
 * outside the domain or not inside src_bytes, a short tmp, B > 65535 return -1 with a message and launch
 * nothing; B == 0 returns 0. The call builds (or takes from a bounded process-wide cache) the tap tables of the batch's
 * extents and uploads them with the descriptors itself, from a staging buffer it owns and re-uses once the
 * previous call's kernels have finished: it is asynchronous on `stream` but NOT capturable in a graph, and a
 * call may wait on the host for the previous one. */
int mec_resize_on_gpu(int H, int W);
int mec_resize_taps(int in_size, int out_size, int32_t* xmin, int32_t* n, int32_t* k, int kmax);
int mec_resize_ragged_u8(const uint8_t* src, const int64_t* offs, const int32_t* hw, int B, int C, size_t src_bytes,
                         uint8_t* tmp, size_t tmp_bytes, uint8_t* out, void* stream);
/* hipEvent timing of the two passes, process-wide (these calls have no handle): enable (on != 0) or disable
 * and forget what was recorded; read the totals of the calls since, in ms, and forget them. */
int mec_resize_prof_enable(int on);
int mec_resize_prof_read(double* horizontal_ms, double* vertical_ms, int* count);

/* Mode conversion and the gray test of a ragged batch in native pixel formats (csrc/image_canon.hip): what
 *   rgb = image.convert('RGB'); gray = (R == G).all() and (R == B).all()   inference/image_inference.py _route
 * give for Pillow's modes L, LA, RGB, RGBA and P, byte for byte: L and LA replicate L, RGBA drops alpha, P looks
 * each index up in getpalette('RGB') zero-padded to 256 entries (an RGBA palette or info['transparency'] does
 * not change the lookup). Image i is u8 [H_i, W_i, bpp(fmt[i])] at byte offs[i] of the device buffer src
 * (src_bytes long), packed as mec_resize_ragged_u8 takes it; any byte alignment. A MEC_PIX_P image names its
 * palette, 768 bytes (256 RGB entries, zero-padded by the caller) in the same buffer, by pal_off[i]; every other
 * format has pal_off[i] == -1. Images may share a palette. The domain is mec_resize_on_gpu's.
 *
 * mec_image_gray_ragged_u8: gray (device int32[B]) takes 1 where every pixel of image i has R == G == B after
 * conversion, else 0. L and LA are gray by definition; a P image is gray when no index byte selects a coloured
 * palette entry (an unused coloured entry does not count); RGBA's alpha does not count.
 *
 * mec_image_canon_ragged_u8: c_out[i] == 3 writes image i converted to RGB, u8 [H_i, W_i, 3], at dst +
 * dst_offs[i]; 1 writes its R channel, u8 [H_i, W_i, 1] (for an image known to be gray; L -> 1 is a copy, which
 * gathers 48 x 48 faces into one batch); 0 writes nothing. dst (device, 16-byte aligned, dst_bytes long) may
 * lie in the allocation of src, so that one mec_resize_ragged_u8 call reads untouched and converted images
 * through one pointer: a written range may overlap no image or palette of the batch (whatever its c_out) and
 * no other written range. dst_offs are multiples of 16. Nothing outside the written ranges is touched.
 *
 * offs, hw, fmt, pal_off, c_out and dst_offs are HOST arrays. Everything is checked on the host before any
 * launch: a null pointer, B < 0, B > 65535, an unknown fmt, an image outside the domain, an image or palette
 * not inside src_bytes, a P image without a palette or a palette on another format, c_out outside {0, 1, 3}, a
 * misaligned or out-of-range dst_off and overlapping ranges return -1 with a message and launch nothing; B == 0
 * returns 0. Each call uploads its descriptors itself from a staging buffer it owns and re-uses once the previous
 * call's kernels have finished: asynchronous on `stream`, NOT capturable in a graph. */
enum { MEC_PIX_L = 0, MEC_PIX_LA = 1, MEC_PIX_RGB = 2, MEC_PIX_RGBA = 3, MEC_PIX_P = 4 };
int mec_image_gray_ragged_u8(const uint8_t* src, const int64_t* offs, const int32_t* hw, const int32_t* fmt,
                             const int64_t* pal_off, int B, size_t src_bytes, int32_t* gray, void* stream);
int mec_image_canon_ragged_u8(const uint8_t* src, const int64_t* offs, const int32_t* hw, const int32_t* fmt,
                              const int64_t* pal_off, const int32_t* c_out, const int64_t* dst_offs, int B,
                              size_t src_bytes, uint8_t* dst, size_t dst_bytes, void* stream);
/* hipEvent timing of the gray kernel and the conversion kernel, process-wide, as mec_resize_prof_*; a call that
 * launches no such kernel (only L / LA images; every c_out 0) is not counted. */
int mec_image_canon_prof_enable(int on);
int mec_image_canon_prof_read(double* gray_ms, int* gray_count, double* canon_ms, int* canon_count);

/* Baseline JPEG decoding of a ragged batch (csrc/jpeg.hip, csrc/jpeg_probe.h): what
 *   Image.open(file).load()   with Pillow 12.2 on libjpeg-turbo (slow-integer IDCT, fancy upsampling)
 * gives, byte for byte, for every file of the domain below; every other file stays with the host.
 *
 * mec_jpeg_probe: host only, needs no GPU, safe on arbitrary bytes (every read is bounds-checked). Returns 1 and
 * fills *desc for a file the GPU decodes, 0 for a file the host decodes (*desc untouched), -1 for a null data or
 * desc, seg_cap < 0, or segs null with seg_cap > 0. On the GPU iff all of: SOI; exactly one frame, SOF0, 8-bit;
 * exactly one SOS naming all the frame's components in frame order with Ss = 0, Se = 63, Ah = Al = 0; only SOF0,
 * DHT, DQT, DRI, APPn other than APP14 and COM segments before it (so no DNL, no Adobe segment, no arithmetic
 * conditioning); one component sampled 1 x 1 (Pillow's L), or components 1, 2, 3 with chroma 1 x 1 and luma
 * 1 x 1, 2 x 1 or 2 x 2 (Pillow's RGB through YCbCr); 8-bit quantization tables; Huffman table ids 0 or 1 whose
 * counts give canonical codes that fit (as libjpeg requires); every table the scan names defined before SOS;
 * mec_resize_on_gpu(H, W); W >= 5 where luma is sampled 2 x (narrower images take libjpeg-turbo's small-width
 * paths, not restated); and entropy-coded data that splits into restart segments: with DRI = n > 0 exactly
 * ceil(MCUs / n) of them, separated by RST0..RST7 in cyclic order, without DRI one; 0xFF00 is a stuffed byte; fill
 * bytes 0xFF before a marker are skipped (before a stuffed zero they send the file to the host); the marker that
 * ends the data is EOI. desc->nseg is the number of segments; where nseg <= seg_cap, segs[2 k] and
 * segs[2 k + 1] take segment k's offset in the file and its length (markers and fill bytes excluded), otherwise
 * segs is untouched: call again with room for nseg pairs.
 *
 * mec_jpeg_desc: H, W; ncomp 1 or 3; hs / vs the components' sampling factors; restart the interval in MCUs (0:
 * none); nseg; qt[c] component c's quantization table, 64 values in zigzag order (as in the file); dc[c] / ac[c]
 * its Huffman tables as the file's 16 counts and values (the library builds its decoding tables).
 *
 * mec_jpeg_workspace_bytes: the device workspace the batch needs (192 bytes per 8 x 8 block of every component,
 * padded to whole MCUs: int16 coefficients, then u8 planes), or -1 for an inconsistent descriptor.
 *
 * mec_jpeg_decode_ragged: src (device, src_bytes long, any alignment) holds the files' bytes, or just their
 * scans; segs (HOST, int64 pairs offset | length, image after image, sum of nseg pairs) places every segment in
 * src. Image i is written as u8 [H_i, W_i, ncomp_i] at dst + dst_offs[i], the packed layout the calls above read
 * as MEC_PIX_L / MEC_PIX_RGB. dst (device, 16-byte aligned, dst_bytes long; dst_offs multiples of 16) may lie in
 * the allocation of src: a written range may overlap no segment, no other written range and not the workspace.
 * ws (device, 16-byte aligned) is the workspace. status (device int32[B]) takes 0 for a decoded image, else one
 * of the problems found in it, MEC_JPEG_ST_*: an invalid Huffman code; a DC category above 11; an AC size above 10;
 * a coefficient index past 63; a segment that ends before its MCUs do; an IDCT intermediate outside int16 or a
 * result outside [-512, 511] before range limiting; a DC or dequantized coefficient outside int16 (in the last
 * two cases libjpeg-turbo's SIMD and C code differ, so Pillow's bytes would be a guess). Inside a segment the
 * byte after an 0xFF is dropped, whatever it is. The bytes of an image with nonzero status are unspecified, but
 * lie in its own range: no kernel reads outside the image's segments or writes outside its workspace and dst range,
 * whatever the segments hold.
 *
 * descs, segs and dst_offs are HOST arrays. Everything is checked on the host before any launch: a null pointer,
 * B < 0, B > 65535, a descriptor outside the domain above (sizes, components, sampling, restart and segment
 * counts, table counts), a segment outside src_bytes, a misaligned or out-of-range dst_off, overlapping ranges
 * and a short workspace return -1 with a message and launch nothing; B == 0 returns 0. The call uploads its
 * descriptors and tables itself from a staging buffer it owns and re-uses once the previous call's kernels have
 * finished: asynchronous on `stream`, NOT capturable in a graph. */
typedef struct mec_jpeg_huff {
  uint8_t counts[16];
  uint8_t vals[256];
} mec_jpeg_huff;
typedef struct mec_jpeg_desc {
  int32_t H, W, ncomp;
  int32_t hs[3], vs[3];
  int32_t restart, nseg;
  uint16_t qt[3][64];
  mec_jpeg_huff dc[3], ac[3];
} mec_jpeg_desc;
enum {
  MEC_JPEG_ST_OK = 0,
  MEC_JPEG_ST_BAD_CODE = 1,
  MEC_JPEG_ST_DC_CATEGORY = 2,
  MEC_JPEG_ST_AC_SIZE = 3,
  MEC_JPEG_ST_COEF_INDEX = 4,
  MEC_JPEG_ST_SEGMENT_END = 5,
  MEC_JPEG_ST_IDCT_RANGE = 6,
  MEC_JPEG_ST_COEF_RANGE = 7
};
int mec_jpeg_probe(const uint8_t* data, size_t n, mec_jpeg_desc* desc, int64_t* segs, int seg_cap);
long long mec_jpeg_workspace_bytes(const mec_jpeg_desc* descs, int B);
int mec_jpeg_decode_ragged(const uint8_t* src, size_t src_bytes, const mec_jpeg_desc* descs, const int64_t* segs,
                           int B, uint8_t* dst, const int64_t* dst_offs, size_t dst_bytes, void* ws, size_t ws_bytes,
                           int32_t* status, void* stream);
/* hipEvent timing of the entropy, IDCT and upsample / colour kernels, process-wide, as mec_resize_prof_*. */
int mec_jpeg_prof_enable(int on);
int mec_jpeg_prof_read(double* entropy_ms, double* idct_ms, double* colour_ms, int* count);
/* C[M,N] = act(A[M,K] . B[N,K]^T + bias (+ R)); f16 operands, fp32 accumulate.
 * act: 0 none, 1 relu, 2 gelu(erf). Any of bias/R/C16/C32 may be NULL (not both outputs). */
/* Split-f16 GEMM (the MEC_PREC_FP32X3 engine): A and B each an f16 hi plane with its lo plane
 * a_lo / b_lo elements further on (x = hi + lo); C = act((A_lo.B_hi + A_hi.B_lo + A_hi.B_hi) *
 * oscale + bias (+ R f32)); C16 (hi plane, lo plane at C16 + c_lo when c_lo != 0) and/or C32.
 * act: 0 none, 1 relu, 4 exact-erf GELU. */
int mec_gemm_f16x3(const void* A, long long a_lo, const void* B, long long b_lo, float oscale, const float* bias,
                   const float* R, void* C16, long long c_lo, float* C32, int M, int N, int K, int act,
                   void* stream);
/* The same GEMM on paired planes: A is one f16 array [M][2K] and B one [N][2K], K % 32 == 0, each holding
 * per 32-element K chunk the chunk's hi halfs followed by its lo halfs: element (r, k) of plane p (0 hi,
 * 1 lo) at r 2K + (k >> 5) 64 + 32 p + (k & 31), so one row's operands of a 32-deep K step are one 128-B
 * line. C16: with c_paired != 0 one array [M][2N] in the same layout (c_lo unused), else hi / lo planes
 * c_lo apart as above. Same values as mec_gemm_f16x3 bit for bit (K-interleaved term order only). */
int mec_gemm_f16x3_paired(const void* A, const void* B, float oscale, const float* bias, const float* R, void* C16,
                          int c_paired, long long c_lo, float* C32, int M, int N, int K, int act, void* stream);
/* mec_gemm_f16x3_paired with the two epilogue inputs it lacks, as mec_gemm_ex names them: r_stats [M][2] =
 * (mean, rstd) with r_gamma, r_beta [N] (all three or none; needs R): the f32 R enters as
 * fma((R - mean) * rstd, gamma, beta), the deferred LayerNorm of BERT's O-projection and FFN2; cscale (1 =
 * none) multiplies the value that the C16 planes carry. act as mec_gemm_ex. range_flag: a device word that
 * the kernel sets to 1 when a C16 plane value leaves the f16 range (NULL: the calling handle's flag, none for
 * a handle-less call); it is never cleared here. */
int mec_gemm_f16x3_paired_ln(const void* A, const void* B, float oscale, const float* bias, const float* R,
                             const float* r_stats, const float* r_gamma, const float* r_beta, void* C16, int c_paired,
                             long long c_lo, float cscale, float* C32, int M, int N, int K, int act,
                             unsigned* range_flag, void* stream);
int mec_gemm_f16(const void* A, const void* B, const float* bias, const void* R, int r_is_f32, void* C16,
                 float* C32, int M, int N, int K, int act, void* stream);
/* Implicit-GEMM conv on NHWC f16: x[n,H,W,C], w[Cout][ks][ks][C], y[n,OH,OW,Cout]. */
int mec_conv_f16(const void* x, const void* w, const float* bias, const void* R, void* y, int n, int H, int W,
                 int C, int Cout, int ks, int stride, int pad, int act, void* stream);
/* fp32 engine (the MEC_PREC_FP32 path): C[M,N] = act(A[M,K] . B[N,K]^T + bias (+ R)), all f32;
 * K % 32 == 0, N % 64 == 0; act 0 none, 1 relu, 4 gelu (libm erf). */
int mec_gemm_f32(const float* A, const float* B, const float* bias, const float* R, float* C, int M, int N, int K,
                 int act, void* stream);
/* Implicit-GEMM conv on NHWC f32 (C % 32 == 0), same geometry as mec_conv_f16. */
int mec_conv_f32(const float* x, const float* w, const float* bias, const float* R, float* y, int n, int H, int W,
                 int C, int Cout, int ks, int stride, int pad, int act, void* stream);
/* One LSTM direction (Keras semantics, gate columns i | f | c | o, h0 = c0 = 0) over hoisted input
 * projections: xz f32[B,L,4u] = x.W + b, U f32[u,4u] the recurrent kernel; per step z = xz_t + h.U,
 * c = sigmoid(z_f) c + sigmoid(z_i) tanh(z_c), h = sigmoid(z_o) tanh(c). reverse = 1 walks t = L-1..0
 * (y_seq stays in time order). y_seq f32[B,L,u] and/or h_last f32[B,u] (the h after the last step walked);
 * either may be NULL, not both. units 64 or 128 and L >= 1; anything else returns -1 without a launch;
 * B == 0 returns 0. The BiLSTM model's recurrent kernel ("lstm_rows" applies). */
int mec_lstm_seq_f32(const float* xz, const float* U, int B, int L, int units, int reverse, float* y_seq,
                     float* h_last, void* stream);
/* Conv geometry (mec_conv_f16, mec_conv_f32, mec_gemm_ex): n >= 1, ks >= 1, stride >= 1, pad >= 0 and
 * ks <= H + 2 pad, ks <= W + 2 pad (OH, OW >= 1); anything else returns -1 before any launch. */

/* Descriptor form of the f16 / split-f16 GEMM engine: every operand view, residual form and output form
 * the models launch, through the same dispatch (tile forcing with "gemm_bn" and the halo-kernel routing
 * included). A zeroed descriptor with oscale = cscale = 1 is mec_gemm_f16 without bias or residual.
 *   amode    MEC_A_PLAIN: A[M,K]. MEC_A_CONV: A = NHWC x[n,H,W,C], implicit im2col, K ordered (kh, kw, c),
 *            B = w[N][ks][ks][C]. MEC_A_DUAL: [A | A2] along K = K1 + C, A[M,K1] and A2 = NHWC [n,H,W,C]
 *            read at (oh stride, ow stride) (ks = 1, pad = 0): a bottleneck's conv3 + strided downsample.
 *            Conv / dual: M = n OH OW and K come from the geometry; the descriptor's M and K are ignored.
 *   a_lo, b_lo  both != 0: split operands, the lo planes that many elements after A (and after A2) / B.
 *   oscale   multiplies the accumulator before the bias (a power of two; 1 = none).
 *   R        residual [M,N]: f32 (r_is_f32), f16, or an f16 hi plane with its lo plane at R + r_lo
 *            (split operands only). r_stats [M][2] = (mean, rstd) with r_gamma, r_beta [N]: the f32 R
 *            enters as fma((R - mean) * rstd, gamma, beta) (a deferred LayerNorm).
 *   C16, C32 outputs (either or both); c_lo != 0: C16 as planes hi = f16(v cscale), lo = f16(v cscale - hi)
 *            at C16 + c_lo (C32 carries v).
 *   act      0 none, 1 relu, 2 gelu (f16 path's rational form), 3 relu6, 4 exact-erf gelu, 5 branch-free erf gelu. */
enum { MEC_A_PLAIN = 0, MEC_A_CONV = 1, MEC_A_DUAL = 2 };
typedef struct mec_gemm_args {
  int amode;
  const void* A;
  long long a_lo;
  const void* A2;
  int K1;
  const void* B;
  long long b_lo;
  float oscale;
  const float* bias;
  const void* R;
  int r_is_f32;
  long long r_lo;
  const float* r_stats;
  const float* r_gamma;
  const float* r_beta;
  void* C16;
  long long c_lo;
  float cscale;
  float* C32;
  int M, N, K, act;
  int n, H, W, C, ks, stride, pad;
} mec_gemm_args;
int mec_gemm_ex(const mec_gemm_args* a, void* stream);

/* Descriptor form of BERT's self-attention kernels: ctx = softmax(Q K^T / 8 + bias) V for `rows` sequences of
 * 128 tokens x 12 heads of 64, through the launchers the text forwards use (every form they launch, nothing else).
 *   precision  MEC_PREC_F16: f16 tensors. MEC_PREC_FP32: f32 tensors. MEC_PREC_FP32X3: f16 hi planes, each with
 *              its lo plane `*_lo` elements further on, or paired ([rows][2K], mec_gemm_f16x3_paired's layout)
 *              where `*_lo` is -1. ctx has the tensors' type (fp32x3: planes at ctx_lo, or paired).
 *   form       0: all 128 queries; ctx [rows*128, 768]. 1: the [CLS] query only: qkv holds K | V
 *              [rows*128, 1536], qc the queries [ns, 768], ctx [ns, 768] compact; sample b reads the K / V of
 *              row b (ns == rows), or with `packed` those of row cidx[b] >> 7, its query sitting in slot
 *              cidx[b] & 127 (cidx int32[ns], each in [0, rows*128): the library TRUSTS it).
 *   fused      0: qkv holds Q | K | V [rows*128, 2304] (form 0). 1 (f16 and fp32x3, form 0 only): the QKV
 *              projection in the same kernel, Q|K|V = (hs[rows*128, 768] . wqkv[2304, 768]^T) oscale + bqkv
 *              (f16: oscale must be 1; fp32x3: hs and wqkv planar or paired together, and the K-interleaved
 *              term order "gemm_x3_order" 1). Follows the process options bert_qkv_attn_heads /
 *              bert_qkv_attn_x3_heads and qkv_x3_late_dma. The fp32x3 form raises the range flag of the
 *              calling handle where mec_gemm_ex's split outputs do (none for this handle-less call).
 *   packed     0: mask int32[rows, 128], a key counts where it is nonzero. 1: mask uint8[rows, 128] segment
 *              ids, a key counts for the queries of its own segment.
 *   qks        fp32x3: the factor on the raw scores, 1/8 2^-(s_q + s_k) for Q, K planes of q 2^s_q, k 2^s_k
 *              (ctx carries V's scale); f16 / fp32: must be 0.125.
 * A row without a valid key attends uniformly to all 128 keys (finfo(f32).min absorbs every finite score, as
 * in transformers). rows (or ns) == 0 returns 0 without a launch; anything no kernel serves returns -1 before
 * any launch. */
typedef struct mec_attn_args {
  int precision, form, fused, packed;
  const void* qkv;
  long long qkv_lo;
  const void* qc;
  long long qc_lo;
  const void* hs;
  long long hs_lo;
  const void* wqkv;
  long long w_lo;
  const float* bqkv;
  float oscale;
  const void* mask;
  const int32_t* cidx;
  void* ctx;
  long long ctx_lo;
  float qks;
  int rows, ns;
} mec_attn_args;
int mec_bert_attn(const mec_attn_args* a, void* stream);

/* Tuning knobs (A/B benchmarking; defaults in brackets). Every handle owns its own copy of
 * the knobs and its own GEMM autotune cache, so two handles in one process never perturb
 * each other: mec_model_set_option sets one handle's knob; mec_set_option sets the process
 * default that handles created AFTERWARDS copy (and that the handle-less kernel entry points
 * use). Every pair of settings of one knob gives bit-identical outputs, except "fusion_r" 4 vs
 * 1|2, "conv3x3_halo" 0 vs 1, "gemm_x3_order" 0 vs 1 and "gelu_x3" 0 vs 1 (fp32 reassociation or
 * erf evaluation, all within the oracle tolerance).
 *   "gemm_bn" [0]|id       force one f16 GEMM tile (0 = autotune), "gemm_autotune" 0|[1]. The tile ids are
 *                          defined in one place, the catalogue csrc/gemm_tiles.h (MEC_GEMM_TILES; fp32 engine:
 *                          MEC_GEMM_F32_TILES); every key below that takes an id accepts 0 and those ids
 *   "gemm_bn_tag" tag*100000+id   force a tile for one launch class (e.g. 3 = BERT O-proj)
 *   "gemm_f32_tile" [0]|1..8  force one fp32 GEMM tile (0 = autotune; 5..8 = 1..4 on 16x16x4; the fp32
 *                          catalogue's ids)
 *   "gemm_f32_tag" tag*100000+id  pin an fp32 tile for one launch class (default: BERT FFN1 -> 8)
 *   "gemm_f32_family" 0|[16]|32  fp32 tiles of one MFMA shape only (16x16x4 / 32x32x2): one k order
 *                          for every shape, so rows do not depend on the batch size
 *   "gemm_prefetch_r" 0|[1]  f16 (and split hi / lo) residual prefetch in short-K GEMMs
 *   "gemm_group_m" 0|2|4|[8]|16  ping-pong GEMM tile order inside each XCD's tile range (0: row-major,
 *                          G: G-panel groups of M walked M-fastest, fewer weight re-fetches)
 *   "gemm_glds_group_m" 0|2|4|[8]|16  the same tile order for the multi-stage GEMM engine
 *   "gemm_x3_order" 0|[1]  split-f16 (fp32x3) GEMM term order: 0 = pass-major (K for lo.hi, then
 *                          hi.lo, then hi.hi), 1 = K-interleaved (each 32-deep k chunk's three terms
 *                          back to back; the catalogue's interleaved-split tiles only, today 70256 / 70128 /
 *                          71128 / 71064 / 70064 / 72128);
 *                          both fp32-accurate, not the same bits
 *   "gemm_x3_tag" tag*100000+id  pin an interleaved split tile (7xxxx; 0 = autotune) for one launch
 *                          class (FusedPipeline pins BERT FFN2 to 70256 at fp32x3); a pin applies where
 *                          its grid has >= 128 tiles (half the CUs), smaller batches autotune (same bits)
 *   GEMM shapes first launched inside hipGraph capture cannot be timed: split (fp32x3) shapes run
 *   the heuristic tile uncached and are autotuned at their first eager launch (every split tile
 *   gives the same bits); f16 / f32 shapes cache the heuristic tile for the handle's lifetime, so
 *   an eager launch after the capture computes the same bits as the graph replay (tiles of those
 *   engines differ in MFMA shape and k order)
 *   "gelu_x3" 0|[1]        fp32x3 BERT FFN1 GELU: 1 = branch-free erf with a one-instruction exp
 *                          (error 1.21e-7 x max(|x|, 1) vs float64), 0 = libm erff (not the same bits)
 *   "conv3x3_direct" 0|[1] layer1 3x3 conv on the halo-tile kernel (mec_conv_f16 too)
 *   "conv3x3_halo" 0|[1]   layers 2-3 stride-1 3x3 convs on the halo kernel (mec_conv_f16 too;
 *                          fp32 accumulation in another order: not bit-identical to 0)
 *   "pw_chain" 0|1|[2]     layer1 seam kernels (1: the 256->64 seams, 2: also 256->128)
 *   "pw_chain_form" [0]|1|2  seam weight placement (LDS / registers)
 *   "pw_chain_x3" 0|1|[2]  fp32x3 layer1 seam kernels (1: the 256->64 seams incl. the downsample one, 2: also 256->128)
 *   "pw_seam_x3" 0|[1]|2  fp32x3 layer2 seam kernels (1: the 512->128 seams, 2: also 512->256 into layer3; same bits)
 *   "bert_qkv_attn_x3_heads" [1]|2  fp32x3 fused QKV + attention: heads per workgroup (same bits)
 *   "bert_qkv_attn_heads" [1]|2  the same for the f16 fused QKV + attention
 *   "bert_qkv_attn" 0|[1]  fused BERT QKV projection + attention
 *   "bert_ln_rows" 1|[2]|4  BERT LayerNorm rows per wave (all loads of a wave's rows in flight first)
 *   "bert_cls_last" 0|[1]  BERT's last layer on the [CLS] rows only (K / V still for every token):
 *                          the pooler, logits and CLS feature read nothing else of it; same bits as 0
 *   "resnet_chunk" [0]|n   ResNet layers 1-2 over n-image chunks (f16 and fp32x3; measured slower)
 *   "mbv2_x3_tile" 0|[4]   fp32x3 MobileNetV2: 4x4 output tiles for the stride-2 blocks at 56 / 28 outputs
 *   "mbv2_x3_tpw" 1|[2]..16 fp32x3 MobileNetV2 fused blocks: output tiles per workgroup, the next tile's
 *                          input loaded into registers while one computes (same bits for every value)
 *   "mbv2_x3_occ" [3]|4    fp32x3 MobileNetV2 4x4-tile blocks: workgroups per CU the registers are
 *                          allocated for (4: 128 VGPRs with an 84-B spill, 3: 168 VGPRs); same bits
 *   "mbv2_x3_sesw" 0|[1]   fp32x3 MobileNetV2 fused blocks: the expanded chunk's rows chunk-swizzled per tile
 *                          shape (fewer LDS bank conflicts on the depthwise reads) or unswizzled; same bits
 *   "qkv_x3_late_dma" [0]|1|2  fp32x3 fused QKV + attention: every other 256-block of workgroups issues its
 *                          stage refill after its first / second MFMA term group (measured neutral); same bits
 *   "gemm_x3_pp" 0|[1]|2   fp32x3 split GEMM, tile 70256 on paired planes (BERT's FFN1, FFN2, O-projection and
 *                          last-layer K|V under x3_layout 1): the four-phase ping-pong schedule with two K
 *                          tiles in flight instead of the two-stage ring. 0 = ring, 1 = ping-pong for the
 *                          launches without an activation (FFN2, O-projection, K|V: faster by the median
 *                          at B = 256; FFN1 measured slower on it and keeps the ring),
 *                          2 = ping-pong for every launch (tests, A/B). Any batch size; same bits. Planar
 *                          operands and every other tile run the ring either way
 *   "x3_plane_scale" 0|[1] fp32x3 activation-plane scales, creation-time (mec_create_opt, or the process
 *                          default before mec_create_ex; mec_model_set_option rejects it): 1 = per-tensor
 *                          power-of-two exponents (the envelope above), 0 = unscaled planes (A/B only:
 *                          narrower envelope, different bits)
 *   "x3_headroom" [0]..24  fp32x3 extra binades of plane headroom, creation-time like x3_plane_scale
 *                          (mec_create_opt above)
 *   "x3_layout" 0|[1]      fp32x3 text model, creation-time like x3_plane_scale: 1 = weight and activation planes
 *                          paired ([rows][2K]: per 32-element K chunk the hi halfs, then the lo halfs; see
 *                          mec_gemm_f16x3_paired), 0 = planar. Same bits. A handle created with gemm_x3_order 0
 *                          is planar, and a paired handle rejects gemm_x3_order 0
 *   "mbv2_layered" 0|7..17 [8]  fp32x3 MobileNetV2: features[k..17] as expand GEMM -> depthwise -> project GEMM
 *                          (0: every block fused but features[17], layered at every setting)
 *   "mbv2_layered16" 0|7..17 [8]  the same on the f16 path
 *   "mbv2_impl" [0]|1|2    MobileNetV2 block form: 0 = time both per block shape, 1 = workgroup, 2 = wave
 *   "fusion_r" 1|2|[4]     samples per fusion workgroup
 *   "fusion_split" 0|[1]   fusion as 3 launches (per-modality projection, cross-attention, head)
 *   "lstm_rows" 1|[2]|4    BiLSTM recurrent kernel: rows of one direction per workgroup, sharing its
 *                          register-resident recurrent weights (same bits for every value)
 * Probe values, which skip work to time a kernel's parts and return WRONG results, exist only
 * in the -DMEC_PROBES build (libmec_hip_probes.so, `make probes`; tools/ only): "gemm_debug"
 * 1..5, "conv3x3_debug" / "stem_debug" 1|2|4|7, "bert_qkv_attn" 2|3,
 * "audio_debug" 1|2|4|8|15, "speech_debug" 1, "speech_spin_limit" >= 0 (the speech DNN's
 * hand-off wait limit: forces expired waits). The product library rejects them (-1). */
int mec_set_option(const char* key, int value);
int mec_model_set_option(mec_model* m, const char* key, int value);

/* Build flags of the loaded library: MEC_BUILD_PROBES set = probe values accepted. */
enum { MEC_BUILD_PROBES = 1 };
int mec_build_flags(void);

/* Tile width the autotuner chose for a plain (amode 0) or conv (amode 1) GEMM shape; 0 = not yet seen. */
int mec_gemm_query(int amode, int M, int N, int K);
/* The same for the fp32 engine: tile id 1 = 256x128 (8 waves), 2 = 128x128, 3 = 128x64, 4 = 256x256
 * on v_mfma_f32_32x32x2_f32; 5..8 the same tiles on v_mfma_f32_16x16x4_f32.
 * Both query the process-default cache of the handle-less entry points (mec_gemm_f16/f32). */
int mec_gemm_f32_query(int amode, int M, int N, int K);
/* The tile a handle's own autotuner chose for a shape it ran (its precision's engine); 0 = not seen. */
int mec_model_gemm_query(mec_model* m, int amode, int M, int N, int K);

/* Errors a kernel can only report after the fact, since the handle's last check: 0 = none,
 * -1 = mec_last_error() says what (and the flag is cleared); MEC_ERR_X3_RANGE (-2) = the fp32x3
 * range flag below (the batch can be re-run on an MEC_PREC_FP32 handle of the same weights). Call once the stream that ran
 * the handle's forwards has been synchronized. Speech: a stage hand-off wait of
 * speech_flow_kernel expired (that forward's probs are NaN). MEC_PREC_FP32X3 text / image
 * handles: an activation left the f16 hi / lo range (|x| >= 65520, NaN or inf; that forward's
 * outputs are invalid). Always 0 for the other kinds and precisions. No reference counterpart:
 * the reference's predict calls have no asynchronous failure (inference/speech_inference.py:69). */
enum { MEC_ERR_X3_RANGE = -2 };
int mec_model_check(mec_model* m);

/* hipEvent timing hook: time every launch of kernel class `tag`. */
int mec_prof_enable(mec_model* m, int tag);
int mec_prof_read(mec_model* m, double* total_ms, int* count);

#ifdef __cplusplus
}
#endif

#endif /* MEC_H_ */
