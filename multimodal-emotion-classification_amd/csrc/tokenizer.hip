// Tokenization on the GPU (include/mec.h mec_tok_*): UTF-8 bytes in, ids / mask / len out, for the
// BiLSTM path (MEC_TOK_KERAS) and the BERT path (MEC_TOK_WORDPIECE). One wave per text. The
// vocabulary is an open-addressing hash table built on the host (tok_table.h); every hash hit is
// confirmed against the byte pool. All stores are ordinary vector stores.
#include <algorithm>

#include "mec.h"
#include "mec_common.h"
#include "tok_table.h"

namespace mec {
namespace tok {

struct Params {
  const Slot* slots;
  const uint8_t* pool;
  const uint8_t* delim;  // 256 bytes, 16-byte aligned
  uint32_t mask;
  int max_len;
  int oov_id, lower, unk_id, cls_id, sep_id, pad_id, max_word;
};

__device__ inline uint64_t lanes_below(int lane) { return (1ull << lane) - 1ull; }

// text i = text[beg, end): every offset clamped into [0, off[B]], the end to at least the start
__device__ inline void text_span(const int64_t* off, int B, int row, int64_t& beg, int64_t& end) {
  const int64_t total = max(off[B], (int64_t)0);
  beg = min(max(off[row], (int64_t)0), total);
  end = min(max(off[row + 1], beg), total);
}

__device__ inline void write_tail(int row, int L, int n, int fill, int32_t* out, int32_t* mask, int32_t* len) {
  const int lane = threadIdx.x;
  for (int j = lane; j < L; j += 64) {
    if (j >= n) out[j] = fill;
    if (mask) mask[(size_t)row * L + j] = j < n;
  }
  if (len && lane == 0) len[row] = n;
}

// KERAS. A chunk is 64 bytes, one per lane; a ballot of "this byte is part of a word" gives the word
// starts (the previous chunk's last bit carried over). The lane at a word's start hashes the word forward,
// at most max_len + 1 bytes of it (a longer word cannot be in the table), so every byte is read by one
// lane once more: linear in the text. A ballot of the lanes that have an id places the ids in order.
__global__ __launch_bounds__(64) void keras_kernel(Params p, const uint8_t* __restrict__ text,
                                                   const int64_t* __restrict__ text_off, int B, int L,
                                                   int32_t* __restrict__ ids, int32_t* __restrict__ mask,
                                                   int32_t* __restrict__ len) {
  __shared__ uint8_t delim[256];
  const int row = blockIdx.x, lane = threadIdx.x;
  reinterpret_cast<uint32_t*>(delim)[lane] = reinterpret_cast<const uint32_t*>(p.delim)[lane];
  __syncthreads();
  int64_t beg, end;
  text_span(text_off, B, row, beg, end);
  int32_t* out = ids + (size_t)row * L;
  int count = 0;
  uint64_t carry = 0;
  for (int64_t base = beg; base < end && count < L; base += 64) {
    const int64_t pos = base + lane;
    const bool inword = pos < end && !delim[text[pos]];
    const uint64_t wm = __ballot(inword);
    const uint64_t starts = wm & ~((wm << 1) | carry);
    carry = wm >> 63;
    int id = -1;
    if ((starts >> lane) & 1) {
      uint32_t h = 0;
      int n = 0;
      while (pos + n < end && n <= p.max_len) {
        const uint8_t b = text[pos + n];
        if (delim[b]) break;
        h = step(h, b);
        ++n;
      }
      if (n <= p.max_len)
        id = lookup(p.slots, p.mask, p.pool, finish(h, n, 0), n, 0, [&](int k) { return text[pos + k]; });
      if (id < 0) id = p.oov_id;
    }
    const uint64_t emit = __ballot(id >= 0);
    if (id >= 0) {
      const int at = count + __popcll(emit & lanes_below(lane));
      if (at < L) out[at] = id;
    }
    count += __popcll(emit);
  }
  write_tail(row, L, min(count, L), 0, out, mask, len);
}

// WORDPIECE. Per 64-byte chunk the lanes classify their bytes (dropped / whitespace / punctuation /
// word character) and three ballots describe the chunk; the wave then walks the chunk's kept bytes in
// order with scalar bit operations: a stretch of word characters is appended to the current word in LDS
// (dropped bytes in between vanish, a word may continue into the next chunk), whitespace ends the word,
// a punctuation byte ends it and is a word of its own. A finished word is matched by the whole wave:
// the lanes hold the word's prefix hashes, and for the current start the lanes test the candidate ends
// in parallel, longest first, so one probe round finds the longest piece.
struct WordState {
  uint8_t* word;     // LDS [kWordCap]
  uint32_t* prefix;  // LDS [kWordCap + 1]: prefix hashes of the word
  uint32_t* power;   // LDS [kWordCap + 1]: kP^k
  int32_t* pieces;   // LDS [kWordCap]
};

// Tokenize the word of n bytes (the first min(n, kWordCap) are in ws.word) and write its pieces at
// out[1 + np ...], as far as they are among the first `need`. Returns the number of pieces.
__device__ inline int flush_word(const Params& p, const WordState& ws, int n, int np, int need, int32_t* out) {
  const int lane = threadIdx.x;
  __syncthreads();  // the word's bytes are in LDS
  int nw = 0;
  bool bad = n > p.max_word;
  if (!bad) {
    uint32_t ha = 0, hb = 0;
    for (int i = 0; i < n; ++i) {
      const uint32_t c = ws.word[i];
      if (i <= lane) ha = step(ha, c);
      if (i <= lane + 64) hb = step(hb, c);
    }
    if (lane == 0) ws.prefix[0] = 0;
    if (lane + 1 <= n) ws.prefix[lane + 1] = ha;
    if (lane + 65 <= n) ws.prefix[lane + 65] = hb;
    __syncthreads();
    int s = 0;
    while (s < n) {
      const int flag = s > 0;
      const int top = min(n, s + p.max_len);  // a longer piece is not in the table
      int found_e = -1, found_id = -1;
      for (int r = 0; r * 64 < top - s; ++r) {
        const int e = top - (r * 64 + lane);
        int id = -1;
        if (e > s) {
          const int l = e - s;
          const uint32_t h = ws.prefix[e] - ws.prefix[s] * ws.power[l];
          id = lookup(p.slots, p.mask, p.pool, finish(h, l, flag), l, flag, [&](int k) { return ws.word[s + k]; });
        }
        const uint64_t hit = __ballot(id >= 0);
        if (hit) {
          const int j = __ffsll((unsigned long long)hit) - 1;  // the lowest lane holds the longest piece
          found_id = __shfl(id, j);
          found_e = top - (r * 64 + j);
          break;
        }
      }
      if (found_e < 0) {
        bad = true;
        break;
      }
      if (lane == 0) ws.pieces[nw] = found_id;
      ++nw;
      s = found_e;
    }
  }
  if (bad) {
    if (lane == 0) ws.pieces[0] = p.unk_id;
    nw = 1;
  }
  __syncthreads();
  for (int i = lane; i < nw; i += 64)
    if (np + i < need) out[1 + np + i] = ws.pieces[i];
  __syncthreads();  // the buffers are free for the next word
  return nw;
}

__global__ __launch_bounds__(64) void wordpiece_kernel(Params p, const uint8_t* __restrict__ text,
                                                       const int64_t* __restrict__ text_off, int B, int L,
                                                       int32_t* __restrict__ ids, int32_t* __restrict__ mask,
                                                       int32_t* __restrict__ len) {
  __shared__ uint8_t s_word[kWordCap];
  __shared__ uint32_t s_prefix[kWordCap + 1];
  __shared__ uint32_t s_power[kWordCap + 1];
  __shared__ int32_t s_pieces[kWordCap];
  const WordState ws{s_word, s_prefix, s_power, s_pieces};
  const int row = blockIdx.x, lane = threadIdx.x;
  {
    uint32_t pw = 1;
    for (int i = 0; i < lane; ++i) pw *= kP;
    s_power[lane] = pw;
    uint32_t p64 = 1;
    for (int i = 0; i < 64; ++i) p64 *= kP;
    s_power[lane + 64] = pw * p64;
    if (lane == 0) s_power[128] = p64 * p64;
  }
  __syncthreads();
  int64_t beg, end;
  text_span(text_off, B, row, beg, end);
  int32_t* out = ids + (size_t)row * L;
  const int need = L - 2;
  int np = 0;    // pieces so far (all words' counts; only the first `need` are written)
  int wlen = 0;  // bytes of the word being collected (counted past kWordCap, stored up to it)
  for (int64_t base = beg; base < end && np < need; base += 64) {
    const int64_t pos = base + lane;
    uint32_t b = pos < end ? text[pos] : ' ';
    if (p.lower && b >= 'A' && b <= 'Z') b += 32;
    const bool space = b == ' ' || b == '\t' || b == '\n' || b == '\r';
    const bool drop = !space && (b < 0x20 || b == 0x7F);
    const bool punct = (b >= 33 && b <= 47) || (b >= 58 && b <= 64) || (b >= 91 && b <= 96) || (b >= 123 && b <= 126);
    const uint64_t chm = __ballot(!space && !drop && !punct), pum = __ballot(punct), spm = __ballot(space);
    uint64_t rem = chm | pum | spm;  // kept bytes not consumed yet
    while (rem && np < need) {
      const int first = __ffsll((unsigned long long)rem) - 1;
      if ((chm >> first) & 1) {
        const uint64_t stop = rem & ~chm;  // the next kept byte that is no word character
        const int q = stop ? __ffsll((unsigned long long)stop) - 1 : 64;
        const uint64_t below_q = q == 64 ? ~0ull : lanes_below(q);
        const uint64_t run = rem & below_q;
        if ((run >> lane) & 1) {
          const int at = wlen + __popcll(run & lanes_below(lane));
          if (at < kWordCap) s_word[at] = (uint8_t)b;
        }
        wlen = min(wlen + __popcll(run), 1 << 20);
        rem &= ~below_q;
        if (q < 64) {
          np += flush_word(p, ws, wlen, np, need, out);
          wlen = 0;
        }
      } else {
        if (wlen) {  // a word from the previous chunk ends at this chunk's first kept byte
          np += flush_word(p, ws, wlen, np, need, out);
          wlen = 0;
          continue;
        }
        if ((pum >> first) & 1) {
          if (lane == first) s_word[0] = (uint8_t)b;
          np += flush_word(p, ws, 1, np, need, out);
          rem &= rem - 1;
        } else {
          const uint64_t next = rem & ~spm;
          rem = next ? rem & ~lanes_below(__ffsll((unsigned long long)next) - 1) : 0;
        }
      }
    }
  }
  if (wlen && np < need) np += flush_word(p, ws, wlen, np, need, out);
  np = min(np, need);
  if (lane == 0) {
    out[0] = p.cls_id;
    out[np + 1] = p.sep_id;
  }
  write_tail(row, L, np + 2, p.pad_id, out, mask, len);
}

}  // namespace tok
}  // namespace mec

struct mec_tokenizer {
  int kind = 0, device = 0;
  mec::DevBuf image;  // slots | pool | delim
  mec::tok::Params p{};
};

using namespace mec;

extern "C" {

int mec_tok_create(const mec_tok_desc* d, int device, mec_tokenizer** out) {
  try {
    if (!out) { set_error("mec_tok_create: out is null"); return -1; }
    *out = nullptr;
    tok::HostTable t;
    std::string err;
    if (tok::build(d, &t, &err) != 0) { set_error(err); return -1; }
    MEC_HIP(hipSetDevice(device));
    const size_t slot_bytes = t.slots.size() * sizeof(tok::Slot);
    const size_t pool_bytes = (t.pool.size() + 15) / 16 * 16;
    std::vector<uint8_t> image(slot_bytes + pool_bytes + 256, 0);
    std::memcpy(image.data(), t.slots.data(), slot_bytes);
    if (!t.pool.empty()) std::memcpy(image.data() + slot_bytes, t.pool.data(), t.pool.size());
    std::memcpy(image.data() + slot_bytes + pool_bytes, d->delim, 256);
    auto* h = new mec_tokenizer;
    h->kind = d->kind;
    h->device = device;
    if (upload(h->image, image.data(), image.size()) != 0) { delete h; return -1; }
    uint8_t* base = h->image.as<uint8_t>();
    h->p = tok::Params{reinterpret_cast<const tok::Slot*>(base), base + slot_bytes, base + slot_bytes + pool_bytes,
                       (uint32_t)(t.slots.size() - 1), t.max_len, d->oov_id, d->lower, d->unk_id, d->cls_id,
                       d->sep_id, d->pad_id, d->max_word};
    *out = h;
    return 0;
  } catch (const std::exception& e) {
    set_error(std::string("mec_tok_create: ") + e.what());
    return -1;
  }
}

int mec_tok_encode(mec_tokenizer* t, const uint8_t* text, const int64_t* text_off, int B, int L, int32_t* ids,
                   int32_t* mask, int32_t* len, void* stream) {
  MEC_REQUIRE(t, "mec_tok_encode: null tokenizer");
  MEC_REQUIRE(B >= 0, "mec_tok_encode: B < 0");
  const int lmin = t->kind == MEC_TOK_WORDPIECE ? 2 : 1;
  MEC_REQUIRE(L >= lmin && L <= 512, "mec_tok_encode: L must be in 1..512 (WORDPIECE: 2..512)");
  if (B == 0) return 0;
  MEC_REQUIRE(text && text_off && ids, "mec_tok_encode: text, text_off or ids is null");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (t->kind == MEC_TOK_KERAS)
    hipLaunchKernelGGL(tok::keras_kernel, dim3(B), dim3(64), 0, s, t->p, text, text_off, B, L, ids, mask, len);
  else
    hipLaunchKernelGGL(tok::wordpiece_kernel, dim3(B), dim3(64), 0, s, t->p, text, text_off, B, L, ids, mask, len);
  MEC_LAUNCH_CHECK();
  return 0;
}

int mec_tok_destroy(mec_tokenizer* t) {
  if (!t) return 0;
  (void)hipSetDevice(t->device);
  delete t;
  return 0;
}

}  // extern "C"
