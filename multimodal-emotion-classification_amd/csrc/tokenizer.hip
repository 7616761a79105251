// Tokenization on the GPU (include/mec.h mec_tok_*): UTF-8 bytes in, ids / mask / len out, for the
// BiLSTM path (MEC_TOK_KERAS) and the BERT path (MEC_TOK_WORDPIECE for 7-bit text, MEC_TOK_WORDPIECE_UTF8
// for any text). One wave per text. The vocabulary is an open-addressing hash table built on the host
// (tok_table.h); every hash hit is confirmed against the byte pool. All stores are ordinary vector stores.
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
  const uint16_t* cp_index;  // WORDPIECE_UTF8: the code-point table (tok_table.h CpTable)
  const uint32_t* cp_block;
  const uint8_t* cp_exp;
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
//
// WORDPIECE_UTF8 is the same kernel with a second walk for the chunks that hold a byte >= 0x80 (a chunk
// without one takes the walk above). There the lanes at a character's first byte decode it, reading up to
// 3 bytes past the chunk but never past the text, and look its class up in the two-stage table; a lane is
// then whitespace, nothing (a continuation byte, a dropped character), a plain word character that stands
// for nb bytes and nc characters (its own bytes, or a MAPPED character's outputs), or a "complex"
// character (one with a punctuation output or the ISOLATE flag), which the walk handles one at a time as
// it handles a punctuation byte. One wave scan of (nc, nb) per chunk places a stretch's bytes in the LDS
// word. A word is at most max_word characters, so its buffers hold 4 * kWordCap bytes. The count of
// continuation bytes that a chunk's last character leaves to the next chunk is carried like the word.
template <int CAP>
struct WordState {
  uint8_t* word;     // LDS [CAP]
  uint32_t* prefix;  // LDS [CAP + 1]: prefix hashes of the word
  uint32_t* power;   // LDS [CAP + 1]: kP^k
  int32_t* pieces;   // LDS [CAP]
};

// Tokenize the word of n bytes and nch characters (the first min(n, CAP) bytes are in ws.word) and write
// its pieces at out[1 + np ...], as far as they are among the first `need`. Returns the number of pieces.
// nch <= max_word <= kWordCap implies n <= CAP: CAP is kWordCap times the longest character.
template <int CAP>
__device__ inline int flush_word(const Params& p, const WordState<CAP>& ws, int n, int nch, int np, int need,
                                 int32_t* out) {
  constexpr int NH = CAP / 64;  // prefix hashes per lane: lane's j-th is that of the first lane + 64 j + 1 bytes
  const int lane = threadIdx.x;
  __syncthreads();  // the word's bytes are in LDS
  int nw = 0;
  bool bad = nch > p.max_word;
  if (!bad) {
    uint32_t h[NH];
#pragma unroll
    for (int j = 0; j < NH; ++j) h[j] = 0;
    for (int i = 0; i < n; ++i) {
      const uint32_t c = ws.word[i];
#pragma unroll
      for (int j = 0; j < NH; ++j)
        if ((j < 2 || j * 64 < n) && i <= lane + 64 * j) h[j] = step(h[j], c);
    }
    if (lane == 0) ws.prefix[0] = 0;
#pragma unroll
    for (int j = 0; j < NH; ++j)
      if (lane + 64 * j + 1 <= n) ws.prefix[lane + 64 * j + 1] = h[j];
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

// What a lane of a chunk with a byte >= 0x80 stands for (WORDPIECE_UTF8).
enum { kNone = 0, kSpace = 1, kChar = 2, kComplex = 3 };
// A complex lane's outputs: count | punctuation flags << 2 | ISOLATE << 5 | byte length of output j << (6 + 3 j)
constexpr int kCxPunct = 2, kCxIsolate = 5, kCxLen = 6;

__device__ inline int utf8_len(uint32_t lead) { return lead < 0x80 ? 1 : lead < 0xE0 ? 2 : lead < 0xF0 ? 3 : 4; }

template <bool UTF8>
__global__ __launch_bounds__(64) void wordpiece_kernel(Params p, const uint8_t* __restrict__ text,
                                                       const int64_t* __restrict__ text_off, int B, int L,
                                                       int32_t* __restrict__ ids, int32_t* __restrict__ mask,
                                                       int32_t* __restrict__ len) {
  constexpr int CAP = UTF8 ? 4 * kWordCap : kWordCap;
  __shared__ uint8_t s_word[CAP];
  __shared__ uint32_t s_prefix[CAP + 1];
  __shared__ uint32_t s_power[CAP + 1];
  __shared__ int32_t s_pieces[CAP];
  const WordState<CAP> ws{s_word, s_prefix, s_power, s_pieces};
  const int row = blockIdx.x, lane = threadIdx.x;
  {
    uint32_t pw = 1;
    for (int i = 0; i < lane; ++i) pw *= kP;
    uint32_t p64 = 1;
    for (int i = 0; i < 64; ++i) p64 *= kP;
    uint32_t hi = 1;
    for (int j = 0; j < CAP / 64; ++j, hi *= p64) s_power[lane + 64 * j] = pw * hi;
    if (lane == 0) s_power[CAP] = hi;
  }
  __syncthreads();
  int64_t beg, end;
  text_span(text_off, B, row, beg, end);
  int32_t* out = ids + (size_t)row * L;
  const int need = L - 2;
  int np = 0;         // pieces so far (all words' counts; only the first `need` are written)
  int wlen = 0;       // bytes of the word being collected (counted past CAP, stored up to it)
  int wch = 0;        // its characters
  int skip = 0;       // UTF8: continuation bytes at the next chunk's start that end this chunk's last character
  bool bad = false;   // UTF8: the text is ill-formed or holds an uncovered code point
  auto flush = [&]() {
    np += flush_word(p, ws, wlen, wch, np, need, out);
    wlen = wch = 0;
  };
  // UTF8 reads the whole text, also past the last piece that fits: the row's validity is the text's
  for (int64_t base = beg; base < end && (UTF8 || np < need); base += 64) {
    const int64_t pos = base + lane;
    uint32_t b = pos < end ? text[pos] : ' ';
    if (UTF8 && __ballot(b >= 0x80)) {
      int kind = kNone, nb = 0, nc = 0, ab = -1, cx = 0, clen = 0;
      const uint8_t* src = text + pos;  // the lane's output bytes, unless ab >= 0 is its one byte
      bool ill = false, cont = false;
      if (pos < end) {
        if (b < 0x80) {
          if (p.lower && b >= 'A' && b <= 'Z') b += 32;
          ab = (int)b;
          if (ascii_space(b)) kind = kSpace;
          else if (ascii_punct(b)) kind = kComplex, cx = 1 | 1 << kCxPunct | 1 << kCxLen;
          else if (!ascii_drop(b)) kind = kChar, nb = nc = 1;
        } else if (b < 0xC0) {
          cont = true;
        } else {
          clen = utf8_len(b);
          ill = b < 0xC2 || b > 0xF4;
          uint32_t cp = b & (0x7Fu >> clen);
          for (int k = 1; k < clen; ++k) {
            const uint32_t c = pos + k < end ? text[pos + k] : 0u;  // the text's end cuts the character off
            ill |= (c & 0xC0) != 0x80;
            cp = cp << 6 | (c & 0x3F);
          }
          ill |= cp < (clen == 2 ? 0x80u : clen == 3 ? 0x800u : 0x10000u) || (cp >= 0xD800 && cp <= 0xDFFF) || cp > 0x10FFFF;
          if (!ill) {
            const uint32_t e = cp_entry(p.cp_index, p.cp_block, cp);
            const int c = e & 7, iso = (e & MEC_CP_ISOLATE) != 0;
            if (c == MEC_CP_UNCOVERED) {
              ill = true;
            } else if (c == MEC_CP_SPACE) {
              kind = kSpace;
            } else if (c == MEC_CP_CHAR && !iso) {
              kind = kChar, nb = clen, nc = 1;
            } else if (c == MEC_CP_CHAR || c == MEC_CP_PUNCT) {
              kind = kComplex, cx = 1 | (c == MEC_CP_PUNCT) << kCxPunct | iso << kCxIsolate | clen << kCxLen;
            } else if (c == MEC_CP_MAPPED) {
              const uint8_t* rec = p.cp_exp + (e >> kCpExpShift);
              const int bytes = rec[0], k = rec[1] & 3, pm = rec[1] >> 2;
              src = rec + 2;
              if (k == 0) {
                kind = iso ? kSpace : kNone;  // no output: it vanishes, or only separates
              } else if (pm || iso) {
                kind = kComplex, cx = k | pm << kCxPunct | iso << kCxIsolate;
                for (int j = 0, o = 0; j < k; ++j) {
                  const int l = utf8_len(src[o]);
                  cx |= l << (kCxLen + 3 * j);
                  o += l;
                }
              } else {
                kind = kChar, nb = bytes, nc = k;
              }
            }
          }
        }
      }
      const uint64_t l2 = __ballot(clen == 2), l3 = __ballot(clen == 3), l4 = __ballot(clen == 4);
      const uint64_t leads = l2 | l3 | l4;
      const uint64_t held = leads << 1 | (l3 | l4) << 2 | l4 << 3 | lanes_below(skip);
      bad = __ballot(ill) != 0 || (__ballot(cont) & ~held) != 0;
      if (bad) break;
      skip = 0;
      if (leads) {
        const int last = 63 - __clzll((long long)leads);
        skip = max(last + ((l2 >> last) & 1 ? 2 : (l3 >> last) & 1 ? 3 : 4) - 64, 0);
      }
      if (np >= need) continue;
      const uint64_t chm = __ballot(kind == kChar), cxm = __ballot(kind == kComplex), spm = __ballot(kind == kSpace);
      // inclusive wave scan of characters << 16 | bytes over the plain word characters
      const int own = kind == kChar ? nc << 16 | nb : 0;
      int inc = own;
      for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(inc, d);
        if (lane >= d) inc += up;
      }
      const int exc = inc - own;
      auto put = [&](int at, int from, int n) {  // this lane's output bytes [from, from + n) to word[at ...]
        for (int k = 0; k < n; ++k)
          if (at + k < CAP) s_word[at + k] = ab >= 0 ? (uint8_t)ab : src[from + k];
      };
      uint64_t rem = chm | cxm | spm;
      while (rem && np < need) {
        const int first = __ffsll((unsigned long long)rem) - 1;
        if ((chm >> first) & 1) {
          const uint64_t stop = rem & ~chm;
          const int q = stop ? __ffsll((unsigned long long)stop) - 1 : 64;
          const uint64_t below_q = q == 64 ? ~0ull : lanes_below(q);
          const int from = __shfl(exc, first);
          const int sum = (q == 64 ? __shfl(inc, 63) : __shfl(exc, q)) - from;
          if (((rem & below_q) >> lane) & 1) put(wlen + ((exc - from) & 0xFFFF), 0, nb);
          wlen = min(wlen + (sum & 0xFFFF), 1 << 20);
          wch = min(wch + (sum >> 16), 1 << 20);
          rem &= ~below_q;
          if (q < 64) flush();
        } else if ((spm >> first) & 1) {
          if (wlen) flush();
          const uint64_t next = rem & ~spm;
          rem = next ? rem & ~lanes_below(__ffsll((unsigned long long)next) - 1) : 0;
        } else {
          const int d = __shfl(cx, first);
          const int iso = (d >> kCxIsolate) & 1;
          if (iso && wlen) flush();
          for (int j = 0, o = 0; j < (d & 3) && np < need; ++j) {
            const int l = (d >> (kCxLen + 3 * j)) & 7;
            if ((d >> (kCxPunct + j)) & 1) {
              if (wlen) flush();
              if (np < need) {
                if (lane == first) put(0, o, l);
                wlen = l, wch = 1;
                flush();
              }
            } else {
              if (lane == first) put(wlen, o, l);
              wlen = min(wlen + l, 1 << 20);
              wch = min(wch + 1, 1 << 20);
            }
            o += l;
          }
          if (iso && wlen && np < need) flush();
          rem &= rem - 1;
        }
      }
      continue;
    }
    skip = 0;  // a character that this chunk cuts off was found ill-formed by its first byte's lane
    if (UTF8 && np >= need) continue;
    if (p.lower && b >= 'A' && b <= 'Z') b += 32;
    const bool space = ascii_space(b), drop = ascii_drop(b), punct = ascii_punct(b);
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
          if (at < CAP) s_word[at] = (uint8_t)b;
        }
        wlen = min(wlen + __popcll(run), 1 << 20);
        wch = min(wch + __popcll(run), 1 << 20);
        rem &= ~below_q;
        if (q < 64) flush();
      } else {
        if (wlen) {  // a word from the previous chunk ends at this chunk's first kept byte
          flush();
          continue;
        }
        if ((pum >> first) & 1) {
          if (lane == first) s_word[0] = (uint8_t)b;
          wlen = wch = 1;
          flush();
          rem &= rem - 1;
        } else {
          const uint64_t next = rem & ~spm;
          rem = next ? rem & ~lanes_below(__ffsll((unsigned long long)next) - 1) : 0;
        }
      }
    }
  }
  if (wlen && np < need && !bad) flush();
  np = min(np, need);
  if (bad) {  // UTF8 only: nothing of the row stands
    for (int j = lane; j < L; j += 64) {
      out[j] = p.pad_id;
      if (mask) mask[(size_t)row * L + j] = 0;
    }
    if (len && lane == 0) len[row] = -1;
    return;
  }
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
  mec::DevBuf image;  // slots | pool | delim, then (WORDPIECE_UTF8) cp index | cp blocks | cp outputs
  mec::tok::Params p{};
};

using namespace mec;

namespace {

size_t pad16(size_t n) { return (n + 15) / 16 * 16; }

// Uploads the tables as one allocation and fills the handle. `cp` is null but for WORDPIECE_UTF8.
int create(const mec_tok_desc* d, const tok::HostTable& t, const tok::CpTable* cp, int device, mec_tokenizer** out) {
  MEC_HIP(hipSetDevice(device));
  const size_t slot_bytes = t.slots.size() * sizeof(tok::Slot);
  const size_t pool_bytes = pad16(t.pool.size());
  const size_t index_at = slot_bytes + pool_bytes + 256;
  const size_t block_at = index_at + (cp ? pad16(cp->index.size() * sizeof(uint16_t)) : 0);
  const size_t exp_at = block_at + (cp ? pad16(cp->block.size() * sizeof(uint32_t)) : 0);
  std::vector<uint8_t> image(exp_at + (cp ? pad16(cp->exp.size()) : 0), 0);
  std::memcpy(image.data(), t.slots.data(), slot_bytes);
  if (!t.pool.empty()) std::memcpy(image.data() + slot_bytes, t.pool.data(), t.pool.size());
  std::memcpy(image.data() + slot_bytes + pool_bytes, d->delim, 256);
  if (cp) {
    std::memcpy(image.data() + index_at, cp->index.data(), cp->index.size() * sizeof(uint16_t));
    std::memcpy(image.data() + block_at, cp->block.data(), cp->block.size() * sizeof(uint32_t));
    if (!cp->exp.empty()) std::memcpy(image.data() + exp_at, cp->exp.data(), cp->exp.size());
  }
  auto* h = new mec_tokenizer;
  h->kind = d->kind;
  h->device = device;
  if (upload(h->image, image.data(), image.size()) != 0) { delete h; return -1; }
  uint8_t* base = h->image.as<uint8_t>();
  h->p = tok::Params{reinterpret_cast<const tok::Slot*>(base), base + slot_bytes, base + slot_bytes + pool_bytes,
                     (uint32_t)(t.slots.size() - 1), t.max_len, d->oov_id, d->lower, d->unk_id, d->cls_id,
                     d->sep_id, d->pad_id, d->max_word,
                     reinterpret_cast<const uint16_t*>(base + index_at),
                     reinterpret_cast<const uint32_t*>(base + block_at), base + exp_at};
  *out = h;
  return 0;
}

}  // namespace

extern "C" {

int mec_tok_create(const mec_tok_desc* d, int device, mec_tokenizer** out) {
  API_GUARD({
    if (!out) { set_error("mec_tok_create: out is null"); return -1; }
    *out = nullptr;
    tok::HostTable t;
    std::string err;
    if (tok::build(d, &t, &err) != 0) { set_error(err); return -1; }
    return create(d, t, nullptr, device, out);
  })
}

int mec_tok_create_utf8(const mec_tok_desc* d, const mec_tok_cpmap* m, int device, mec_tokenizer** out) {
  API_GUARD({
    if (!out) { set_error("mec_tok_create_utf8: out is null"); return -1; }
    *out = nullptr;
    tok::HostTable t;
    tok::CpTable cp;
    std::string err;
    if (tok::build(d, &t, &err, true) != 0 || tok::build_cpmap(m, d->lower, &cp, &err) != 0) { set_error(err); return -1; }
    return create(d, t, &cp, device, out);
  })
}

int mec_tok_encode(mec_tokenizer* t, const uint8_t* text, const int64_t* text_off, int B, int L, int32_t* ids,
                   int32_t* mask, int32_t* len, void* stream) {
  MEC_REQUIRE(t, "mec_tok_encode: null tokenizer");
  MEC_REQUIRE(B >= 0, "mec_tok_encode: B < 0");
  const int lmin = t->kind == MEC_TOK_KERAS ? 1 : 2;
  MEC_REQUIRE(L >= lmin && L <= 512, "mec_tok_encode: L must be in 1..512 (WORDPIECE: 2..512)");
  if (B == 0) return 0;
  MEC_REQUIRE(text && text_off && ids, "mec_tok_encode: text, text_off or ids is null");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (t->kind == MEC_TOK_KERAS)
    hipLaunchKernelGGL(tok::keras_kernel, dim3(B), dim3(64), 0, s, t->p, text, text_off, B, L, ids, mask, len);
  else if (t->kind == MEC_TOK_WORDPIECE)
    hipLaunchKernelGGL(tok::wordpiece_kernel<false>, dim3(B), dim3(64), 0, s, t->p, text, text_off, B, L, ids, mask, len);
  else
    hipLaunchKernelGGL(tok::wordpiece_kernel<true>, dim3(B), dim3(64), 0, s, t->p, text, text_off, B, L, ids, mask, len);
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
