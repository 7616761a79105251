// The tokenizer's vocabulary table (include/mec.h mec_tok_create): the hash, the slot layout and the
// lookup shared by the host builder and the kernels of tokenizer.hip, and the host builder itself.
// Plain C++ apart from the __host__ __device__ marks, so the builder also compiles into a stand-alone
// host program (tools/tok_table_check.cpp, run under the address and undefined-behaviour sanitizers).
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "mec.h"

#if defined(__HIPCC__)
#define MEC_TOK_HD __host__ __device__ inline
#else
#define MEC_TOK_HD inline
#endif

namespace mec {
namespace tok {

// Key = (flag, bytes): flag 1 marks a WordPiece continuation entry ("##" + bytes in the pool form).
// The hash is polynomial mod 2^32, h = sum (b_i + 1) P^(len-1-i), so that the kernel gets the hash of any
// substring of a word from the word's prefix hashes: h[s,e) = H[e] - H[s] P^(e-s). finish() mixes in the
// length and the flag and avalanches, since the low bits of h depend on the low bits of the bytes only.
constexpr uint32_t kP = 0x01000193u;
constexpr int kMaxEntry = 65535;  // bytes per entry
constexpr int kFlagShift = 20;    // lenflag = len | flag << 20; negative = empty slot
constexpr int kWordCap = 128;     // mec_tok_desc.max_word's bound: the kernel's per-word buffers

struct alignas(16) Slot {
  uint32_t hash;
  int32_t off;      // of the entry's bytes (after "##") in the device pool
  int32_t lenflag;
  int32_t id;
};

MEC_TOK_HD uint32_t step(uint32_t h, uint32_t b) { return h * kP + b + 1u; }

MEC_TOK_HD uint32_t finish(uint32_t h, int len, int flag) {
  uint32_t x = h + (uint32_t)len * 0x9E3779B1u + (uint32_t)flag * 0x7F4A7C15u;
  x ^= x >> 16;
  x *= 0x85EBCA6Bu;
  x ^= x >> 13;
  x *= 0xC2B2AE35u;
  x ^= x >> 16;
  return x;
}

MEC_TOK_HD int32_t lenflag(int len, int flag) { return len | (flag << kFlagShift); }

// The id of (flag, key(0) .. key(len-1)), or -1. `mask` = slots - 1 (a power of two); the builder keeps
// the load factor <= 1/2, so a probe sequence always meets an empty slot.
template <class Key>
MEC_TOK_HD int lookup(const Slot* slots, uint32_t mask, const uint8_t* pool, uint32_t hash, int len, int flag,
                      Key key) {
  const int32_t lf = lenflag(len, flag);
  uint32_t i = hash & mask;
  for (uint32_t probe = 0; probe <= mask; ++probe, i = (i + 1) & mask) {
    const Slot s = slots[i];
    if (s.lenflag < 0) return -1;
    if (s.hash == hash && s.lenflag == lf) {
      int k = 0;
      while (k < len && pool[s.off + k] == key(k)) ++k;
      if (k == len) return s.id;
    }
  }
  return -1;
}

struct HostTable {
  std::vector<Slot> slots;
  std::vector<uint8_t> pool;
  int max_len = 0;  // longest entry (without "##"): a longer word or piece cannot match
};

// Validates the descriptor and builds the table. 0, or -1 with *err set.
inline int build(const mec_tok_desc* d, HostTable* t, std::string* err) {
  auto fail = [&](const std::string& m) {
    *err = "mec_tok_create: " + m;
    return -1;
  };
  if (!d) return fail("the descriptor is null");
  if (d->kind != MEC_TOK_KERAS && d->kind != MEC_TOK_WORDPIECE) return fail("kind must be MEC_TOK_KERAS or MEC_TOK_WORDPIECE");
  const bool wp = d->kind == MEC_TOK_WORDPIECE;
  if (d->n < 0) return fail("n < 0");
  if (d->n > (1 << 26)) return fail("n > 2^26 entries");
  if (d->n > 0 && (!d->off || !d->id)) return fail("off or id is null");
  if (wp) {
    if (d->unk_id < 0 || d->cls_id < 0 || d->sep_id < 0 || d->pad_id < 0) return fail("unk_id, cls_id, sep_id and pad_id must be >= 0");
    if (d->max_word < 1 || d->max_word > kWordCap) return fail("max_word must be in 1..128");
  } else if (d->oov_id < -1) {
    return fail("oov_id must be >= 0, or -1 to drop unknown words");
  }
  const int n = d->n;
  const int64_t base = n ? d->off[0] : 0;
  if (base < 0) return fail("off[0] < 0");
  for (int e = 0; e < n; ++e) {
    if (d->off[e + 1] < d->off[e]) return fail("off is not monotone at entry " + std::to_string(e));
    if (d->off[e + 1] - d->off[e] > kMaxEntry) return fail("entry " + std::to_string(e) + " is longer than 65535 bytes");
    if (d->id[e] < 0) return fail("entry " + std::to_string(e) + " has an id < 0");
  }
  const int64_t bytes = n ? d->off[n] - base : 0;
  if (bytes > 0 && !d->pool) return fail("pool is null");
  if (bytes >= (int64_t(1) << 31)) return fail("the pool holds 2^31 bytes or more");
  t->pool.assign(d->pool + (bytes ? base : 0), d->pool + (bytes ? base : 0) + bytes);
  if (wp)
    for (int64_t i = 0; i < bytes; ++i)
      if (t->pool[i] >= 0x80) return fail("a WORDPIECE entry holds a byte >= 0x80 (7-bit entries only)");
  size_t cap = 16;
  while (cap < 2 * (size_t)n) cap <<= 1;
  t->slots.assign(cap, Slot{0u, 0, -1, 0});
  t->max_len = 0;
  const uint32_t mask = (uint32_t)(cap - 1);
  const uint8_t* pool = t->pool.data();
  for (int e = 0; e < n; ++e) {
    int off = (int)(d->off[e] - base), len = (int)(d->off[e + 1] - d->off[e]), flag = 0;
    if (wp && len > 2 && pool[off] == '#' && pool[off + 1] == '#') off += 2, len -= 2, flag = 1;
    uint32_t h = 0;
    for (int k = 0; k < len; ++k) h = step(h, pool[off + k]);
    h = finish(h, len, flag);
    const int32_t lf = lenflag(len, flag);
    uint32_t i = h & mask;
    for (; t->slots[i].lenflag >= 0; i = (i + 1) & mask) {
      const Slot& s = t->slots[i];
      if (s.hash == h && s.lenflag == lf && (len == 0 || std::memcmp(pool + s.off, pool + off, (size_t)len) == 0))
        return fail("entry " + std::to_string(e) + " duplicates an earlier entry");
    }
    t->slots[i] = Slot{h, off, lf, d->id[e]};
    if (len > t->max_len) t->max_len = len;
  }
  return 0;
}

}  // namespace tok
}  // namespace mec
