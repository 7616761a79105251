// The tokenizer's vocabulary table (include/mec.h mec_tok_create): the hash, the slot layout and the
// lookup shared by the host builder and the kernels of tokenizer.hip, and the host builder itself; then the
// same for the code-point table of MEC_TOK_WORDPIECE_UTF8 (mec_tok_create_utf8).
// Plain C++ apart from the __host__ __device__ marks, so the builders also compile into stand-alone host
// programs (tools/tok_table_check.cpp and tools/tok_cpmap_check.cpp, run under the address and
// undefined-behaviour sanitizers).
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
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

// The 7-bit rules of both WORDPIECE kinds, shared by the kernels and the code-point table's builder.
MEC_TOK_HD bool ascii_space(uint32_t b) { return b == ' ' || b == '\t' || b == '\n' || b == '\r'; }
MEC_TOK_HD bool ascii_drop(uint32_t b) { return !ascii_space(b) && (b < 0x20 || b == 0x7F); }
MEC_TOK_HD bool ascii_punct(uint32_t b) {
  return (b >= 33 && b <= 47) || (b >= 58 && b <= 64) || (b >= 91 && b <= 96) || (b >= 123 && b <= 126);
}

// Is s[0, n) well-formed UTF-8 (no overlong form, no surrogate, nothing above 0x10FFFF, nothing cut off)?
inline bool utf8_well_formed(const uint8_t* s, int64_t n) {
  for (int64_t i = 0; i < n;) {
    const uint32_t b = s[i];
    if (b < 0x80) {
      ++i;
      continue;
    }
    const int len = b < 0xC2 ? 0 : b < 0xE0 ? 2 : b < 0xF0 ? 3 : b <= 0xF4 ? 4 : 0;
    if (!len || i + len > n) return false;
    uint32_t cp = b & (0x7Fu >> len);
    for (int k = 1; k < len; ++k) {
      if ((s[i + k] & 0xC0) != 0x80) return false;
      cp = cp << 6 | (s[i + k] & 0x3Fu);
    }
    if (cp < (len == 2 ? 0x80u : len == 3 ? 0x800u : 0x10000u) || (cp >= 0xD800 && cp <= 0xDFFF) || cp > 0x10FFFF)
      return false;
    i += len;
  }
  return true;
}

// Validates the descriptor and builds the table. 0, or -1 with *err set. MEC_TOK_WORDPIECE_UTF8 is a valid
// kind only with `utf8` (mec_tok_create_utf8); its entries are any well-formed UTF-8.
inline int build(const mec_tok_desc* d, HostTable* t, std::string* err, bool utf8 = false) {
  auto fail = [&](const std::string& m) {
    *err = (utf8 ? "mec_tok_create_utf8: " : "mec_tok_create: ") + m;
    return -1;
  };
  if (!d) return fail("the descriptor is null");
  if (utf8) {
    if (d->kind != MEC_TOK_WORDPIECE_UTF8) return fail("kind must be MEC_TOK_WORDPIECE_UTF8");
  } else if (d->kind != MEC_TOK_KERAS && d->kind != MEC_TOK_WORDPIECE) {
    return fail("kind must be MEC_TOK_KERAS or MEC_TOK_WORDPIECE");
  }
  const bool wp = d->kind != MEC_TOK_KERAS;
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
  if (utf8) {
    for (int e = 0; e < n; ++e)
      if (!utf8_well_formed(t->pool.data() + (d->off[e] - base), d->off[e + 1] - d->off[e]))
        return fail("entry " + std::to_string(e) + " is not well-formed UTF-8");
  } else if (wp) {
    for (int64_t i = 0; i < bytes; ++i)
      if (t->pool[i] >= 0x80) return fail("a WORDPIECE entry holds a byte >= 0x80 (7-bit entries only)");
  }
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

// The code-point table of MEC_TOK_WORDPIECE_UTF8 (mec_tok_cpmap) in the form the kernel reads: two stages,
// entry(cp) = block[index[cp >> 7] * 128 + (cp & 127)], identical blocks stored once. An entry is
// class | ISOLATE | (offset into `exp`) << 4; the offset is used by MAPPED entries only and names a record
// {bytes, outputs | punctuation flags << 2, the outputs' UTF-8 bytes}, identical records stored once.
constexpr int kCpLimit = 0x110000, kCpBlock = 128, kCpBlocks = kCpLimit / kCpBlock;
constexpr int kCpExpShift = 4, kCpMaxOut = 3;

struct CpTable {
  std::vector<uint16_t> index;  // [kCpBlocks]
  std::vector<uint32_t> block;  // [blocks * kCpBlock]
  std::vector<uint8_t> exp;
};

MEC_TOK_HD uint32_t cp_entry(const uint16_t* index, const uint32_t* block, uint32_t cp) {
  return block[(uint32_t)index[cp >> 7] * kCpBlock + (cp & 127)];
}

inline int utf8_put(uint32_t cp, uint8_t* out) {
  if (cp < 0x80) return out[0] = (uint8_t)cp, 1;
  if (cp < 0x800) return out[0] = (uint8_t)(0xC0 | cp >> 6), out[1] = (uint8_t)(0x80 | (cp & 0x3F)), 2;
  if (cp < 0x10000)
    return out[0] = (uint8_t)(0xE0 | cp >> 12), out[1] = (uint8_t)(0x80 | (cp >> 6 & 0x3F)),
           out[2] = (uint8_t)(0x80 | (cp & 0x3F)), 3;
  return out[0] = (uint8_t)(0xF0 | cp >> 18), out[1] = (uint8_t)(0x80 | (cp >> 12 & 0x3F)),
         out[2] = (uint8_t)(0x80 | (cp >> 6 & 0x3F)), out[3] = (uint8_t)(0x80 | (cp & 0x3F)), 4;
}

// Validates the map and builds the table. 0, or -1 with *err set. `lower` folds A-Z among the outputs.
inline int build_cpmap(const mec_tok_cpmap* m, int lower, CpTable* t, std::string* err) {
  auto fail = [&](const std::string& s) {
    *err = "mec_tok_create_utf8: " + s;
    return -1;
  };
  auto hex = [](int64_t cp) {
    char buf[32];
    std::snprintf(buf, sizeof buf, "U+%04llX", (unsigned long long)cp);
    return std::string(buf);
  };
  auto surrogate = [](int64_t cp) { return cp >= 0xD800 && cp <= 0xDFFF; };
  if (!m) return fail("the code-point map is null");
  if (!m->cls) return fail("cls is null");
  if (m->n_map < 0) return fail("n_map < 0");
  if (!m->map_off || (m->n_map > 0 && !m->map_cp)) return fail("map_cp or map_off is null");
  const uint8_t* cls = m->cls;
  int mapped = 0;
  for (int cp = 0x80; cp < kCpLimit; ++cp) {
    const int c = cls[cp] & 7;
    if ((cls[cp] & ~(7 | MEC_CP_ISOLATE)) || c > MEC_CP_MAPPED) return fail(hex(cp) + " has an unknown class");
    if (surrogate(cp) && c != MEC_CP_UNCOVERED) return fail("the surrogate " + hex(cp) + " is not UNCOVERED");
    mapped += c == MEC_CP_MAPPED;
  }
  if (m->map_off[0] != 0) return fail("map_off[0] != 0");
  for (int i = 0; i < m->n_map; ++i) {
    const int64_t cp = m->map_cp[i];
    if (cp < 0x80 || cp >= kCpLimit) return fail("map_cp holds " + hex(cp) + ", outside 0x80..0x10FFFF");
    if (i && cp <= m->map_cp[i - 1]) return fail("map_cp is not ascending at " + hex(cp));
    if ((cls[cp] & 7) != MEC_CP_MAPPED) return fail("map_cp holds " + hex(cp) + ", whose class is not MAPPED");
    const int64_t k = (int64_t)m->map_off[i + 1] - m->map_off[i];
    if (k < 0) return fail("map_off is not monotone at " + hex(cp));
    if (k > kCpMaxOut) return fail(hex(cp) + " has more than 3 outputs");
    if (k > 0 && !m->map_out) return fail("map_out is null");
  }
  if (mapped != m->n_map) return fail("a code point of class MAPPED is missing from map_cp");
  t->exp.clear();
  std::map<std::string, uint32_t> records;
  std::vector<uint32_t> entry(kCpLimit);
  for (int cp = 0; cp < kCpLimit; ++cp) entry[cp] = cp < 0x80 ? 0u : cls[cp];
  for (int i = 0; i < m->n_map; ++i) {
    std::string rec(2, '\0');
    int flags = 0;
    const int k = m->map_off[i + 1] - m->map_off[i];
    for (int j = 0; j < k; ++j) {
      int64_t o = m->map_out[m->map_off[i] + j];
      if (o < 0 || o >= kCpLimit || surrogate(o)) return fail(hex(m->map_cp[i]) + " has an output that is no code point");
      bool punct;
      if (o < 0x80) {
        if (ascii_space((uint32_t)o) || ascii_drop((uint32_t)o))
          return fail(hex(m->map_cp[i]) + " has the output " + hex(o) + ", which the 7-bit rules do not keep");
        if (lower && o >= 'A' && o <= 'Z') o += 32;
        punct = ascii_punct((uint32_t)o);
      } else {
        const int c = cls[o] & 7;
        if (c != MEC_CP_CHAR && c != MEC_CP_PUNCT)
          return fail(hex(m->map_cp[i]) + " has the output " + hex(o) + ", whose class is not CHAR or PUNCT");
        punct = c == MEC_CP_PUNCT;
      }
      uint8_t buf[4];
      rec.append(reinterpret_cast<const char*>(buf), (size_t)utf8_put((uint32_t)o, buf));
      flags |= (int)punct << j;
    }
    rec[0] = (char)(rec.size() - 2);
    rec[1] = (char)(k | flags << 2);
    auto it = records.find(rec);
    if (it == records.end()) {
      it = records.emplace(rec, (uint32_t)t->exp.size()).first;
      t->exp.insert(t->exp.end(), rec.begin(), rec.end());
    }
    entry[m->map_cp[i]] |= it->second << kCpExpShift;
  }
  t->index.assign(kCpBlocks, 0);
  t->block.clear();
  std::map<std::vector<uint32_t>, uint16_t> blocks;
  for (int b = 0; b < kCpBlocks; ++b) {
    std::vector<uint32_t> blk(entry.begin() + (size_t)b * kCpBlock, entry.begin() + (size_t)(b + 1) * kCpBlock);
    auto it = blocks.find(blk);
    if (it == blocks.end()) {
      it = blocks.emplace(blk, (uint16_t)blocks.size()).first;
      t->block.insert(t->block.end(), blk.begin(), blk.end());
    }
    t->index[b] = it->second;
  }
  return 0;
}

}  // namespace tok
}  // namespace mec
