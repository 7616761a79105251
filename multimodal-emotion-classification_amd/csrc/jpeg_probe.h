// mec_jpeg_probe's parser (include/mec.h): which JPEG files the GPU decodes, their descriptor and their restart
// segments. Plain host C++ with no HIP in it, so that tools/jpeg_probe_check.cpp can build it with a sanitizer.
// Every read goes through Reader, which knows the file's length: arbitrary bytes give "host", never a read
// outside them.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "mec.h"

namespace mec {
namespace jp {

inline bool size_on_gpu(long long H, long long W) {  // mec_resize_on_gpu's domain (resize.hip rr::on_gpu)
  return H >= 1 && H <= 4096 && W >= 1 && W <= 4096 && H <= 100 * W;
}

// A Huffman table's 16 counts give canonical codes that fit their lengths, as libjpeg requires them (the
// all-ones code of a length is not allowed), and at most 256 values.
inline bool huff_ok(const uint8_t* counts) {
  int last = -1, total = 0;
  for (int l = 0; l < 16; ++l) {
    total += counts[l];
    if (counts[l]) last = l;
  }
  if (total > 256) return false;
  long long code = 0;
  for (int l = 0; l <= last; ++l) {
    code += counts[l];
    if (code >= (1LL << (l + 1))) return false;
    code <<= 1;
  }
  return true;
}

// The MCU grid of a frame: a one-component scan is not interleaved, its MCU is one block.
inline void mcu_grid(const mec_jpeg_desc& d, int* mx, int* my) {
  const int hmax = d.ncomp == 1 ? 1 : d.hs[0], vmax = d.ncomp == 1 ? 1 : d.vs[0];
  *mx = (d.W + 8 * hmax - 1) / (8 * hmax);
  *my = (d.H + 8 * vmax - 1) / (8 * vmax);
}

struct Reader {
  const uint8_t* d;
  size_t n;
  bool has(size_t pos, size_t k) const { return pos <= n && k <= n - pos; }
};

// 1: on the GPU, *desc filled and, where desc->nseg <= seg_cap, segs[2 k], segs[2 k + 1] = segment k's offset and
// length in the file. 0: the host decodes this file.
inline int probe(const uint8_t* data, size_t n, mec_jpeg_desc* out, int64_t* segs, int seg_cap) {
  const Reader r{data, n};
  if (!r.has(0, 4) || data[0] != 0xFF || data[1] != 0xD8) return 0;
  struct Huff {
    bool defined = false;
    mec_jpeg_huff t;
  } huff[2][2];
  bool qdef[4] = {false, false, false, false};
  uint16_t qt[4][64];
  bool have_frame = false;
  int H = 0, W = 0, nf = 0, cid[3], ch[3], cv[3], ctq[3];
  int restart = 0;
  size_t pos = 2;
  mec_jpeg_desc d;
  std::memset(&d, 0, sizeof d);
  for (;;) {
    if (!r.has(pos, 1) || data[pos] != 0xFF) return 0;
    while (pos < n && data[pos] == 0xFF) ++pos;  // fill bytes
    if (pos >= n) return 0;
    const int m = data[pos++];
    const bool known = m == 0xC0 || m == 0xC4 || m == 0xDB || m == 0xDD || m == 0xDA || m == 0xFE ||
                       (m >= 0xE0 && m <= 0xEF && m != 0xEE);
    if (!known) return 0;  // progressive, arithmetic, Adobe, DNL, a stand-alone marker, EOI before a scan, ...
    if (!r.has(pos, 2)) return 0;
    const size_t L = ((size_t)data[pos] << 8) | data[pos + 1];
    if (L < 2 || !r.has(pos, L)) return 0;
    const uint8_t* seg = data + pos + 2;
    const size_t sl = L - 2;
    pos += L;
    if (m == 0xC0) {
      if (have_frame || sl < 6) return 0;
      const int P = seg[0];
      H = (seg[1] << 8) | seg[2];
      W = (seg[3] << 8) | seg[4];
      nf = seg[5];
      if (P != 8 || (nf != 1 && nf != 3) || sl != (size_t)(6 + 3 * nf)) return 0;
      for (int i = 0; i < nf; ++i) {
        cid[i] = seg[6 + 3 * i];
        ch[i] = seg[7 + 3 * i] >> 4;
        cv[i] = seg[7 + 3 * i] & 15;
        ctq[i] = seg[8 + 3 * i];
        if (ctq[i] > 3) return 0;
      }
      if (nf == 1) {
        if (ch[0] != 1 || cv[0] != 1) return 0;
      } else {
        if (cid[0] != 1 || cid[1] != 2 || cid[2] != 3) return 0;
        if (ch[1] != 1 || cv[1] != 1 || ch[2] != 1 || cv[2] != 1) return 0;
        const bool ok = (ch[0] == 1 && cv[0] == 1) || (ch[0] == 2 && cv[0] == 1) || (ch[0] == 2 && cv[0] == 2);
        if (!ok) return 0;
      }
      if (!size_on_gpu(H, W) || (ch[0] == 2 && W < 5)) return 0;
      have_frame = true;
    } else if (m == 0xC4) {
      size_t at = 0;
      while (at < sl) {
        if (sl - at < 17) return 0;
        const int tc = seg[at] >> 4, th = seg[at] & 15;
        if (tc > 1 || th > 1 || !huff_ok(seg + at + 1)) return 0;
        size_t nv = 0;
        for (int l = 0; l < 16; ++l) nv += seg[at + 1 + l];
        if (sl - at - 17 < nv) return 0;
        Huff& h = huff[tc][th];
        h.defined = true;
        std::memset(&h.t, 0, sizeof h.t);
        std::memcpy(h.t.counts, seg + at + 1, 16);
        std::memcpy(h.t.vals, seg + at + 17, nv);
        at += 17 + nv;
      }
    } else if (m == 0xDB) {
      size_t at = 0;
      while (at < sl) {
        if ((seg[at] >> 4) != 0 || (seg[at] & 15) > 3 || sl - at < 65) return 0;
        const int tq = seg[at] & 15;
        qdef[tq] = true;
        for (int k = 0; k < 64; ++k) qt[tq][k] = seg[at + 1 + k];
        at += 65;
      }
    } else if (m == 0xDD) {
      if (sl != 2) return 0;
      restart = (seg[0] << 8) | seg[1];
    } else if (m == 0xDA) {
      if (!have_frame || sl != (size_t)(4 + 2 * nf) || seg[0] != nf) return 0;
      d.H = H;
      d.W = W;
      d.ncomp = nf;
      d.restart = restart;
      for (int i = 0; i < nf; ++i) {
        const int td = seg[2 + 2 * i] >> 4, ta = seg[2 + 2 * i] & 15;
        if (seg[1 + 2 * i] != cid[i] || td > 1 || ta > 1) return 0;
        if (!qdef[ctq[i]] || !huff[0][td].defined || !huff[1][ta].defined) return 0;
        d.hs[i] = ch[i];
        d.vs[i] = cv[i];
        std::memcpy(d.qt[i], qt[ctq[i]], sizeof d.qt[i]);
        d.dc[i] = huff[0][td].t;
        d.ac[i] = huff[1][ta].t;
      }
      if (seg[1 + 2 * nf] != 0 || seg[2 + 2 * nf] != 63 || seg[3 + 2 * nf] != 0) return 0;
      break;
    }
  }
  // the entropy-coded data, up to the next marker that is no RSTn; it must be EOI
  int mx, my;
  mcu_grid(d, &mx, &my);
  const long long mcus = (long long)mx * my;
  const long long want = restart ? (mcus + restart - 1) / restart : 1;
  long long nseg = 0;
  int expect = 0;
  size_t start = pos, p = pos;
  for (;;) {
    const void* f = p < n ? std::memchr(data + p, 0xFF, n - p) : nullptr;
    if (!f) return 0;  // the data ends without a marker
    p = (size_t)(static_cast<const uint8_t*>(f) - data);
    size_t q = p;
    while (q < n && data[q] == 0xFF) ++q;
    if (q >= n) return 0;
    const int b = data[q];
    if (b == 0) {
      if (q != p + 1) return 0;  // fill bytes before a stuffed zero
      p = q + 1;
      continue;
    }
    if (nseg >= want) return 0;
    if (nseg < seg_cap && segs) {
      segs[2 * nseg] = (int64_t)start;
      segs[2 * nseg + 1] = (int64_t)(p - start);
    }
    ++nseg;
    if (b >= 0xD0 && b <= 0xD7) {
      if (restart == 0 || b != 0xD0 + expect) return 0;
      expect = (expect + 1) & 7;
      start = p = q + 1;
      continue;
    }
    if (b != 0xD9) return 0;
    break;
  }
  if (nseg != want || nseg > 0x7fffffff) return 0;
  d.nseg = (int32_t)nseg;
  *out = d;
  return 1;
}

}  // namespace jp
}  // namespace mec
