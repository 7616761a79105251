// Pipelined fp16 MFMA GEMM / implicit-GEMM conv for gfx950 (the main GEMM engine).
//
//   C[M,N] = epilogue( A'[M,K] . B[N,K]^T ),  A' = A (A_PLAIN) or im2col(NHWC) (A_CONV)
//   or [A | 1x1/stride-s view of A2] concatenated along K (A_DUAL: a ResNet bottleneck's
//   conv3 and its downsample projection as one GEMM)
//
// * Tile BM=256 x BN (64/128/256) x BK=64, 512 threads = 8 waves (WM x WN), each wave a
//   (BM/WM) x (BN/WN) block of v_mfma_f32_32x32x16_f16 accumulators.
// * Operands move HBM/L2 -> LDS by global_load_lds_dwordx4 (no VGPR staging) into an
//   NS-stage ring; a tile is waited for with a counted `s_waitcnt vmcnt` (later tiles
//   stay in flight) and published with a raw s_barrier. LDS rows are 128 B with the
//   chunk XOR swizzle kc ^ ((row>>1)&7) applied on the per-lane SOURCE address (the DMA
//   destination is lane-linear), so the ds_read_b128 fragment reads are conflict-free.
// * Conv padding / M-tail rows: the lane's source is redirected to a zero page, so the
//   DMA itself writes the zeros (no predicated stores into the image).
// * Epilogue: each wave stages 32-row slabs of its accumulators through LDS and writes
//   them back row-contiguous: bias, residual (f16/f32), ReLU/GELU, f16 and/or f32 out
//   with 16-byte loads/stores.
// * XCD-aware bijective block remap: blocks that share an A panel share an L2.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <mutex>

#include "gemm_common.h"
#include "gemm_tiles.h"

namespace mec {

__device__ __attribute__((aligned(64))) uint4 g_zero_page[16];

template <int BM, int BN, int WM, int WN, int NS, int AM, int DBG = 0, int MF = 32, int BK = 64, int PRE = 0,
          int ACT = -1, int SP = 0>
__global__ __launch_bounds__(64 * WM * WN, (WM * WN == 4) ? 2 : 1) void gemm_glds_kernel(const GemmParams p) {
  // MF: 32 = v_mfma_f32_32x32x16_f16 tiles, 16 = v_mfma_f32_16x16x32_f16 tiles
  // DBG (probe builds only): 1 = no operand loads inside the K loop, 2 = no epilogue
  // PRE: the residual tile (1 = f16, 2 = f32, 3 = f16 hi / lo planes of a split residual) is
  // loaded into registers before the main loop,
  // so its HBM read hides under the operand loads and MFMAs instead of following them
  // (ResNet's short-K conv3 GEMMs, BERT's O-projection)
  // SP: split-f16 operands (GemmParams::split). SP = 1 (pass-major): the K loop runs over 3 K
  // passes, pass 0 reading the A lo plane, pass 1 the B lo plane, pass 2 both hi planes. SP = 2
  // (interleaved, opt().gemm_x3_order 1): one K loop; a stage holds the hi AND lo tiles of A and B
  // (two halves), and each 32-deep k chunk runs its three MFMA terms (lo.hi, hi.lo, hi.hi) back to
  // back: every operand byte is fetched and staged once instead of 1.5 times on average, and four
  // fragment reads feed three MFMAs instead of six. 16x16x32 tiles only (one k-chunk order).
  // SP = 3 (paired, GemmParams::a_pair / b_pair): SP = 2's loop on operands stored [rows][2K], each
  // 32-deep K chunk's hi halfs followed by its lo halfs. A stage is [BM + BN] rows of 64 halfs (hi in
  // chunks 0-3, lo in 4-7), filled by 8-row x 128-B pieces (whole cache lines; SP = 2's 16-row x 64-B
  // pieces take half lines of one plane) and swizzled with sw<64>; the fragment of plane h is chunk
  // 4 h + lq, the f16 BK = 64 path's address pattern. Same piece count, fragments and MFMA order as
  // SP = 2: same bits. Plain A only.
  static_assert(BK == 64 || BK == 32, "BK");
  static_assert(SP == 0 || PRE == 0 || PRE == 3, "split operands: split residual prefetch only");
  static_assert(SP < 2 || MF == 16, "interleaved split: 16x16x32 tiles only");
  static_assert(SP != 3 || (BK == 32 && AM == A_PLAIN && PRE == 0), "paired split: 32-deep stages, plain A");
  // NS = 1 (tile 72128, interleaved split operands): one stage, read whole into fragment registers; once every
  // wave holds them the stage is refilled for step t + 1 under step t's MFMAs (bert_qkv_attn_x3_kernel's
  // schedule). 48 KB of LDS lets two workgroups share a CU, so one's barriers, loads and epilogue run under
  // the other's MFMAs. Same fragments, same MFMA order as the ring tiles: same bits.
  static_assert(NS != 1 || (SP >= 2 && BK == 32 && DBG == 0), "one-stage tile: interleaved split operands only");
  constexpr int LBK = SP == 3 ? 64 : BK;       // halfs per LDS row (paired: a K chunk's hi and lo halfs)
  constexpr int CH = LBK / 8;                  // 16-B chunks per LDS row
  constexpr int RPI = 64 / CH;                 // rows per glds wave-instruction (1 KB)
  constexpr int NW = WM * WN;
  static_assert(NW == 8 || NW == 4, "4 or 8 waves");
  constexpr int TM = BM / WM, TN = BN / WN;    // wave tile
  constexpr int TI = TM / MF, TJ = TN / MF;    // MFxMF MFMA tiles per wave
  typedef float accv __attribute__((ext_vector_type(MF == 32 ? 16 : 4)));
  constexpr int NACC = MF == 32 ? 16 : 4;
  constexpr int AI = BM / RPI / NW;            // glds wave-instructions per stage (A)
  constexpr int BI = BN / RPI / NW;            // (B)
  static_assert(BI >= 1 && AI >= 1, "tile too small for 8 waves");
  constexpr int NPL = SP == 2 ? 2 : 1;         // operand planes per stage
  constexpr int LPT = (AI + BI) * NPL;
  constexpr int HALF = (BM + BN) * LBK;        // halfs per plane of a stage (paired: the whole stage)
  constexpr int STAGE = HALF * NPL;            // halfs per stage
  constexpr int EPI_LD = TN + 4;               // f32 staging row (padded)
  constexpr int EPI = NW * 32 * EPI_LD;        // floats for the epilogue staging
  constexpr int SMEM_H = (NS * STAGE > EPI * 2) ? NS * STAGE : EPI * 2;
  __shared__ __attribute__((aligned(16))) f16 smem[SMEM_H];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave - (wave / WN) * WN;
  const int M = p.M, N = p.N, K = p.K;
  const int LDK = SP == 3 ? 2 * K : K;  // halfs per operand row in memory
  const int nbn = N / BN;
  const int nbm = (M + BM - 1) / BM;
  const int nwg = nbm * nbn;
  int bid = blockIdx.x;
  {
    const int xcd = bid & 7, q = nwg >> 3, r = nwg & 7;
    bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
  }
  int bm, bn;
  tile_coords(bid, nbm, nbn, p.group_m, bm, bn);
  const int m0 = bm * BM, n0 = bn * BN;

  // ---- per-lane DMA sources: lane -> (row in its 8-row group, physical chunk)
  const int lrow = lane / CH, pchunk = lane % CH;
  const f16* a_src[AI];
  const f16* a2_src[AI];  // A_DUAL: second source (1x1 / stride-s view of an NHWC tensor)
  int a_ih0[AI], a_iw0[AI];
  bool a_ok[AI];
#pragma unroll
  for (int i = 0; i < AI; ++i) {
    const int r = (wave * AI + i) * RPI + lrow;  // row within tile
    const int m = m0 + r;
    a_ok[i] = m < M;
    const int mc = a_ok[i] ? m : 0;
    const int kc = sw<LBK>(r, pchunk);
    if constexpr (AM == A_PLAIN) {
      a_src[i] = reinterpret_cast<const f16*>(p.A) + (size_t)mc * LDK + kc * 8;
    } else if constexpr (AM == A_DUAL) {
      a_src[i] = reinterpret_cast<const f16*>(p.A) + (size_t)mc * p.K1 + kc * 8;
      const int ohw = p.OH * p.OW;
      const int n = mc / ohw;
      const int rem = mc - n * ohw;
      const int oh = rem / p.OW;
      const int ow = rem - oh * p.OW;
      a2_src[i] = reinterpret_cast<const f16*>(p.A2) +
                  (((size_t)n * p.H + oh * p.stride) * p.W + ow * p.stride) * p.C + kc * 8;
    } else {
      const int ohw = p.OH * p.OW;
      const int n = mc / ohw;
      const int rem = mc - n * ohw;
      const int oh = rem / p.OW;
      const int ow = rem - oh * p.OW;
      a_ih0[i] = oh * p.stride - p.pad;
      a_iw0[i] = ow * p.stride - p.pad;
      a_src[i] = reinterpret_cast<const f16*>(p.A) + (size_t)n * p.H * p.W * p.C + kc * 8;
    }
  }
  const f16* b_src[BI];
#pragma unroll
  for (int j = 0; j < BI; ++j) {
    const int r = (wave * BI + j) * RPI + lrow;
    const int kc = sw<LBK>(r, pchunk);
    b_src[j] = p.B + (size_t)(n0 + r) * LDK + kc * 8;
  }
  const f16* zero = reinterpret_cast<const f16*>(g_zero_page);

  const int nk0 = K / BK;  // K tiles per pass
  // one plane of K tile kt into stage `stage` (its half h): A at aoff, B at boff from the hi planes (glds16:
  // the fragment reads below keep counted lgkmcnt waits)
  auto issue_plane = [&](int stage, int kt, int h, long long aoff, long long boff) {
    const int k0 = kt * LBK;
    f16* sA = smem + stage * STAGE + h * HALF;
    f16* sB = sA + BM * LBK;
    if constexpr (AM == A_PLAIN) {
#pragma unroll
      for (int i = 0; i < AI; ++i) {
        const f16* src = a_ok[i] ? a_src[i] + aoff + k0 : zero;
        glds16(src, (lds_vptr)(sA + (wave * AI + i) * RPI * LBK));
      }
    } else if constexpr (AM == A_DUAL) {
      const bool first = k0 < p.K1;
#pragma unroll
      for (int i = 0; i < AI; ++i) {  // split: both sources' lo planes at the same offset a_lo
        const f16* src = !a_ok[i] ? zero : (first ? a_src[i] + aoff + k0 : a2_src[i] + aoff + (k0 - p.K1));
        glds16(src, (lds_vptr)(sA + (wave * AI + i) * RPI * LBK));
      }
    } else {
      const int tap = k0 / p.C;
      const int c0 = k0 - tap * p.C;
      const int kh = tap / p.ks;
      const int kw = tap - kh * p.ks;
#pragma unroll
      for (int i = 0; i < AI; ++i) {
        const int ih = a_ih0[i] + kh, iw = a_iw0[i] + kw;
        const bool ok = a_ok[i] && ih >= 0 && ih < p.H && iw >= 0 && iw < p.W;
        const f16* src = ok ? a_src[i] + aoff + ((size_t)ih * p.W + iw) * p.C + c0 : zero;
        glds16(src, (lds_vptr)(sA + (wave * AI + i) * RPI * LBK));
      }
    }
#pragma unroll
    for (int j = 0; j < BI; ++j)
      glds16(b_src[j] + boff + k0, (lds_vptr)(sB + (wave * BI + j) * RPI * LBK));
  };
  auto issue = [&](int stage, int kt) {
    if constexpr (SP == 1) {  // pass 0: A_lo . B_hi, pass 1: A_hi . B_lo, pass 2: A_hi . B_hi
      const int pl = (kt >= nk0) + (kt >= 2 * nk0);
      issue_plane(stage, kt - pl * nk0, 0, pl == 0 ? p.a_lo : 0, pl == 1 ? p.b_lo : 0);
    } else if constexpr (SP == 2) {  // hi planes into half 0, lo planes into half 1
      issue_plane(stage, kt, 0, 0, 0);
      issue_plane(stage, kt, 1, p.a_lo, p.b_lo);
    } else {  // (paired: one 128-B row piece carries both planes)
      issue_plane(stage, kt, 0, 0, 0);
    }
  };
  // fragment of plane h (0 hi, 1 lo) of stage row r, 16-B k chunk kcs, in the A or B tile at s
  auto frag = [&](const f16* s, int h, int r, int kcs) {
    if constexpr (SP == 3) return *reinterpret_cast<const half8*>(s + r * 64 + sw<64>(r, 4 * h + kcs) * 8);
    else return *reinterpret_cast<const half8*>(s + h * HALF + r * BK + sw<BK>(r, kcs) * 8);
  };

  using EG = EpiGeom<BM, BN, WM, WN>;
  half8 rpre[(PRE == 1 || PRE == 3) ? EG::SLABS : 1][EG::NPS];
  half8 rplo[PRE == 3 ? EG::SLABS : 1][EG::NPS];
  float4 rpre32[PRE == 2 ? EG::SLABS : 1][EG::NPS][2];
  if constexpr (PRE != 0) {
    const int ech = lane % EG::CPR, erow = lane / EG::CPR;
    const int col0 = n0 + wn * TN + ech * 8;
#pragma unroll
    for (int i = 0; i < EG::SLABS; ++i)
#pragma unroll
      for (int ps = 0; ps < EG::NPS; ++ps) {
        const size_t off = (size_t)min(m0 + wm * TM + i * 32 + ps * EG::RPP + erow, M - 1) * N + col0;
        if constexpr (PRE == 1 || PRE == 3) {
          rpre[i][ps] = *reinterpret_cast<const half8*>(reinterpret_cast<const f16*>(p.R) + off);
          if constexpr (PRE == 3) rplo[i][ps] = *reinterpret_cast<const half8*>(reinterpret_cast<const f16*>(p.R) + off + p.r_lo);
        } else {
          const float* R = reinterpret_cast<const float*>(p.R) + off;
          rpre32[i][ps][0] = *reinterpret_cast<const float4*>(R);
          rpre32[i][ps][1] = *reinterpret_cast<const float4*>(R + 4);
        }
      }
  }

  accv acc[TI][TJ];
#pragma unroll
  for (int i = 0; i < TI; ++i)
#pragma unroll
    for (int j = 0; j < TJ; ++j)
#pragma unroll
      for (int e = 0; e < NACC; ++e) acc[i][j][e] = 0.f;

  const int nk = SP == 1 ? 3 * nk0 : nk0;
#pragma unroll
  for (int s = 0; s < (NS == 1 ? 1 : NS - 1); ++s)
    if (s < nk) issue(s, s);

  const int lr = lane & 31, lh = lane >> 5;
  if constexpr (NS == 1) {
    const int l16 = lane & 15, lq = lane >> 4;
    for (int t = 0; t < nk; ++t) {
      wait_vm<0>();
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      const f16* sA = smem;
      const f16* sB = sA + BM * LBK;
      half8 af[2][TI], bf[2][TJ];  // [plane: 0 hi, 1 lo]
#pragma unroll
      for (int h = 0; h < 2; ++h) {
#pragma unroll
        for (int i = 0; i < TI; ++i) {
          const int r = wm * TM + i * 16 + l16;
          af[h][i] = frag(sA, h, r, lq);
        }
#pragma unroll
        for (int j = 0; j < TJ; ++j) {
          const int r = wn * TN + j * 16 + l16;
          bf[h][j] = frag(sB, h, r, lq);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();  // every wave holds its fragments: the stage is free
      if (t + 1 < nk) issue(0, t + 1);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int j = 0; j < TJ; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[1][i], bf[0][j], acc[i][j], 0, 0, 0);
#pragma unroll
      for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int j = 0; j < TJ; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[0][i], bf[1][j], acc[i][j], 0, 0, 0);
#pragma unroll
      for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int j = 0; j < TJ; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[0][i], bf[0][j], acc[i][j], 0, 0, 0);
    }
  } else
  for (int t = 0; t < nk; ++t) {
    // tile t must have landed; tiles t+1..t+ahead (issued) may stay in flight
    const int ahead = min(nk - 1 - t, NS - 2);
    if constexpr (NS >= 5) {
      if (ahead >= 3) wait_vm<LPT * 3>();
      else if (ahead == 2) wait_vm<LPT * 2>();
      else if (ahead == 1) wait_vm<LPT>();
      else wait_vm<0>();
    } else if constexpr (NS == 4) {
      if (ahead >= 2) wait_vm<LPT * 2>();
      else if (ahead == 1) wait_vm<LPT>();
      else wait_vm<0>();
    } else if constexpr (NS == 3) {
      if (ahead >= 1) wait_vm<LPT>();
      else wait_vm<0>();
    } else {
      wait_vm<0>();
    }
    (void)ahead;
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    // Late DMA issue (interleaved split tiles): the upper half of the waves -- the second wave of each
    // SIMD -- issues its share of the next stage's DMA after the lo.hi term group of the step's first k chunk
    // instead of right after the barrier, so the two waves of a SIMD never both sit in the DMA issue
    // (≈ 60-185 cycles per instruction, MI355X_MICROARCH.md) while the matrix core idles. The stage is free
    // either way (every wave passed this barrier, so step t - 1's reads of it are done); same fragments and
    // MFMAs: same bits
    // (measured and dropped, DESIGN_HISTORY.md: the first half of the waves issuing after its first fragment
    // reads; the second half issuing after the first I1 rows of lo.hi, halfway through hi.lo, after hi.lo, or
    // its hi planes after lo.hi and lo planes after hi.lo; every wave issuing right after the barrier; MFMA
    // sections at wave priority 1; an early restage of the 2-stage rings; a start stagger between the
    // workgroups sharing a CU)
    const bool late = SP >= 2 && wave >= NW / 2;
    const bool nxt = DBG != 1 && t + NS - 1 < nk;
    if (nxt && !late) issue((t + NS - 1) % NS, t + NS - 1);
    auto issue_late = [&]() {
      __builtin_amdgcn_sched_barrier(0);
      issue((t + NS - 1) % NS, t + NS - 1);
      __builtin_amdgcn_sched_barrier(0);
    };
    const f16* sA = smem + ((DBG == 1 ? 0 : t) % NS) * STAGE;
    const f16* sB = sA + BM * LBK;
    if constexpr (MF == 32) {
#pragma unroll
      for (int s = 0; s < BK / 16; ++s) {
        const int kcs = 2 * s + lh;
        half8 af[TI], bf[TJ];
#pragma unroll
        for (int i = 0; i < TI; ++i) {
          const int r = wm * TM + i * 32 + lr;
          af[i] = *reinterpret_cast<const half8*>(sA + r * BK + sw<BK>(r, kcs) * 8);
        }
#pragma unroll
        for (int j = 0; j < TJ; ++j) {
          const int r = wn * TN + j * 32 + lr;
          bf[j] = *reinterpret_cast<const half8*>(sB + r * BK + sw<BK>(r, kcs) * 8);
        }
#pragma unroll
        for (int i = 0; i < TI; ++i)
#pragma unroll
          for (int j = 0; j < TJ; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[i], bf[j], acc[i][j], 0, 0, 0);
      }
    } else if constexpr (SP >= 2) {
      // interleaved split: per 32-deep k chunk the hi and lo fragments of A and B, then the three
      // terms term-major (each accumulator: lo.hi, hi.lo, hi.hi of the chunk, in that order).
      // The fragment reads go in two groups, each ahead of the terms that consume it: (B hi, A lo) for
      // lo.hi, then (B lo, A hi) once the first I1 rows of lo.hi have their operands, so that no more than
      // 15 LDS reads are ever outstanding. lgkmcnt is a 4-bit field: with all 2 (TI + TJ) reads issued at
      // once (24 on the 256 x 256 tile) the compiler drains every one before the first MFMA, and the waves,
      // in step after the barrier, leave the MFMAs idle while the LDS serves the whole stage. In groups,
      // the second lands under the first's MFMAs. Same MFMAs in the same order per accumulator: same bits.
      const int l16 = lane & 15, lq = lane >> 4;
      constexpr int KS = BK / 32;
      constexpr int GR = TI + TJ;  // reads per group
      constexpr int I1 = 2 * GR <= 15 ? 0 : (TI + GR - 15 > 1 ? TI + GR - 15 : 1);
      static_assert(GR <= 15 && I1 <= TI, "fragment read groups");
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        const int kcs = 4 * s + lq;
        half8 af[2][TI], bf[2][TJ];  // [plane: 0 hi, 1 lo]
        auto read_a = [&](int h) {
#pragma unroll
          for (int i = 0; i < TI; ++i) {
            const int r = wm * TM + i * 16 + l16;
            af[h][i] = frag(sA, h, r, kcs);
          }
        };
        auto read_b = [&](int h) {
#pragma unroll
          for (int j = 0; j < TJ; ++j) {
            const int r = wn * TN + j * 16 + l16;
            bf[h][j] = frag(sB, h, r, kcs);
          }
        };
        read_b(0);
        read_a(1);
        if constexpr (I1 == 0) {
          read_b(1);
          read_a(0);
        }
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (I1 > 0) {
#pragma unroll
          for (int i = 0; i < I1; ++i)
#pragma unroll
            for (int j = 0; j < TJ; ++j)
              acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[1][i], bf[0][j], acc[i][j], 0, 0, 0);
          __builtin_amdgcn_sched_barrier(0);
          read_b(1);
          read_a(0);
          __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int i = I1; i < TI; ++i)
#pragma unroll
          for (int j = 0; j < TJ; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[1][i], bf[0][j], acc[i][j], 0, 0, 0);
        if (late && s == 0 && nxt) issue_late();
#pragma unroll
        for (int i = 0; i < TI; ++i)
#pragma unroll
          for (int j = 0; j < TJ; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[0][i], bf[1][j], acc[i][j], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < TI; ++i)
#pragma unroll
          for (int j = 0; j < TJ; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[0][i], bf[0][j], acc[i][j], 0, 0, 0);
      }
    } else {
      // 16x16x32: lane l holds A[row l&15][k 8(l>>4)..+7] of each 32-deep k step. Both
      // k steps' fragments are requested up front, so the second step's LDS reads are in
      // flight under the first step's MFMAs (counted lgkmcnt instead of a drain per group).
      const int l16 = lane & 15, lq = lane >> 4;
      constexpr int KS = BK / 32;
      half8 af[KS][TI], bf[KS][TJ];
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        const int kcs = 4 * s + lq;
#pragma unroll
        for (int i = 0; i < TI; ++i) {
          const int r = wm * TM + i * 16 + l16;
          af[s][i] = *reinterpret_cast<const half8*>(sA + r * BK + sw<BK>(r, kcs) * 8);
        }
#pragma unroll
        for (int j = 0; j < TJ; ++j) {
          const int r = wn * TN + j * 16 + l16;
          bf[s][j] = *reinterpret_cast<const half8*>(sB + r * BK + sw<BK>(r, kcs) * 8);
        }
      }
      __builtin_amdgcn_sched_barrier(0);  // keep all fragment reads ahead of the MFMAs
#pragma unroll
      for (int s = 0; s < KS; ++s)
#pragma unroll
        for (int i = 0; i < TI; ++i)
#pragma unroll
          for (int j = 0; j < TJ; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[s][i], bf[s][j], acc[i][j], 0, 0, 0);
    }
  }
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");

  if constexpr (DBG == 2) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
      for (int j = 0; j < TJ; ++j)
#pragma unroll
        for (int e = 0; e < NACC; ++e) s += acc[i][j][e];
    if (s == 12345.678f) p.C32[0] = s;  // keeps the accumulators live
    return;
  }
  // DBG 3 (probe builds only): the whole epilogue but (almost) no stores, pricing the plane stores
  gemm_epilogue<BM, BN, WM, WN, MF, accv, TI, TJ, PRE, DBG == 3, ACT>(p, acc, smem, m0, n0, wm, wn, wave, lane, rpre,
                                                                      rpre32, rplo);
}



// Epilogue of the ping-pong tile. Its MFMAs compute out^T = W . X^T, so a lane holds 4
// consecutive output features of one token per 16x16 block (acc[ia][jb]: token block ia of the
// wave's BM/2 rows, feature block jb of its 64 columns): the LDS staging writes are whole 8-B
// (f16) / 16-B (f32) vectors instead of single floats, and every wave stages and stores its own
// region (no workgroup barrier). Same expressions and order as gemm_epilogue, so the same bits:
// ((acc + bias) + residual') -> act -> f16 / f32, residual' = R, or the deferred LayerNorm
// fma((R - mean) rstd, g, b), or +0.
//   * no residual, f16 out only (BERT FFN1, ResNet 1x1): bias, act and the f16 rounding happen
//     in registers; the wave's f16 region (BM/2 rows x 128 B, 16-B chunk x of row r at
//     x ^ ((r >> 1) & 7)) is then stored as whole 128-B row segments;
//   * otherwise (BERT FFN2): (acc + bias) in f32 slabs of 32 rows x 256 B per wave (chunk x of row
//     r at x ^ (r & 15)); each slab's residual loads are all issued before any is consumed.
//   * X3 (paired split operands, gemm_pp_kernel SP = 3): every output form of the split engine --
//     f32 residual (plain or deferred LayerNorm) -> f32 for BERT's O-projection and FFN2, paired or
//     planar hi / lo planes for FFN1 and K|V -- through the same 32-row f32 slabs, read back with
//     gemm_epilogue's lane map (8 lanes x 8 features per row, 8 rows per pass): 16-B residual loads
//     and stores, and a paired row's hi and lo stores of four adjacent lanes fill one 128-B line.
// NOSTORE (probe builds only): everything computed, (almost) nothing stored.
template <int BM, bool NOSTORE = false, int ACT = -1, bool X3 = false>
__device__ __forceinline__ void pp_epilogue(const GemmParams& p, floatx4 (&acc)[BM / 32][4], char* smem, int m0,
                                            int n0, int wm, int wn, int tid, int lane) {
  constexpr int HB = BM / 2;    // rows per wave
  constexpr int NIA = BM / 32;  // 16-row token blocks per wave
  const int M = p.M, N = p.N;
  const int l16 = lane & 15, q = lane >> 4;
  const int wave = tid >> 6;
  const int rw0 = m0 + wm * HB, cw0 = n0 + wn * 64;  // the wave's first row / column
  char* reg = smem + wave * (HB * 128 > 8192 ? HB * 128 : 8192);
  float4 bb[4];
#pragma unroll
  for (int jb = 0; jb < 4; ++jb)
    bb[jb] = p.bias ? *reinterpret_cast<const float4*>(p.bias + cw0 + jb * 16 + 4 * q)
                    : make_float4(0.f, 0.f, 0.f, 0.f);
  const int act = ACT >= 0 ? ACT : p.act;  // compile-time where the launch knows it
  auto act4 = [&](float (&v)[4]) {
    if (act == ACT_RELU) {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
    } else if (act == ACT_RELU6) {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = fminf(fmaxf(v[e], 0.f), 6.f);
    } else if (act == ACT_GELU) {
#pragma unroll
      for (int e = 0; e < 4; e += 2) {
        const f32x2 r = gelu_erf_x2(f32x2{v[e], v[e + 1]});
        v[e] = r.x;
        v[e + 1] = r.y;
      }
    } else if (act == ACT_GELU_EXACT) {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = (v[e] * 0.5f) * (1.0f + erff(v[e] * 0.70710678118654752f));
    } else if (act == ACT_GELU_F32) {
#pragma unroll
      for (int e = 0; e < 4; e += 2) {
        const f32x2 r = gelu_f32_x2(f32x2{v[e], v[e + 1]});
        v[e] = r.x;
        v[e + 1] = r.y;
      }
    }
  };
  const float os = p.oscale;  // 1 except on split operands: fma(acc, 1, b) == acc + b
  if constexpr (X3) {
    static_assert(BM == 256, "paired split operands: the 256-row tile only");
    // lane -> row (lane >> 3) of each 8-row pass, features 8 (lane & 7)..+7 = slab chunks 2 (lane & 7), + 1
    const int ech = lane & 7, erow = lane >> 3;
    const int col0 = cw0 + ech * 8;
    float lng[8], lnb[8];
    if (p.r_stats) {
#pragma unroll
      for (int e = 0; e < 8; ++e) { lng[e] = p.r_g[col0 + e]; lnb[e] = p.r_b[col0 + e]; }
    }
    bool x3bad = false;  // split output left the f16 range (raised once, after the slabs)
#pragma unroll
    for (int sl = 0; sl < HB / 32; ++sl) {
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int jb = 0; jb < 4; ++jb) {
          const int ia = sl * 2 + a;
          const float4 v = make_float4(__builtin_fmaf(acc[ia][jb][0], os, bb[jb].x),
                                       __builtin_fmaf(acc[ia][jb][1], os, bb[jb].y),
                                       __builtin_fmaf(acc[ia][jb][2], os, bb[jb].z),
                                       __builtin_fmaf(acc[ia][jb][3], os, bb[jb].w));
          const int r = a * 16 + l16, x = jb * 4 + q;
          *reinterpret_cast<float4*>(reg + r * 256 + ((x ^ (r & 15)) << 4)) = v;
        }
      float rv[4][8];  // every residual load of the slab is issued before any is consumed
#pragma unroll
      for (int ps = 0; ps < 4; ++ps) {
#pragma unroll
        for (int e = 0; e < 8; ++e) rv[ps][e] = 0.f;
        if (p.R) {
          const int rowc = min(rw0 + sl * 32 + ps * 8 + erow, M - 1);
          const size_t base = (size_t)rowc * N + col0;
          if (p.r_f32) {
            const float* R = reinterpret_cast<const float*>(p.R) + base;
            const float4 r0 = *reinterpret_cast<const float4*>(R);
            const float4 r1 = *reinterpret_cast<const float4*>(R + 4);
            rv[ps][0] = r0.x; rv[ps][1] = r0.y; rv[ps][2] = r0.z; rv[ps][3] = r0.w;
            rv[ps][4] = r1.x; rv[ps][5] = r1.y; rv[ps][6] = r1.z; rv[ps][7] = r1.w;
            if (p.r_stats) {
              const float2 st = p.r_stats[rowc];
#pragma unroll
              for (int e = 0; e < 8; ++e) rv[ps][e] = __builtin_fmaf((rv[ps][e] - st.x) * st.y, lng[e], lnb[e]);
            }
          } else {  // (launch_gemm: paired operands take no split residual)
            const half8 r8 = *reinterpret_cast<const half8*>(reinterpret_cast<const f16*>(p.R) + base);
#pragma unroll
            for (int e = 0; e < 8; ++e) rv[ps][e] = (float)r8[e];
          }
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
      for (int ps = 0; ps < 4; ++ps) {
        const int sr = ps * 8 + erow, row = rw0 + sl * 32 + sr;
        const float4 x0 = *reinterpret_cast<const float4*>(reg + sr * 256 + (((2 * ech) ^ (sr & 15)) << 4));
        const float4 x1 = *reinterpret_cast<const float4*>(reg + sr * 256 + (((2 * ech + 1) ^ (sr & 15)) << 4));
        float v[2][4] = {{x0.x + rv[ps][0], x0.y + rv[ps][1], x0.z + rv[ps][2], x0.w + rv[ps][3]},
                         {x1.x + rv[ps][4], x1.y + rv[ps][5], x1.z + rv[ps][6], x1.w + rv[ps][7]}};
        act4(v[0]);
        act4(v[1]);
        if (row < M && (!NOSTORE || v[0][0] == 1234.5f)) {
          const size_t base = (size_t)row * N + col0;
          if (p.C16 && (p.c_lo || p.c_pair)) {  // split output: planes of v * cscale, the lo plane carries the rest
            float u[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) u[e] = v[e >> 2][e & 3];
            if (p.cscale != 1.f) {  // (a uniform branch: most split outputs carry their scale in the bias)
#pragma unroll
              for (int e = 0; e < 8; ++e) u[e] *= p.cscale;
            }
            half8 h, l;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              h[e] = (f16)u[e];
              l[e] = (f16)(u[e] - (float)h[e]);
              x3bad |= x3_out_of_range(u[e]);
            }
            if (p.c_pair) {  // the lane's 8 columns sit in one 32-column chunk: hi at o, lo 32 halfs on
              f16* o = p.C16 + x3_pair_index(row, col0, N, 0);
              *reinterpret_cast<half8*>(o) = h;
              *reinterpret_cast<half8*>(o + 32) = l;
            } else {
              *reinterpret_cast<half8*>(p.C16 + base) = h;
              *reinterpret_cast<half8*>(p.C16 + p.c_lo + base) = l;
            }
          } else if (p.C16) {
            half8 h;
#pragma unroll
            for (int e = 0; e < 8; ++e) h[e] = (f16)v[e >> 2][e & 3];
            *reinterpret_cast<half8*>(p.C16 + base) = h;
          }
          if (p.C32) {
            *reinterpret_cast<float4*>(p.C32 + base) = make_float4(v[0][0], v[0][1], v[0][2], v[0][3]);
            *reinterpret_cast<float4*>(p.C32 + base + 4) = make_float4(v[1][0], v[1][1], v[1][2], v[1][3]);
          }
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
    if (p.c_lo || p.c_pair) x3_raise(p.ovf, x3bad);
    return;
  }
  if (!p.R && p.C16 && !p.C32 && !p.c_lo) {
#pragma unroll
    for (int ia = 0; ia < NIA; ++ia)
#pragma unroll
      for (int jb = 0; jb < 4; ++jb) {
        float v[4] = {__builtin_fmaf(acc[ia][jb][0], os, bb[jb].x), __builtin_fmaf(acc[ia][jb][1], os, bb[jb].y),
                      __builtin_fmaf(acc[ia][jb][2], os, bb[jb].z), __builtin_fmaf(acc[ia][jb][3], os, bb[jb].w)};
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] += 0.f;  // gemm_epilogue's "+ residual" with none: -0 -> +0
        act4(v);
        half4 h;
#pragma unroll
        for (int e = 0; e < 4; ++e) h[e] = (f16)v[e];
        const int r = ia * 16 + l16, x = jb * 2 + (q >> 1);
        *reinterpret_cast<half4*>(reg + r * 128 + ((x ^ ((r >> 1) & 7)) << 4) + (q & 1) * 8) = h;
      }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int it = 0; it < HB / 8; ++it) {
      const int r = it * 8 + (lane >> 3), x = lane & 7;
      const uint4 v = *reinterpret_cast<const uint4*>(reg + r * 128 + ((x ^ ((r >> 1) & 7)) << 4));
      if (rw0 + r < M && (!NOSTORE || v.x == 0x12345678u))
        *reinterpret_cast<uint4*>(p.C16 + (size_t)(rw0 + r) * N + cw0 + x * 8) = v;
    }
    return;
  }
  // f32 slabs: lane -> row (lane >> 4) of each 4-row group, 16-B chunk (lane & 15) = 4 features
  const int sc = lane & 15, col = cw0 + sc * 4;
  bool x3bad = false;  // split output left the f16 range (raised once, after the slabs)
  float4 g4 = make_float4(0.f, 0.f, 0.f, 0.f), b4 = g4;
  if (p.r_stats) {
    g4 = *reinterpret_cast<const float4*>(p.r_g + col);
    b4 = *reinterpret_cast<const float4*>(p.r_b + col);
  }
#pragma unroll
  for (int sl = 0; sl < HB / 32; ++sl) {
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int jb = 0; jb < 4; ++jb) {
        const int ia = sl * 2 + a;
        const float4 v = make_float4(__builtin_fmaf(acc[ia][jb][0], os, bb[jb].x),
                                     __builtin_fmaf(acc[ia][jb][1], os, bb[jb].y),
                                     __builtin_fmaf(acc[ia][jb][2], os, bb[jb].z),
                                     __builtin_fmaf(acc[ia][jb][3], os, bb[jb].w));
        const int r = a * 16 + l16, x = jb * 4 + q;
        *reinterpret_cast<float4*>(reg + r * 256 + ((x ^ (r & 15)) << 4)) = v;
      }
    float rv[8][4];
#pragma unroll
    for (int it = 0; it < 8; ++it) {
      const int rowc = min(rw0 + sl * 32 + it * 4 + (lane >> 4), M - 1);
      const size_t base = (size_t)rowc * N + col;
#pragma unroll
      for (int e = 0; e < 4; ++e) rv[it][e] = 0.f;
      if (p.R) {
        if (p.r_f32) {
          const float4 r4 = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(p.R) + base);
          rv[it][0] = r4.x; rv[it][1] = r4.y; rv[it][2] = r4.z; rv[it][3] = r4.w;
          if (p.r_stats) {
            const float2 st = p.r_stats[rowc];
            rv[it][0] = __builtin_fmaf((rv[it][0] - st.x) * st.y, g4.x, b4.x);
            rv[it][1] = __builtin_fmaf((rv[it][1] - st.x) * st.y, g4.y, b4.y);
            rv[it][2] = __builtin_fmaf((rv[it][2] - st.x) * st.y, g4.z, b4.z);
            rv[it][3] = __builtin_fmaf((rv[it][3] - st.x) * st.y, g4.w, b4.w);
          }
        } else {
          const f16* R16 = reinterpret_cast<const f16*>(p.R) + base;
          const half4 r4 = *reinterpret_cast<const half4*>(R16);
#pragma unroll
          for (int e = 0; e < 4; ++e) rv[it][e] = (float)r4[e];
          if (p.r_lo) {  // split residual: hi + lo (exact in f32)
            const half4 l4 = *reinterpret_cast<const half4*>(R16 + p.r_lo);
#pragma unroll
            for (int e = 0; e < 4; ++e) rv[it][e] += (float)l4[e];
          }
        }
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int it = 0; it < 8; ++it) {
      const int r = it * 4 + (lane >> 4), row = rw0 + sl * 32 + r;
      const float4 sv = *reinterpret_cast<const float4*>(reg + r * 256 + ((sc ^ (r & 15)) << 4));
      float v[4] = {sv.x + rv[it][0], sv.y + rv[it][1], sv.z + rv[it][2], sv.w + rv[it][3]};
      act4(v);
      if (row < M && (!NOSTORE || v[0] == 1234.5f)) {
        const size_t base = (size_t)row * N + col;
        if (p.C16 && p.c_lo) {  // split output: planes of v * cscale, the lo plane carries the rest
          float u[4] = {v[0], v[1], v[2], v[3]};
          if (p.cscale != 1.f) {  // (a uniform branch: most split outputs carry their scale in the bias)
#pragma unroll
            for (int e = 0; e < 4; ++e) u[e] *= p.cscale;
          }
          half4 h, l;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            h[e] = (f16)u[e];
            l[e] = (f16)(u[e] - (float)h[e]);
            x3bad |= x3_out_of_range(u[e]);
          }
          *reinterpret_cast<half4*>(p.C16 + base) = h;
          *reinterpret_cast<half4*>(p.C16 + p.c_lo + base) = l;
        } else if (p.C16) {
          half4 h;
#pragma unroll
          for (int e = 0; e < 4; ++e) h[e] = (f16)v[e];
          *reinterpret_cast<half4*>(p.C16 + base) = h;
        }
        if (p.C32) *reinterpret_cast<float4*>(p.C32 + base) = make_float4(v[0], v[1], v[2], v[3]);
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  }
  if (p.c_lo) x3_raise(p.ovf, x3bad);
}

// ---- 256x256x64 ping-pong GEMM (A_PLAIN), v_mfma_f32_16x16x32_f16, 8 waves (2 x 4).
// Each K tile lives in one of two LDS buffers as four 16-KB pieces: A0/A1 = the 64-row
// halves of both wave rows' 128-row strips, B0/B1 = the 32-column halves of the four wave
// columns. A K tile is consumed in four phases, one output quadrant each:
//   ph0 (A0,B0)  ph1 (A0,B1)  ph2 (A1,B1)  ph3 (A1,B0)
// so the pieces fall free in the order A0, B1, A1, B0 and each is restaged for tile t+2
// (same buffer) one phase after its last read: ph1 A0, ph2 B1, ph3 A1, next ph0 B0.
// Every phase: ds_read its fragments + issue one piece (2 glds per lane), retire the
// reads (lgkmcnt(0)) BEFORE the first barrier, then 16 MFMAs between two barriers. The
// second wave row runs one barrier behind the first, so on each SIMD one wave is in its
// MFMA section while its partner loads. ph3 waits vmcnt(6): everything but the three
// pieces issued for tile t+2 has landed, i.e. all of tile t+1, read one phase later.
// Same k order per output as every other tile, so results are bit-identical to them.
// SP = 1: pass-major split operands (three K passes over planar planes). SP = 3: paired split
// operands (GemmParams::a_pair / b_pair, [rows][2K]): a K tile is 32 of K, whose paired row -- the
// chunk's 32 hi halfs, then its 32 lo halfs -- is byte for byte the f16 tile's 128-B row, so pieces,
// swizzle, fragment reads and the barrier / vmcnt structure are the f16 loop's; af / bf index the
// plane instead of the k half, and a phase runs the quadrant's three terms (lo.hi, hi.lo, hi.hi per
// accumulator, gemm_glds_kernel SP = 3's order: same bits), 24 MFMAs between its barrier pair. How
// tile 70256 serves paired operands under gemm_x3_pp 1 (launch_x3i).
// DBG = 4 (probe build, tools/pp_trace.py): s_memtime at four points of every phase of the
// first 12 K tiles, per wave, kept in spare LDS and dumped by one block into C32. DBG = 5
// (probe): the epilogue computes everything but stores nothing.
template <int AM, int DBG = 0, int BM = 256, int ACT = -1, int SP = 0>
__global__ __launch_bounds__(512) void gemm_pp_kernel(const GemmParams p) {
  static_assert(AM == A_PLAIN, "ping-pong tile: plain A only");
  static_assert(BM == 256 || BM == 128, "BM");
  static_assert(SP == 0 || SP == 1 || (SP == 3 && BM == 256), "SP: pass-major, or paired on the 256-row tile");
  constexpr int BN = 256, BK = 64, WM = 2, WN = 4;
  constexpr int PA = BM / 2;            // rows per A piece (two wave rows x BM/4)
  constexpr int PB = 128;               // rows per B piece (four wave columns x 32)
  constexpr int GA = PA / 64, GB = 2;   // glds per lane per piece
  constexpr int QI = BM / 64;           // 16-row MFMA tiles per quadrant
  constexpr int OFF_A1 = PA * BK, OFF_B0 = 2 * PA * BK, OFF_B1 = OFF_B0 + PB * BK;
  constexpr int BUF = 2 * (PA + PB) * BK;  // halfs per buffer
  constexpr int VM = (2 * GA + GB) * 1;    // glds of the three pieces issued for tile t+2
  typedef float accv __attribute__((ext_vector_type(4)));
  __shared__ __attribute__((aligned(16))) f16 smem[2 * BUF];
  constexpr int TRN = DBG == 4 ? 12 * 4 * 4 : 1;  // DBG 4 (probe): s_memtime phase trace
  __shared__ unsigned long long trace[DBG == 4 ? 8 : 1][TRN];
  int trk = 0;
  auto tmark = [&]() {
    if constexpr (DBG == 4) {
      const unsigned long long t = __builtin_amdgcn_s_memtime();
      if ((threadIdx.x & 63) == 0 && trk < TRN) trace[threadIdx.x >> 6][trk] = t;
      ++trk;
    }
  };

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave - (wave / WN) * WN;
  const int M = p.M, N = p.N, K = p.K;
  const int LDK = SP == 3 ? 2 * K : K;  // halfs per operand row in memory
  const int nbn = N / BN;
  const int nbm = (M + BM - 1) / BM;
  const int nwg = nbm * nbn;
  int bid = blockIdx.x;
  {
    const int xcd = bid & 7, q = nwg >> 3, r = nwg & 7;
    bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
  }
  int bm, bn;
  tile_coords(bid, nbm, nbn, p.group_m, bm, bn);
  const int m0 = bm * BM, n0 = bn * BN;

  const int lrow = lane >> 3, pchunk = lane & 7;
  const f16* a_src[2][GA];
  const f16* b_src[2][GB];
  bool a_ok[2][GA];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
#pragma unroll
    for (int i = 0; i < GA; ++i) {
      const int pr = (wave * GA + i) * 8 + lrow;  // A-piece row
      const int m = m0 + (pr / (PA / 2)) * (BM / 2) + h * (BM / 4) + pr % (PA / 2);
      a_ok[h][i] = m < M;
      a_src[h][i] = reinterpret_cast<const f16*>(p.A) + (size_t)(a_ok[h][i] ? m : 0) * LDK + sw<64>(pr, pchunk) * 8;
    }
#pragma unroll
    for (int i = 0; i < GB; ++i) {
      const int pr = (wave * GB + i) * 8 + lrow;  // B-piece row
      const int n = n0 + (pr >> 5) * 64 + h * 32 + (pr & 31);
      b_src[h][i] = p.B + (size_t)n * LDK + sw<64>(pr, pchunk) * 8;
    }
  }
  const f16* zero = reinterpret_cast<const f16*>(g_zero_page);
  // K tiles per pass (SP = 1: three passes, as gemm_glds_kernel; SP = 3: a tile is 32 of K, 64 paired halfs)
  const int nk0 = SP == 3 ? K / 32 : K / BK;
  // piece: 0 = A0, 1 = A1, 2 = B0, 3 = B1
  auto issue = [&](const int piece, const int kt) {
    f16* base = smem + (kt & 1) * BUF;
    int kk = kt;
    long long aoff = 0, boff = 0;
    if constexpr (SP == 1) {
      const int pl = (kt >= nk0) + (kt >= 2 * nk0);
      kk = kt - pl * nk0;
      aoff = pl == 0 ? p.a_lo : 0;
      boff = pl == 1 ? p.b_lo : 0;
    }
    const int k0 = kk * BK;
    if (piece < 2) {
      f16* dst = base + piece * OFF_A1;
#pragma unroll
      for (int i = 0; i < GA; ++i) {
        const f16* src = a_ok[piece][i] ? a_src[piece][i] + aoff + k0 : zero;
        __builtin_amdgcn_global_load_lds((const void*)src, (lds_vptr)(dst + (wave * GA + i) * 8 * BK), 16, 0, 0);
      }
    } else {
      f16* dst = base + (piece == 2 ? OFF_B0 : OFF_B1);
#pragma unroll
      for (int i = 0; i < GB; ++i)
        __builtin_amdgcn_global_load_lds((const void*)(b_src[piece - 2][i] + boff + k0),
                                         (lds_vptr)(dst + (wave * GB + i) * 8 * BK), 16, 0, 0);
    }
  };

  accv acc[2 * QI][4];
#pragma unroll
  for (int i = 0; i < 2 * QI; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = accv{0.f, 0.f, 0.f, 0.f};

  const int l16 = lane & 15, lq = lane >> 4;
  half8 af[2][QI], bf[2][2];
  auto read_a = [&](const int buf, const int h) {
    const f16* s = smem + buf * BUF + h * OFF_A1;
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
      for (int i = 0; i < QI; ++i) {
        const int r = wm * (PA / 2) + i * 16 + l16;
        af[k][i] = *reinterpret_cast<const half8*>(s + r * BK + sw<64>(r, 4 * k + lq) * 8);
      }
  };
  auto read_b = [&](const int buf, const int h) {
    const f16* s = smem + buf * BUF + (h ? OFF_B1 : OFF_B0);
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int r = wn * 32 + j * 16 + l16;
        bf[k][j] = *reinterpret_cast<const half8*>(s + r * BK + sw<64>(r, 4 * k + lq) * 8);
      }
  };
  auto mma = [&](const int qa, const int qb) {
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    tmark();
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    tmark();
    __builtin_amdgcn_s_setprio(1);
    if constexpr (SP == 3) {  // the quadrant's three terms, term-major: each accumulator lo.hi, hi.lo, hi.hi
#pragma unroll
      for (int term = 0; term < 3; ++term)
#pragma unroll
        for (int i = 0; i < QI; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j)
            acc[qa * QI + i][qb * 2 + j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(
                bf[term == 1][j], af[term == 0][i], acc[qa * QI + i][qb * 2 + j], 0, 0, 0);
    } else {
#pragma unroll
      for (int k = 0; k < 2; ++k)
#pragma unroll
        for (int i = 0; i < QI; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j)
            acc[qa * QI + i][qb * 2 + j] =
                __builtin_amdgcn_mfma_f32_16x16x32_f16(bf[k][j], af[k][i], acc[qa * QI + i][qb * 2 + j], 0, 0, 0);
    }
    __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_sched_barrier(0);
    tmark();
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
  };

  const int nk = SP == 1 ? 3 * nk0 : nk0;
  issue(0, 0);
  issue(3, 0);
  issue(1, 0);
  issue(2, 0);
  if (nk > 1) {
    issue(0, 1);
    issue(3, 1);
    issue(1, 1);
    wait_vm<VM>();
  } else {
    wait_vm<0>();
  }
  __builtin_amdgcn_s_barrier();
  if (wm == 1) __builtin_amdgcn_s_barrier();  // stagger the second wave row by one barrier
  __builtin_amdgcn_sched_barrier(0);

  for (int t = 0; t < nk; ++t) {
    const int buf = t & 1;
    const bool n1 = t + 1 < nk, n2 = t + 2 < nk;
    // ph0 (A0, B0)
    tmark();
    read_a(buf, 0);
    read_b(buf, 0);
    if (n1) issue(2, t + 1);
    mma(0, 0);
    // ph1 (A0, B1)
    tmark();
    read_b(buf, 1);
    if (n2) issue(0, t + 2);
    mma(0, 1);
    // ph2 (A1, B1)
    tmark();
    read_a(buf, 1);
    if (n2) issue(3, t + 2);
    mma(1, 1);
    // ph3 (A1, B0)
    tmark();
    read_b(buf, 0);
    if (n2) {
      issue(1, t + 2);
      wait_vm<VM>();
    } else {
      wait_vm<0>();
    }
    mma(1, 0);
  }
  if (wm == 0) __builtin_amdgcn_s_barrier();  // re-align the two wave rows
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  if constexpr (DBG == 4) {  // probe build: block gridDim.x / 2 dumps its trace into C32
    __syncthreads();
    if (blockIdx.x == gridDim.x / 2)
      for (int i = tid; i < 8 * TRN; i += blockDim.x)
        reinterpret_cast<unsigned long long*>(p.C32)[i] = trace[i / TRN][i % TRN];
    return;
  }
  if constexpr (DBG == 2) {  // probe build: no epilogue
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 2 * QI; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) s += acc[i][j][0] + acc[i][j][1] + acc[i][j][2] + acc[i][j][3];
    if (s == 12345.678f) p.C32[0] = s;
    return;
  }
  pp_epilogue<BM, DBG == 5, ACT, SP == 3>(p, acc, reinterpret_cast<char*>(smem), m0, n0, wm, wn, tid, lane);
}

// BM=256 tiles: (BN, WM, WN, NS)

// K-interleaved split operands (16x16x32, 32-deep stages) in each A mode
template <int BM, int BN, int WM, int WN, int NS, int BK>
static int launch_x3i(const GemmParams& p, hipStream_t s, int nwg, dim3 blk) {
  const int pp = opt().gemm_x3_pp;
  if (BM == 256 && BN == 256 && NS == 2 && p.a_pair && (pp == 2 || (pp == 1 && p.act == ACT_NONE))) {
    // tile 70256 on paired planes: the ping-pong schedule (same grid, same tile walk -- p.group_m is
    // launch_cfg's gemm_glds_group_m --, same bits). gemm_x3_pp 1 gives it the launch classes whose median
    // it lowered at B = 256 (profiles/x3_pp_gemm.txt, two runs): BERT's FFN2 by 9.5 / 8.7 % (not `clear` by
    // the tool's rule: one slow ring round per run widens the ring arm's spread past the gain, though every
    // ping-pong round is below every ring round), O-projection 4.3 / 4.1 % (clear), last-layer K|V 1.1 /
    // 2.5 % (clear in one run). FFN1, the one class with an activation in its epilogue, was 2.3 / 1.3 %
    // slower and stays on the ring: the activation is the dispatch's stand-in for that launch class, so a new
    // paired launch class wants its own measurement. 2 runs every class on it (tests, A/B)
    if constexpr (BM == 256 && BN == 256 && NS == 2)
      hipLaunchKernelGGL((gemm_pp_kernel<A_PLAIN, 0, 256, -1, 3>), dim3(nwg), dim3(512), 0, s, p);
  } else if (p.a_pair) {  // paired planes (launch_gemm: plain A, both operands paired, no split residual)
    hipLaunchKernelGGL((gemm_glds_kernel<BM, BN, WM, WN, NS, A_PLAIN, 0, 16, BK, 0, -1, 3>), dim3(nwg), blk, 0, s, p);
  } else if (BM * BN <= 128 * 128 && opt().gemm_prefetch_r && p.amode == A_PLAIN && p.R && p.r_lo && p.K <= 512) {
    if constexpr (BM * BN <= 128 * 128)
      hipLaunchKernelGGL((gemm_glds_kernel<BM, BN, WM, WN, NS, A_PLAIN, 0, 16, BK, 3, -1, 2>), dim3(nwg), blk, 0, s, p);
  } else if (p.amode == A_PLAIN)
    hipLaunchKernelGGL((gemm_glds_kernel<BM, BN, WM, WN, NS, A_PLAIN, 0, 16, BK, 0, -1, 2>), dim3(nwg), blk, 0, s, p);
  else if (p.amode == A_CONV)
    hipLaunchKernelGGL((gemm_glds_kernel<BM, BN, WM, WN, NS, A_CONV, 0, 16, BK, 0, -1, 2>), dim3(nwg), blk, 0, s, p);
  else
    hipLaunchKernelGGL((gemm_glds_kernel<BM, BN, WM, WN, NS, A_DUAL, 0, 16, BK, 0, -1, 2>), dim3(nwg), blk, 0, s, p);
  MEC_LAUNCH_CHECK();
  return 0;
}

// f16 operands and pass-major split operands (the TILE_GLDS tiles) in each A mode
template <int BM, int BN, int WM, int WN, int NS, int MF, int BK, int ACT>
static int launch_cfg_act(const GemmParams& p, hipStream_t s, int nwg, dim3 blk) {
  if (p.split) {  // split-f16 operands (fp32x3 path): three K passes, runtime activation
    if (BM * BN <= 128 * 128 && opt().gemm_prefetch_r && p.amode == A_PLAIN && p.R && p.r_lo && p.K <= 512) {
      // split identity residual of ResNet's conv3 GEMMs, both planes prefetched (PRE = 3)
      if constexpr (BM * BN <= 128 * 128)
        hipLaunchKernelGGL((gemm_glds_kernel<BM, BN, WM, WN, NS, A_PLAIN, 0, MF, BK, 3, -1, 1>), dim3(nwg), blk, 0, s, p);
    } else if (p.amode == A_PLAIN)
      hipLaunchKernelGGL((gemm_glds_kernel<BM, BN, WM, WN, NS, A_PLAIN, 0, MF, BK, 0, -1, 1>), dim3(nwg), blk, 0, s, p);
    else if (p.amode == A_CONV)
      hipLaunchKernelGGL((gemm_glds_kernel<BM, BN, WM, WN, NS, A_CONV, 0, MF, BK, 0, -1, 1>), dim3(nwg), blk, 0, s, p);
    else
      hipLaunchKernelGGL((gemm_glds_kernel<BM, BN, WM, WN, NS, A_DUAL, 0, MF, BK, 0, -1, 1>), dim3(nwg), blk, 0, s, p);
  } else if (BM * BN <= 128 * 128 && opt().gemm_prefetch_r && p.amode == A_PLAIN && p.R && !p.r_f32 && p.K <= 512) {
    // f16 residual prefetch for ResNet's short-K conv3 GEMMs (small tiles only: no spills);
    // 225 -> 170 us on layer1's conv3. The f32 form (PRE = 2, BERT's O-projection, K = 768)
    // measured 10-15% slower than no prefetch, so it is not dispatched.
    if constexpr (BM * BN <= 128 * 128)
      hipLaunchKernelGGL((gemm_glds_kernel<BM, BN, WM, WN, NS, A_PLAIN, 0, MF, BK, 1, ACT>), dim3(nwg), blk, 0, s, p);
  } else if (p.amode == A_PLAIN)
    hipLaunchKernelGGL((gemm_glds_kernel<BM, BN, WM, WN, NS, A_PLAIN, 0, MF, BK, 0, ACT>), dim3(nwg), blk, 0, s, p);
  else if (p.amode == A_DUAL)
    hipLaunchKernelGGL((gemm_glds_kernel<BM, BN, WM, WN, NS, A_DUAL, 0, MF, BK, 0, ACT>), dim3(nwg), blk, 0, s, p);
  else
    hipLaunchKernelGGL((gemm_glds_kernel<BM, BN, WM, WN, NS, A_CONV, 0, MF, BK, 0, ACT>), dim3(nwg), blk, 0, s, p);
  MEC_LAUNCH_CHECK();
  return 0;
}

// One gemm_glds_kernel tile. KIND (the catalogue's, gemm_tiles.h) says which operands the tile serves, so
// only those kernels exist: a TILE_X3I tile has the K-interleaved split kernels and no others, a
// TILE_GLDS tile has none of them.
template <TileKind KIND, int BM, int BN, int WM, int WN, int NS, int MF, int BK>
static int launch_cfg(const GemmParams& p0, hipStream_t s) {
  static_assert(KIND != TILE_X3I || (MF == 16 && BK == 32 && 4 * (BM + BN) * BK * NS <= 160 * 1024),
                "interleaved split operands need a 16x16x32 tile with 32-deep stages that fit the LDS");
  static_assert(KIND == TILE_X3I || NS > 1, "the one-stage loader reads interleaved split operands only");
  if (KIND != TILE_X3I && p0.split == 2) {
    set_error("gemm_glds: interleaved split operands need a 16x16x32 tile with 32-deep stages (tiles 7xxxx)");
    return -1;
  }
  if (KIND == TILE_X3I && p0.split != 2) {
    set_error(NS == 1 ? "gemm_glds: the one-stage tile (72128) takes interleaved split operands only"
                      : "gemm_glds: tiles 7xxxx serve (only) interleaved split operands");
    return -1;
  }
  GemmParams p = p0;
  p.group_m = opt().gemm_glds_group_m;
  const int nwg = ((p.M + BM - 1) / BM) * (p.N / BN);
  const dim3 blk(64 * WM * WN);
#ifdef MEC_PROBES
  if constexpr (BM == 256 && BN == 256 && KIND == TILE_X3I) {  // the 256 x 256 tiles only
    // the K-interleaved split tile (the fp32x3 FFN1 roofline kernel) with no operand loads inside its K loop
    // (gemm_debug 1: MFMA + LDS fragment reads + epilogue only, so its time against the real kernel's prices
    // the loads) or with no epilogue (gemm_debug 2: prices the epilogue)
    // (gemm_debug 3: the epilogue without its stores; 6: with a plain (no GELU) epilogue -- prices the GELU)
    if ((opt().gemm_debug == 1 || opt().gemm_debug == 2 || opt().gemm_debug == 3 || opt().gemm_debug == 6) &&
        p.amode == A_PLAIN && !p.a_pair) {
      if (opt().gemm_debug == 1)
        hipLaunchKernelGGL((gemm_glds_kernel<BM, BN, WM, WN, NS, A_PLAIN, 1, MF, BK, 0, -1, 2>), dim3(nwg), blk, 0, s, p);
      else if (opt().gemm_debug == 2)
        hipLaunchKernelGGL((gemm_glds_kernel<BM, BN, WM, WN, NS, A_PLAIN, 2, MF, BK, 0, -1, 2>), dim3(nwg), blk, 0, s, p);
      else if (opt().gemm_debug == 3)
        hipLaunchKernelGGL((gemm_glds_kernel<BM, BN, WM, WN, NS, A_PLAIN, 3, MF, BK, 0, -1, 2>), dim3(nwg), blk, 0, s, p);
      else {
        GemmParams q = p;
        q.act = ACT_NONE;
        hipLaunchKernelGGL((gemm_glds_kernel<BM, BN, WM, WN, NS, A_PLAIN, 0, MF, BK, 0, -1, 2>), dim3(nwg), blk, 0, s, q);
      }
      MEC_LAUNCH_CHECK();
      return 0;
    }
  } else if constexpr (BM == 256 && BN == 256) {
    if (opt().gemm_debug && p.amode == A_PLAIN) {
      if (opt().gemm_debug == 1)
        hipLaunchKernelGGL((gemm_glds_kernel<BM, BN, WM, WN, NS, A_PLAIN, 1, MF, BK>), dim3(nwg), blk, 0, s, p);
      else
        hipLaunchKernelGGL((gemm_glds_kernel<BM, BN, WM, WN, NS, A_PLAIN, 2, MF, BK>), dim3(nwg), blk, 0, s, p);
      MEC_LAUNCH_CHECK();
      return 0;
    }
  }
#endif
  if constexpr (KIND == TILE_X3I) {
    return launch_x3i<BM, BN, WM, WN, NS, BK>(p, s, nwg, blk);
  } else {
    // the activation is a template argument for ReLU (ResNet) and none (BERT O-proj); others runtime
    if (p.split) return launch_cfg_act<BM, BN, WM, WN, NS, MF, BK, -1>(p, s, nwg, blk);
    if (p.act == ACT_RELU) return launch_cfg_act<BM, BN, WM, WN, NS, MF, BK, ACT_RELU>(p, s, nwg, blk);
    if (p.act == ACT_NONE) return launch_cfg_act<BM, BN, WM, WN, NS, MF, BK, ACT_NONE>(p, s, nwg, blk);
    return launch_cfg_act<BM, BN, WM, WN, NS, MF, BK, -1>(p, s, nwg, blk);
  }
}

// The ping-pong schedule (the TILE_PP tiles: BM x 256, plain A only).
template <int BM>
static int launch_pp(const GemmParams& p0, hipStream_t s) {
  if (p0.amode != A_PLAIN) { set_error("gemm_glds: ping-pong tiles take a plain A only"); return -1; }
  GemmParams p = p0;
  p.group_m = opt().gemm_group_m;
  const dim3 blk(512);
  const dim3 grd(((p.M + BM - 1) / BM) * (p.N / 256));
#ifdef MEC_PROBES
  const int dbg = opt().gemm_debug;
  if constexpr (BM == 256) {
    if (dbg == 4 || dbg == 5) {
      if (dbg == 4)
        hipLaunchKernelGGL((gemm_pp_kernel<A_PLAIN, 4, 256>), grd, blk, 0, s, p);
      else if (p.act == ACT_GELU)
        hipLaunchKernelGGL((gemm_pp_kernel<A_PLAIN, 5, 256, ACT_GELU>), grd, blk, 0, s, p);
      else
        hipLaunchKernelGGL((gemm_pp_kernel<A_PLAIN, 5, 256>), grd, blk, 0, s, p);
      MEC_LAUNCH_CHECK();
      return 0;
    }
  }
  if (dbg == 2) {
    hipLaunchKernelGGL((gemm_pp_kernel<A_PLAIN, 2, BM>), grd, blk, 0, s, p);
    MEC_LAUNCH_CHECK();
    return 0;
  }
#endif
  // the activation is a template argument for the common cases: one epilogue path per kernel
  if (p.split) {
    hipLaunchKernelGGL((gemm_pp_kernel<A_PLAIN, 0, BM, -1, 1>), grd, blk, 0, s, p);
  } else if (BM == 256 && p.act == ACT_GELU) {
    if constexpr (BM == 256) hipLaunchKernelGGL((gemm_pp_kernel<A_PLAIN, 0, 256, ACT_GELU>), grd, blk, 0, s, p);
  } else if (p.act == ACT_RELU) {
    hipLaunchKernelGGL((gemm_pp_kernel<A_PLAIN, 0, BM, ACT_RELU>), grd, blk, 0, s, p);
  } else if (p.act == ACT_NONE) {
    hipLaunchKernelGGL((gemm_pp_kernel<A_PLAIN, 0, BM, ACT_NONE>), grd, blk, 0, s, p);
  } else {
    hipLaunchKernelGGL((gemm_pp_kernel<A_PLAIN, 0, BM>), grd, blk, 0, s, p);
  }
  MEC_LAUNCH_CHECK();
  return 0;
}

// Tile-width choice. Every BN computes each output with the same k-ordered MFMA chain, so
// the choice changes speed only, never results. The first launch of each distinct shape
// times every legal width on the caller's stream (hipEvents; skipped while the stream is
// being captured into a graph) and caches the fastest; `gemm_bn` forces a width.
// Cache key: this engine's slot for the operands (TuneEngine) + the shape; the cache is the calling
// handle's (tune_cache(), mec_common.h).
static std::array<int, 11> gemm_key(const GemmParams& p) {
  const int engine = p.split == 2 ? (p.a_pair ? ENGINE_X3I_PAIRED : ENGINE_X3I) : p.split ? ENGINE_X3_PASS : ENGINE_F16;
  return {engine, p.amode, p.M, p.N, p.K, p.H, p.W, p.C, p.ks, p.stride, p.pad};
}

template <TileKind KIND, int BM, int BN, int WM, int WN, int NS, int MF, int BK>
static int launch_tile(const GemmParams& p, hipStream_t s) {
  if constexpr (KIND == TILE_PP) {
    static_assert(BN == 256 && WM == 2 && WN == 4 && NS == 2 && MF == 16 && BK == 64, "gemm_pp_kernel's fixed shape");
    return launch_pp<BM>(p, s);
  } else {
    return launch_cfg<KIND, BM, BN, WM, WN, NS, MF, BK>(p, s);
  }
}

// One case per catalogue line (gemm_tiles.h).
static int launch_bn(const GemmParams& p, hipStream_t s, int id) {
  switch (id) {
#define MEC_TILE_CASE(ID, BM, BN, WM, WN, NS, MF, BK, KIND, TUNED) \
  case ID: return launch_tile<KIND, BM, BN, WM, WN, NS, MF, BK>(p, s);
    MEC_GEMM_TILES(MEC_TILE_CASE)
#undef MEC_TILE_CASE
    default: set_error("gemm_glds: unsupported tile id"); return -1;
  }
}

// Untuned tile (gemm_autotune 0, or a first launch inside graph capture). K-interleaved split
// operands take only the 7xxxx tiles: every one of them sums in the same k order, so this choice,
// like the autotuner's, changes speed only.
static int heuristic_bn(const GemmParams& p) {
  const long nbm = (p.M + 255) / 256;
  if (p.split == 2) {
    if (p.N % 256 == 0 && nbm * (p.N / 256) >= 256) return 70256;
    if (p.N % 128 == 0) return 71128;
    return 71064;
  }
  if (p.N % 256 == 0 && nbm * (p.N / 256) >= 4 * 256 && p.K >= 768) return 256;
  if (p.N % 128 == 0 && p.K >= 1024) return 128;
  if (p.N % 128 == 0 && p.K <= 64) return 128;
  return 64;
}

int gemm_tuned_bn(int amode, int M, int N, int K) {  // this engine's f16 result, else the split-operand ones'
  for (int engine : {ENGINE_F16, ENGINE_X3_PASS, ENGINE_X3I, ENGINE_X3I_PAIRED})
    if (int t = tune_cache().find_shape(engine, amode, M, N, K)) return t;
  return 0;
}

int launch_gemm_glds(const GemmParams& p0, hipStream_t s, int force_bn) {
  GemmParams p = p0;
  if (p.split && opt().gemm_x3_order == 1) p.split = 2;  // K-interleaved split terms
  if (force_bn) {
    const GemmTile* t = gemm_tile(force_bn);
    if (!t) return launch_bn(p, s, force_bn);  // (its "unsupported tile id")
    MEC_REQUIRE(p.N % t->bn == 0, "gemm_glds: forced tile width does not divide N");
    MEC_REQUIRE((p.split == 2) == (t->kind == TILE_X3I), "gemm_glds: tiles 7xxxx serve (only) interleaved split operands");
    return launch_bn(p, s, force_bn);
  }
  const auto key = gemm_key(p);
  int bn = tune_cache().find(key);
  if (!bn) {
    // a launch inside graph capture cannot time tiles: it runs the heuristic tile. For K-interleaved
    // split operands it does not cache it, so the first launch outside capture still tunes the shape
    // (every 7xxxx tile sums in one k order: same bits either way); other operands cache it, since
    // their tiles differ in MFMA shape and k order, and a graph replay and an eager launch of one
    // shape must compute the same bits
    MEC_TRY(first_launch_tile(
        key, s, p.split != 2,
        [&](int* out) {  // the median of 5 launches of every candidate (gemm_tiles.h), in catalogue order
          return tune_tiles<5>(
              kGemmTiles, [&](const GemmTile& t) { return gemm_tile_candidate(t, p); },
              [&](int id) { return launch_bn(p, s, id); }, s, heuristic_bn(p), out);
        },
        [&] { return heuristic_bn(p); },
        [&](int id) {  // one line per distinct shape, at its first launch
          fprintf(stderr, "MEC_GEMM amode=%d M=%d N=%d K=%d H=%d C=%d ks=%d stride=%d act=%d R=%d r_f32=%d split=%d tile=%d\n",
                  p.amode, p.M, p.N, p.K, p.H, p.C, p.ks, p.stride, p.act, p.R != nullptr, p.r_f32, p.split, id);
        },
        &bn));
  }
  return launch_bn(p, s, bn);
}

// Seven kernels no tile launches, kept for the compiler's sake alone: each shares its inlined
// gemm_epilogue<..., PRE != 0> instantiation with one live residual-prefetch kernel (11128 / 11064 at BK 64
// with PRE 1, 70064 at SP 2 with PRE 3), and with that second user gone the optimiser schedules the live
// kernel's epilogue differently (same registers and occupancy, other instruction order). With them the
// device code of every launchable kernel is the same as before the catalogue, byte for byte
// (tools/asm_kernel_diff.py); drop them together with a measurement of those seven kernels.
template __global__ void gemm_glds_kernel<128, 128, 2, 2, 2, A_PLAIN, 0, 16, 32, 1, ACT_NONE, 0>(const GemmParams);
template __global__ void gemm_glds_kernel<128, 128, 2, 2, 2, A_PLAIN, 0, 16, 32, 1, ACT_RELU, 0>(const GemmParams);
template __global__ void gemm_glds_kernel<128, 128, 2, 2, 2, A_PLAIN, 0, 16, 32, 1, -1, 0>(const GemmParams);
template __global__ void gemm_glds_kernel<128, 64, 2, 2, 2, A_PLAIN, 0, 16, 32, 1, ACT_NONE, 0>(const GemmParams);
template __global__ void gemm_glds_kernel<128, 64, 2, 2, 2, A_PLAIN, 0, 16, 32, 1, ACT_RELU, 0>(const GemmParams);
template __global__ void gemm_glds_kernel<128, 64, 2, 2, 2, A_PLAIN, 0, 16, 32, 1, -1, 0>(const GemmParams);
template __global__ void gemm_glds_kernel<256, 64, 2, 2, 2, A_PLAIN, 0, 16, 32, 3, -1, 1>(const GemmParams);

}  // namespace mec
