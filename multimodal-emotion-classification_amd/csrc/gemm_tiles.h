// The GEMM tile catalogues (host only): the one place a tile id is defined, for the f16 / split engine
// (gemm_glds.hip) and for the fp32 engine (gemm_f32.hip), plus the autotune loop and the first-launch
// flow both engines run. Everything that needs to know a tile -- the launch switches, the width and
// height lookups, what mec_set_option accepts, the autotuner's candidates -- is derived from these lists.
#pragma once
#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "mec_common.h"

namespace mec {

// Which kernels a tile of the f16 / split engine has:
//   TILE_GLDS  gemm_glds_kernel on f16 operands and on pass-major split operands (split == 1)
//   TILE_X3I   gemm_glds_kernel on K-interleaved split operands only (split == 2, gemm_x3_order 1)
//   TILE_PP    the ping-pong schedule (gemm_pp_kernel): f16 and pass-major split operands, plain A only
enum TileKind { TILE_GLDS, TILE_X3I, TILE_PP };

// f16 / split engine: X(id, BM, BN, WM, WN, NS, MF, BK, kind, tuned). `tuned` = the autotuner offers it;
// the autotuner times its candidates in this order.
// 256 / 128 / 64 = 256 x BN with 8 waves; 1128 / 1064 = 128 x BN with 4 waves (64 / 48 KB of LDS, so two
// blocks share a CU and one block's epilogue overlaps the other's MFMA loop).
// +10000: the same tile on v_mfma_f32_16x16x32_f16.
// +20000 / +30000: 16x16x32 MFMA with 32-deep K stages and a deeper ring (256 x 256: 4 / 5
// stages = 3 / 4 tiles in flight; 256 x 128: 6 stages), same K order, so same results.
// 40256 / 41256: the 256 x 256 / 128 x 256 ping-pong schedule (gemm_pp_kernel), plain A only.
// 50128 / 60128: 256 x 128 on 4 waves (wave tile 128 x 64), 32-deep K stages, 3 / 2 stages
// (74 / 49 KB LDS): two blocks per CU, so one block's epilogue runs under the other's MFMAs.
// 50256: the same for 128 x 256.
// 7xxxx: interleaved split operands only (id = 7 | shape | width): 32-deep K stages holding the hi and lo
// tiles of A and B (LDS: 256 x 256 2 x 64 KB; 256 x 128 3 x 48 KB; 128 x 128 2 x 32 KB, two blocks per
// CU; 128 x 64 2 x 24 KB; 256 x 64 on 4 waves 2 x 40 KB).
// 72128: 256 x 128 on 4 waves (wave tile 128 x 64) with ONE 48-KB stage (read whole into fragments): two
// workgroups per CU (BERT FFN2's pin outside the fused step, mec_common.h gemm_x3_tag; not an autotune
// candidate).
// (measured and dropped: 4-wave 128 x 256, 256 x 128 and 256 x 256 interleaved forms, one wave per SIMD
// with 64 x 128 / 128 x 64 / 128 x 128 wave tiles: 10-45 % slower on every BERT shape,
// profiles/r03_split_tiles_x3i.log)
#define MEC_GEMM_TILES(X)                          \
  X(64, 256, 64, 4, 2, 3, 32, 64, TILE_GLDS, 1)    \
  X(128, 256, 128, 4, 2, 3, 32, 64, TILE_GLDS, 1)  \
  X(256, 256, 256, 2, 4, 2, 32, 64, TILE_GLDS, 1)  \
  X(1128, 128, 128, 2, 2, 2, 32, 64, TILE_GLDS, 1) \
  X(1064, 128, 64, 2, 2, 2, 32, 64, TILE_GLDS, 1)  \
  X(10064, 256, 64, 4, 2, 3, 16, 64, TILE_GLDS, 1) \
  X(10128, 256, 128, 4, 2, 3, 16, 64, TILE_GLDS, 1) \
  X(10256, 256, 256, 2, 4, 2, 16, 64, TILE_GLDS, 1) \
  X(11128, 128, 128, 2, 2, 2, 16, 64, TILE_GLDS, 1) \
  X(11064, 128, 64, 2, 2, 2, 16, 64, TILE_GLDS, 1) \
  X(20256, 256, 256, 2, 4, 4, 16, 32, TILE_GLDS, 1) \
  X(30256, 256, 256, 2, 4, 5, 16, 32, TILE_GLDS, 1) \
  X(20128, 256, 128, 4, 2, 6, 16, 32, TILE_GLDS, 1) \
  X(40256, 256, 256, 2, 4, 2, 16, 64, TILE_PP, 1)  \
  X(41256, 128, 256, 2, 4, 2, 16, 64, TILE_PP, 1)  \
  X(50128, 256, 128, 2, 2, 3, 16, 32, TILE_GLDS, 1) \
  X(60128, 256, 128, 2, 2, 2, 16, 32, TILE_GLDS, 1) \
  X(50256, 128, 256, 2, 2, 3, 16, 32, TILE_GLDS, 1) \
  X(70256, 256, 256, 2, 4, 2, 16, 32, TILE_X3I, 1) \
  X(70128, 256, 128, 4, 2, 3, 16, 32, TILE_X3I, 1) \
  X(71128, 128, 128, 2, 2, 2, 16, 32, TILE_X3I, 1) \
  X(71064, 128, 64, 2, 2, 2, 16, 32, TILE_X3I, 1)  \
  X(70064, 256, 64, 2, 2, 2, 16, 32, TILE_X3I, 1)  \
  X(72128, 256, 128, 2, 2, 1, 16, 32, TILE_X3I, 0)

// fp32 engine: X(id, BM, BN, WM, WN, NS, MF). 1 = 256 x 128 on 8 waves (2 stages, 96 KB), 2 = 128 x 128
// on 4 waves (2 stages, 64 KB: two blocks per CU), 3 = 128 x 64 on 4 waves (3 stages), 4 = 256 x 256 on
// 8 waves (wave tile 128 x 64, 2 stages, 128 KB), all on the 32x32x2 MFMA; 5..8 = the same tiles on
// the 16x16x4 MFMA. Tiles of one MFMA shape (family MF) accumulate each output along the same k order
// (bit-identical); the two shapes sum in different orders (rounding-level difference).
#define MEC_GEMM_F32_TILES(X)  \
  X(1, 256, 128, 4, 2, 2, 32)  \
  X(2, 128, 128, 2, 2, 2, 32)  \
  X(3, 128, 64, 2, 2, 3, 32)   \
  X(4, 256, 256, 2, 4, 2, 32)  \
  X(5, 256, 128, 4, 2, 2, 16)  \
  X(6, 128, 128, 2, 2, 2, 16)  \
  X(7, 128, 64, 2, 2, 3, 16)   \
  X(8, 256, 256, 2, 4, 2, 16)

struct GemmTile {
  int id, bm, bn;
  TileKind kind;
  bool tuned;
};
struct GemmF32Tile {
  int id, bm, bn, mf;
};

#define MEC_TILE_ROW(ID, BM, BN, WM, WN, NS, MF, BK, KIND, TUNED) {ID, BM, BN, KIND, TUNED != 0},
constexpr GemmTile kGemmTiles[] = {MEC_GEMM_TILES(MEC_TILE_ROW)};
#undef MEC_TILE_ROW
#define MEC_TILE_ROW(ID, BM, BN, WM, WN, NS, MF) {ID, BM, BN, MF},
constexpr GemmF32Tile kGemmF32Tiles[] = {MEC_GEMM_F32_TILES(MEC_TILE_ROW)};
#undef MEC_TILE_ROW

// The catalogue entry of an id; null = not a tile (0, "autotune", included).
template <class T, size_t N>
inline const T* find_tile(const T (&tiles)[N], int id) {
  for (const T& t : tiles)
    if (t.id == id) return &t;
  return nullptr;
}
inline const GemmTile* gemm_tile(int id) { return find_tile(kGemmTiles, id); }
inline const GemmF32Tile* f32_tile(int id) { return find_tile(kGemmF32Tiles, id); }
inline bool gemm_tile_x3i(int id) { return gemm_tile(id) && gemm_tile(id)->kind == TILE_X3I; }

// Whether the autotuner may time tile t on this problem: t is offered, divides N, serves these operands
// (K-interleaved split operands <-> the TILE_X3I tiles) and, for the ping-pong schedule, A is plain.
inline bool gemm_tile_candidate(const GemmTile& t, const GemmParams& p) {
  return t.tuned && p.N % t.bn == 0 && (t.kind == TILE_X3I) == (p.split == 2) && (t.kind != TILE_PP || p.amode == A_PLAIN);
}

// The autotune loop of both engines: every tile of `tiles` that is `legal` gets one warm launch and REPS
// timed ones (hipEvents on the caller's stream); the tile with the smallest median wins, `fallback` if no
// tile is legal.
template <int REPS, class T, size_t N, class Legal, class Launch>
int tune_tiles(const T (&tiles)[N], Legal legal, Launch launch, hipStream_t s, int fallback, int* out) {
  hipEvent_t ev[REPS + 1];
  for (auto& e : ev) MEC_HIP(hipEventCreate(&e));
  float best = 1e30f;
  int best_id = fallback;
  for (const T& tile : tiles) {
    if (!legal(tile)) continue;
    MEC_TRY(launch(tile.id));  // warm
    MEC_HIP(hipEventRecord(ev[0], s));
    for (int r = 0; r < REPS; ++r) {
      MEC_TRY(launch(tile.id));
      MEC_HIP(hipEventRecord(ev[r + 1], s));
    }
    MEC_HIP(hipEventSynchronize(ev[REPS]));
    float t[REPS];
    for (int r = 0; r < REPS; ++r) MEC_HIP(hipEventElapsedTime(&t[r], ev[r], ev[r + 1]));
    std::sort(t, t + REPS);
    if (t[REPS / 2] < best) { best = t[REPS / 2]; best_id = tile.id; }  // median launch
  }
  for (auto& e : ev) (void)hipEventDestroy(e);
  *out = best_id;
  return 0;
}

// The first launch of a shape (a tune-cache miss): time the tiles (`tune(&id)`) where gemm_autotune is set
// and the stream is not being captured into a graph -- a capture cannot time -- else take `heuristic()`;
// cache the result, except inside a capture where the engine says not to (`cache_in_capture`, see its
// caller); then one MEC_GEMM_TRACE line per distinct shape (`trace(id)`).
template <class Tune, class Heuristic, class Trace>
int first_launch_tile(const std::array<int, 11>& key, hipStream_t s, bool cache_in_capture, Tune tune,
                      Heuristic heuristic, Trace trace, int* id) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  const bool capturing = !(hipStreamIsCapturing(s, &cs) == hipSuccess && cs == hipStreamCaptureStatusNone);
  if (opt().gemm_autotune && !capturing) {
    MEC_TRY(tune(id));
  } else {
    *id = heuristic();
  }
  if (!capturing || cache_in_capture) tune_cache().put(key, *id);
  if (getenv("MEC_GEMM_TRACE")) trace(*id);
  return 0;
}

}  // namespace mec
