// foldplan.h — how the ordered group fold (fold.hip, foldmulti.hip) is cut
// into workgroups: the members of a tile, the buckets of a window and the
// member contexts a tile preloads.  One (tile, window) pair is one workgroup,
// so this plan decides the fold's speed and nothing of its results.  Host
// code without a device header: the engine calls it for the single and the
// multi-aggregator fold alike, tests/test_fold_plan_cpu.py compiles it alone.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace otsdb {

// members per tile of the ordered fold: one tile is one workgroup that
// streams all its members' points, so big groups (C3's 7.8k-series
// datacenters per GPU) are cut finer than the row path's 256-series chunks —
// 256-member tiles of one day of points leave the last round of workgroups
// half empty (C3 fold: 256 -> 2.9 ms, 64 -> 2.57 ms, 32 -> 2.53 ms)
#ifndef OTSDB_FOLD_CHUNK  // tuning builds override
#define OTSDB_FOLD_CHUNK 32
#endif
constexpr int64_t kFoldChunk = OTSDB_FOLD_CHUNK;
// groups of more than kFoldChunk members (C3's 7.8k-series datacenters):
// tiles of kFoldChunkLarge, twice as many workgroups again for the grid's
// last round (C3 fold: 32 -> 2.59 ms, 16 -> 2.50, 8 -> 2.46); groups up to
// kFoldChunk members (C1 / C2 hosts) stay one tile
#ifndef OTSDB_FOLD_CHUNK_LARGE  // tuning builds override
#define OTSDB_FOLD_CHUNK_LARGE 8
#endif
constexpr int64_t kFoldChunkLarge = OTSDB_FOLD_CHUNK_LARGE;
#ifndef OTSDB_FOLD_CTX  // tuning builds: 0 = no preloaded member contexts
#define OTSDB_FOLD_CTX 1
#endif
// Order-sensitive aggregators whose merge of partial states is
// ill-conditioned (dev: Chan's merge of Welford runs over offset data lands
// ~1e-11 from the reference's one sequential pass, Aggregators.java:547-568)
// reduce a group's members in ONE sequential chain per (group, bucket) while
// the group fits: fold tiles of up to kOrderedFoldChunk members (the LDS
// progress marks of one workgroup); past that the engine's row path takes
// over (engine.hip: kOrderedChunk)
constexpr int64_t kOrderedFoldChunk = 256;
// below this many (tile, window) workgroups the fold narrows its windows,
// down to kFoldMinWindow buckets
#ifndef OTSDB_FOLD_MIN_BLOCKS  // tuning builds override
#define OTSDB_FOLD_MIN_BLOCKS 1024
#endif
#ifndef OTSDB_FOLD_MIN_WINDOW
#define OTSDB_FOLD_MIN_WINDOW 128
#endif
constexpr int64_t kFoldMinBlocks = OTSDB_FOLD_MIN_BLOCKS;
constexpr int64_t kFoldMinWindow = OTSDB_FOLD_MIN_WINDOW;

// The fold's tiles: groups of at most whole_upto members are one tile, larger
// ones are cut into tiles of `chunk` (the engine's build_tiles takes the
// pair).  An ordered fold keeps a group one chain while a workgroup's
// progress marks hold it.
struct FoldTiling {
  int64_t chunk, whole_upto;
};
inline FoldTiling fold_tiling(bool ordered) {
  return ordered ? FoldTiling{kFoldChunk, kOrderedFoldChunk}
                 : FoldTiling{kFoldChunkLarge, kFoldChunk};
}

struct FoldPlan {
  int64_t WB, NW;    // buckets per window, windows of the grid
  int32_t fold_wb;   // Params.fold_wb: WB when narrowed, else 0 (the cap)
  int32_t fold_ctx;  // Params.fold_ctx: member contexts preloaded, 0: none
};

// goff: the groups' member offsets; n_tiles: the tiles fold_tiling cut them
// into; NB: buckets of the grid; wb_cap: the most buckets of the fold's state
// one window holds in LDS (fold_wb<A>(), launch.h); may_narrow: windows after
// the first may start from prepared contexts (not the verbatim cells fold)
inline FoldPlan fold_plan(const std::vector<int64_t>& goff, int64_t n_tiles,
                          int64_t NB, int64_t wb_cap, bool ordered,
                          bool may_narrow) {
  FoldPlan p{wb_cap, (NB + wb_cap - 1) / wb_cap, 0, 0};
  if (OTSDB_FOLD_CTX) {
    // tiles of up to 64 members load every member context at workgroup
    // start (k_fold; ds_tu.hip drops it when the LDS would cost occupancy)
    // (non-ordered: the largest tile, a group kept whole or one chunk of a
    // larger one; ordered: bounded by its whole-group size)
    int64_t tile_max = 0;
    for (size_t g = 0; g + 1 < goff.size(); ++g) {
      const int64_t k = goff[g + 1] - goff[g];
      tile_max = std::max(
          tile_max, ordered ? std::min(k, kOrderedFoldChunk)
                            : (k <= kFoldChunk ? k : std::min(k, kFoldChunkLarge)));
    }
    if (tile_max > 0 && tile_max <= 64) p.fold_ctx = (int32_t)tile_max;
  }
  // few tiles (small queries, e.g. C1's 100 groups of 10 series): narrower
  // fold windows give the grid more workgroups — each window's workgroup
  // streams only that window's points (k_fold_prep hands it the context)
  if (may_narrow && n_tiles > 0 && NB > kFoldMinWindow &&
      n_tiles * p.NW < kFoldMinBlocks) {
    const int64_t want = (kFoldMinBlocks + n_tiles - 1) / n_tiles;  // windows
    int64_t wb = (NB + want - 1) / want;
    wb = (wb + 63) / 64 * 64;
    if (wb < kFoldMinWindow) wb = kFoldMinWindow;
    if (wb < p.WB) {
      p.WB = wb;
      p.NW = (NB + wb - 1) / wb;
      p.fold_wb = (int32_t)wb;
    }
  }
  return p;
}

}  // namespace otsdb
