// foldplan.h — how the ordered group fold (fold.hip, foldmulti.hip) is cut
// into workgroups: the members of a tile, the buckets of a window and the
// member contexts a tile preloads.  One (tile, window) pair is one workgroup,
// so this plan decides the fold's speed and nothing of its results.  Also the
// cut of every path's groups into tiles (cut_tiles) and the rule for the
// two-level combine.  Host code without a device header: the engine calls it
// for the single and the multi-aggregator fold alike, tests/test_fold_plan_
// cpu.py and tests/test_group_shapes_cpu.py compile it alone.
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

// series per cross-series chunk of the row path (k_group)
constexpr int64_t kChunk = 256;

// two-level ordered combine for groups of more than kCombineL1 chunks: the
// single-level k_combine is one dependent chain of max_chunks loads per
// (group, bucket) thread (C4: 1,953 chunks, 1.9 ms); first-level slices
// cut it to ~max_chunks / kCombineSlices
constexpr int64_t kCombineL1 = 128;
constexpr int64_t kCombineSlices = 64;

// whether n groups of up to max_chunks tiles combine in two levels (the
// first-level slices within the budget)
inline bool two_level_combine(int64_t max_chunks, int64_t n, int64_t NB) {
  return max_chunks > kCombineL1 &&
         (double)n * kCombineSlices * NB * 33.0 < 2.0e9;
}

// The cut of the groups into tiles, as the kernels read it (the engine's
// build_tiles copies it to the device): tile t holds members [tm0, tm1) of
// group tg and `single` says it is its group's only one; mg / mt0 / mt1 are
// the groups of several tiles (k_combine's work), ag / at0 / at1 every
// group's tile range (a group without members has none); lg_* the groups
// for the radix select and their k_xsel_scan chunks.
struct TileCut {
  std::vector<int64_t> tg, tm0, tm1, mg, mt0, mt1, ag, at0, at1;
  std::vector<int64_t> lgg, lgo, lgk, lgc{0};
  std::vector<uint8_t> single;
  int64_t max_chunks = 0;
};

// sel_all: every group (even one without local members) joins the radix
// select lists — the cross-rank selection protocol needs global segments
// whole_upto: groups of at most this many members are one tile (one
// sequential chain), larger ones are cut into chunks of `chunk`
// sel_k: groups of more members than the LDS sort holds (kernels.hip: SEL_K)
// go to the radix select, in chunks of sel_chunk keys (select.hip: SEL_CHUNK)
inline TileCut cut_tiles(const std::vector<int64_t>& goff, bool sel_all,
                         int64_t chunk, int64_t whole_upto, int64_t sel_k,
                         int64_t sel_chunk) {
  TileCut c;
  const int64_t G = (int64_t)goff.size() - 1;
  for (int64_t g = 0; g < G; ++g) {
    const int64_t a = goff[g], b = goff[g + 1];
    const int64_t t0 = (int64_t)c.tg.size();
    const int64_t ch = (b - a <= whole_upto) ? std::max<int64_t>(b - a, 1) : chunk;
    for (int64_t m = a; m < b; m += ch) {
      c.tg.push_back(g);
      c.tm0.push_back(m);
      c.tm1.push_back(std::min(b, m + ch));
    }
    const int64_t t1 = (int64_t)c.tg.size();
    for (int64_t t = t0; t < t1; ++t) c.single.push_back(t1 - t0 == 1);
    if (t1 - t0 > 1) {
      c.mg.push_back(g);
      c.mt0.push_back(t0);
      c.mt1.push_back(t1);
    }
    c.ag.push_back(g);
    c.at0.push_back(t0);
    c.at1.push_back(t1);
    if (b - a > sel_k || sel_all) {
      c.lgg.push_back(g);
      c.lgo.push_back(a);
      c.lgk.push_back(b - a);
      c.lgc.push_back(c.lgc.back() + (b - a + sel_chunk - 1) / sel_chunk);
    }
  }
  for (int64_t k = 0; k < G; ++k)
    c.max_chunks = std::max(c.max_chunks, c.at1[k] - c.at0[k]);
  return c;
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
