// launch.h — the host-side record through which the engine launches the
// kernels templated on the DOWNSAMPLING monoid.  Those kernels (k_prep, the
// ring k_bucketize_k, the rate-fused one, k_bucketize_cells, k_fold_prep and
// the ordered group fold k_fold x every aggregator, k_fold_multi over the
// envelope state; from compacted columns the cells prep kernels and the four
// cells variants of either fold) are compiled in two translation units per
// downsampling monoid (ds_tu.hip), in parallel.  How a fold is cut into
// tiles and windows is foldplan.h's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dispatch.h"
#include "kernels.h"

namespace otsdb {

// compacted columns of a query (otsdb_cells, device pointers)
struct CellsDev {
  int64_t R;
  const int64_t* row_series;
  const int64_t* row_base_s;
  const int64_t* qual_off;
  const uint8_t* qual;
  const int64_t* val_off;
  const uint8_t* val;
};

// per (series, inner window boundary j = 1 .. NW-1) of the ordered fold,
// window start W = j*WB (fold.hip)
struct WinCtx {
  int64_t bnd;      // first point with ts >= bucket_ts(W)
  int64_t prev_ts;  // last real bucket before W: its timestamp (INT64_MIN:
  double prev_val;  //   none) and downsampled value
  int64_t next_ts;  // first real bucket at or after W (INT64_MIN: none)
  double next_val;
};

// A cells fold (k_cells_prep -> k_fold / k_fold_multi<..., CELLS>,
// cellfold.hip; CELLS = 2 / 4: the general member walker over 2- / 4-byte
// qualifiers, 10 / 12: the uniform one): the compacted columns and what the
// prep derives per series.  A series' points
// are numbered by qualifier: point p's qualifier sits at byte
// qual_off[first row] + qw * p (rows are contiguous in the pools).
struct CellsFold {
  CellsDev C;
  const int64_t* series_row;  // [S + 1] first row of each series
  int64_t* rlo;               // row holding point lo
  int64_t* vlo;               // byte offset in C.val of point lo's value
  uint8_t* qw;                // qualifier width of the series (2 / 4)
  uint8_t* vl0;               // value length of point lo (first guess)
  // grids of several fold windows: the stream's cursor at each inner window
  // boundary (per (series, boundary), k_cells_fold_prep)
  int64_t* wrlo;
  int64_t* wvlo;
  uint8_t* wvl0;
  int* wide;                  // k_cells_prep: bit 0 / 1 = some kept series
                              // has 4- / 2-byte qualifiers (one width: the
                              // fold with that width fixed runs); bit 2
                              // (k_cells_uniform): some kept series is not
                              // uniform
  // k_cells_uniform: the series' one flags nibble (value length and type)
  // when every row of it is uniform — one qualifier width, value bytes
  // adding up to points x length (+ the meta byte of a multi-point column)
  // — else 0xFF
  uint8_t* uf;
};

// buckets per fold window: the aggregator states of a window live in LDS
// (2,048 x 24-byte dev / diff states + ring + marks: 57 KB, within the
// 64 KB a workgroup may hold; the states are dynamic LDS sized for the
// grid, fold_lds_bytes)
#ifndef OTSDB_FOLD_WB_MAX  // tuning builds: a smaller window cap
#define OTSDB_FOLD_WB_MAX 2048
#endif
template <class A>
constexpr int fold_wb() {
  return sizeof(A) <= 24 ? OTSDB_FOLD_WB_MAX
                         : (OTSDB_FOLD_WB_MAX < 1024 ? OTSDB_FOLD_WB_MAX : 1024);
}

// the fold's window: P.fold_wb buckets when the engine narrowed it (more
// workgroups for queries with few tiles), else fold_wb<A>()
template <class A>
__host__ __device__ constexpr int64_t fold_window(const Params& P) {
  return P.fold_wb > 0 ? (int64_t)P.fold_wb : (int64_t)fold_wb<A>();
}
// dynamic LDS of k_fold: the states of min(window, nb) buckets, then as
// many emit flags (16-byte aligned pieces)
template <class A>
__host__ __device__ constexpr int64_t fold_cap(const Params& P) {
  return P.nb < fold_window<A>(P) ? P.nb : fold_window<A>(P);
}
template <class A>
__host__ __device__ constexpr size_t fold_lds_states(const Params& P) {
  return (((size_t)fold_cap<A>(P) * sizeof(A)) + 15) & ~(size_t)15;
}
template <class A>
constexpr size_t fold_lds_bytes(const Params& P) {
  return fold_lds_states<A>(P) + ((((size_t)fold_cap<A>(P)) + 15) & ~(size_t)15);
}

enum DsKernel {
  DS_PREP,       // k_prep: bounds, seek, point past the window
  DS_RING,       // k_bucketize_k, LDS ring sink -> sentinel series rows
  DS_RATE,       // k_bucketize_k with RateSpan fused into the ring flush
  DS_CELLS,      // k_bucketize_cells: decode fused into the downsample
  DS_FOLD_PREP,  // k_fold_prep: window boundaries of the ordered fold
  DS_FOLD,       // k_fold: downsample + contribution + ordered aggregator
  DS_CELLS_PREP, // k_cells_prep: bounds / cursors of a cells fold
  DS_CELLS_FOLD, // k_fold from compacted columns, the kernel of
                 // DsLaunch.cells_variant: the kept series' one qualifier
                 // width a compile-time constant (a batch that mixes widths
                 // is rewritten with one, k_requal), the general or the
                 // uniform member walker (fold_member_cells_u)
  DS_CELLS_FOLD_PREP, // k_cells_fold_prep: window boundaries of a cells fold
  DS_PREP_FOLD,   // k_prep_fold: k_prep + k_fold_prep in one launch
  DS_CELLS_UNIFORM, // k_cells_uniform: which kept series are uniform
  DS_FOLD_MULTI,    // k_fold_multi: the fold over the envelope state, one
                    // pass for every output of a multi-aggregator call
  DS_CELLS_MULTI    // k_fold_multi from compacted columns (launch_cells),
                    // the kernel of DsLaunch.cells_variant as DS_CELLS_FOLD
};

// What a multi-aggregator fold (k_fold_multi, foldmulti.hip) finishes from
// the envelope state: the kind of each output and where it goes.
enum : int32_t { FM_SUM = 0, FM_AVG = 1, FM_CNT = 2, FM_MIN = 3, FM_MAX = 4 };
struct FoldMultiOut {
  double* val;    // [G * nb]
  uint8_t* emit;  // [G * nb]
  int* err;       // this output's device error word
};
struct FoldMultiArgs {
  int32_t n_out;
  int32_t kind[OTSDB_MULTI_MAX];  // FM_* of output j
  FoldMultiOut out[OTSDB_MULTI_MAX];
  // tiles of a group of several: the partials k_combine<M> merges per output,
  // [n_tiles * nb] each, null when no output needs them — (s, n) for sum /
  // avg / count (MSum<*>::pack), mn for min, mx for max (MMinMax<*>::pack)
  Packed *part_sn, *part_mn, *part_mx;
};

struct DsLaunch {
  hipStream_t st;
  Params P;
  BatchDev B;
  SeriesMeta SM;
  Rows R;
  int* err;
  // DS_CELLS
  CellsDev cells;
  const int64_t* series_row;
  // the folds and their prep kernels (DS_*FOLD*, DS_*MULTI): windows, tiles
  WinCtx* wc;
  int64_t NW, WB;
  int64_t n_tiles;
  const int64_t *tg, *tm0, *tm1;
  const uint8_t* single;
  const int64_t* members;
  Packed* partial;
  uint8_t* tile_emit;
  double* out_val;
  uint8_t* out_emit;
  int always_partial;
  int agg_id;
  // launch_cells' kernels (DS_CELLS_PREP ... DS_CELLS_MULTI)
  CellsFold cf;
  // DS_CELLS_FOLD / DS_CELLS_MULTI: the kernel's CELLS template value — 2 / 4:
  // 2- / 4-byte qualifiers, the general member walker; 10 / 12: the uniform
  int cells_variant;
  // DS_FOLD_MULTI / DS_CELLS_MULTI (beside DS_FOLD's tiles, windows and
  // tile_emit)
  const FoldMultiArgs* fm;
};

// Debug builds (-DOTSDB_DEBUG_SYNC): every launch reports itself and waits
// for the device, so a kernel that does not finish names itself.
#ifdef OTSDB_DEBUG_SYNC
#include <cstdio>
#define OTSDB_DBG(st, what)                                              \
  do {                                                                   \
    fprintf(stderr, "[otsdb] %s ...\n", what);                          \
    fflush(stderr);                                                      \
    hipError_t e_ = hipStreamSynchronize(st);                            \
    fprintf(stderr, "[otsdb] %s done (%s)\n", what, hipGetErrorString(e_)); \
    fflush(stderr);                                                      \
  } while (0)
#else
#define OTSDB_DBG(st, what) \
  do {                      \
  } while (0)
#endif

// Defined (explicitly instantiated) in ds_tu.hip for every downsampling
// monoid; false when the kernel does not exist for (M, agg).
template <class M>
bool launch_ds(DsKernel k, const DsLaunch& a);
// the cells fold kernels (ds_tu.hip part 1, their own translation units)
template <class M>
bool launch_cells(DsKernel k, const DsLaunch& a);

// Rollup queries (rollup.hip): DS_PREP and DS_RING over a
// rollup downsampling state, the points' value_count column beside the batch
// (device pointer; read by ROLLUP_AVG only).  No other kernel exists for them.
enum RollupKind {
  ROLLUP_NONE = 0,  // the ordinary downsampling function
  ROLLUP_AVG,       // sum of sum cells / sum of count cells (MRollAvg)
  ROLLUP_COUNT      // sum of count cells (MRollCount)
};
bool launch_rollup(RollupKind kind, DsKernel k, const DsLaunch& a,
                   const int64_t* value_count);

}  // namespace otsdb
