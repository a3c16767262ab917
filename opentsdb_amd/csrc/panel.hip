// panel.hip — panel queries: several downsampling functions over one pass of
// the point stream (otsdb_agg_run_panel*).
//
// k_bucketize_panel is the production ring kernel (k_bucketize_k<M, 8, ...,
// DPP = 1, WIN = OTSDB_RING_WIN>) over one combined state, the envelope
// MEnv = {sum, count, min, max}: bucketize_series / reduce_step run unchanged
// — 8 points a lane through fold_fast / fold_lane, the carry between steps,
// the DPP segmented scan with its run-length skipping, one close per run —
// and the sink writes up to five rows from each closed state (sum, avg,
// count, min, max), each through its own per-wavefront LDS ring.  Every
// component of MEnv is MSum<0|1|3> / MMinMax<false|true> operation for
// operation, in the same order, so row i is bit for bit the row
// k_bucketize_k<M_i> writes.  The same from compacted cells, below:
// k_bucketize_panel_cells, k_bucketize_cells' walk over MEnv (DESIGN.md
// §4.2.1).  (Included by engine.hip after kernels.hip and decode.hip.)
#ifndef OTSDB_RING_WIN
#define OTSDB_RING_WIN 256
#endif
#ifndef OTSDB_RING_FL
#define OTSDB_RING_FL 64
#endif
#include "menv.h"  // the envelope state MEnv

namespace otsdb {

// the rows a panel pass can write; a request's set is a kernel-uniform mask
enum : uint32_t {
  PF_SUM = 1,  // sum / zimsum / pfsum
  PF_AVG = 2,
  PF_CNT = 4,
  PF_MIN = 8,  // min / mimmin
  PF_MAX = 16  // max / mimmax
};
constexpr int kPanelFns = 5;

// (the envelope state MEnv: menv.h)

// the row matrices of one panel pass ([S * nb] each; null where fn has no bit)
struct PanelRows {
  double *sum, *avg, *cnt, *min, *max;
  uint32_t fn;
};

// RowSink's ring form for up to five rows: one series row and one LDS ring
// per function of the mask (values only: sentinel rows, no state bytes)
struct PanelSink {
  double *row_sum, *row_avg, *row_cnt, *row_min, *row_max;
  double *rg_sum, *rg_avg, *rg_cnt, *rg_min, *rg_max;
  uint32_t fn;  // kernel-uniform
  int mask;     // WIN - 1
  int direct;   // wave-uniform: write straight to HBM this step
  DEV void put1(double* rowv, double* rv, int k, double v) const {
    v = is_nan(v) ? qnan() : v;  // never the absent pattern
    if (direct) rowv[k] = v;
    else rv[k & mask] = v;
  }
  DEV void close(int k, const MEnv& m, int& err) {
    if (fn & PF_SUM) put1(row_sum, rg_sum, k, m.sum());
    if (fn & PF_AVG) put1(row_avg, rg_avg, k, m.avg());
    if (fn & PF_CNT) put1(row_cnt, rg_cnt, k, m.count());
    if (fn & PF_MIN) put1(row_min, rg_min, k, m.min());
    if (fn & PF_MAX) put1(row_max, rg_max, k, m.max());
  }
  DEV static void drain1(double* rowv, double* rv, int64_t b, int i) {
    rowv[b] = rv[i];
    rv[i] = absent_value();
  }
  DEV void drain(int64_t b) {
    const int i = (int)(b & mask);
    if (fn & PF_SUM) drain1(row_sum, rg_sum, b, i);
    if (fn & PF_AVG) drain1(row_avg, rg_avg, b, i);
    if (fn & PF_CNT) drain1(row_cnt, rg_cnt, b, i);
    if (fn & PF_MIN) drain1(row_min, rg_min, b, i);
    if (fn & PF_MAX) drain1(row_max, rg_max, b, i);
  }
  DEV void absent(int64_t b) {
    if (fn & PF_SUM) row_sum[b] = absent_value();
    if (fn & PF_AVG) row_avg[b] = absent_value();
    if (fn & PF_CNT) row_cnt[b] = absent_value();
    if (fn & PF_MIN) row_min[b] = absent_value();
    if (fn & PF_MAX) row_max[b] = absent_value();
  }
  DEV void clear(int i) {
    if (fn & PF_SUM) rg_sum[i] = absent_value();
    if (fn & PF_AVG) rg_avg[i] = absent_value();
    if (fn & PF_CNT) rg_cnt[i] = absent_value();
    if (fn & PF_MIN) rg_min[i] = absent_value();
    if (fn & PF_MAX) rg_max[i] = absent_value();
  }
};

// One wavefront per series, four a workgroup.  Dynamic LDS: D rings of WIN
// doubles per wavefront, D the functions of the mask (panel_lds_bytes): 16 KB
// a workgroup for two functions, 24 KB for min / avg / max, 40 KB for all
// five — 10, 6 and 4 workgroups a CU by LDS (160 KB).
template <int WIN, int FL>
__global__ __launch_bounds__(256) void k_bucketize_panel(Params P, BatchDev B,
                                                         SeriesMeta SM,
                                                         PanelRows R) {
  extern __shared__ double panel_ring[];
  const int w = threadIdx.x >> 6;
  const int64_t s = (int64_t)blockIdx.x * 4 + w;
  if (s >= B.S) return;
  const int D = __popc(R.fn);
  double* ring = panel_ring + (size_t)w * D * WIN;
  const int64_t row = s * P.nb;
  PanelSink S;
  S.fn = R.fn;
  S.mask = WIN - 1;
  S.direct = 0;
  // ring r of this wavefront goes to the r-th function of the mask
  int r = 0;
  S.row_sum = R.sum + row;
  S.rg_sum = ring + r * WIN;
  r += (R.fn & PF_SUM) ? 1 : 0;
  S.row_avg = R.avg + row;
  S.rg_avg = ring + r * WIN;
  r += (R.fn & PF_AVG) ? 1 : 0;
  S.row_cnt = R.cnt + row;
  S.rg_cnt = ring + r * WIN;
  r += (R.fn & PF_CNT) ? 1 : 0;
  S.row_min = R.min + row;
  S.rg_min = ring + r * WIN;
  r += (R.fn & PF_MIN) ? 1 : 0;
  S.row_max = R.max + row;
  S.rg_max = ring + r * WIN;
  bucketize_series<MEnv, 8, 0, 0, 0, 1, WIN, FL, 0>(P, B, SM, S, s);
}

inline size_t panel_lds_bytes(uint32_t fn) {
  return (size_t)__builtin_popcount(fn) * 4 * OTSDB_RING_WIN * sizeof(double);
}

inline void launch_panel(hipStream_t st, const Params& P, const BatchDev& B,
                         const SeriesMeta& SM, const PanelRows& R) {
  if (B.S <= 0 || !R.fn) return;
  hipLaunchKernelGGL((k_bucketize_panel<OTSDB_RING_WIN, OTSDB_RING_FL>),
                     dim3((unsigned)((B.S + 3) / 4)), dim3(256),
                     (unsigned)panel_lds_bytes(R.fn), st, P, B, SM, R);
}

// ------------------------------------------------ the panel pass from cells
// k_bucketize_panel_cells is k_bucketize_cells (decode.hip: one wavefront per
// series, row metadata 64 rows at a time, the LDS-DMA double buffers, the
// uniform and mixed value-length decode, the seek / stop counting, the
// corrupt / generic flags) instantiated over MEnv and PanelCells: the
// compacted bytes are read and decoded once for every function of the mask.
// The cells row path writes rows directly, value plus state byte
// (Params.sentinel = 0), so the sink is a direct one; the decode and the
// lanes' summation tree are the single kernel's, so row i is bit for bit the
// row k_bucketize_cells<M_i> writes.  (engine.hip includes decode.hip first.)
#ifndef OTSDB_PANEL_CELLS_K    // points a lane per step (even; the static LDS
#define OTSDB_PANEL_CELLS_K 6  // scales with it): k_bucketize_cells' own
#endif

// the matrices of one panel pass from cells: value and state rows [S * nb]
// and the per-series value of the bucket past the window [S], per function
// (null where fn has no bit)
struct PanelCellsRows {
  double *sum, *avg, *cnt, *min, *max;
  uint8_t *st_sum, *st_avg, *st_cnt, *st_min, *st_max;
  double *of_sum, *of_avg, *of_cnt, *of_min, *of_max;
  uint32_t fn;
};

// RowSink's direct form with state bytes (states = 1) for up to five rows
struct PanelCellsSink {
  double *row_sum, *row_avg, *row_cnt, *row_min, *row_max;
  uint8_t *st_sum, *st_avg, *st_cnt, *st_min, *st_max;
  uint32_t fn;  // kernel-uniform
  DEV static void put1(double* rowv, uint8_t* rows, int k, double v) {
    rowv[k] = v;
    rows[k] = ST_REAL;
  }
  DEV void close(int k, const MEnv& m, int& err) {
    if (fn & PF_SUM) put1(row_sum, st_sum, k, m.sum());
    if (fn & PF_AVG) put1(row_avg, st_avg, k, m.avg());
    if (fn & PF_CNT) put1(row_cnt, st_cnt, k, m.count());
    if (fn & PF_MIN) put1(row_min, st_min, k, m.min());
    if (fn & PF_MAX) put1(row_max, st_max, k, m.max());
  }
};

// CellsOne's counterpart: the five-row sink, and the bucket past the window
// kept as its envelope and finished into every function's own of_val (what
// that function's rows interpolate toward); SeriesMeta's other arrays (keep,
// lo, hi, kf, kl, of_has, of_ts) do not depend on the function and are shared
struct PanelCells {
  using Rows = PanelCellsRows;
  using Sink = PanelCellsSink;
  using OfVal = MEnv;
  static constexpr bool kRate = false;  // (rate queries take no shared pass)
  DEV static PanelCellsSink sink(const Rows& R, int64_t s, int64_t nb) {
    const int64_t row = s * nb;
    return PanelCellsSink{R.sum + row,    R.avg + row,    R.cnt + row,
                          R.min + row,    R.max + row,    R.st_sum + row,
                          R.st_avg + row, R.st_cnt + row, R.st_min + row,
                          R.st_max + row, R.fn};
  }
  DEV static MEnv of_zero() { return MEnv::init(); }
  DEV static MEnv of_finish(const MEnv& st) { return st; }
  DEV static void of_store(const SeriesMeta&, const Rows& R, int64_t s,
                           const MEnv& m) {
    if (R.fn & PF_SUM) R.of_sum[s] = m.sum();
    if (R.fn & PF_AVG) R.of_avg[s] = m.avg();
    if (R.fn & PF_CNT) R.of_cnt[s] = m.count();
    if (R.fn & PF_MIN) R.of_min[s] = m.min();
    if (R.fn & PF_MAX) R.of_max[s] = m.max();
  }
};

// (Params, CellsDev, series_row, S, SeriesMeta, PanelCellsRows, err_word)
template <int K>
constexpr auto k_bucketize_panel_cells =
    &k_bucketize_cells<MEnv, K, 1, 0, PanelCells>;

inline void launch_panel_cells(hipStream_t st, const Params& P,
                               const CellsDev& C, const int64_t* series_row,
                               int64_t S, const SeriesMeta& SM,
                               const PanelCellsRows& R, int* err_word) {
  if (S <= 0 || !R.fn) return;
  hipLaunchKernelGGL(k_bucketize_panel_cells<OTSDB_PANEL_CELLS_K>,
                     dim3((unsigned)((S + 3) / 4)), dim3(256), 0, st, P, C,
                     series_row, S, SM, R, err_word);
}

}  // namespace otsdb
