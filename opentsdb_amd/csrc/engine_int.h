// engine_int.h — what the engine's host units share (engine.hip,
// engine_rows.hip, engine_hist.hip): the context, the error text, the scopes
// of one call and the functions one unit calls in another.  Host only, never
// installed.  Every function declared here is defined once, in engine.hip,
// unless its comment names another unit.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "../../include/otsdb_agg.h"
#include "kernels.h"
#include "launch.h"

namespace otsdb {
struct SelState;  // select.hip
struct XSel;
namespace eng {
// sets the calling thread's otsdb_last_error() text; returns st
otsdb_status fail(otsdb_status st, const char* fmt, ...);
}  // namespace eng
}  // namespace otsdb

#define HIP_TRY(x)                                                        \
  do {                                                                    \
    hipError_t e_ = (x);                                                  \
    if (e_ != hipSuccess)                                                 \
      return fail(OTSDB_E_DEVICE, "%s: %s", #x, hipGetErrorString(e_));   \
  } while (0)

namespace otsdb {
namespace eng {

struct AggInfo {
  const char* key;   // Aggregators.get() name
  const char* name;  // toString()
  int interp;
};
extern const AggInfo kAggs[OTSDB_AGG_COUNT_IDS];

inline int64_t jmod(int64_t a, int64_t b) { return a % b; }
inline int64_t align_down(int64_t t, int64_t iv) { return t - jmod(t, iv); }

struct Carve {
  char* base;
  size_t off = 0;
  template <class T>
  T* take(size_t n) {
    off = (off + 255) & ~(size_t)255;
    T* p = reinterpret_cast<T*>(base + off);
    off += n * sizeof(T);
    return p;
  }
};

// device buffers of one query's pipeline, carved from the context workspace
struct Work {
  SeriesMeta SM;
  Rows R;
  Packed* partial;
  uint8_t* tile_emit;
  double* out_val;
  uint8_t* out_emit;
  int64_t* counts;
  uint64_t* keys = nullptr;
  uint64_t* key_mm = nullptr;  // per (bucket, 64-member tile) min / max key
  uint32_t* key_cnt = nullptr;  // per (bucket, tile) non-NaN keys (fill mode)
  uint32_t* lg_kept = nullptr;  // per large group: holds a kept series
  SelState* sel = nullptr;
  XSel* xsel = nullptr;        // cross-rank selection (mode 2)
  Packed* comb = nullptr;      // two-level combine: first-level slices
  uint8_t* comb_emit = nullptr;
  uint8_t* redo = nullptr;     // fused-rate series handed back (Params.redo)
  bool sel_fused = false;      // fill-mode selection: keys + counts by the transpose
};

// A device buffer the context keeps between calls.  ensure grows it to at
// least `need` bytes (1 MiB or more; the old block is freed first, its
// contents are not kept); the context's destruction frees it.
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() {
    if (p) hipFree(p);
  }
  otsdb_status ensure(size_t need);
};

}  // namespace eng
}  // namespace otsdb

struct otsdb_ctx {
  using DevBuf = otsdb::eng::DevBuf;
  int device = 0;
  hipStream_t stream = nullptr;
  DevBuf ws;
  DevBuf stage;
  int* d_err = nullptr;                 // device error word
  unsigned long long* d_mm = nullptr;   // k_bounds min/max
  int64_t* h_small = nullptr;           // pinned readback
  // {error word, total points} of the last compaction, written by the
  // kernel straight into host memory (coherent, mapped): no read-back copy
  int64_t* h_done = nullptr;
  int64_t* d_done = nullptr;            // its device address
  // tile plan cache (keyed by the group offsets)
  std::vector<int64_t> goff_cache;
  DevBuf d_tiles;
  int64_t n_tiles = 0, n_multi = 0, n_large = 0, n_large_chunks = 0;
  int64_t max_chunks = 0;  // most chunks in one group
  bool tiles_sel_all = false;
  int64_t tiles_chunk = 0;
  int64_t tiles_whole = 0;
  bool verbatim = false;  // run_raw_verbatim: the cells query's rows as stored
  // a rollup call (otsdb_agg_run_rollup*, RollupScope): the rollup state its
  // rows are built with and the points' value_count column (device)
  otsdb::RollupKind rollup = otsdb::ROLLUP_NONE;
  const int64_t* rollup_cnt = nullptr;
  // the cells fold's uniform kernel met a qualifier that is not its series'
  // (ERR_CELLS_NONUNI): this call's next attempt takes the general kernel
  bool cells_no_uni = false;
  // otsdb_ctx_counters: cells folds launched uniform / general, uniform
  // folds that missed (ERR_CELLS_NONUNI, re-run with the general kernel)
  int64_t n_cells_uniform = 0, n_cells_general = 0, n_cells_uni_miss = 0;
  bool spec_miss = false;  // ... and they cannot be: the caller compacts
  bool result_short = false;  // the last E_CAPACITY was the result's (finish)
  std::mutex mu;  // one query at a time per context
  // stage timing (otsdb_prof_*)
  bool prof = false;
  std::vector<hipEvent_t> ev_pool;
  std::vector<std::pair<int, std::pair<hipEvent_t, hipEvent_t>>> ev_pending;
  size_t ev_used = 0;
  double prof_ms[14] = {0};
  int64_t prof_n[14] = {0};
  DevBuf cells_ws;   // cells query: series row / point offsets
  DevBuf cells_col;  // cells query fallback: decoded columns
  DevBuf cal;        // calendar bucket edges of the current query
  DevBuf acal_fill;  // stage A' (calendar fill): compacted batch
  DevBuf acal;  // per-series calendar: chains, anchors, series' chain
                // positions and bucket-start timestamps
  DevBuf dec_ws;  // decode workspace
  int dec_generic = 0;  // the last decode count pass: bit 0 / 1, k_decode_generic counts / writes
  DevBuf ws2;  // raw group-by: candidates, sort, selection slab
  DevBuf rows_ws;  // storage-row compaction / span assembly: per-row and
                   // per-series plan arrays
  DevBuf rows_scr;  // GENERAL-row cell records + staging / replay arenas
  DevBuf rows_large;  // LARGE rows: ranked columns, keys, sort temp
  DevBuf raw_cells[2];  // raw-row query: compacted rows, then the assembled spans
  DevBuf raw_stage;  // otsdb_agg_run_raw: host rows staged in HBM
  // single-pass compaction (k_compact1): per-group look-back granules and
  // the call's epoch; {error word, total} read back in one copy
  DevBuf cmp_flags;
  uint32_t cmp_epoch = 0;
  // the device error word is known to be zero (the last call ended with the
  // one-pass compaction, which zeroes it): the next pipeline skips its
  // memset.  clean_entry: that mark as the current call found it (CtxLock)
  bool err_clean = false;
  bool clean_entry = false;
  bool small_ready = false;  // k_compact1 wrote {error word, total}
  // multi-aggregator calls (otsdb_agg_run_multi*): one device error word per
  // output, and per output the compaction's {error word, total, look-back
  // mark, -} in mapped host memory (the call synchronises once, at its end)
  int* d_merr = nullptr;
  int64_t* h_mdone = nullptr;
  int64_t* d_mdone = nullptr;
  int multi_failed = -1;  // the output whose status the last multi call returned
  int64_t multi_total[OTSDB_MULTI_MAX] = {0};  // points of each output
  // otsdb_ctx_counters [5..8], of the last multi call: downsample passes over
  // the point stream, group-stage passes over a row matrix, key transposes,
  // transform passes
  int64_t n_multi_ds = 0, n_multi_group = 0, n_multi_kt = 0, n_multi_tf = 0;
  // otsdb_ctx_counters [12], of the last multi call: k_fold_multi launches
  // (OTSDB_SPEC_MULTI_FOLD on an eligible request: 1, else 0)
  int64_t n_multi_fold = 0;
  // otsdb_ctx_counters [10..11], of the last panel call: passes over the
  // point stream, row matrices built
  int64_t n_panel_passes = 0, n_panel_mats = 0;
  // otsdb_ctx_counters [13..14], of the last otsdb_hist_* call: k_hist_fold
  // launches, percentile passes over the dense sums
  int64_t n_hist_fold = 0, n_hist_pct = 0;
  // otsdb_ctx_counters [15..17], of the last otsdb_hist_*rows* call: cells
  // decoded into points, cells skipped as undecodable, points dropped by a
  // same-key merge
  int64_t n_hr_decoded = 0, n_hr_skipped = 0, n_hr_dropped = 0;
  // otsdb_ctx_counters [18..20], of the last otsdb_topn_* call: runs of the
  // grid path, of the general path, grid promises missed (re-run general)
  int64_t n_topn_grid = 0, n_topn_general = 0, n_topn_miss = 0;
  // what a top-N call reports through: mapped host memory the last kernels
  // write {error word, total, n_picked, flags}, picked and key into
  int64_t* h_topn = nullptr;
  int64_t* d_topn = nullptr;
  size_t topn_host_cap = 0;
  // cross-rank selection session (otsdb_sel_*): lives in `ws` between calls
  struct {
    bool active = false;
    otsdb::Params P;
    otsdb_query_spec spec;
    otsdb::eng::Work W;
    int64_t G = 0, NB = 0, M = 0;
    int median = 0;
    int32_t next_pass = 0;   // the pass otsdb_sel_hist_device expects
    bool more = false;       // the last planned pass has work
    bool pool_built = false;  // pass 1 compacted the candidates
    bool need_pick = false;
    // diagnostics (otsdb_ctx_counters): passes over the local key matrix
    // and histogram passes of the last session
    int64_t key_reads = 0, passes = 0;
    int64_t sessions = 0;  // prepared since the context was created ([9])
    DevBuf pool;  // candidates: keys [pool_cap] | segments [pool_cap]
    int64_t pool_cap = 0;
    // per segment: pool bounds [GB+1] | region offsets [GB+1] | fill [GB] |
    // the offsets' scan storage
    DevBuf segmem;
    size_t scan_tmp = 0;
  } sel;
};

namespace otsdb {
namespace eng {

// One call at a time per context.  Also takes the "error word known zero"
// mark for this call (clean_entry) and clears it: only the one-pass
// compaction's read-back (finish) sets it again, after k_compact1 zeroed
// the word — any other call may leave bits in it.
// A cross-rank selection session lives in the workspace the other entries
// overwrite: every call ends it, except the session's own entries and the
// diagnostics (keep_session), so that a late otsdb_sel_* call reports
// E_ILLEGAL_STATE instead of reading another query's bytes.
struct CtxLock {
  std::lock_guard<std::mutex> lk;
  explicit CtxLock(otsdb_ctx* c, bool keep_session = false) : lk(c->mu) {
    c->clean_entry = c->err_clean;
    c->err_clean = false;
    if (!keep_session) c->sel.active = false;
  }
};

// Binds a caller's stream to the context for one call and restores the
// context's own stream on every exit path (early HIP_TRY returns included).
struct StreamBinding {
  otsdb_ctx* c;
  hipStream_t saved;
  StreamBinding(otsdb_ctx* c_, void* hip_stream) : c(c_), saved(c_->stream) {
    if (hip_stream) c->stream = (hipStream_t)hip_stream;
  }
  ~StreamBinding() { c->stream = saved; }
};

// the context's error word after everything queued on its stream
otsdb_status read_err(otsdb_ctx* c, int* e);
BatchDev batch_dev(const otsdb_batch* b);
otsdb_status check_spec(const otsdb_query_spec* s);
// Grid of buckets every series row is laid out on (with a context, a
// calendar grid's edge table is copied to the device).
otsdb_status make_params(const otsdb_query_spec* s, Params* P,
                         otsdb_ctx* c = nullptr);
// the group offsets of a batch (device: b holds device pointers), checked
otsdb_status read_goff(otsdb_ctx* c, const otsdb_batch* b, bool device,
                       std::vector<int64_t>& goff);
// a host entry's result too small: the offsets the whole result needs go
// back to the caller, then the status
otsdb_status copy_offsets_back(otsdb_ctx* c, otsdb_result* out,
                               const int64_t* d_offsets, int64_t G,
                               otsdb_status rc);
// one exclusive scan of n + 1 int64 (in[n] must be 0), on st, and the
// temporary storage it needs
otsdb_status scan_excl(void* tmp, size_t tmp_bytes, const int64_t* in,
                       int64_t* out, int64_t n, hipStream_t st);
size_t scan_tmp_bytes(int64_t n, hipStream_t st);
// the storage rows cannot be taken verbatim (run_raw_verbatim): flagged on
// the context, never returned through the C-ABI
otsdb_status spec_miss(otsdb_ctx* c);
// Non-template kernels of engine.hip that the other units launch too (a
// kernel is defined in one unit): k_scan over n counts, k_series_rows and
// k_series_offsets, each with the geometry of every other launch of it.
void launch_scan(int64_t n, const int64_t* counts, int64_t* offsets,
                 hipStream_t st);
void launch_series_rows(int64_t R, int64_t S, const int64_t* row_series,
                        int64_t* series_row, hipStream_t st);
void launch_series_offsets(int64_t R, int64_t S, const int64_t* row_series,
                           const int64_t* row_out, int64_t* offsets,
                           hipStream_t st);

inline bool anchored(const otsdb_query_spec* s) {
  return s->use_calendar && !s->run_all && s->n_cal_anchors > 0 &&
         s->ds_interval_ms > 0;
}

// Brackets a pipeline stage with HIP events when profiling is enabled.
struct StageTimer {
  otsdb_ctx* c;
  int stage;
  hipEvent_t a = nullptr, b = nullptr;
  hipEvent_t get() {
    if (c->ev_used == c->ev_pool.size()) {
      hipEvent_t e;
      hipEventCreate(&e);
      c->ev_pool.push_back(e);
    }
    return c->ev_pool[c->ev_used++];
  }
  StageTimer(otsdb_ctx* c_, int s_) : c(c_), stage(s_) {
    if (c->prof) {
      a = get();
      hipEventRecord(a, c->stream);
    }
  }
  ~StageTimer() {
    if (c->prof) {
      b = get();
      hipEventRecord(b, c->stream);
      c->ev_pending.push_back({stage, {a, b}});
    }
  }
};

inline unsigned blocks_for(int64_t n, int per) {
  return (unsigned)((n + per - 1) / per);
}

// A device entry's scope: the context locked, its device selected, the
// caller's stream bound and the group offsets read (from the caller's host
// copy where the batch has one), in that order.  rc: the first failure.
struct DeviceCall {
  CtxLock lk;
  otsdb_status rc;
  StreamBinding bind;
  std::vector<int64_t> goff;
  DeviceCall(otsdb_ctx* c, const otsdb_batch* b, void* hip_stream)
      : lk(c), rc(select_device(c)), bind(c, hip_stream) {
    if (!rc) rc = read_goff(c, b, true, goff);
  }
  static otsdb_status select_device(otsdb_ctx* c) {
    HIP_TRY(hipSetDevice(c->device));
    return OTSDB_OK;
  }
};

// a rollup call's table side (otsdb_agg_run_rollup*)
struct Rollup {
  int32_t agg;         // R, RollupQuery.getRollupAgg()
  const int64_t* cnt;  // every point's valueCount()
};

// the outputs of one multi-aggregator or panel request
struct Req {
  int32_t n;
  const int32_t* ds;  // null: every output downsamples with spec->ds_agg_id
  const int32_t* aggs;
  const int32_t* interps;  // null: every output its aggregator's own
  otsdb_result* outs;
  // the request's first error word / compaction slot (d_merr, h_mdone): the
  // functions of a panel call run as one request each over one set of slots
  int32_t e0 = 0;
};

// The query implementations that cross units (the context locked, the
// stream bound, device pointers throughout).
otsdb_status run_device_impl(otsdb_ctx* c, const otsdb_query_spec* spec,
                             const otsdb_batch* b, otsdb_result* out,
                             std::vector<int64_t>& goff);
otsdb_status check_rollup(const otsdb_query_spec* s, const Rollup& r,
                          RollupKind* kind);
otsdb_status run_rollup_impl(otsdb_ctx* c, const otsdb_query_spec* spec,
                             const otsdb_batch* b, const Rollup& r,
                             otsdb_result* out, std::vector<int64_t>& goff);
otsdb_status run_cells_impl(otsdb_ctx* c, const otsdb_query_spec* spec,
                            const otsdb_cells* cells, const otsdb_batch* b,
                            otsdb_result* out, std::vector<int64_t>& goff,
                            const Req* mq = nullptr);
// engine_rows.hip
otsdb_status run_raw_impl(otsdb_ctx* c, const otsdb_query_spec* spec,
                          const otsdb_raw_rows* raw, int fix,
                          const otsdb_batch* b, otsdb_result* out,
                          std::vector<int64_t>& goff);

}  // namespace eng
}  // namespace otsdb

