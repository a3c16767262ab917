// engine.hip — host side of libotsdb_agg.so: the C-ABI of include/otsdb_agg.h.
//
// Plans one query (bucket grid, series chunks), carves a reusable HBM
// workspace, launches the kernel pipeline of kernels.hip on the context's
// stream and maps the device error word back onto the reference's
// exceptions.  No CPU fallback exists: every data point is produced on the
// GPU.
//
// The storage-row and histogram families live in units of their own
// (engine_rows.hip, engine_hist.hip); engine_int.h holds what the three
// share, and every shared function is defined here: the plumbing first, then
// this unit's own code, then the query implementations the others call, then
// the C-ABI.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cctype>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_segmented_radix_sort.hpp>
#include <rocprim/device/device_select.hpp>

#include "../../include/otsdb_agg.h"
#include "kernels.hip"
#include "compact.hip"
#include "select.hip"
#include "decode.hip"
#include "raw.hip"
#include "calendar.hip"
#include "multi.hip"
#include "panel.hip"
#include "topn.hip"
#include "launch.h"
#include "foldplan.h"
#include "engine_int.h"

using namespace otsdb;
using namespace otsdb::eng;

// ------------------------------------------- shared plumbing (engine_int.h)

namespace otsdb {
namespace eng {

static thread_local std::string g_last_error;  // otsdb_last_error()

otsdb_status fail(otsdb_status st, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_last_error = buf;
  return st;
}

const AggInfo kAggs[OTSDB_AGG_COUNT_IDS] = {
    {"sum", "sum", 0},          {"pfsum", "pfsum", 4},
    {"min", "min", 0},          {"max", "max", 0},
    {"avg", "avg", 0},          {"median", "median", 0},
    {"none", "raw", 1},         {"mult", "multiply", 0},
    {"dev", "dev", 0},          {"diff", "diff", 0},
    {"zimsum", "zimsum", 1},    {"mimmin", "mimmin", 2},
    {"mimmax", "mimmax", 3},    {"squareSum", "squareSum", 1},
    {"count", "count", 1},      {"first", "first", 1},
    {"last", "last", 1},        {"p999", "p999", 0},
    {"p99", "p99", 0},          {"p95", "p95", 0},
    {"p90", "p90", 0},          {"p75", "p75", 0},
    {"p50", "p50", 0},          {"ep999r3", "ep999r3", 0},
    {"ep99r3", "ep99r3", 0},    {"ep95r3", "ep95r3", 0},
    {"ep90r3", "ep90r3", 0},    {"ep75r3", "ep75r3", 0},
    {"ep50r3", "ep50r3", 0},    {"ep999r7", "ep999r7", 0},
    {"ep99r7", "ep99r7", 0},    {"ep95r7", "ep95r7", 0},
    {"ep90r7", "ep90r7", 0},    {"ep75r7", "ep75r7", 0},
    {"ep50r7", "ep50r7", 0},
};

otsdb_status DevBuf::ensure(size_t need) {
  if (need <= cap) return OTSDB_OK;
  if (p) hipFree(p);
  p = nullptr;
  cap = 0;
  size_t n = std::max(need, (size_t)1 << 20);
  hipError_t e = hipMalloc(&p, n);
  if (e != hipSuccess)
    return fail(OTSDB_E_DEVICE, "hipMalloc(%zu): %s", n, hipGetErrorString(e));
  cap = n;
  return OTSDB_OK;
}

// the context's error word after everything queued on its stream
otsdb_status read_err(otsdb_ctx* c, int* e) {
  HIP_TRY(hipMemcpyAsync(&c->h_small[0], c->d_err, sizeof(int),
                         hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  *e = (int)(c->h_small[0] & 0xFFFFFFFF);
  return OTSDB_OK;
}

BatchDev batch_dev(const otsdb_batch* b) {
  return BatchDev{b->n_series, b->offsets, b->ts_ms, b->val, b->is_float,
                  b->series_float};
}

otsdb_status check_spec(const otsdb_query_spec* s) {
  if (s->agg_id < 0 || s->agg_id >= OTSDB_AGG_COUNT_IDS)
    return fail(OTSDB_E_NO_SUCH_ELEMENT, "No such aggregator: %d", s->agg_id);
  if (s->interp < -1 || s->interp > OTSDB_INTERP_PREV)
    return fail(OTSDB_E_ILLEGAL_ARGUMENT, "bad interpolation %d", s->interp);
  const bool ds = s->ds_interval_ms > 0 || s->run_all;
  if (!ds) {  // raw group-by (raw.hip)
    if (s->start_ms < 0)
      return fail(OTSDB_E_ILLEGAL_ARGUMENT, "negative start");
    return OTSDB_OK;
  }
  if (s->ds_agg_id < 0 || s->ds_agg_id >= OTSDB_AGG_COUNT_IDS)
    return fail(OTSDB_E_ILLEGAL_ARGUMENT, "No such downsampling function");
  if (s->ds_agg_id == OTSDB_AGG_NONE)
    return fail(OTSDB_E_ILLEGAL_ARGUMENT,
                "cannot use the NONE aggregator for downsampling");
  if (s->use_calendar && !s->run_all && s->n_cal_anchors > 0) {
    // per-series anchors: chains ended by INT64_MAX, anchors ascending, each
    // naming its chain edge
    const int64_t n = s->n_cal_edges, na = s->n_cal_anchors;
    if (!s->cal_edges || n < 3 || !s->cal_anchors || !s->cal_anchor_edge)
      return fail(OTSDB_E_ILLEGAL_ARGUMENT, "anchored calendar without tables");
    if (s->cal_edges[n - 1] != INT64_MAX)
      return fail(OTSDB_E_ILLEGAL_ARGUMENT,
                  "anchored cal_edges must end with INT64_MAX");
    for (int64_t k = 1; k < n; ++k)
      if (s->cal_edges[k - 1] != INT64_MAX && s->cal_edges[k] != INT64_MAX &&
          s->cal_edges[k] <= s->cal_edges[k - 1])
        return fail(OTSDB_E_ILLEGAL_ARGUMENT,
                    "cal_edges chains must increase strictly (index %lld)",
                    (long long)k);
    for (int64_t j = 0; j < na; ++j) {
      const int64_t e = s->cal_anchor_edge[j];
      if ((j && s->cal_anchors[j] <= s->cal_anchors[j - 1]) || e < 0 ||
          e >= n || s->cal_edges[e] != s->cal_anchors[j])
        return fail(OTSDB_E_ILLEGAL_ARGUMENT, "bad calendar anchor %lld",
                    (long long)j);
    }
    if (s->cal_anchors[0] > s->start_ms)
      return fail(OTSDB_E_ILLEGAL_ARGUMENT,
                  "no calendar anchor at or before start_ms");
  } else if (s->use_calendar && !s->run_all) {
    if (!s->cal_edges || s->n_cal_edges < 2)
      return fail(OTSDB_E_UNSUPPORTED,
                  "calendar downsampling without a bucket-edge table");
    for (int64_t k = 1; k < s->n_cal_edges; ++k)
      if (s->cal_edges[k] <= s->cal_edges[k - 1])
        return fail(OTSDB_E_ILLEGAL_ARGUMENT,
                    "cal_edges must increase strictly (index %lld)",
                    (long long)k);
    if (s->cal_edges[0] > s->start_ms)
      return fail(OTSDB_E_ILLEGAL_ARGUMENT,
                  "cal_edges[0] must be previousInterval(start_ms)");
  }
  if (s->fill == OTSDB_FILL_SCALAR)
    return fail(OTSDB_E_UNSUPPORTED, "unhandled fill policy");
  if (s->fill < 0 || s->fill > OTSDB_FILL_SCALAR)
    return fail(OTSDB_E_ILLEGAL_ARGUMENT, "bad fill policy %d", s->fill);
  if (s->interp < -1 || s->interp > OTSDB_INTERP_PREV)
    return fail(OTSDB_E_ILLEGAL_ARGUMENT, "bad interpolation %d", s->interp);
  if (!s->run_all && s->start_ms < 0)
    return fail(OTSDB_E_ILLEGAL_ARGUMENT, "negative start");
  return OTSDB_OK;
}

// a host entry's result too small: the caller still gets the offsets the
// whole result needs (offsets[G] = its point count), then the status
otsdb_status copy_offsets_back(otsdb_ctx* c, otsdb_result* out,
                               const int64_t* d_offsets, int64_t G,
                               otsdb_status rc) {
  HIP_TRY(hipMemcpyAsync(out->offsets, d_offsets, 8 * (G + 1),
                         hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return rc;
}

otsdb_status read_goff(otsdb_ctx* c, const otsdb_batch* b, bool device,
                       std::vector<int64_t>& goff) {
  goff.resize(b->n_groups + 1);
  if (b->n_groups < 0) return fail(OTSDB_E_ILLEGAL_ARGUMENT, "n_groups < 0");
  if (!b->group_offsets) return fail(OTSDB_E_ILLEGAL_ARGUMENT, "no groups");
  if (device && b->group_offsets_host) {
    // the caller's host copy of the same offsets: no read-back, no sync
    // (the caller keeps it equal to the device array: include/otsdb_agg.h)
    memcpy(goff.data(), b->group_offsets_host, sizeof(int64_t) * goff.size());
#ifdef OTSDB_DEBUG_SYNC
    {  // debug builds: the host copy's total against the device's
      int64_t last = 0;
      HIP_TRY(hipMemcpyAsync(&last, b->group_offsets + b->n_groups,
                             sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(hipStreamSynchronize(c->stream));
      if (last != goff.back())
        return fail(OTSDB_E_ILLEGAL_ARGUMENT,
                    "group_offsets_host[G] %lld != device %lld",
                    (long long)goff.back(), (long long)last);
    }
#endif
  } else if (device) {
    HIP_TRY(hipMemcpyAsync(goff.data(), b->group_offsets,
                           sizeof(int64_t) * goff.size(),
                           hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
  } else {
    memcpy(goff.data(), b->group_offsets, sizeof(int64_t) * goff.size());
  }
  for (size_t i = 1; i < goff.size(); ++i)
    if (goff[i] < goff[i - 1])
      return fail(OTSDB_E_ILLEGAL_ARGUMENT, "group_offsets not monotonic");
  return OTSDB_OK;
}

// one exclusive scan of n + 1 int64 (in[n] must be 0), on st
otsdb_status scan_excl(void* tmp, size_t tmp_bytes, const int64_t* in,
                       int64_t* out, int64_t n, hipStream_t st) {
  size_t t = tmp_bytes;
  HIP_TRY(rocprim::exclusive_scan(tmp, t, in, out, (int64_t)0, (size_t)(n + 1),
                                  rocprim::plus<int64_t>(), st));
  return OTSDB_OK;
}

size_t scan_tmp_bytes(int64_t n, hipStream_t st) {
  size_t b = 0;
  rocprim::exclusive_scan(nullptr, b, (const int64_t*)nullptr, (int64_t*)nullptr,
                          (int64_t)0, (size_t)(n + 1), rocprim::plus<int64_t>(),
                          st);
  return (b + 255) & ~(size_t)255;
}

// the storage rows cannot be taken verbatim (run_raw_verbatim): flagged on
// the context, never returned through the C-ABI
otsdb_status spec_miss(otsdb_ctx* c) {
  c->spec_miss = true;
  return OTSDB_E_UNSUPPORTED;
}

// (kernels of this unit for the other units: engine_int.h)
void launch_scan(int64_t n, const int64_t* counts, int64_t* offsets,
                 hipStream_t st) {
  hipLaunchKernelGGL(k_scan, dim3(1), dim3(1024), 0, st, n, counts, offsets);
}

void launch_series_rows(int64_t R, int64_t S, const int64_t* row_series,
                        int64_t* series_row, hipStream_t st) {
  hipLaunchKernelGGL(k_series_rows, dim3(blocks_for(R + 1, 256)), dim3(256), 0,
                     st, R, S, row_series, series_row);
}

void launch_series_offsets(int64_t R, int64_t S, const int64_t* row_series,
                           const int64_t* row_out, int64_t* offsets,
                           hipStream_t st) {
  hipLaunchKernelGGL(k_series_offsets, dim3(blocks_for(R + 1, 256)), dim3(256),
                     0, st, R, S, row_series, row_out, offsets);
}

}  // namespace eng
}  // namespace otsdb

namespace {

bool is_selection(int agg) {
  return agg == OTSDB_AGG_MEDIAN || agg >= OTSDB_AGG_P999;
}

double pct_of(int agg) {  // PercentileAgg(percentile).evaluate(): p / 100d
  static const double P[6] = {99.9, 99.0, 95.0, 90.0, 75.0, 50.0};
  return P[(agg - OTSDB_AGG_P999) % 6] / 100.0;
}

// k_keys_transpose's grid: KT_M members x OTSDB_KT_SLICES bucket slices
dim3 kt_grid(int64_t M, int64_t NB) {
  const int64_t ntb = (NB + 63) / 64;
  const int64_t sl = ntb < OTSDB_KT_SLICES ? (ntb > 0 ? ntb : 1) : OTSDB_KT_SLICES;
  return dim3((unsigned)((M + KT_M - 1) / KT_M), (unsigned)sl);
}

// (the ordered fold's tile sizes and window rule: foldplan.h)
// An ordered (dev) group past one fold tile (kOrderedFoldChunk) takes the row
// path's k_group with one chain of up to kOrderedChunk members (one thread
// walks them in SpanCmp order; ~100 ns a member: tools/chain_probe.hip, 69 ns
// with no memory at all, so a 500k-member chain — C4 — would cost ~50 ms).
// Larger groups merge 256-member chunk partials in order (Chan); across ranks
// the chain is handed on (otsdb_agg_partials_chained_device).
constexpr int64_t kOrderedChunk = 65536;
constexpr int64_t kOrderedChunkMerged = 16384;
// the row path's bucket rows an ordered (dev) query may take for groups past
// one fold tile: fixed, so the path (and the reduction order) never depends
// on the device's free memory at call time
constexpr double kOrderedRowBudget = 48.0e9;
// up to this many (series, window boundary) pairs k_prep and k_fold_prep run
// as one launch (each pair's thread finds its series' bounds again: cheap
// next to a launch on small queries, not on the named query's 400,000)
#ifndef OTSDB_PREP_FOLD_MAX
#define OTSDB_PREP_FOLD_MAX 65536
#endif
// (the environment's OTSDB_PREP_FOLD_MAX overrides it: the tests run both
// forms on one process)
int64_t prep_fold_max() {
  const char* e = getenv("OTSDB_PREP_FOLD_MAX");
  return e ? atoll(e) : (int64_t)OTSDB_PREP_FOLD_MAX;
}

// The blocks run_pipeline's and multi_build's carves have in common, each in
// the one order of takes both rely on.
void carve_series(Carve& cv, Work& W, int64_t S) {
  W.SM.lo = cv.take<int64_t>(S);
  W.SM.hi = cv.take<int64_t>(S);
  W.SM.of_ts = cv.take<int64_t>(S);
  W.SM.of_val = cv.take<double>(S);
  W.SM.of_rate = cv.take<double>(S);
  W.SM.kf = cv.take<int32_t>(S);
  W.SM.kl = cv.take<int32_t>(S);
  W.SM.keep = cv.take<uint8_t>(S);
  W.SM.of_has = cv.take<uint8_t>(S);
  W.redo = cv.take<uint8_t>(S);
}

// members: all groups' (goff.back()); LG: the large groups; xsel: mode 2
void carve_selection(Carve& cv, Work& W, int64_t members, int64_t LG,
                     int64_t NB, bool xsel) {
  const size_t kt = (size_t)((members + KT_M - 1) / KT_M) * NB;
  W.keys = cv.take<uint64_t>((size_t)members * NB);
  W.key_mm = cv.take<uint64_t>(kt * 2);
  W.key_cnt = cv.take<uint32_t>(kt);
  W.lg_kept = cv.take<uint32_t>((size_t)LG + 1);
  W.sel = cv.take<SelState>((size_t)LG * NB);
  if (xsel) W.xsel = cv.take<XSel>((size_t)LG * NB);
}

// ERR_RATE_TS as the entries that leave partials report it
otsdb_status rate_ts_error() {
  return fail(OTSDB_E_ILLEGAL_STATE,
              "Next timestamp is supposed to be strictly greater");
}

// ts_ms / val off the 16-byte alignment of the streaming loads
bool misaligned(const otsdb_batch* b) {
  return ((((uintptr_t)b->ts_ms) | ((uintptr_t)b->val)) & 15) != 0;
}

// what a multi-aggregator call counts: downsample and group passes (0, 0:
// the reset), no key transpose or class transform yet
void multi_counters(otsdb_ctx* c, int64_t ds, int64_t group) {
  c->n_multi_ds = ds;
  c->n_multi_group = group;
  c->n_multi_kt = c->n_multi_tf = 0;
  c->n_multi_fold = 0;
}

// --------------------------------------------------------------- planning
struct Plan {
  Params P;
  int64_t S, G, M, N;
  bool sel;  // percentile/median across series
};

// Calendar grid (otsdb_query_spec.cal_edges): the fixed-interval rules of
// make_params restated on the edge table — seek to the first edge >= start
// (ValuesInInterval.seekInterval rounds up, Downsampler.java:431-441), NONE:
// every edge <= end_ms; filling: [previousInterval(start),
// previousInterval(end)) advanced once when both coincide
// (FillingDownsampler.java:113-131).  With a context the table is copied to
// the device and P->cal points at the grid's bucket 0.
otsdb_status make_cal_params(const otsdb_query_spec* s, Params* P,
                             otsdb_ctx* c) {
  const int64_t* e = s->cal_edges;
  const int64_t n = s->n_cal_edges;
  auto first_ge = [&](int64_t t) {
    return (int64_t)(std::lower_bound(e, e + n, t) - e);
  };
  auto last_le = [&](int64_t t) {
    return (int64_t)(std::upper_bound(e, e + n, t) - e) - 1;
  };
  const int64_t k_seek = first_ge(s->start_ms);
  int64_t nb;
  if (P->fill) {
    const int64_t kA = last_le(s->start_ms);
    int64_t kE = last_le(s->end_ms);
    if (kE == kA) kE = kA + 1;
    nb = std::max<int64_t>(0, kE - k_seek);
    if (kA >= 0 && kA < k_seek) {
      P->rate_origin_ts = e[kA];
      P->rate_origin_val = P->fill_value;
    }
  } else {
    nb = std::max<int64_t>(0, last_le(s->end_ms) - k_seek + 1);
  }
  if (k_seek + nb >= n)
    return fail(OTSDB_E_UNSUPPORTED,
                "calendar table ends before the window (%lld edges)",
                (long long)n);
  P->nb = nb;
  P->gbase = e[k_seek];
  P->seek_ts = e[k_seek];
  P->stop_ts = e[k_seek + nb];
  P->narrow = 0;
  P->cal_lo = -k_seek;
  P->cal_n = n - k_seek;
  P->cal = nullptr;
  if (c) {
    otsdb_status rc = c->cal.ensure(sizeof(int64_t) * n);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(c->cal.p, e, sizeof(int64_t) * n,
                           hipMemcpyHostToDevice, c->stream));
    P->cal = (const int64_t*)c->cal.p + k_seek;
  }
  return OTSDB_OK;
}

// What of Params depends on the cross-series aggregator (a multi-aggregator
// call sets it per output over one shared grid).
void agg_params(Params* P, int agg_id, int interp) {
  P->interp = interp >= 0 ? interp : kAggs[agg_id].interp;
  P->pct = agg_id >= OTSDB_AGG_P999 ? pct_of(agg_id) : 0.0;
  P->pct_est = agg_id < OTSDB_AGG_P999   ? 0
               : agg_id < OTSDB_AGG_EP999R3 ? 0
               : agg_id < OTSDB_AGG_EP999R7 ? 3
                                            : 7;
}

// Per-series calendar grids (calendar.hip): the union grid U of stage B,
// each anchor's chain terminator, the window's seek and the stage-B spec.
struct AnchoredPlan {
  std::vector<int64_t> U, chain_end;
  int64_t seek_ts = 0;
  int64_t stop_b = 0;  // stage B's stop bound (NONE: U's first edge > end)
  // fill != none: FillingDownsampler's own grid FD (U then holds FD, then
  // the table's end t_end and t_end + 1: calendar.hip)
  std::vector<int64_t> FD;
  int64_t t_end = 0;
  otsdb_query_spec derived;
};

otsdb_status plan_anchored(const otsdb_query_spec* s, AnchoredPlan* A) {
  const int64_t n = s->n_cal_edges, na = s->n_cal_anchors;
  const int64_t* e = s->cal_edges;
  A->U.clear();
  A->U.reserve(n);
  for (int64_t k = 0; k < n; ++k)
    if (e[k] != INT64_MAX) A->U.push_back(e[k]);
  std::sort(A->U.begin(), A->U.end());
  A->U.erase(std::unique(A->U.begin(), A->U.end()), A->U.end());
  std::vector<int64_t> term(n + 1, n);
  for (int64_t k = n - 1; k >= 0; --k) term[k] = e[k] == INT64_MAX ? k : term[k + 1];
  A->chain_end.resize(na);
  for (int64_t j = 0; j < na; ++j) A->chain_end[j] = term[s->cal_anchor_edge[j]];
  // ValuesInInterval.seekInterval(start): previousInterval(start), stepped
  // once when start lies past it (Downsampler.java:419-429)
  const int64_t j = (int64_t)(std::upper_bound(s->cal_anchors,
                                               s->cal_anchors + na,
                                               s->start_ms) -
                              s->cal_anchors) - 1;
  int64_t k = s->cal_anchor_edge[j];
  if (s->start_ms > e[k]) ++k;
  if (e[k] == INT64_MAX)
    return fail(OTSDB_E_UNSUPPORTED, "calendar chain ends before the seek");
  A->seek_ts = e[k];
  if (s->fill != OTSDB_FILL_NONE) {
    // FillingDownsampler.java:113-135: previousInterval(start) = e[k0], then
    // the chain's steps while < previousInterval(end), advanced once when
    // the two coincide
    const int64_t k0 = s->cal_anchor_edge[j];
    const int64_t je = (int64_t)(std::upper_bound(s->cal_anchors,
                                                  s->cal_anchors + na,
                                                  s->end_ms) -
                                 s->cal_anchors) - 1;
    int64_t end_ts = s->cal_anchors[je];
    if (end_ts == e[k0]) {
      if (e[k0 + 1] == INT64_MAX)
        return fail(OTSDB_E_UNSUPPORTED, "calendar chain ends at the start");
      end_ts = e[k0 + 1];
    }
    A->FD.clear();
    int64_t kk = k0;
    for (; e[kk] != INT64_MAX && e[kk] < end_ts; ++kk) A->FD.push_back(e[kk]);
    if (e[kk] == INT64_MAX)
      return fail(OTSDB_E_UNSUPPORTED, "calendar chain ends before the window");
    // every point stage A' keeps lies on an FD edge: the last bucket's end
    // only has to lie past it (and at end_ms, so the table's grid ends there)
    A->t_end = std::max(s->end_ms, A->FD.back() + 1);
    A->U = A->FD;
    A->U.push_back(A->t_end);
    A->U.push_back(A->t_end + 1);
  }
  {
    const auto it = std::upper_bound(A->U.begin(), A->U.end(), s->end_ms);
    A->stop_b = it == A->U.end() ? INT64_MAX : *it;
  }
  A->derived = *s;
  A->derived.cal_edges = A->U.data();
  A->derived.n_cal_edges = (int64_t)A->U.size();
  A->derived.cal_anchors = nullptr;
  A->derived.cal_anchor_edge = nullptr;
  A->derived.n_cal_anchors = 0;
  return check_spec(&A->derived);
}

// The groups' tiles on the device (the cut itself: foldplan.h, cut_tiles),
// cached on its arguments
otsdb_status build_tiles(otsdb_ctx* c, const std::vector<int64_t>& goff,
                         bool sel_all = false, int64_t chunk = kChunk,
                         int64_t whole_upto = 0) {
  if (c->d_tiles.p && goff == c->goff_cache && sel_all == c->tiles_sel_all &&
      chunk == c->tiles_chunk && whole_upto == c->tiles_whole)
    return OTSDB_OK;
  const int64_t G = (int64_t)goff.size() - 1;
  const TileCut tc = cut_tiles(goff, sel_all, chunk, whole_upto, SEL_K, SEL_CHUNK);
  const auto &tg = tc.tg, &tm0 = tc.tm0, &tm1 = tc.tm1, &mg = tc.mg,
             &mt0 = tc.mt0, &mt1 = tc.mt1, &ag = tc.ag, &at0 = tc.at0,
             &at1 = tc.at1, &lgg = tc.lgg, &lgo = tc.lgo, &lgk = tc.lgk,
             &lgc = tc.lgc;
  const std::vector<uint8_t>& single = tc.single;
  const int64_t LG = (int64_t)lgg.size();
  const int64_t T = (int64_t)tg.size(), MG = (int64_t)mg.size();
  const int64_t max_chunks = tc.max_chunks;
  // layout: tg tm0 tm1 [T] | mg mt0 mt1 [MG] | ag at0 at1 [G] |
  //         lg_g lg_off lg_k [LG] | lg_ch0 [LG+1] | single [T]
  const size_t n64 = 3 * T + 3 * MG + 3 * G + 4 * LG + 1;
  const size_t bytes = n64 * 8 + T + 64;
  otsdb_status st = c->d_tiles.ensure(bytes);
  if (st) return st;
  std::vector<int64_t> h;
  h.reserve(n64);
  h.insert(h.end(), tg.begin(), tg.end());
  h.insert(h.end(), tm0.begin(), tm0.end());
  h.insert(h.end(), tm1.begin(), tm1.end());
  h.insert(h.end(), mg.begin(), mg.end());
  h.insert(h.end(), mt0.begin(), mt0.end());
  h.insert(h.end(), mt1.begin(), mt1.end());
  h.insert(h.end(), ag.begin(), ag.end());
  h.insert(h.end(), at0.begin(), at0.end());
  h.insert(h.end(), at1.begin(), at1.end());
  h.insert(h.end(), lgg.begin(), lgg.end());
  h.insert(h.end(), lgo.begin(), lgo.end());
  h.insert(h.end(), lgk.begin(), lgk.end());
  h.insert(h.end(), lgc.begin(), lgc.end());
  if (!h.empty())
    HIP_TRY(hipMemcpyAsync(c->d_tiles.p, h.data(), n64 * 8,
                           hipMemcpyHostToDevice, c->stream));
  if (T)
    HIP_TRY(hipMemcpyAsync((char*)c->d_tiles.p + n64 * 8, single.data(), T,
                           hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->goff_cache = goff;
  c->tiles_sel_all = sel_all;
  c->tiles_chunk = chunk;
  c->tiles_whole = whole_upto;
  c->n_tiles = T;
  c->n_multi = MG;
  c->n_large = LG;
  c->n_large_chunks = lgc.back();
  c->max_chunks = max_chunks;
  return OTSDB_OK;
}

struct Tiles {
  const int64_t *tg, *tm0, *tm1, *mg, *mt0, *mt1, *ag, *at0, *at1;
  const int64_t *lg_g, *lg_off, *lg_k, *lg_ch0;
  const uint8_t* single;
  int64_t T, MG, G, LG, LGCH;
  int64_t max_chunks;
};

Tiles tiles_of(otsdb_ctx* c, int64_t G) {
  Tiles t;
  const int64_t T = c->n_tiles, MG = c->n_multi;
  const int64_t* b = (const int64_t*)c->d_tiles.p;
  t.tg = b;
  t.tm0 = b + T;
  t.tm1 = b + 2 * T;
  t.mg = b + 3 * T;
  t.mt0 = t.mg + MG;
  t.mt1 = t.mg + 2 * MG;
  t.ag = b + 3 * T + 3 * MG;
  t.at0 = t.ag + G;
  t.at1 = t.ag + 2 * G;
  const int64_t LG = c->n_large;
  t.lg_g = b + 3 * T + 3 * MG + 3 * G;
  t.lg_off = t.lg_g + LG;
  t.lg_k = t.lg_g + 2 * LG;
  t.lg_ch0 = t.lg_g + 3 * LG;
  t.single = (const uint8_t*)(b + 3 * T + 3 * MG + 3 * G + 4 * LG + 1);
  t.LG = LG;
  t.LGCH = c->n_large_chunks;
  t.T = T;
  t.MG = MG;
  t.G = G;
  t.max_chunks = c->max_chunks;
  return t;
}

// (kCombineL1, kCombineSlices and two_level_combine: foldplan.h)
// the first-level slices' buffers
void carve_combine(Carve& cv, Work& W, int64_t n_comb, int64_t NB) {
  W.comb = cv.take<Packed>((size_t)n_comb * kCombineSlices * NB);
  W.comb_emit = cv.take<uint8_t>((size_t)n_comb * kCombineSlices * NB);
}

template <class M>
void launch_combine(otsdb_ctx* c, const Work& W, int64_t NB, int64_t n,
                    const int64_t* g, const int64_t* t0, const int64_t* t1,
                    double* out_val, uint8_t* out_emit, Packed* out_partial,
                    bool two_level, int keep_empty = 0, int* err = nullptr) {
  hipStream_t st = c->stream;
  if (!err) err = c->d_err;
  if (!two_level) {
    hipLaunchKernelGGL(k_combine<M>, dim3(blocks_for(n * NB, 256)), dim3(256),
                       0, st, NB, n, g, t0, t1, (const Packed*)W.partial,
                       (const uint8_t*)W.tile_emit, out_val, out_emit,
                       out_partial, err, (int64_t)0, keep_empty);
    return;
  }
  hipLaunchKernelGGL(k_combine_l1<M>,
                     dim3(blocks_for(n * kCombineSlices * NB, 256)), dim3(256),
                     0, st, NB, n, kCombineSlices, t0, t1,
                     (const Packed*)W.partial, (const uint8_t*)W.tile_emit,
                     W.comb, W.comb_emit);
  hipLaunchKernelGGL(k_combine<M>, dim3(blocks_for(n * NB, 256)), dim3(256), 0,
                     st, NB, n, g, t0, t1, (const Packed*)W.comb,
                     (const uint8_t*)W.comb_emit, out_val, out_emit,
                     out_partial, err, kCombineSlices, keep_empty);
}

// The per-downsampler kernels live in one translation unit per downsampling
// monoid (ds_tu.hip, built in parallel); this fills their launch record.
DsLaunch ds_args(otsdb_ctx* c, const Params& P, const BatchDev& B,
                 const Work& W) {
  DsLaunch a{};
  a.st = c->stream;
  a.P = P;
  a.B = B;
  a.SM = W.SM;
  a.R = W.R;
  a.err = c->d_err;
  return a;
}

// Whether the ordered group fold (fold.hip) runs this query: every
// downsampled, non-rate query with a monoid aggregator, fill or not (from
// compacted cells, cellfold.hip: when the grid fits one fold window).
// Rate queries keep RateSpan in k_bucketize_k's ring flush + k_group: a
// RateSpan-in-the-fold build measured slower on C4.
bool fold_path(const otsdb_query_spec* spec, const Params& P, int mode) {
  return !P.ds_sel && !P.rate && !P.run_all && !is_selection(spec->agg_id) &&
         mode != 2;
}

// ---- the fold's launch, shared by run_pipeline and multi_fold_pass --------
// The cells fold's per-series cursors (launch.h CellsFold), carved where the
// caller's layout has them; NW: the windows of THIS fold's state.
void carve_cells_fold(Carve& cv, CellsFold& CF, otsdb_ctx* c,
                      const CellsDev& cells, const int64_t* series_row,
                      int64_t S, int64_t NW) {
  CF.C = cells;
  CF.series_row = series_row;
  CF.wide = c->d_err + 1;
  CF.rlo = cv.take<int64_t>(S);
  CF.vlo = cv.take<int64_t>(S);
  CF.qw = cv.take<uint8_t>(S);
  CF.vl0 = cv.take<uint8_t>(S);
  CF.uf = cv.take<uint8_t>(S);
  if (NW > 1) {
    CF.wrlo = cv.take<int64_t>((size_t)S * (NW - 1));
    CF.wvlo = cv.take<int64_t>((size_t)S * (NW - 1));
    CF.wvl0 = cv.take<uint8_t>((size_t)S * (NW - 1));
  }
}

// the tiles and windows of a fold, for its prep kernels and the fold itself
void fold_args(DsLaunch& a, const Tiles& T, const int64_t* d_members,
               WinCtx* wc, int64_t NW, int64_t WB, uint8_t* tile_emit) {
  a.n_tiles = T.T;
  a.tg = T.tg;
  a.tm0 = T.tm0;
  a.tm1 = T.tm1;
  a.single = T.single;
  a.members = d_members;
  a.wc = wc;
  a.NW = NW;
  a.WB = WB;
  a.tile_emit = tile_emit;
}

// every series' bounds and, for grids of several windows, its context at
// each inner window boundary; cells: from compacted columns (a.cf)
template <class M>
void fold_prep(otsdb_ctx* c, const DsLaunch& a, bool cells) {
  StageTimer tm(c, 3);
  if (cells) {
    launch_cells<M>(DS_CELLS_PREP, a);
    if (!c->cells_no_uni) launch_cells<M>(DS_CELLS_UNIFORM, a);
    if (a.NW > 1) launch_cells<M>(DS_CELLS_FOLD_PREP, a);
  } else if (a.NW > 1 && a.B.S * (a.NW - 1) <= prep_fold_max()) {
    launch_ds<M>(DS_PREP_FOLD, a);
  } else {
    launch_ds<M>(DS_PREP, a);
    if (a.NW > 1) launch_ds<M>(DS_FOLD_PREP, a);
  }
}

// Which cells fold kernel runs (DsLaunch.cells_variant), 0: none.  The
// kernels fix the qualifier width at compile time (one copy of the member
// loop per kernel: 14 % faster on C2's cells than a width read per member).
// k_cells_prep's bits 0 / 1: 4- / 2-byte series kept; both ->
// ERR_CELLS_GENERIC and nothing is launched: the engine rewrites the batch
// with one width (k_requal) and runs again.  k_cells_uniform's bit 2: some
// kept series is not uniform (or the uniform kernel already missed in this
// call): the general walker.  Waits for the prep kernels.
int cells_fold_variant(otsdb_ctx* c) {
  hipStream_t st = c->stream;
  int widths = 3;
  bool uniform = false;
  if (hipMemcpyAsync(&c->h_small[2], c->d_err, 2 * sizeof(int),
                     hipMemcpyDeviceToHost, st) == hipSuccess &&
      hipStreamSynchronize(st) == hipSuccess) {
    widths = (int)((c->h_small[2] >> 32) & 3);
    uniform = !c->cells_no_uni && !((c->h_small[2] >> 32) & 4);
  }
  if (widths == 3) {
    const int e = (int)(c->h_small[2] & 0xFFFFFFFF) | ERR_CELLS_GENERIC;
    c->h_small[3] = e;
    hipMemcpyAsync(c->d_err, &c->h_small[3], sizeof(int),
                   hipMemcpyHostToDevice, st);
    return 0;
  }
  ++(uniform ? c->n_cells_uniform : c->n_cells_general);
  return (widths == 1 ? 4 : 2) + (uniform ? 8 : 0);
}

// ---- the row path, part 1: "build the rows" ------------------------------
// Per-series bucket rows W.R from the point stream (or the compacted
// columns): prep + k_bucketize_k / the rate-fused ring / k_ds_select /
// k_bucketize_cells.  Nothing here depends on the cross-series aggregator,
// so a multi-aggregator call runs it once.
otsdb_status build_rows(otsdb_ctx* c, const otsdb_query_spec* spec,
                        const Params& P, const BatchDev& B, const Work& W,
                        const CellsDev* cells, const int64_t* series_row,
                        bool rate_fused) {
  hipStream_t st = c->stream;
  const int64_t S = B.S;
  DsLaunch a = ds_args(c, P, B, W);
  bool ok = true;
  if (cells) {
    // decode fused into the downsample (decode.hip)
    ok = with_monoid(spec->ds_agg_id, [&](auto tag) {
      using M = decltype(tag);
      StageTimer tm(c, 0);
      a.cells = *cells;
      a.series_row = series_row;
      launch_ds<M>(DS_CELLS, a);
    });
  } else if (c->rollup) {
    // rollup avg / count (rollup.hip): the same prep and ring, the counts
    // beside the batch
    {
      StageTimer tm(c, 3);
      launch_rollup(c->rollup, DS_PREP, a, c->rollup_cnt);
    }
    StageTimer tm(c, 0);
    launch_rollup(c->rollup, DS_RING, a, c->rollup_cnt);
  } else if (P.ds_sel) {
    // median / percentile downsampling: per-bucket selection
    {
      StageTimer tm(c, 3);
      launch_ds<MSum<3>>(DS_PREP, a);
    }
    StageTimer tm(c, 0);
    hipLaunchKernelGGL(k_ds_select, dim3((unsigned)S), dim3(64), 0, st, P, B,
                       W.SM, W.R);
  } else {
    ok = with_monoid(spec->ds_agg_id, [&](auto tag) {
      using M = decltype(tag);
      {
        StageTimer tm(c, 3);
        launch_ds<M>(DS_PREP, a);
      }
      StageTimer tm(c, 0);
      if (rate_fused) {
        // RateSpan fused into the ring flush (1,024-bucket ring: a step
        // hands its series back only across a gap of ~1,000 buckets); then
        // the plain ring kernel for the series handed back
        a.P.redo = W.redo;
        launch_ds<M>(DS_RATE, a);
        a.P.only_redo = 1;
        launch_ds<M>(DS_RING, a);
      } else {
        launch_ds<M>(DS_RING, a);
      }
    });
  }
  if (!ok) return fail(OTSDB_E_UNSUPPORTED, "downsampler %d", spec->ds_agg_id);
  return OTSDB_OK;
}

// ---- the row path, part 2: "aggregate the rows" --------------------------
// k_transform in place: what each series contributes at every bucket (fill,
// rate, interpolation P.interp).
void transform_rows(otsdb_ctx* c, Params& P, const BatchDev& B, const Work& W,
                    bool rate_fused) {
  StageTimer tm(c, 1);
  if (rate_fused) {  // only the series the fused kernel handed back
    P.redo = W.redo;
    P.only_redo = 1;
  }
  hipLaunchKernelGGL(k_transform<0>, dim3(blocks_for(B.S, 4)), dim3(256), 0,
                     c->stream, P, B, W.SM, W.R, c->d_err);
  P.only_redo = 0;
}

// what the group stage needs beside the rows, the tiles and the outputs
struct AggStage {
  const int64_t* d_members;
  int64_t M;  // members of all groups
  int mode;
  bool fold, two_level;
  Packed* gpart;
  uint8_t* gemit;
  const Packed* ginit;
  const uint8_t* ginit_emit;
};

// percentiles over a FillingDownsampler grid with every group large: the
// keys transpose applies the fill and counts, no k_transform / k_group
// (cross-rank, mode 2: the same transpose; otsdb_sel_prepare_device
// derives the counts from its per-tile counts)
bool sel_fused_path(int agg_id, int mode, const Params& P, const Tiles& T,
                    int64_t G) {
  return is_selection(agg_id) && (mode == 0 || mode == 2) && P.sentinel &&
         P.fill && !P.rate && !P.run_all && T.LG > 0 && T.LG == G;
}

otsdb_status sel_fused_keys(otsdb_ctx* c, const Params& P, const Work& W,
                            const Tiles& T, int64_t NB, const AggStage& A) {
  hipStream_t st = c->stream;
  HIP_TRY(hipMemsetAsync(W.lg_kept, 0, (size_t)T.LG * 4, st));
  SelFill F{W.SM.keep, W.SM.kf, W.SM.kl, P.fill_value, W.key_cnt,
            T.lg_off, T.LG, W.lg_kept};
  if (A.M > 0)
    hipLaunchKernelGGL(k_keys_transpose<true>, kt_grid(A.M, NB),
                       dim3(KT_THREADS), 0, st, NB, A.M, A.d_members, W.R,
                       W.keys, W.key_mm, F);
  return OTSDB_OK;
}

void sel_fused_select(otsdb_ctx* c, const Work& W, const Tiles& T, int64_t NB,
                      const AggStage& A, int median, double pct,
                      double* out_val, uint8_t* out_emit, int* err) {
  const int64_t NSEG = T.LG * NB;
  hipLaunchKernelGGL(k_seg_select, dim3((unsigned)NSEG), dim3(SS_THREADS), 0,
                     c->stream, NB, A.M, T.LG, T.lg_g, T.lg_off, T.lg_k,
                     (const uint64_t*)W.keys, (const SelState*)nullptr,
                     (const uint8_t*)nullptr, out_val, err, median, pct,
                     (const uint64_t*)W.key_mm, (const uint32_t*)W.key_cnt,
                     (const uint32_t*)W.lg_kept, out_emit);
}

// n (non-NaN contributions) and the emit mask of every group, into
// W.out_val / W.out_emit: the same for every selection over the same rows
void sel_counts(otsdb_ctx* c, const Work& W, const Tiles& T, int64_t NB,
                const AggStage& A, int* err) {
  using MC = MSum<3>;
  if (T.T > 0)
    hipLaunchKernelGGL(k_group<MC>, dim3(blocks_for(T.T * NB, 256)), dim3(256),
                       0, c->stream, NB, T.T, T.tg, T.tm0, T.tm1, T.single,
                       A.d_members, W.R, W.partial, W.tile_emit, W.out_val,
                       W.out_emit, err, 0, (const Packed*)nullptr,
                       (const uint8_t*)nullptr);
  if (T.MG > 0)
    launch_combine<MC>(c, W, NB, T.MG, T.mg, T.mt0, T.mt1, W.out_val,
                       W.out_emit, nullptr, A.two_level, 0, err);
}

// the rows' keys, member-major per bucket (read-only afterwards)
void sel_keys(otsdb_ctx* c, const Work& W, int64_t NB, const AggStage& A) {
  if (A.M > 0)
    hipLaunchKernelGGL(k_keys_transpose<false>, kt_grid(A.M, NB),
                       dim3(KT_THREADS), 0, c->stream, NB, A.M, A.d_members,
                       W.R, W.keys, W.key_mm, SelFill{});
}

// one selection over counts (W.out_val / W.out_emit, overwritten with the
// results) and keys; transpose: the keys are not built yet
void sel_finish(otsdb_ctx* c, const Work& W, const Tiles& T, int64_t NB,
                const AggStage& A, int median, double pct, bool transpose,
                int* err) {
  hipStream_t st = c->stream;
  // groups of <= SEL_K series: sort in LDS
  hipLaunchKernelGGL(k_group_select, dim3(blocks_for(T.T * NB, SEL_THREADS)),
                     dim3(SEL_THREADS), 0, st, NB, T.T, T.tg, T.tm0, T.tm1,
                     T.single, A.d_members, W.R, W.out_val, W.out_emit, err,
                     median, pct);
  // larger groups: radix select over transposed keys
  if (T.LG > 0) {
    const int64_t NSEG = T.LG * NB;
    if (transpose) sel_keys(c, W, NB, A);
    hipLaunchKernelGGL(k_sel_init, dim3(blocks_for(NSEG, 256)), dim3(256), 0,
                       st, NB, T.LG, T.lg_g, (const double*)W.out_val,
                       (const uint8_t*)W.out_emit, W.sel, median, pct);
    // one workgroup per (group, bucket) segment: min/max, 11-bit digit
    // passes until <= SS_CAP candidates, LDS gather + count select
    hipLaunchKernelGGL(k_seg_select, dim3((unsigned)NSEG), dim3(SS_THREADS), 0,
                       st, NB, A.M, T.LG, T.lg_g, T.lg_off, T.lg_k,
                       (const uint64_t*)W.keys, (const SelState*)W.sel,
                       (const uint8_t*)W.out_emit, W.out_val, err, median, pct,
                       (const uint64_t*)W.key_mm, (const uint32_t*)nullptr,
                       (const uint32_t*)nullptr, (uint8_t*)nullptr);
  }
}

// a monoid aggregator: k_group over the rows (not after the ordered fold,
// which left the tile partials itself), then the chunk merge
otsdb_status group_rows(otsdb_ctx* c, int agg_id, const Work& W,
                        const Tiles& T, int64_t NB, int64_t G,
                        const AggStage& A, int* err) {
  const bool ok = with_monoid(agg_id, [&](auto tag) {
    using M = decltype(tag);
    if (!A.fold && T.T > 0)
      hipLaunchKernelGGL(k_group<M>, dim3(blocks_for(T.T * NB, 256)), dim3(256),
                         0, c->stream, NB, T.T, T.tg, T.tm0, T.tm1, T.single,
                         A.d_members, W.R, W.partial, W.tile_emit, W.out_val,
                         W.out_emit, err, A.mode, A.ginit, A.ginit_emit);
    if (A.mode == 0) {
      if (T.MG > 0)
        launch_combine<M>(c, W, NB, T.MG, T.mg, T.mt0, T.mt1, W.out_val,
                          W.out_emit, nullptr, A.two_level, 0, err);
    } else {
      launch_combine<M>(c, W, NB, G, T.ag, T.at0, T.at1, W.out_val, A.gemit,
                        A.gpart, A.two_level, A.ginit ? 1 : 0, err);
    }
  });
  if (!ok) return fail(OTSDB_E_NO_SUCH_ELEMENT, "aggregator %d", agg_id);
  return OTSDB_OK;
}

// Which path a query takes and how its groups are tiled.  Values only: no
// device state is touched.
struct Route {
  bool fold;       // the ordered group fold (else the row path)
  bool ordered;    // the aggregator reduces a group in one chain (dev)
  int64_t wb_cap;  // fold: the most buckets of a window, fold_wb<A>()
  int64_t chunk, whole_upto;  // build_tiles' cut of the groups
};

// cells: the series come as compacted columns; chained: the chains continue
// a previous rank's states (ginit)
otsdb_status route_pipeline(otsdb_ctx* c, const otsdb_query_spec* spec,
                            const std::vector<int64_t>& goff, const Params& P,
                            int64_t S, int mode, bool cells, bool chained,
                            Route* R) {
  const int64_t NB = P.nb;
  // chained partials continue each group's state in k_group (the row path)
  // (a rollup call's states exist only for the row path's prep and ring)
  bool fold = fold_path(spec, P, mode) && !chained && !c->rollup;
  int64_t WB = 0;
  if (fold && !with_monoid(spec->agg_id, [&](auto tag) {
        WB = fold_wb<decltype(tag)>();
      }))
    return fail(OTSDB_E_NO_SUCH_ELEMENT, "aggregator %d", spec->agg_id);
  // the cells fold runs on narrow grids (32-bit times), windows after the
  // first starting from k_cells_fold_prep's cursors; calendar grids from
  // cells take k_bucketize_cells and the row pipeline
  if (cells && !P.narrow) fold = false;
  bool ordered = false;
  with_monoid(spec->agg_id, [&](auto tag) {
    ordered = decltype(tag)::kOrdered;
  });
  // OTSDB_SPEC_EXACT_ORDER: every group one chain, whatever its size
  const bool exact = ordered && (spec->flags & OTSDB_SPEC_EXACT_ORDER) != 0;
  if (ordered && fold) {
    // a group past one fold tile takes the row path (one chain per bucket)
    // when its bucket matrix (8-byte value + state byte per series and
    // bucket) fits the fixed row budget — a bound of the query alone, so
    // identical queries always take the same path (and the same order);
    // otherwise the fold's tiles stay, merged in order (Chan) like a group
    // past the exact-chain bound, or E_CAPACITY when the caller asked for
    // the exact order
    int64_t kmax = 0;
    for (size_t g = 0; g + 1 < goff.size(); ++g)
      kmax = std::max(kmax, goff[g + 1] - goff[g]);
    if (kmax > kOrderedFoldChunk) {
      if ((double)S * (double)NB * 9.0 <= kOrderedRowBudget) {
        fold = false;
      } else if (exact) {
        return fail(OTSDB_E_CAPACITY,
                    "exact-order dev: %lld x %lld bucket rows past the row "
                    "budget", (long long)S, (long long)NB);
      }
    }
  }
  const bool cfold = cells && fold;
  // verbatim storage rows: the single-window cells fold only (it checks
  // what compaction would change; window boundaries it does not see)
  if (c->verbatim && (!cfold || NB > WB)) return spec_miss(c);
  // the chained entry always takes the row path (its chains continue from
  // the previous rank's states): past the row budget a clear E_CAPACITY
  if (chained && (double)S * (double)NB * 9.0 > kOrderedRowBudget)
    return fail(OTSDB_E_CAPACITY,
                "chained partials: %lld x %lld bucket rows past the row budget",
                (long long)S, (long long)NB);
  if (exact && mode == 1 && !chained)
    return fail(OTSDB_E_UNSUPPORTED,
                "exact-order dev across ranks: hand the chains on "
                "(otsdb_agg_partials_chained_device)");
  R->fold = fold;
  R->ordered = ordered;
  R->wb_cap = WB;
  if (fold) {
    const FoldTiling ft = fold_tiling(ordered);
    R->chunk = ft.chunk;
    R->whole_upto = ft.whole_upto;
  } else {
    // the row path's k_group: one chain per (group, bucket) up to
    // kOrderedChunk members; partials for the merge across ranks (a group
    // too large to hand on, dist.py) keep round 4's shorter chains, merged
    // in order anyway
    R->chunk = kChunk;
    R->whole_upto = !ordered ? 0
                    : exact  ? INT64_MAX
                    : mode == 1 && !chained ? kOrderedChunkMerged
                                            : kOrderedChunk;
  }
  return OTSDB_OK;
}

// Everything up to dense (group, bucket) results / partials.
// mode 0: final dense results; mode 1: per-group partials into `gpart/gemit`;
// mode 2: the cross-rank selection protocol's local part.
// cells != null: the series come as compacted columns (k_bucketize_cells
// decodes them inside the downsample; B carries only S)
otsdb_status run_pipeline(otsdb_ctx* c, const otsdb_query_spec* spec,
                          const BatchDev& B, const int64_t* d_members,
                          std::vector<int64_t>& goff, Params& P, Work& W,
                          int mode, Packed* gpart, uint8_t* gemit,
                          const CellsDev* cells = nullptr,
                          const int64_t* series_row = nullptr,
                          const Packed* ginit = nullptr,
                          const uint8_t* ginit_emit = nullptr) {
  hipStream_t st = c->stream;
  const int64_t S = B.S;
  const int64_t G = (int64_t)goff.size() - 1;
  const int64_t nb = P.nb;

  // grid trimming for very wide windows (NONE fill only): the rows span only
  // the buckets that hold data
  if (!cells && !P.run_all && !P.fill && !P.cal &&
      (double)S * (double)nb > 4.0e9) {
    unsigned long long init[2] = {~0ULL, 0ULL};
    HIP_TRY(hipMemcpyAsync(c->d_mm, init, 16, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_bounds, dim3(blocks_for(S, 256)), dim3(256), 0, st, P,
                       B, c->d_mm);
    unsigned long long mm[2];
    HIP_TRY(hipMemcpyAsync(mm, c->d_mm, 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (mm[0] > mm[1]) {
      P.nb = 0;
    } else {
      const int64_t b_lo = ((int64_t)mm[0] - P.gbase) / P.interval;
      const int64_t b_hi = ((int64_t)mm[1] - P.gbase) / P.interval;
      P.gbase += b_lo * P.interval;
      P.nb = b_hi - b_lo + 1;
    }
  }
  const int64_t NB = P.nb;
  // bucket indices are 32-bit inside the kernels (SeriesMeta.kf/kl, the
  // wave-scan keys): a wider grid would wrap silently
  if (NB > (int64_t)INT32_MAX - 2)
    return fail(OTSDB_E_UNSUPPORTED, "bucket grid of %lld buckets per series",
                (long long)NB);
  Route R;
  otsdb_status rc =
      route_pipeline(c, spec, goff, P, S, mode, cells != nullptr,
                     ginit != nullptr, &R);
  if (rc) return rc;
  const bool fold = R.fold, cfold = cells && fold;
  rc = build_tiles(c, goff, mode == 2, R.chunk, R.whole_upto);
  if (rc) return rc;
  const Tiles T = tiles_of(c, G);
  // the fold's windows and member contexts (foldplan.h); verbatim rows keep
  // their one window
  P.fold_wb = 0;  // (P may come from an earlier pipeline run)
  P.fold_ctx = 0;
  int64_t WB = 0, NW = 0;
  if (fold) {
    const FoldPlan fp =
        fold_plan(goff, T.T, NB, R.wb_cap, R.ordered, !c->verbatim);
    WB = fp.WB;
    NW = fp.NW;
    P.fold_wb = fp.fold_wb;
    P.fold_ctx = fp.fold_ctx;
  }
  // the bucket matrix (series rows) exists only off the fold path
  if (!fold && (double)S * (double)NB > 2.0e10)
    return fail(OTSDB_E_UNSUPPORTED, "bucket grid too large (%lld x %lld)",
                (long long)S, (long long)NB);

  // workspace
  const bool sel_large = is_selection(spec->agg_id) && (T.LG > 0 || mode == 2);
  const int64_t n_comb = (mode == 1) ? G : T.MG;
  const bool two_level = two_level_combine(T.max_chunks, n_comb, NB);
  const size_t rows = fold ? 0 : (size_t)S * NB;
  WinCtx* wc = nullptr;
  CellsFold CF{};
  auto carve = [&](char* base) {
    Carve cv{base};
    carve_series(cv, W, S);
    W.R.val = cv.take<double>(rows);
    W.R.state = cv.take<uint8_t>(rows);
    W.partial = cv.take<Packed>((size_t)T.T * NB);
    W.tile_emit = cv.take<uint8_t>((size_t)T.T * NB);
    W.out_val = cv.take<double>((size_t)G * NB);
    W.out_emit = cv.take<uint8_t>((size_t)G * NB);
    W.counts = cv.take<int64_t>(G + 1);
    if (NW > 1) wc = cv.take<WinCtx>((size_t)S * (NW - 1));
    if (cfold) carve_cells_fold(cv, CF, c, *cells, series_row, S, NW);
    if (two_level) carve_combine(cv, W, n_comb, NB);
    if (sel_large) carve_selection(cv, W, goff.back(), T.LG, NB, mode == 2);
    return cv.off + 256;
  };
  const size_t need = carve(nullptr);
  rc = c->ws.ensure(need);
  if (rc) return rc;
  carve((char*)c->ws.p);

  // the error word (+ the cells fold's "wide" word): zero already when the
  // previous call ended in the one-pass compaction
  if (cells || mode != 0 || !c->clean_entry)
    HIP_TRY(hipMemsetAsync(c->d_err, 0, 2 * sizeof(int), st));
  c->clean_entry = false;
  // every (group, bucket) emit flag is written by the fold / k_group /
  // k_combine of a group with members; only empty groups need the zeroes
  bool empty_group = false;
  for (int64_t g = 0; g < G && !empty_group; ++g)
    empty_group = goff[g + 1] == goff[g];
  if (G * NB > 0 && mode != 1 && empty_group)
    HIP_TRY(hipMemsetAsync(W.out_emit, 0, (size_t)G * NB, st));
  // the ring-sink k_bucketize leaves sentinel rows whose states k_transform
  // writes; the cells and selection downsamplers store states into a
  // zeroed row
  P.sentinel = !fold && !cells && !P.ds_sel;
  if (!fold && S > 0 && NB > 0 && !P.sentinel)
    HIP_TRY(hipMemsetAsync(W.R.state, 0, (size_t)S * NB, st));
  // RateSpan inside k_bucketize (NONE fill; the FillingDownsampler's rate
  // origin and fill points stay with k_transform)
  const bool rate_fused =
      P.sentinel && P.rate && !P.fill && !P.run_all && !c->rollup;

#ifdef OTSDB_DEBUG_SYNC
  fprintf(stderr, "[otsdb] pipeline S=%lld NB=%lld fold=%d NW=%lld T=%lld G=%lld\n",
          (long long)S, (long long)NB, (int)fold, (long long)NW, (long long)T.T,
          (long long)G);
#endif
  OTSDB_DBG(st, "setup");
  if (fold && S > 0 && NB > 0) {
    // downsample + contribution + aggregator in one ordered pass
    DsLaunch a = ds_args(c, P, B, W);
    fold_args(a, T, d_members, wc, NW, WB, W.tile_emit);
    a.cf = CF;
    a.partial = W.partial;
    a.out_val = W.out_val;
    a.out_emit = W.out_emit;
    a.always_partial = mode == 1;
    a.agg_id = spec->agg_id;
    const bool ok = with_monoid(spec->ds_agg_id, [&](auto tag) {
      using M = decltype(tag);
      fold_prep<M>(c, a, cfold);
      StageTimer tm(c, 0);
      if (T.T == 0) return;
      if (!cfold) {
        launch_ds<M>(DS_FOLD, a);
      } else if ((a.cells_variant = cells_fold_variant(c)) != 0) {
        launch_cells<M>(DS_CELLS_FOLD, a);
      }
    });
    if (!ok) return fail(OTSDB_E_UNSUPPORTED, "downsampler %d", spec->ds_agg_id);
  } else if (S > 0 && NB > 0) {
    rc = build_rows(c, spec, P, B, W, cells, series_row, rate_fused);
    if (rc) return rc;
  }
  const bool sel_fused = sel_fused_path(spec->agg_id, mode, P, T, G);
  if (!fold && S > 0 && NB > 0 && !sel_fused)
    transform_rows(c, P, B, W, rate_fused);
  if (G > 0 && NB > 0) {
    StageTimer tm(c, 2);
    const AggStage A{d_members, goff.back(), mode, fold, two_level,
                     gpart,     gemit,       ginit, ginit_emit};
    if (is_selection(spec->agg_id)) {
      if (mode == 1)
        return fail(OTSDB_E_UNSUPPORTED,
                    "percentiles across ranks: use the otsdb_sel_* protocol");
      const int median = spec->agg_id == OTSDB_AGG_MEDIAN ? 1 : 0;
      if (sel_fused) {
        rc = sel_fused_keys(c, P, W, T, NB, A);
        if (rc) return rc;
        W.sel_fused = true;
        if (mode == 2) {
          HIP_TRY(hipGetLastError());
          return OTSDB_OK;
        }
        sel_fused_select(c, W, T, NB, A, median, P.pct, W.out_val, W.out_emit,
                         c->d_err);
        HIP_TRY(hipGetLastError());
        return OTSDB_OK;
      }
      sel_counts(c, W, T, NB, A, c->d_err);
      if (mode == 2) {
        // cross-rank protocol: local counts + keys only (otsdb_sel_*)
        sel_keys(c, W, NB, A);
        HIP_TRY(hipGetLastError());
        return OTSDB_OK;
      }
      sel_finish(c, W, T, NB, A, median, P.pct, /*transpose=*/true, c->d_err);
    } else {
      rc = group_rows(c, spec->agg_id, W, T, NB, G, A, c->d_err);
      if (rc) return rc;
    }
  }
  HIP_TRY(hipGetLastError());
  return OTSDB_OK;
}

// err / small: the error word the compaction swaps out and where its
// {error word, total} lands (default: the context's, read by finish)
otsdb_status compact(otsdb_ctx* c, const Params& P, int64_t G,
                     const double* out_val, const uint8_t* out_emit,
                     int64_t* counts, otsdb_result* out, int* err = nullptr,
                     int64_t* small = nullptr) {
  hipStream_t st = c->stream;
  if (!err) err = c->d_err;
  if (!small) small = c->d_done;
  if (G == 0) {
    HIP_TRY(hipMemsetAsync(out->offsets, 0, sizeof(int64_t), st));
    return OTSDB_OK;
  }
  if (P.nb == 0) {
    HIP_TRY(hipMemsetAsync(out->offsets, 0, sizeof(int64_t) * (G + 1), st));
    return OTSDB_OK;
  }
  StageTimer tm(c, 4);
  // grids of up to kCmpRegBuckets: one pass (k_compact1: count, look-back
  // scan, scatter); longer: k_compact_count, k_scan, k_compact_scatter.
  // Either way the call's {error word, total} lands in `small` (mapped host
  // memory) for finish.  Scratch: flags [G] (one pass) or counts [G]
  const size_t need = (size_t)G * 8 + 256;
  const bool grow = need > c->cmp_flags.cap;
  otsdb_status rc = c->cmp_flags.ensure(need);
  if (rc) return rc;
  void* p = c->cmp_flags.p;
  const size_t cap = c->cmp_flags.cap;
  // epochs 1, 2, ..., 2^24 - 1, then 4, 5, ...: never 0 (fresh granules)
  // and always one ticket slot on from the last call's (k_compact1).  A
  // granule is taken as this call's by its epoch alone, so when the epoch
  // wraps every granule is cleared: one a call 2^24 - 4 calls ago left (a
  // group index only smaller or long-grid calls used since) would otherwise
  // read as published now
  const bool wrap = c->cmp_epoch + 1 == (1u << 24);
  c->cmp_epoch = wrap ? 4u : c->cmp_epoch + 1;
  if (grow || wrap) HIP_TRY(hipMemsetAsync(p, 0, cap, st));  // no stale epochs
  unsigned long long* ticket = (unsigned long long*)((char*)c->d_err + 192);
  // few groups (C1's 100): one group (wavefront) per block, spread over more
  // CUs; many (C2's 10k): four per block (one wave per block ran C2's
  // compaction 0.20 -> 0.27 ms)
  const int gpb = G < 4096 ? 1 : 4;
  if (P.nb <= kCmpRegBuckets) {
    hipLaunchKernelGGL(k_compact1, dim3(blocks_for(G, gpb)),
                       dim3(64 * gpb), 0, st, P, G, out_val, out_emit,
                       (unsigned long long*)p, ticket, c->cmp_epoch,
                       out->offsets, out->capacity, out->ts, out->val,
                       out->is_int, err, small);
  } else {
    int64_t* cnt = (int64_t*)p;
    hipLaunchKernelGGL(k_compact_count, dim3(blocks_for(G, gpb)),
                       dim3(64 * gpb), 0, st, P, G, out_emit, cnt, ticket,
                       c->cmp_epoch);
    hipLaunchKernelGGL(k_scan, dim3(1), dim3(1024), 0, st, G,
                       (const int64_t*)cnt, out->offsets);
    hipLaunchKernelGGL(k_compact_scatter, dim3(blocks_for(G, gpb)),
                       dim3(64 * gpb), 0, st, P, G, out_val, out_emit,
                       (const int64_t*)cnt, (const int64_t*)out->offsets,
                       out->capacity, out->ts, out->val, out->is_int,
                       err, small);
  }
  HIP_TRY(hipGetLastError());
  c->small_ready = true;
  return OTSDB_OK;
}

// the status of one result: its device error word, then its capacity
otsdb_status result_status(int err, int64_t total, int64_t capacity) {
  if (err & ERR_NONE_MULTI)
    return fail(OTSDB_E_ILLEGAL_DATA, "More than one value in aggregator raw");
  if (err & ERR_RATE_TS)
    return fail(OTSDB_E_ILLEGAL_STATE,
                "Next timestamp is supposed to be strictly greater than the "
                "previous one");
  if (err & ERR_INFINITY)
    return fail(OTSDB_E_ILLEGAL_STATE, "Got Infinity");
  if (err & ERR_RAW_DUP)
    return fail(OTSDB_E_UNSUPPORTED,
                "raw group-by: timestamps decrease inside a span, or a "
                "timestamp repeats more than 65,536 times");
  if (err & ERR_X1_MASK)
    return fail(OTSDB_E_ILLEGAL_STATE, "x1 beyond the millisecond mask");
  if (err & ERR_SEL_TOO_BIG)
    return fail(OTSDB_E_UNSUPPORTED,
                "percentile/median over groups of more than %d series is not "
                "offloaded yet", SEL_K);
  if (err & ERR_CAL_RANGE)
    return fail(OTSDB_E_UNSUPPORTED,
                "a point past the window lies outside the calendar table");
  if (err & ERR_INTERNAL)
    return fail(OTSDB_E_DEVICE, "internal: bucket outside the group row");
  if (total > capacity)
    return fail(OTSDB_E_CAPACITY, "result capacity %lld < %lld points",
                (long long)capacity, (long long)total);
  return OTSDB_OK;
}

// reads the error word and the total point count; maps to a status
otsdb_status finish(otsdb_ctx* c, int64_t G, otsdb_result* out) {
  hipStream_t st = c->stream;
  if (c->small_ready) {
    // the compaction left {error word, total} in host memory and zeroed the
    // word (one synchronisation, no copy launch)
    c->small_ready = false;
    HIP_TRY(hipStreamSynchronize(st));
    c->h_small[0] = __atomic_load_n(&c->h_done[0], __ATOMIC_ACQUIRE);
    c->h_small[1] = __atomic_load_n(&c->h_done[1], __ATOMIC_ACQUIRE);
    // a look-back that gave up (k_compact1's bounded spin: never expected)
    // marks h_done[2] with a plain store, after the last group may already
    // have swapped the error word out: report it here, and leave the device
    // word (which may hold its bit) to the next call's memset
    if (__atomic_load_n(&c->h_done[2], __ATOMIC_ACQUIRE)) {
      c->h_done[2] = 0;
      c->h_small[0] |= ERR_INTERNAL;
    } else {
      c->err_clean = true;
    }
  } else {
    HIP_TRY(hipMemcpyAsync(&c->h_small[0], c->d_err, sizeof(int),
                           hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&c->h_small[1], out->offsets + G, sizeof(int64_t),
                           hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
  }
  const otsdb_status rc = result_status((int)(c->h_small[0] & 0xFFFFFFFF),
                                        c->h_small[1], out->capacity);
  if (rc == OTSDB_E_CAPACITY)
    c->result_short = true;  // the offsets are whole: the host entries return them
  return rc;
}

// Raw (non-downsampled) group-by, raw.hip.  Device pointers throughout.
otsdb_status run_raw(otsdb_ctx* c, const otsdb_query_spec* spec,
                     const otsdb_batch* b, const BatchDev& B,
                     const std::vector<int64_t>& goff, const Params& P,
                     otsdb_result* out) {
  hipStream_t st = c->stream;
  const int64_t S = B.S, N = b->n_points;
  const int64_t G = (int64_t)goff.size() - 1, M = goff.back();
  const bool rate = P.rate != 0;
  int64_t kmax = 0;
  for (int64_t g = 0; g < G; ++g) kmax = std::max(kmax, goff[g + 1] - goff[g]);
  // ---- phase 1 workspace: per series / member / group
  int64_t *lo, *hi, *rts = nullptr, *rval = nullptr, *ccount, *coff, *segb,
      *sege, *counts;
  auto carve1 = [&](char* base) {
    Carve cv{base};
    lo = cv.take<int64_t>(S + 1);
    hi = cv.take<int64_t>(S + 1);
    if (rate) {
      rts = cv.take<int64_t>(N + 1);
      rval = cv.take<int64_t>(N + 1);
    }
    ccount = cv.take<int64_t>(M + 1);
    coff = cv.take<int64_t>(M + 1);
    segb = cv.take<int64_t>(G + 1);
    sege = cv.take<int64_t>(G + 1);
    counts = cv.take<int64_t>(G + 1);
    return cv.off + 256;
  };
  otsdb_status rc = c->ws.ensure(carve1(nullptr));
  if (rc) return rc;
  carve1((char*)c->ws.p);
  HIP_TRY(hipMemsetAsync(c->d_err, 0, sizeof(int), st));
  if (G == 0) {
    HIP_TRY(hipMemsetAsync(out->offsets, 0, sizeof(int64_t), st));
    return finish(c, G, out);
  }
  if (S > 0) {
    hipLaunchKernelGGL(k_raw_prep, dim3(blocks_for(S, 256)), dim3(256), 0, st,
                       P, B, lo, hi);
    if (rate)
      hipLaunchKernelGGL(k_raw_rate, dim3(blocks_for(S, 4)), dim3(256), 0, st,
                         P, B, lo, hi, rts, rval, c->d_err);
  }
  RawView V;
  V.ts = rate ? rts : B.ts;
  V.val = rate ? rval : B.val;
  V.is_float = rate ? nullptr : B.is_float;
  V.series_float = rate ? nullptr : B.series_float;
  V.all_double = rate || (!B.is_float && !B.series_float);
  V.lo = lo;
  V.hi = hi;
  const int mixed = !V.all_double;
  HIP_TRY(hipMemsetAsync(coff, 0, sizeof(int64_t) * (M + 1), st));
  if (M > 0) {
    hipLaunchKernelGGL(k_raw_cand_count, dim3(blocks_for(M, 256)), dim3(256), 0,
                       st, P, V, M, b->group_members, ccount);
    hipLaunchKernelGGL(k_scan, dim3(1), dim3(1024), 0, st, M,
                       (const int64_t*)ccount, coff);
  }
  HIP_TRY(hipMemcpyAsync(&c->h_small[2], coff + M, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  const int64_t C = c->h_small[2];
  if (C >= (int64_t(1) << 32))
    return fail(OTSDB_E_UNSUPPORTED, "raw group-by over %lld candidate points",
                (long long)C);
  // ---- phase 2 workspace: candidates, sort temp, emitted-point groups
  // keys (ts << 16) | occurrence (raw.hip); candidates have ts <= end_ms
  if (spec->end_ms >= kRawTsMax)
    return fail(OTSDB_E_UNSUPPORTED, "raw group-by past 2^47 ms");
  const int end_bit = kOccBits + std::max(1, 64 - __builtin_clzll((uint64_t)std::max<int64_t>(spec->end_ms, 1)));
  size_t sort_tmp = 0;
  if (C > 0)
    HIP_TRY(rocprim::segmented_radix_sort_keys(
        nullptr, sort_tmp, (const uint64_t*)nullptr, (uint64_t*)nullptr,
        (unsigned)C, (unsigned)G, segb, sege, 0, end_bit, st));
  uint64_t *kin, *kout;
  void* tmp;
  int32_t *ugrp, *uocc;
  auto carve2 = [&](char* base) {
    Carve cv{base};
    kin = cv.take<uint64_t>(C + 1);
    kout = cv.take<uint64_t>(C + 1);
    ugrp = cv.take<int32_t>(C + 1);
    uocc = cv.take<int32_t>(C + 1);
    tmp = cv.take<char>(sort_tmp + 1);
    return cv.off + 256;
  };
  rc = c->ws2.ensure(carve2(nullptr));
  if (rc) return rc;
  carve2((char*)c->ws2.p);
  if (M > 0)
    hipLaunchKernelGGL(k_raw_cand_fill, dim3(blocks_for(M, 4)), dim3(256), 0,
                       st, P, V, M, b->group_members, (const int64_t*)coff, kin,
                       c->d_err);
  hipLaunchKernelGGL(k_raw_segments, dim3(blocks_for(G, 256)), dim3(256), 0, st,
                     G, b->group_offsets, (const int64_t*)coff, segb, sege);
  if (C > 0)
    HIP_TRY(rocprim::segmented_radix_sort_keys(
        tmp, sort_tmp, (const uint64_t*)kin, kout, (unsigned)C, (unsigned)G,
        segb, sege, 0, end_bit, st));
  hipLaunchKernelGGL(k_raw_unique, dim3(blocks_for(G, 4)), dim3(256), 0, st, G,
                     (const int64_t*)segb, (const int64_t*)sege,
                     (const uint64_t*)kout, counts, (const int64_t*)nullptr,
                     (int64_t)0, (int64_t*)nullptr, (int32_t*)nullptr,
                     (int32_t*)nullptr, 0);
  hipLaunchKernelGGL(k_scan, dim3(1), dim3(1024), 0, st, G,
                     (const int64_t*)counts, out->offsets);
  hipLaunchKernelGGL(k_raw_unique, dim3(blocks_for(G, 4)), dim3(256), 0, st, G,
                     (const int64_t*)segb, (const int64_t*)sege,
                     (const uint64_t*)kout, counts,
                     (const int64_t*)out->offsets, out->capacity, out->ts, ugrp,
                     uocc, 1);
  HIP_TRY(hipMemcpyAsync(&c->h_small[2], out->offsets + G, 8,
                         hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  const int64_t n_out = std::min<int64_t>(c->h_small[2], out->capacity);
  if (n_out > 0) {
    if (is_selection(spec->agg_id)) {
      const int median = spec->agg_id == OTSDB_AGG_MEDIAN ? 1 : 0;
      // keys slab: one kmax-key row per block, at most 64 Mi keys per launch
      const int64_t per = std::max<int64_t>(
          1, std::min<int64_t>(n_out, ((int64_t)1 << 26) / std::max<int64_t>(kmax, 1)));
      rc = c->dec_ws.ensure((size_t)(per * std::max<int64_t>(kmax, 1)) * 8);
      if (rc) return rc;
      for (int64_t u0 = 0; u0 < n_out; u0 += per) {
        const int64_t nb = std::min(per, n_out - u0);
        hipLaunchKernelGGL(k_raw_select, dim3((unsigned)nb), dim3(64), 0, st, P,
                           V, median, u0, n_out, b->group_offsets,
                           b->group_members, (const int32_t*)ugrp,
                           (const int32_t*)uocc, (const int64_t*)out->ts,
                           out->val, out->is_int,
                           (uint64_t*)c->dec_ws.p, std::max<int64_t>(kmax, 1),
                           c->d_err);
      }
    } else {
      const bool ok = with_monoid(spec->agg_id, [&](auto tag) {
        using Mo = decltype(tag);
        hipLaunchKernelGGL(k_raw_eval<Mo>, dim3(blocks_for(n_out, 256)),
                           dim3(256), 0, st, P, V, (int)spec->agg_id, mixed,
                           n_out, b->group_offsets, b->group_members,
                           (const int32_t*)ugrp, (const int32_t*)uocc,
                           (const int64_t*)out->ts, out->val, out->is_int,
                           c->d_err);
      });
      if (!ok) return fail(OTSDB_E_NO_SUCH_ELEMENT, "aggregator %d", spec->agg_id);
    }
  }
  HIP_TRY(hipGetLastError());
  return finish(c, G, out);
}

// FillingDownsampler over per-series grids (calendar.hip, stage A'): the
// points whose own bucket starts on the filling grid, compacted, then the
// filling calendar pipeline over that grid.
otsdb_status run_anchored_fill(otsdb_ctx* c, const AnchoredPlan& A,
                               const otsdb_batch* b, int64_t* vts,
                               const AnchoredCal& AC,
                               const std::vector<void*>& pp, otsdb_result* out,
                               std::vector<int64_t>& goff) {
  hipStream_t st = c->stream;
  const otsdb_query_spec* spec = &A.derived;
  const int64_t S = b->n_series;
  int64_t Np = 0;
  if (S > 0) {
    HIP_TRY(hipMemcpyAsync(&Np, b->offsets + S, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
  }
  const int64_t nfd = (int64_t)A.FD.size();
  const size_t tmpb = scan_tmp_bytes(S, st);
  // (upper bound of the compacted copy: every point + 2 per series)
  const int64_t Nc = Np + 2 * S;
  auto carve = [&](char* base) {
    Carve cv{base};
    void* p[7];
    p[0] = cv.take<int64_t>(nfd);
    p[1] = cv.take<uint8_t>(std::max<int64_t>(Np, 1));
    p[2] = cv.take<int64_t>(S + 1);
    p[3] = cv.take<int64_t>(S + 1);
    p[4] = cv.take<int64_t>(std::max<int64_t>(Nc, 2));
    p[5] = cv.take<int64_t>(std::max<int64_t>(Nc, 2));
    p[6] = cv.take<uint8_t>(std::max<int64_t>(Nc, 1));
    void* t = cv.take<char>(tmpb);
    return std::make_pair(cv.off + 256, std::vector<void*>{p[0], p[1], p[2], p[3],
                                                          p[4], p[5], p[6], t});
  };
  otsdb_status rc = c->acal_fill.ensure(carve(nullptr).first);
  if (rc) return rc;
  auto q = carve((char*)c->acal_fill.p).second;
  int64_t* fd = (int64_t*)q[0];
  uint8_t* on = (uint8_t*)q[1];
  int64_t* cnt = (int64_t*)q[2];
  int64_t* offs = (int64_t*)q[3];
  int64_t* ts2 = (int64_t*)q[4];
  int64_t* val2 = (int64_t*)q[5];
  uint8_t* isf2 = b->is_float ? (uint8_t*)q[6] : nullptr;
  HIP_TRY(hipMemcpyAsync(fd, A.FD.data(), 8 * nfd, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemsetAsync(cnt + S, 0, 8, st));
  const BatchDev B = batch_dev(b);
  if (S > 0) {
    hipLaunchKernelGGL(k_cal_fill_count, dim3(blocks_for(S, 4)), dim3(256), 0,
                       st, spec->start_ms, spec->end_ms, B, AC,
                       (const int64_t*)pp[4], (const int64_t*)pp[5],
                       (const int64_t*)pp[6], fd, nfd, vts, on, cnt, c->d_err);
    rc = scan_excl(q[7], tmpb, cnt, offs, S, st);
    if (rc) return rc;
    hipLaunchKernelGGL(k_cal_fill_write, dim3(blocks_for(S, 4)), dim3(256), 0,
                       st, spec->start_ms, A.t_end, B, (const int64_t*)vts, on,
                       (const int64_t*)offs, ts2, val2, isf2);
    HIP_TRY(hipGetLastError());
    int e;
    if ((rc = read_err(c, &e))) return rc;
    if (e & ERR_CAL_RANGE)
      return fail(OTSDB_E_UNSUPPORTED,
                  "a point lies before its series' calendar chain");
  }
  otsdb_batch vb = *b;
  vb.n_points = 0;
  if (S > 0) {
    HIP_TRY(hipMemcpyAsync(&vb.n_points, offs + S, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
  }
  vb.offsets = offs;
  vb.ts_ms = ts2;
  vb.val = val2;
  vb.is_float = isf2;
  return run_device_impl(c, spec, &vb, out, goff);
}

// Per-series calendar grids: stage A rewrites the timestamps to the series'
// own bucket starts (calendar.hip), stage B runs the calendar pipeline over
// the union grid.
otsdb_status run_anchored(otsdb_ctx* c, const otsdb_query_spec* spec,
                          const otsdb_batch* b, otsdb_result* out,
                          std::vector<int64_t>& goff) {
  AnchoredPlan A;
  otsdb_status rc = plan_anchored(spec, &A);
  if (rc) return rc;
  hipStream_t st = c->stream;
  const int64_t S = b->n_series, n = spec->n_cal_edges,
                na = spec->n_cal_anchors;
  int64_t N = 0;
  if (S > 0) {
    HIP_TRY(hipMemcpyAsync(&N, b->offsets + S, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
  }
  auto carve = [&](char* base) {
    Carve cv{base};
    void* p[8];
    p[0] = cv.take<int64_t>(n);
    p[1] = cv.take<int64_t>(na);
    p[2] = cv.take<int64_t>(na);
    p[3] = cv.take<int64_t>(na);
    p[4] = cv.take<int64_t>(S + 1);
    p[5] = cv.take<int64_t>(S + 1);
    p[6] = cv.take<int64_t>(S + 1);
    p[7] = cv.take<int64_t>(std::max<int64_t>(N, 2));
    return std::make_pair(cv.off + 256, std::vector<void*>(p, p + 8));
  };
  rc = c->acal.ensure(carve(nullptr).first);
  if (rc) return rc;
  auto pp = carve((char*)c->acal.p).second;
  HIP_TRY(hipMemcpyAsync(pp[0], spec->cal_edges, 8 * n, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(pp[1], spec->cal_anchors, 8 * na, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(pp[2], spec->cal_anchor_edge, 8 * na,
                         hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(pp[3], A.chain_end.data(), 8 * na,
                         hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemsetAsync(c->d_err, 0, sizeof(int), st));
  AnchoredCal AC{(const int64_t*)pp[0], (const int64_t*)pp[1],
                 (const int64_t*)pp[2], (const int64_t*)pp[3], na};
  const BatchDev B = batch_dev(b);
  int64_t* vts = (int64_t*)pp[7];
  if (S > 0) {
    hipLaunchKernelGGL(k_cal_anchor, dim3(blocks_for(S, 256)), dim3(256), 0,
                       st, spec->start_ms, spec->end_ms, A.seek_ts, B, AC,
                       (int64_t*)pp[4], (int64_t*)pp[5], (int64_t*)pp[6],
                       c->d_err);
    if (A.FD.empty())
      hipLaunchKernelGGL(k_cal_vts, dim3(blocks_for(S, 4)), dim3(256), 0, st,
                         spec->start_ms, A.stop_b, (int)spec->rate, B, AC,
                         (const int64_t*)pp[4], (const int64_t*)pp[5],
                         (const int64_t*)pp[6], vts, c->d_err);
    HIP_TRY(hipGetLastError());
    int e;
    if ((rc = read_err(c, &e))) return rc;
    if (e & ERR_CAL_RANGE)
      return fail(OTSDB_E_UNSUPPORTED,
                  "a point lies outside its series' calendar chain");
  }
  otsdb_batch vb = *b;
  vb.ts_ms = vts;
  if (!A.FD.empty()) return run_anchored_fill(c, A, b, vts, AC, pp, out, goff);
  return run_device_impl(c, &A.derived, &vb, out, goff);
}

// the context's rollup state for one call, cleared on every exit path
struct RollupScope {
  otsdb_ctx* c;
  RollupScope(otsdb_ctx* c_, RollupKind kind, const int64_t* cnt) : c(c_) {
    c->rollup = kind;
    c->rollup_cnt = kind == ROLLUP_AVG ? cnt : nullptr;
  }
  ~RollupScope() {
    c->rollup = ROLLUP_NONE;
    c->rollup_cnt = nullptr;
  }
};

// ----------------------------------- multi-aggregator and panel queries
// otsdb_agg_run_multi*: n outputs that differ in the cross-series aggregator
// (and its interpolation) over one query.  DESIGN.md §4.
// otsdb_agg_run_panel*: they differ in the downsampling function as well
// (ds set).  DESIGN.md §4.2.
otsdb_query_spec req_spec(const otsdb_query_spec* s, const Req& q, int i) {
  otsdb_query_spec r = *s;
  if (q.ds) r.ds_agg_id = q.ds[i];
  r.agg_id = q.aggs[i];
  r.interp = q.interps ? q.interps[i] : OTSDB_INTERP_DEFAULT;
  return r;
}

// panel: the entry takes downsampling functions (a null q.ds is its error)
otsdb_status check_req(const otsdb_query_spec* spec, const Req& q,
                       bool panel = false) {
  if (q.n < 1 || q.n > OTSDB_MULTI_MAX)
    return fail(OTSDB_E_ILLEGAL_ARGUMENT, "n_out %d outside [1, %d]", (int)q.n,
                OTSDB_MULTI_MAX);
  if (panel && (!q.ds || !q.aggs))
    return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null ds_agg_ids / agg_ids");
  if (!q.aggs) return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null agg_ids");
  const bool ds = spec->ds_interval_ms > 0 || spec->run_all;
  for (int i = 0; i < q.n; ++i) {
    // (raw group-by has no downsampler: the functions are ignored)
    if (q.ds && ds && (q.ds[i] < 0 || q.ds[i] >= OTSDB_AGG_COUNT_IDS))
      return fail(OTSDB_E_NO_SUCH_ELEMENT, "No such downsampling function: %d",
                  q.ds[i]);
    const otsdb_query_spec si = req_spec(spec, q, i);
    const otsdb_status rc = check_spec(&si);
    if (rc) return rc;
  }
  return OTSDB_OK;
}

enum { MK_SCALAR = 0, MK_ORDERED = 1, MK_SELECT = 2 };

int multi_kind(int agg) {
  if (is_selection(agg)) return MK_SELECT;
  bool ordered = false;
  with_monoid(agg, [&](auto tag) { ordered = decltype(tag)::kOrdered; });
  return ordered ? MK_ORDERED : MK_SCALAR;
}

// The interpolation classes of the outputs: k_transform bakes P.interp into
// the rows only for NONE fill without rate (its interpolation branch); the
// fill branch and transform_rate never read it, so such queries have one
// class.  cls[i]: class of output i; interp[k]: class k's interpolation.
int multi_classes(const Req& q, const Params& P, int* cls, int* interp) {
  const bool baked = !(P.fill != 0 && !P.run_all) && !P.rate;
  int n = 0;
  for (int i = 0; i < q.n; ++i) {
    const int m = !baked ? 0
                  : (q.interps && q.interps[i] >= 0) ? q.interps[i]
                                                     : kAggs[q.aggs[i]].interp;
    int k = 0;
    while (k < n && interp[k] != m) ++k;
    if (k == n) interp[n++] = m;
    cls[i] = k;
  }
  return n;
}

// Whether the outputs can share one row matrix.  Not: raw group-by,
// per-series calendar anchors, nothing to aggregate, a grid the single path
// would first trim to the data (past 4e9 cells), dev past the row budget
// (with the pristine rows kept beside a class matrix: twice the rows).  Such
// calls run their outputs one after another through the single-query path.
// A panel call asks per downsampling function (panel_shared): a function may
// have one output (min_n = 1), and the cell and row budgets hold for the
// `mats` row matrices of the call together.
bool multi_shares_rows(const otsdb_query_spec* spec, const Req& q,
                       const Params& P, int64_t S,
                       const std::vector<int64_t>& goff, int min_n = 2,
                       int mats = 1) {
  if (q.n < min_n) return false;
  if (!(spec->ds_interval_ms > 0 || spec->run_all) || anchored(spec))
    return false;
  const int64_t G = (int64_t)goff.size() - 1;
  if (S <= 0 || G <= 0 || P.nb <= 0 || goff.back() <= 0) return false;
  if (P.nb > (int64_t)INT32_MAX - 2) return false;
  const double rows = (double)S * (double)P.nb * (double)mats;
  if (rows > 4.0e9) return false;
  int cls[OTSDB_MULTI_MAX], ci[OTSDB_MULTI_MAX];
  const int n_cls = multi_classes(q, P, cls, ci);
  bool dev = false;
  for (int i = 0; i < q.n; ++i) dev |= multi_kind(q.aggs[i]) == MK_ORDERED;
  if (dev) {
    int64_t kmax = 0;
    for (int64_t g = 0; g < G; ++g) kmax = std::max(kmax, goff[g + 1] - goff[g]);
    if (kmax > kOrderedFoldChunk &&
        rows * 9.0 * (n_cls > 1 ? 2.0 : 1.0) > kOrderedRowBudget)
      return false;
  }
  return true;
}

struct MultiState {
  const otsdb_query_spec* spec;
  Req q;
  BatchDev B;
  const int64_t* d_members;
  std::vector<int64_t>* goff;
  Params P;
  Work W;   // W.R: the downsampler's rows; W.out_*: the selections' counts
  Rows R2;  // one interpolation class's matrix (several classes only)
  int64_t S, G, NB;
  int cls[OTSDB_MULTI_MAX], cls_interp[OTSDB_MULTI_MAX], n_cls;
  int kind[OTSDB_MULTI_MAX];
  double* out_val[OTSDB_MULTI_MAX];
  uint8_t* out_emit[OTSDB_MULTI_MAX];
  Packed* partial[kMultiSlots];
  bool rate_fused, sel_fused, two_level, two_level_dev, exact, empty_group;
  // tiles of the scalar outputs and the selections' count pass: the ones the
  // single query reduces over, so that each output has its bits — the
  // ordered fold's (groups up to kFoldChunk whole, larger ones in tiles of
  // kFoldChunkLarge, merged in order) where the single query folds, else
  // the row path's kChunk.  (The selections only count over them: groups
  // of up to SEL_K = kFoldChunk members are one tile either way.)
  int64_t chunk, whole;
};

// multi_build as one downsampling function of a panel call (panel_shared):
// the function's buffers are carved at ws_off of a workspace the panel call
// sizes (size_only: the sizing pass) and clears; the call builds the rows of
// all its functions itself, in one pass.
struct PanelPart {
  size_t ws_off;
  size_t ws_need;  // out: bytes of this function's carve
  bool size_only;
};

otsdb_status multi_buffers(otsdb_ctx* c) {
  if (c->d_merr) return OTSDB_OK;
  HIP_TRY(hipMalloc(&c->d_merr, OTSDB_MULTI_MAX * sizeof(int)));
  HIP_TRY(hipHostMalloc(&c->h_mdone, OTSDB_MULTI_MAX * 4 * sizeof(int64_t),
                        hipHostMallocMapped | hipHostMallocCoherent));
  HIP_TRY(hipHostGetDevicePointer((void**)&c->d_mdone, c->h_mdone, 0));
  for (int i = 0; i < OTSDB_MULTI_MAX * 4; ++i) c->h_mdone[i] = 0;
  return OTSDB_OK;
}

// "Build the rows" once for every output: the tiles, the workspace of the
// whole call and the downsample pass (fold off: the rows are what is
// shared).  cells: as run_pipeline's.  partial: the call leaves partials for
// the merge across ranks (multi_partials) — dev's chains are those of the
// single partials entry (kOrderedChunkMerged), its merge covers every group.
otsdb_status multi_build(otsdb_ctx* c, const otsdb_query_spec* spec,
                         const Req& q, const BatchDev& B,
                         const int64_t* d_members, std::vector<int64_t>& goff,
                         const Params& P0, const CellsDev* cells,
                         const int64_t* series_row, MultiState& M,
                         bool partial = false, PanelPart* part = nullptr) {
  hipStream_t st = c->stream;
  otsdb_status rc = multi_buffers(c);
  if (rc) return rc;
  M.spec = spec;
  M.q = q;
  M.B = B;
  M.d_members = d_members;
  M.goff = &goff;
  M.P = P0;
  Params& P = M.P;
  const int64_t S = M.S = B.S;
  const int64_t G = M.G = (int64_t)goff.size() - 1;
  const int64_t NB = M.NB = P.nb;
  P.fold_wb = 0;
  P.fold_ctx = 0;
  P.sentinel = !cells && !P.ds_sel;
  M.rate_fused = P.sentinel && P.rate && !P.fill && !P.run_all;
  M.exact = (spec->flags & OTSDB_SPEC_EXACT_ORDER) != 0;
  M.n_cls = multi_classes(q, P, M.cls, M.cls_interp);
  uint32_t mask = 0;
  bool any_sel = false, all_sel = true;
  for (int i = 0; i < q.n; ++i) {
    M.kind[i] = multi_kind(q.aggs[i]);
    any_sel |= M.kind[i] == MK_SELECT;
    all_sel &= M.kind[i] == MK_SELECT;
    if (M.kind[i] == MK_SCALAR)
      with_monoid(q.aggs[i], [&](auto tag) {
        constexpr int k = MultiSlot<decltype(tag)>::value;
        if (k >= 0) mask |= 1u << (k & 31);
      });
  }
  const bool folds = !P.ds_sel && !P.rate && !P.run_all &&
                     !(cells && !P.narrow) && kFoldChunk >= (int64_t)SEL_K;
  M.chunk = folds ? kFoldChunkLarge : kChunk;
  M.whole = folds ? kFoldChunk : 0;
  rc = build_tiles(c, goff, false, M.chunk, M.whole);
  if (rc) return rc;
  const Tiles T = tiles_of(c, G);
  M.sel_fused = all_sel && sel_fused_path(q.aggs[0], 0, P, T, G);
  const bool sel_large = any_sel && T.LG > 0;
  M.two_level = two_level_combine(T.max_chunks, T.MG, NB);
  // dev's own tiles (one chain per group up to kOrderedChunk members): how
  // many groups its merge covers, and its longest
  int64_t mg_dev = 0, max_dev = 0;
  const int64_t whole = partial ? kOrderedChunkMerged
                                : (M.exact ? INT64_MAX : kOrderedChunk);
  M.empty_group = false;
  for (int64_t g = 0; g < G; ++g) {
    const int64_t k = goff[g + 1] - goff[g];
    M.empty_group |= k == 0;
    if (k > whole) {
      ++mg_dev;
      max_dev = std::max(max_dev, (k + kChunk - 1) / kChunk);
    }
  }
  if (partial) mg_dev = G;  // k_combine packs every group's state
  M.two_level_dev = two_level_combine(max_dev, mg_dev, NB);
  const int64_t n_comb = std::max(M.two_level ? T.MG : 0,
                                  M.two_level_dev ? mg_dev : 0);
  const size_t rows = (size_t)S * NB;
  Work& W = M.W;
  auto carve = [&](char* base) {
    Carve cv{base};
    carve_series(cv, W, S);
    W.R.val = cv.take<double>(rows);
    W.R.state = cv.take<uint8_t>(rows);
    M.R2 = Rows{nullptr, nullptr};
    if (M.n_cls > 1) {
      M.R2.val = cv.take<double>(rows);
      M.R2.state = cv.take<uint8_t>(rows);
    }
    // one partial slot per requested monoid (slot 0 always: the selections'
    // count pass and dev borrow it between launches)
    for (int k = 0; k < kMultiSlots; ++k)
      M.partial[k] = (k == 0 || (mask >> k & 1))
                         ? cv.take<Packed>((size_t)T.T * NB)
                         : nullptr;
    W.partial = M.partial[0];
    W.tile_emit = cv.take<uint8_t>((size_t)T.T * NB);
    W.out_val = cv.take<double>((size_t)G * NB);
    W.out_emit = cv.take<uint8_t>((size_t)G * NB);
    for (int i = 0; i < q.n; ++i) {
      M.out_val[i] = partial ? nullptr : cv.take<double>((size_t)G * NB);
      M.out_emit[i] = partial ? nullptr : cv.take<uint8_t>((size_t)G * NB);
    }
    W.counts = nullptr;
    if (n_comb > 0) carve_combine(cv, W, n_comb, NB);
    if (sel_large) carve_selection(cv, W, goff.back(), T.LG, NB, false);
    return cv.off + 256;
  };
  if (part) {
    part->ws_need = carve(nullptr);
    if (part->size_only) return OTSDB_OK;
    carve((char*)c->ws.p + part->ws_off);
  } else {
    rc = c->ws.ensure(carve(nullptr));
    if (rc) return rc;
    carve((char*)c->ws.p);

    // every output its own error word; the shared stages report into the
    // context's (folded into every output's status at the end)
    HIP_TRY(hipMemsetAsync(c->d_err, 0, 2 * sizeof(int), st));
    HIP_TRY(hipMemsetAsync(c->d_merr, 0, OTSDB_MULTI_MAX * sizeof(int), st));
    c->clean_entry = false;
  }
  if (M.empty_group && !partial) {
    HIP_TRY(hipMemsetAsync(W.out_emit, 0, (size_t)G * NB, st));
    for (int i = 0; i < q.n; ++i)
      HIP_TRY(hipMemsetAsync(M.out_emit[i], 0, (size_t)G * NB, st));
  }
  if (!P.sentinel) HIP_TRY(hipMemsetAsync(W.R.state, 0, rows, st));
  if (part) return OTSDB_OK;  // (the panel call's one pass builds the rows)
  multi_counters(c, 0, 0);
  rc = build_rows(c, spec, P, B, W, cells, series_row, M.rate_fused);
  if (rc) return rc;
  ++c->n_multi_ds;
  HIP_TRY(hipGetLastError());
  return OTSDB_OK;
}

// Wc: the work set over interpolation class k's matrix — k_transform in
// place for one class, k_transform_interp into the second matrix for several
otsdb_status multi_class_rows(otsdb_ctx* c, MultiState& M, int k, Work& Wc) {
  const int64_t NB = M.NB, S = M.S;
  Params& P = M.P;
  Wc = M.W;
  if (M.n_cls == 1) {
    P.interp = M.cls_interp[0];
    transform_rows(c, P, M.B, M.W, M.rate_fused);
  } else {
    StageTimer tm(c, 1);
    Params Pc = P;
    Pc.interp = M.cls_interp[k];
    if (!P.sentinel)
      HIP_TRY(hipMemsetAsync(M.R2.state, 0, (size_t)S * NB, c->stream));
    hipLaunchKernelGGL(k_transform_interp, dim3(blocks_for(S, 4)), dim3(256),
                       0, c->stream, Pc, M.B, M.W.SM, M.W.R, M.R2);
    Wc.R = M.R2;
  }
  ++c->n_multi_tf;
  return OTSDB_OK;
}

// k_group_multi's request for the scalar, unordered outputs of class k:
// slots, mask and tile partials (MA.out[j] is the caller's); who[j]: the
// output behind launch output j
void multi_scalar_args(const MultiState& M, int k, MultiArgs& MA, int* who) {
  const Req& q = M.q;
  for (int i = 0; i < q.n; ++i) {
    if (M.cls[i] != k || M.kind[i] != MK_SCALAR) continue;
    const int j = MA.n_out++;
    who[j] = i;
    with_monoid(q.aggs[i], [&](auto tag) {
      MA.slot[j] = MultiSlot<decltype(tag)>::value;
    });
    MA.mask |= 1u << (MA.slot[j] & 31);
  }
  for (int s = 0; s < kMultiSlots; ++s) MA.partial[s] = M.partial[s];
}

// Every output through the existing compaction into its own result, one
// synchronisation, the status of the lowest-index failing output.
otsdb_status multi_compact_launch(otsdb_ctx* c, const Req& q,
                                  const Params& P, int64_t G,
                                  double* const* out_val,
                                  uint8_t* const* out_emit) {
  for (int i = 0; i < q.n; ++i) {
    Params Pi = P;
    agg_params(&Pi, q.aggs[i], q.interps ? q.interps[i] : OTSDB_INTERP_DEFAULT);
    const otsdb_status rc =
        compact(c, Pi, G, out_val[i], out_emit[i], nullptr, &q.outs[i],
                c->d_merr + q.e0 + i, c->d_mdone + 4 * (q.e0 + i));
    if (rc) return rc;
  }
  return OTSDB_OK;
}

// The one synchronisation and the statuses of the compacted outputs.  orig:
// the caller's index of each output (a panel call runs them grouped by
// function); the lowest of those decides.
otsdb_status multi_compact_wait(otsdb_ctx* c, const Req& q,
                                const int* orig = nullptr) {
  // (the next call of any kind clears the context's word itself: err_clean
  // stays false, as after a single query that did not end in k_compact1)
  c->small_ready = false;
  c->h_small[0] = 0;
  int shared;
  const otsdb_status rs = read_err(c, &shared);
  if (rs) return rs;
  int failed = -1;
  otsdb_status failed_rc = OTSDB_OK;
  std::string failed_msg;
  for (int j = 0; j < q.n; ++j) {
    const int i = orig ? orig[j] : j;
    int64_t* d = c->h_mdone + 4 * (q.e0 + j);
    int e = shared | (int)(__atomic_load_n(&d[0], __ATOMIC_ACQUIRE) & 0xFFFFFFFF);
    c->multi_total[i] = __atomic_load_n(&d[1], __ATOMIC_ACQUIRE);
    if (__atomic_load_n(&d[2], __ATOMIC_ACQUIRE)) {
      d[2] = 0;
      e |= ERR_INTERNAL;
    }
    const otsdb_status rc =
        result_status(e, c->multi_total[i], q.outs[j].capacity);
    if (rc && (failed < 0 || i < failed)) {
      failed = i;
      failed_rc = rc;
      failed_msg = g_last_error;
    }
    if (rc && !orig) break;
  }
  if (failed < 0) return OTSDB_OK;
  c->multi_failed = failed;
  if (failed_rc == OTSDB_E_CAPACITY) c->result_short = true;
  g_last_error = failed_msg;
  return failed_rc;
}

otsdb_status multi_compact_outputs(otsdb_ctx* c, const Req& q,
                                   const Params& P, int64_t G,
                                   double* const* out_val,
                                   uint8_t* const* out_emit) {
  const otsdb_status rc = multi_compact_launch(c, q, P, G, out_val, out_emit);
  if (rc) return rc;
  return multi_compact_wait(c, q);
}

// "Aggregate the rows" per interpolation class and output, compact every
// output into its result, synchronise once and report the status of the
// lowest-index failing output.
otsdb_status multi_aggregate(otsdb_ctx* c, MultiState& M,
                             bool compact_now = true) {
  hipStream_t st = c->stream;
  const Req& q = M.q;
  int* const merr = c->d_merr + q.e0;  // this request's error words
  const int64_t G = M.G, NB = M.NB, S = M.S;
  Params& P = M.P;
  otsdb_status rc;
  auto stage = [&](const Tiles& T, bool two_level) {
    return AggStage{M.d_members, M.goff->back(), 0,       false, two_level,
                    nullptr,     nullptr,        nullptr, nullptr};
  };
  auto sel_of = [&](int i, int* median, double* pct) {
    *median = q.aggs[i] == OTSDB_AGG_MEDIAN ? 1 : 0;
    *pct = q.aggs[i] >= OTSDB_AGG_P999 ? pct_of(q.aggs[i]) : 0.0;
  };
  if (M.sel_fused) {
    // every output a selection over a filling grid of large groups: the one
    // transpose applies the fill and counts, then one select per output
    StageTimer tm(c, 2);
    const Tiles T = tiles_of(c, G);
    const AggStage A = stage(T, M.two_level);
    rc = sel_fused_keys(c, P, M.W, T, NB, A);
    if (rc) return rc;
    ++c->n_multi_kt;
    for (int i = 0; i < q.n; ++i) {
      int median;
      double pct;
      sel_of(i, &median, &pct);
      sel_fused_select(c, M.W, T, NB, A, median, pct, M.out_val[i],
                       M.out_emit[i], merr + i);
      ++c->n_multi_group;
    }
  }
  for (int k = 0; k < M.n_cls && !M.sel_fused; ++k) {
    Work Wc;  // this class's matrix
    rc = multi_class_rows(c, M, k, Wc);
    if (rc) return rc;
    StageTimer tm(c, 2);
    rc = build_tiles(c, *M.goff, false, M.chunk, M.whole);  // (cached unless dev ran)
    if (rc) return rc;
    const Tiles T = tiles_of(c, G);
    const AggStage A = stage(T, M.two_level);
    // ---- the scalar, unordered outputs: one pass for all of them
    MultiArgs MA{};
    int who[OTSDB_MULTI_MAX];
    multi_scalar_args(M, k, MA, who);
    for (int j = 0; j < MA.n_out; ++j)
      MA.out[j] = MultiOut{M.out_val[who[j]], M.out_emit[who[j]],
                           merr + who[j], nullptr};
    if (MA.n_out > 0 && T.T > 0) {
      hipLaunchKernelGGL(k_group_multi<false>, dim3(blocks_for(T.T * NB, 256)),
                         dim3(256), 0, st, NB, T.T, T.tg, T.tm0, T.tm1,
                         T.single, M.d_members, Wc.R, M.W.tile_emit, MA);
      ++c->n_multi_group;
      if (T.MG > 0)
        for (int j = 0; j < MA.n_out; ++j) {
          const int i = who[j];
          Work Ws = Wc;
          Ws.partial = M.partial[MA.slot[j]];
          with_monoid(q.aggs[i], [&](auto tag) {
            launch_combine<decltype(tag)>(c, Ws, NB, T.MG, T.mg, T.mt0, T.mt1,
                                          M.out_val[i], M.out_emit[i], nullptr,
                                          M.two_level, 0, merr + i);
          });
        }
    }
    // ---- the selections: one count pass and one key transpose, then a
    // select per output over the shared, read-only keys
    bool counted = false;
    for (int i = 0; i < q.n; ++i) {
      if (M.cls[i] != k || M.kind[i] != MK_SELECT) continue;
      if (!counted) {
        sel_counts(c, Wc, T, NB, A, c->d_err);
        ++c->n_multi_group;
        if (T.LG > 0) {
          sel_keys(c, Wc, NB, A);
          ++c->n_multi_kt;
        }
        counted = true;
      }
      HIP_TRY(hipMemcpyAsync(M.out_val[i], Wc.out_val, (size_t)G * NB * 8,
                             hipMemcpyDeviceToDevice, st));
      HIP_TRY(hipMemcpyAsync(M.out_emit[i], Wc.out_emit, (size_t)G * NB,
                             hipMemcpyDeviceToDevice, st));
      Work Wo = Wc;
      Wo.out_val = M.out_val[i];
      Wo.out_emit = M.out_emit[i];
      int median;
      double pct;
      sel_of(i, &median, &pct);
      sel_finish(c, Wo, T, NB, A, median, pct, /*transpose=*/false,
                 merr + i);
      ++c->n_multi_group;
    }
    // ---- the ordered outputs (dev): their own group pass over the tiles
    // the single query's row path builds (one chain per group up to
    // kOrderedChunk members, Chan's merge beyond, EXACT_ORDER honoured)
    bool dev_tiles = false;
    for (int i = 0; i < q.n; ++i) {
      if (M.cls[i] != k || M.kind[i] != MK_ORDERED) continue;
      if (!dev_tiles) {
        rc = build_tiles(c, *M.goff, false, kChunk,
                         M.exact ? INT64_MAX : kOrderedChunk);
        if (rc) return rc;
        dev_tiles = true;
      }
      const Tiles Td = tiles_of(c, G);
      const AggStage Ad = stage(Td, M.two_level_dev);
      Work Wd = Wc;
      Wd.out_val = M.out_val[i];
      Wd.out_emit = M.out_emit[i];
      rc = group_rows(c, q.aggs[i], Wd, Td, NB, G, Ad, merr + i);
      if (rc) return rc;
      ++c->n_multi_group;
    }
  }
  HIP_TRY(hipGetLastError());
  // (a panel call compacts the outputs of all its functions, then waits once)
  if (!compact_now) return OTSDB_OK;
  return multi_compact_outputs(c, q, P, G, M.out_val, M.out_emit);
}

// multi_aggregate's partial-emitting form (otsdb_agg_partials_multi_device):
// output i's per-(group, bucket) states into partials[i][G * NB], one emit
// mask for all outputs.  Scalar outputs: one k_group_multi<PARTIAL> launch
// per class, groups of several tiles through k_combine<M>'s packing form,
// groups without a local member the monoid's identity; dev: k_group<MDev>
// over the single partials entry's tiles, every group through k_combine.
otsdb_status multi_partials(otsdb_ctx* c, MultiState& M, Packed* partials,
                            uint8_t* emit) {
  hipStream_t st = c->stream;
  const Req& q = M.q;
  const int64_t G = M.G, NB = M.NB, GB = G * NB;
  otsdb_status rc;
  for (int k = 0; k < M.n_cls; ++k) {
    Work Wc;
    rc = multi_class_rows(c, M, k, Wc);
    if (rc) return rc;
    StageTimer tm(c, 2);
    rc = build_tiles(c, *M.goff, false, M.chunk, M.whole);  // (cached unless dev ran)
    if (rc) return rc;
    const Tiles T = tiles_of(c, G);
    MultiArgs MA{};
    int who[OTSDB_MULTI_MAX];
    multi_scalar_args(M, k, MA, who);
    for (int j = 0; j < MA.n_out; ++j)
      MA.out[j] = MultiOut{nullptr, emit, c->d_merr + who[j],
                           partials + (size_t)who[j] * GB};
    if (MA.n_out > 0) {
      if (T.T > 0)
        hipLaunchKernelGGL(k_group_multi<true>, dim3(blocks_for(T.T * NB, 256)),
                           dim3(256), 0, st, NB, T.T, T.tg, T.tm0, T.tm1,
                           T.single, M.d_members, Wc.R, M.W.tile_emit, MA);
      ++c->n_multi_group;
      if (T.MG > 0)
        for (int j = 0; j < MA.n_out; ++j) {
          Work Ws = Wc;
          Ws.partial = M.partial[MA.slot[j]];
          with_monoid(q.aggs[who[j]], [&](auto tag) {
            launch_combine<decltype(tag)>(c, Ws, NB, T.MG, T.mg, T.mt0, T.mt1,
                                          nullptr, emit, MA.out[j].part,
                                          M.two_level, 0, c->d_merr + who[j]);
          });
        }
      if (M.empty_group)
        hipLaunchKernelGGL(k_partial_empty_multi, dim3(blocks_for(GB, 256)),
                           dim3(256), 0, st, NB, G, T.at0, T.at1, MA);
    }
    bool dev_tiles = false;
    for (int i = 0; i < q.n; ++i) {
      if (M.cls[i] != k || M.kind[i] != MK_ORDERED) continue;
      if (!dev_tiles) {
        rc = build_tiles(c, *M.goff, false, kChunk, kOrderedChunkMerged);
        if (rc) return rc;
        dev_tiles = true;
      }
      const Tiles Td = tiles_of(c, G);
      const AggStage Ad{M.d_members, M.goff->back(), 1,       false,
                        M.two_level_dev,
                        partials + (size_t)i * GB, emit, nullptr, nullptr};
      rc = group_rows(c, q.aggs[i], Wc, Td, NB, G, Ad, c->d_merr + i);
      if (rc) return rc;
      ++c->n_multi_group;
    }
  }
  HIP_TRY(hipGetLastError());
  return OTSDB_OK;
}

// The outputs one after another through the single-query path (what cannot
// share the rows): the same results, nothing shared.
otsdb_status multi_sequential(otsdb_ctx* c, const otsdb_query_spec* spec,
                              const Req& q, const otsdb_batch* b,
                              std::vector<int64_t>& goff) {
  multi_counters(c, 0, 0);
  for (int i = 0; i < q.n; ++i) {
    const otsdb_query_spec si = req_spec(spec, q, i);
    // the "error word known zero" mark is the last single query's alone
    c->err_clean = false;
    const otsdb_status rc = run_device_impl(c, &si, b, &q.outs[i], goff);
    if (rc) {
      c->multi_failed = i;
      return rc;
    }
    c->multi_total[i] = c->h_small[1];
    ++c->n_multi_ds;
    ++c->n_multi_group;
  }
  return OTSDB_OK;
}

// ---- OTSDB_SPEC_MULTI_FOLD: every output from one ordered fold ------------
// the component of the envelope state (menv.h) an aggregator finishes from,
// -1: not in the envelope set
int fold_multi_kind(int agg) {
  switch (agg) {
    case OTSDB_AGG_SUM:
    case OTSDB_AGG_PFSUM:
    case OTSDB_AGG_ZIMSUM: return FM_SUM;
    case OTSDB_AGG_AVG: return FM_AVG;
    case OTSDB_AGG_COUNT: return FM_CNT;
    case OTSDB_AGG_MIN:
    case OTSDB_AGG_MIMMIN: return FM_MIN;
    case OTSDB_AGG_MAX:
    case OTSDB_AGG_MIMMAX: return FM_MAX;
    default: return -1;
  }
}

// Whether a multi call that can share its rows (multi_shares_rows) takes the
// fold instead: the caller asked for it, the single queries would fold
// (fold_path), every aggregator is a component of the envelope state and all
// outputs contribute through one interpolation class (the fold bakes it into
// the contributions as it pushes them).  bit: the flag that asks — the
// columnar entries' or the cells entry's (OTSDB_SPEC_CELLS_MULTI_FOLD).
bool multi_folds(const otsdb_query_spec* s0, const Req& q, const Params& P,
                 int bit = OTSDB_SPEC_MULTI_FOLD) {
  if (!(s0->flags & bit) || q.n < 2) return false;
  for (int i = 0; i < q.n; ++i) {
    const otsdb_query_spec si = req_spec(s0, q, i);
    if (fold_multi_kind(si.agg_id) < 0 || !fold_path(&si, P, 0)) return false;
  }
  int cls[OTSDB_MULTI_MAX], ci[OTSDB_MULTI_MAX];
  return multi_classes(q, P, cls, ci) == 1;
}

// The folded multi call: k_fold_multi over the single fold's tiles
// (fold_tiling), windows and member contexts (fold_plan over
// fold_wb<MEnv>() buckets) after the single fold's prep (fold_prep), then
// k_combine<M> per output over the tiles of larger groups and the
// compaction of every output.  No row matrix, no transform, no group pass.
// cells / series_row (as run_pipeline's): the members are streamed from
// compacted columns — the cursors sized for THIS state's windows, and
// k_fold_multi's cells variant by cells_fold_variant, as the single cells
// fold chooses k_fold's.  The pass ends with the launches (the
// cells attempt loop reads the error word before anything is compacted);
// multi_fold_finish compacts the outputs.
struct MultiFoldRun {
  Params P;
  int64_t G;
  double* out_val[OTSDB_MULTI_MAX];
  uint8_t* out_emit[OTSDB_MULTI_MAX];
};

otsdb_status multi_fold_pass(otsdb_ctx* c, const otsdb_query_spec* s0,
                             const Req& q, const BatchDev& B,
                             const int64_t* d_members,
                             std::vector<int64_t>& goff, const Params& P0,
                             const CellsDev* cells, const int64_t* series_row,
                             MultiFoldRun& X) {
  hipStream_t st = c->stream;
  otsdb_status rc = multi_buffers(c);
  if (rc) return rc;
  Params& P = X.P;
  P = P0;
  double** const out_val = X.out_val;
  uint8_t** const out_emit = X.out_emit;
  const int64_t S = B.S, NB = P.nb;
  const int64_t G = X.G = (int64_t)goff.size() - 1;
  int cls[OTSDB_MULTI_MAX], ci[OTSDB_MULTI_MAX];
  multi_classes(q, P, cls, ci);
  P.interp = ci[0];
  P.sentinel = 0;
  const FoldTiling ft = fold_tiling(false);
  rc = build_tiles(c, goff, false, ft.chunk, ft.whole_upto);
  if (rc) return rc;
  const Tiles T = tiles_of(c, G);
  const FoldPlan fp = fold_plan(goff, T.T, NB, fold_wb<MEnv>(), false, true);
  const int64_t WB = fp.WB, NW = fp.NW;
  P.fold_wb = fp.fold_wb;
  P.fold_ctx = fp.fold_ctx;
  bool empty_group = false;
  for (int64_t g = 0; g < G && !empty_group; ++g)
    empty_group = goff[g + 1] == goff[g];
  // which partials the tiles of larger groups leave
  FoldMultiArgs FM{};
  FM.n_out = q.n;
  bool need_sn = false, need_mn = false, need_mx = false;
  for (int i = 0; i < q.n; ++i) {
    const int k = FM.kind[i] = fold_multi_kind(q.aggs[i]);
    need_sn |= k == FM_SUM || k == FM_AVG || k == FM_CNT;
    need_mn |= k == FM_MIN;
    need_mx |= k == FM_MAX;
  }
  const bool two_level = two_level_combine(T.max_chunks, T.MG, NB);
  Work W;
  WinCtx* wc = nullptr;
  CellsFold CF{};
  auto carve = [&](char* base) {
    Carve cv{base};
    carve_series(cv, W, S);
    const size_t tp = T.MG > 0 ? (size_t)T.T * NB : 0;
    FM.part_sn = need_sn && tp ? cv.take<Packed>(tp) : nullptr;
    FM.part_mn = need_mn && tp ? cv.take<Packed>(tp) : nullptr;
    FM.part_mx = need_mx && tp ? cv.take<Packed>(tp) : nullptr;
    W.tile_emit = cv.take<uint8_t>((size_t)T.T * NB);
    for (int i = 0; i < q.n; ++i) {
      out_val[i] = cv.take<double>((size_t)G * NB);
      out_emit[i] = cv.take<uint8_t>((size_t)G * NB);
    }
    if (NW > 1) wc = cv.take<WinCtx>((size_t)S * (NW - 1));
    if (cells) carve_cells_fold(cv, CF, c, *cells, series_row, S, NW);
    if (two_level) carve_combine(cv, W, T.MG, NB);
    return cv.off + 256;
  };
  rc = c->ws.ensure(carve(nullptr));
  if (rc) return rc;
  carve((char*)c->ws.p);
  W.R = Rows{nullptr, nullptr};
  W.partial = nullptr;
  W.out_val = nullptr;
  W.out_emit = nullptr;
  W.counts = nullptr;
  // every output its own error word; prep and the fold's watchdog report
  // into the context's (folded into every output's status at the end)
  HIP_TRY(hipMemsetAsync(c->d_err, 0, 2 * sizeof(int), st));
  HIP_TRY(hipMemsetAsync(c->d_merr, 0, OTSDB_MULTI_MAX * sizeof(int), st));
  c->clean_entry = false;
  // the fold / k_combine write every emit flag of a group with members
  if (empty_group && G * NB > 0)
    for (int i = 0; i < q.n; ++i)
      HIP_TRY(hipMemsetAsync(out_emit[i], 0, (size_t)G * NB, st));
  for (int i = 0; i < q.n; ++i)
    FM.out[i] = FoldMultiOut{out_val[i], out_emit[i], c->d_merr + q.e0 + i};
  {
    // (the cells attempts of one call add their fold launches up)
    const int64_t folds = cells ? c->n_multi_fold : 0;
    multi_counters(c, 0, 0);
    c->n_multi_fold = folds;
  }
  // (multi_shares_rows: series, members and buckets exist, so every dense
  // output below is written by the fold or by k_combine)
  if (S > 0 && NB > 0 && T.T > 0) {
    DsLaunch a = ds_args(c, P, B, W);
    fold_args(a, T, d_members, wc, NW, WB, W.tile_emit);
    a.cf = CF;
    a.fm = &FM;
    const bool ok = with_monoid(s0->ds_agg_id, [&](auto tag) {
      using M = decltype(tag);
      fold_prep<M>(c, a, cells != nullptr);
      StageTimer tm(c, 0);
      if (!cells) {
        launch_ds<M>(DS_FOLD_MULTI, a);
      } else if ((a.cells_variant = cells_fold_variant(c)) != 0) {
        launch_cells<M>(DS_CELLS_MULTI, a);
      } else {
        return;  // mixed widths: the attempt loop rewrites the columns
      }
      ++c->n_multi_fold;
    });
    if (!ok) return fail(OTSDB_E_UNSUPPORTED, "downsampler %d", s0->ds_agg_id);
    ++c->n_multi_ds;
    if (T.MG > 0) {
      StageTimer tm(c, 2);
      for (int i = 0; i < q.n; ++i) {
        Work Ws = W;
        Ws.partial = FM.kind[i] == FM_MIN   ? FM.part_mn
                     : FM.kind[i] == FM_MAX ? FM.part_mx
                                            : FM.part_sn;
        with_monoid(q.aggs[i], [&](auto tag) {
          launch_combine<decltype(tag)>(c, Ws, NB, T.MG, T.mg, T.mt0, T.mt1,
                                        out_val[i], out_emit[i], nullptr,
                                        two_level, 0, c->d_merr + q.e0 + i);
        });
      }
    }
  }
  HIP_TRY(hipGetLastError());
  return OTSDB_OK;
}

otsdb_status multi_fold_finish(otsdb_ctx* c, const Req& q,
                               const MultiFoldRun& X) {
  return multi_compact_outputs(c, q, X.P, X.G, X.out_val, X.out_emit);
}

otsdb_status multi_fold(otsdb_ctx* c, const otsdb_query_spec* s0,
                        const Req& q, const BatchDev& B,
                        const int64_t* d_members, std::vector<int64_t>& goff,
                        const Params& P0) {
  MultiFoldRun X;
  const otsdb_status rc = multi_fold_pass(c, s0, q, B, d_members, goff, P0,
                                          nullptr, nullptr, X);
  return rc ? rc : multi_fold_finish(c, q, X);
}

otsdb_status run_multi_impl(otsdb_ctx* c, const otsdb_query_spec* spec,
                            const Req& q, const otsdb_batch* b,
                            std::vector<int64_t>& goff, bool may_fold = true) {
  c->multi_failed = -1;
  c->n_multi_fold = 0;
  if (q.n == 1 || !(spec->ds_interval_ms > 0 || spec->run_all) ||
      anchored(spec))
    return multi_sequential(c, spec, q, b, goff);
  const otsdb_query_spec s0 = req_spec(spec, q, 0);
  Params P;
  otsdb_status rc = make_params(&s0, &P, c);
  if (rc) {
    c->multi_failed = 0;
    return rc;
  }
  // (a misaligned batch: the single path reports it)
  if (misaligned(b) || !multi_shares_rows(spec, q, P, b->n_series, goff))
    return multi_sequential(c, spec, q, b, goff);
  const BatchDev B = batch_dev(b);
  if (may_fold && multi_folds(&s0, q, P))
    return multi_fold(c, &s0, q, B, b->group_members, goff, P);
  MultiState M;
  rc = multi_build(c, &s0, q, B, b->group_members, goff, P, nullptr, nullptr, M);
  if (rc) return rc;
  return multi_aggregate(c, M);
}

// ------------------------------------------------------------ panel queries
// the envelope row of a downsampling function (panel.hip), 0: not in the set
uint32_t panel_fn(int ds) {
  switch (ds) {
    case OTSDB_AGG_SUM:
    case OTSDB_AGG_PFSUM:
    case OTSDB_AGG_ZIMSUM: return PF_SUM;
    case OTSDB_AGG_AVG: return PF_AVG;
    case OTSDB_AGG_COUNT: return PF_CNT;
    case OTSDB_AGG_MIN:
    case OTSDB_AGG_MIMMIN: return PF_MIN;
    case OTSDB_AGG_MAX:
    case OTSDB_AGG_MIMMAX: return PF_MAX;
    default: return 0;
  }
}

// One distinct downsampling function of a panel request and its outputs (in
// the caller's order).  Aliases of one reduction (sum / zimsum / pfsum, min /
// mimmin, max / mimmax) are one function.
struct PanelFunc {
  int ds;        // the id its calls run with
  uint32_t fn;   // envelope row, or 0
  std::vector<int> idx;
  std::vector<int32_t> aggs, interps;
  std::vector<otsdb_result> outs;
  Req req(const Req& q, int e0) {
    return Req{(int32_t)idx.size(), nullptr, aggs.data(),
               q.interps ? interps.data() : nullptr, outs.data(), e0};
  }
};

std::vector<PanelFunc> panel_funcs(const otsdb_query_spec* spec,
                                   const Req& q) {
  const bool ds = spec->ds_interval_ms > 0 || spec->run_all;
  std::vector<PanelFunc> F;
  for (int i = 0; i < q.n; ++i) {
    const int id = ds ? q.ds[i] : spec->ds_agg_id;
    const uint32_t fn = ds ? panel_fn(id) : 0;
    size_t k = 0;
    while (k < F.size() && !(fn ? F[k].fn == fn : (!F[k].fn && F[k].ds == id)))
      ++k;
    if (k == F.size()) {
      F.emplace_back();
      F[k].ds = id;
      F[k].fn = fn;
    }
    F[k].idx.push_back(i);
    F[k].aggs.push_back(q.aggs[i]);
    F[k].interps.push_back(q.interps ? q.interps[i] : OTSDB_INTERP_DEFAULT);
    F[k].outs.push_back(q.outs[i]);
  }
  return F;
}

// what a panel call remembers of its sub-calls: the totals in the caller's
// order and the failing output of the lowest index
struct PanelOutcome {
  int64_t total[OTSDB_MULTI_MAX] = {0};
  int failed = -1;
  otsdb_status rc = OTSDB_OK;
  std::string msg;
  bool result_short = false;
  void fail_at(otsdb_ctx* c, int i, otsdb_status r) {
    if (failed >= 0 && failed <= i) return;
    failed = i;
    rc = r;
    msg = g_last_error;
    result_short = c->result_short;
  }
  // function f's own call (one multi call) returned r: its passes, and its
  // totals or its failing output, both in the caller's order
  void record(otsdb_ctx* c, const PanelFunc& f, otsdb_status r) {
    c->n_panel_passes += c->n_multi_ds;
    c->n_panel_mats += c->n_multi_ds;
    if (r) return fail_at(c, f.idx[(size_t)std::max(c->multi_failed, 0)], r);
    for (size_t j = 0; j < f.idx.size(); ++j)
      total[f.idx[j]] = c->multi_total[j];
  }
  // the call's totals and status into the context
  otsdb_status publish(otsdb_ctx* c, int n) {
    for (int i = 0; i < n; ++i) c->multi_total[i] = total[i];
    if (failed < 0) return OTSDB_OK;
    c->multi_failed = failed;
    c->result_short = result_short;
    g_last_error = msg;
    return rc;
  }
};

// The envelope functions E of a request as one pass: every function's request,
// spec and work set, and the outputs in the order the pass compacts them.
struct PanelPass {
  std::vector<MultiState> MS;
  std::vector<otsdb_query_spec> sp;
  std::vector<Req> qs;
  std::vector<int> orig;
  std::vector<otsdb_result> outs;
  PanelPass(const otsdb_query_spec* spec, const Req& q,
            std::vector<PanelFunc*>& E)
      : MS(E.size()), sp(E.size(), *spec), qs(E.size()) {
    for (size_t d = 0; d < E.size(); ++d) {
      sp[d].ds_agg_id = E[d]->ds;
      qs[d] = E[d]->req(q, (int)orig.size());
      sp[d].agg_id = qs[d].aggs[0];
      for (size_t j = 0; j < E[d]->idx.size(); ++j) {
        orig.push_back(E[d]->idx[j]);
        outs.push_back(E[d]->outs[j]);
      }
    }
  }
};

// every function's buffers carved from one workspace (multi_build: a sizing
// pass, ensure, the carving pass), the error words and the counters cleared
otsdb_status panel_build(otsdb_ctx* c, PanelPass& X, const BatchDev& B,
                         const int64_t* d_members, std::vector<int64_t>& goff,
                         const Params& P, const CellsDev* cells) {
  hipStream_t st = c->stream;
  const int D = (int)X.MS.size();
  otsdb_status rc;
  size_t total = 0;
  for (int pass = 0; pass < 2; ++pass) {
    if (pass == 1) {
      rc = c->ws.ensure(total);
      if (rc) return rc;
    }
    size_t off = 0;
    for (int d = 0; d < D; ++d) {
      PanelPart part{off, 0, pass == 0};
      rc = multi_build(c, &X.sp[d], X.qs[d], B, d_members, goff, P, cells,
                       nullptr, X.MS[d], false, &part);
      if (rc) return rc;
      off += (part.ws_need + 255) & ~(size_t)255;
    }
    total = off;
  }
  HIP_TRY(hipMemsetAsync(c->d_err, 0, 2 * sizeof(int), st));
  HIP_TRY(hipMemsetAsync(c->d_merr, 0, OTSDB_MULTI_MAX * sizeof(int), st));
  c->clean_entry = false;
  multi_counters(c, 0, 0);
  return OTSDB_OK;
}

// the existing multi_aggregate over each matrix, every output compacted, one
// synchronisation
otsdb_status panel_finish(otsdb_ctx* c, PanelPass& X, PanelOutcome& O) {
  const int D = (int)X.MS.size();
  otsdb_status rc;
  for (int d = 0; d < D; ++d) {
    rc = multi_aggregate(c, X.MS[d], /*compact_now=*/false);
    if (rc) return rc;
  }
  for (int d = 0; d < D; ++d) {
    rc = multi_compact_launch(c, X.qs[d], X.MS[d].P, X.MS[d].G,
                              X.MS[d].out_val, X.MS[d].out_emit);
    if (rc) return rc;
  }
  const Req all{(int32_t)X.orig.size(), nullptr, nullptr, nullptr,
                X.outs.data()};
  rc = multi_compact_wait(c, all, X.orig.data());
  for (size_t j = 0; j < X.orig.size(); ++j)
    O.total[X.orig[j]] = c->multi_total[X.orig[j]];
  if (rc) O.fail_at(c, c->multi_failed, rc);
  return OTSDB_OK;
}

// The envelope functions E of a request over one pass of the point stream:
// every function's buffers carved from one workspace (multi_build), prep, the
// envelope kernel into the D row matrices, the existing multi_aggregate over
// each matrix, every output compacted, one synchronisation.
otsdb_status panel_shared(otsdb_ctx* c, const otsdb_query_spec* spec,
                          const Req& q, const otsdb_batch* b,
                          std::vector<int64_t>& goff, const Params& P,
                          std::vector<PanelFunc*>& E, PanelOutcome& O) {
  hipStream_t st = c->stream;
  const int D = (int)E.size();
  const BatchDev B = batch_dev(b);
  PanelPass X(spec, q, E);
  std::vector<MultiState>& MS = X.MS;
  otsdb_status rc = panel_build(c, X, B, b->group_members, goff, P, nullptr);
  if (rc) return rc;
  // ---- prep.  Bounds, seek and the first / last bucket do not depend on
  // the function: one launch, shared by every function's work set.  Only
  // under NONE fill k_prep also downsamples the bucket past the window with
  // its monoid (SeriesMeta.of_val, what the rows interpolate toward): there
  // each function runs its own k_prep — S threads, no pass over the stream.
  const Params& Pr = MS[0].P;
  uint32_t fn = 0;
  PanelRows R{nullptr, nullptr, nullptr, nullptr, nullptr, 0};
  {
    StageTimer tm(c, 3);
    if (Pr.fill == 0 && !Pr.run_all) {
      for (int d = 0; d < D; ++d) {
        DsLaunch a = ds_args(c, Pr, B, MS[d].W);
        with_monoid(E[d]->ds, [&](auto tag) {
          launch_ds<decltype(tag)>(DS_PREP, a);
        });
      }
    } else {
      launch_ds<MSum<3>>(DS_PREP, ds_args(c, Pr, B, MS[0].W));
      for (int d = 1; d < D; ++d) MS[d].W.SM = MS[0].W.SM;
    }
  }
  for (int d = 0; d < D; ++d) {
    double* v = MS[d].W.R.val;
    switch (E[d]->fn) {
      case PF_SUM: R.sum = v; break;
      case PF_AVG: R.avg = v; break;
      case PF_CNT: R.cnt = v; break;
      case PF_MIN: R.min = v; break;
      default: R.max = v; break;
    }
    fn |= E[d]->fn;
  }
  R.fn = fn;
  {
    StageTimer tm(c, 0);
    launch_panel(st, Pr, B, MS[0].W.SM, R);
  }
  HIP_TRY(hipGetLastError());
  ++c->n_multi_ds;
  ++c->n_panel_passes;
  c->n_panel_mats += D;
  return panel_finish(c, X, O);
}

// the envelope functions of a request's functions F
std::vector<PanelFunc*> panel_envelope(std::vector<PanelFunc>& F) {
  std::vector<PanelFunc*> E;
  for (PanelFunc& f : F)
    if (f.fn) E.push_back(&f);
  return E;
}

// What the columnar and the cells call ask alike before the envelope
// functions E share one pass: two or more of them, a query without rate or
// per-series anchors, and every function's outputs within the budgets of the
// |E| row matrices together.  *P: the grid (of E[0]'s first output).
bool panel_shares_rows(otsdb_ctx* c, const otsdb_query_spec* spec, const Req& q,
                       std::vector<PanelFunc*>& E, int64_t S,
                       const std::vector<int64_t>& goff, Params* P) {
  if (E.size() < 2 || spec->rate || anchored(spec)) return false;
  const otsdb_query_spec s0 = req_spec(spec, q, E[0]->idx[0]);
  if (make_params(&s0, P, c) != OTSDB_OK) return false;  // (the calls report it)
  for (PanelFunc* f : E) {
    otsdb_query_spec sd = *spec;
    sd.ds_agg_id = f->ds;
    if (!multi_shares_rows(&sd, f->req(q, 0), *P, S, goff, 1, (int)E.size()))
      return false;
  }
  return true;
}

otsdb_status run_panel_impl(otsdb_ctx* c, const otsdb_query_spec* spec,
                            const Req& q, const otsdb_batch* b,
                            std::vector<int64_t>& goff) {
  c->multi_failed = -1;
  c->n_panel_passes = c->n_panel_mats = 0;
  std::vector<PanelFunc> F = panel_funcs(spec, q);
  PanelOutcome O;
  // ---- the shared pass: two or more envelope functions of a downsampled,
  // columnar query without rate or per-series anchors, within the budgets
  std::vector<PanelFunc*> E = panel_envelope(F);
  Params P;
  const bool shared = !misaligned(b) &&
                      panel_shares_rows(c, spec, q, E, b->n_series, goff, &P);
  if (shared) {
    const otsdb_status rc = panel_shared(c, spec, q, b, goff, P, E, O);
    if (rc) return rc;  // (the device or the workspace, not an output)
  }
  // ---- everything else function by function: one multi call each
  for (PanelFunc& f : F) {
    if (shared && f.fn) continue;
    otsdb_query_spec sf = *spec;
    sf.ds_agg_id = f.ds;
    c->result_short = false;
    // (OTSDB_SPEC_MULTI_FOLD: a panel of one distinct function is the multi
    // call; several functions keep the row path)
    O.record(c, f, run_multi_impl(c, &sf, f.req(q, 0), b, goff,
                                  /*may_fold=*/F.size() == 1));
  }
  return O.publish(c, q.n);
}

// otsdb_decode_cells_device without the lock (also the fallback of the
// fused cells query)
// counted: an earlier call on the same cells (ts_ms null) left the row
// counts, output offsets and uniform flags in the context's decode workspace
// and the series offsets in `offsets`: only the write pass runs.
otsdb_status decode_impl(otsdb_ctx* c, const otsdb_cells* cells,
                         int64_t n_series, int64_t* offsets, int64_t* ts_ms,
                         int64_t* val, uint8_t* is_float, int64_t capacity,
                         hipStream_t st, bool counted = false) {
  const int64_t R = cells->n_rows, S = n_series;
  if (R < 0 || S < 0) return fail(OTSDB_E_ILLEGAL_ARGUMENT, "negative sizes");
  // workspace: row counts, row output offsets, uniform-column flags and the
  // device scan's temporary storage
  size_t scan_tmp = 0;
  HIP_TRY(rocprim::exclusive_scan(nullptr, scan_tmp, (const int64_t*)nullptr,
                                  (int64_t*)nullptr, (int64_t)0,
                                  (size_t)(R + 1), rocprim::plus<int64_t>(),
                                  st));
  const size_t ws_need = (size_t)(2 * R + 2) * 8 + (size_t)R + 128 + scan_tmp;
  otsdb_status rc = c->dec_ws.ensure(ws_need);
  if (rc) return rc;
  int64_t* row_count = (int64_t*)c->dec_ws.p;
  int64_t* row_out = row_count + (R + 1);
  uint8_t* fast = (uint8_t*)(row_out + (R + 1));
  int* flags = (int*)(((uintptr_t)(fast + R) + 15) & ~(uintptr_t)15);
  void* tmp = (void*)(((uintptr_t)(flags + 4) + 63) & ~(uintptr_t)63);
  CellsDev C{R, cells->row_series, cells->row_base_s, cells->qual_off,
             cells->qual, cells->val_off, cells->val};
  // the write pass: k_decode for the uniform rows, k_decode_generic for the
  // rest when the count pass saw any (c->dec_generic)
  auto write_pass = [&]() -> otsdb_status {
    if (R > 0) {
      hipLaunchKernelGGL(k_decode, dim3(blocks_for(R, 4)), dim3(256), 0, st, C,
                         1, row_count, (const int64_t*)row_out, fast, capacity,
                         ts_ms, val, is_float, c->d_err, flags);
      if (c->dec_generic & 2)
        hipLaunchKernelGGL(k_decode_generic, dim3(blocks_for(R, 4)), dim3(256),
                           0, st, C, 1, row_count, (const int64_t*)row_out,
                           (const uint8_t*)fast, capacity, ts_ms, val, is_float,
                           c->d_err);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    return OTSDB_OK;
  };
  if (counted) return write_pass();
  HIP_TRY(hipMemsetAsync(c->d_err, 0, sizeof(int), st));
  HIP_TRY(hipMemsetAsync(flags, 0, 2 * sizeof(int), st));
  c->dec_generic = 0;
  if (R > 0) {
    hipLaunchKernelGGL(k_decode, dim3(blocks_for(R, 4)), dim3(256), 0, st, C,
                       0, row_count, (const int64_t*)nullptr, fast, (int64_t)0,
                       (int64_t*)nullptr, (int64_t*)nullptr,
                       (uint8_t*)nullptr, c->d_err, flags);
    int hf[2];
    HIP_TRY(hipMemcpyAsync(hf, flags, sizeof(hf), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    c->dec_generic = (hf[0] ? 1 : 0) | (hf[1] ? 2 : 0);
    if (c->dec_generic & 1)
      hipLaunchKernelGGL(k_decode_generic, dim3(blocks_for(R, 4)), dim3(256), 0,
                         st, C, 0, row_count, (const int64_t*)nullptr,
                         (const uint8_t*)fast, (int64_t)0, (int64_t*)nullptr,
                         (int64_t*)nullptr, (uint8_t*)nullptr, c->d_err);
    // row_count[R] = 0, so row_out[R] = the total
    HIP_TRY(hipMemsetAsync(row_count + R, 0, 8, st));
    HIP_TRY(rocprim::exclusive_scan(tmp, scan_tmp, (const int64_t*)row_count,
                                    row_out, (int64_t)0, (size_t)(R + 1),
                                    rocprim::plus<int64_t>(), st));
  } else {
    HIP_TRY(hipMemsetAsync(row_out, 0, 8, st));
  }
  hipLaunchKernelGGL(k_series_offsets, dim3(blocks_for(R + 1, 256)), dim3(256),
                     0, st, R, S, cells->row_series, (const int64_t*)row_out,
                     offsets);
  HIP_TRY(hipMemcpyAsync(&c->h_small[0], c->d_err, sizeof(int),
                         hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(&c->h_small[1], row_out + R, 8, hipMemcpyDeviceToHost,
                         st));
  HIP_TRY(hipStreamSynchronize(st));
  if (c->h_small[0] & ERR_CORRUPT_CELL)
    return fail(OTSDB_E_ILLEGAL_DATA,
                "Corrupted value: couldn't break down into individual values");
  const int64_t total = c->h_small[1];
  if (!ts_ms) return OTSDB_OK;
  if (total > capacity)
    return fail(OTSDB_E_CAPACITY, "decode capacity %lld < %lld points",
                (long long)capacity, (long long)total);
  return write_pass();
}

// Columns of mixed qualifier widths rewritten with one (k_requal, decode.hip)
// into the context's cells_col buffer: *out views the rewritten qualifier
// pool with the original rows and value pool.  A count pass, a scan of the
// row counts, a write pass.
otsdb_status requal_impl(otsdb_ctx* c, const CellsDev& C, CellsDev* out,
                         hipStream_t st) {
  const int64_t R = C.R;
  size_t scan_tmp = 0;
  HIP_TRY(rocprim::exclusive_scan(nullptr, scan_tmp, (const int64_t*)nullptr,
                                  (int64_t*)nullptr, (int64_t)0,
                                  (size_t)(R + 1), rocprim::plus<int64_t>(),
                                  st));
  otsdb_status rc = c->dec_ws.ensure((size_t)(2 * R + 2) * 8 + 128 + scan_tmp);
  if (rc) return rc;
  int64_t* row_count = (int64_t*)c->dec_ws.p;
  int64_t* row_out = row_count + (R + 1);
  void* tmp = (void*)(((uintptr_t)(row_out + R + 1) + 63) & ~(uintptr_t)63);
  HIP_TRY(hipMemsetAsync(c->d_err, 0, sizeof(int), st));
  HIP_TRY(hipMemsetAsync(row_count + R, 0, 8, st));
  if (R > 0)
    hipLaunchKernelGGL(k_requal<0>, dim3(blocks_for(R, 4 * OTSDB_RQ_RPW)), dim3(256), 0, st,
                       C, row_count, (const int64_t*)nullptr, (int64_t*)nullptr,
                       (uint8_t*)nullptr, c->d_err);
  HIP_TRY(hipGetLastError());
  HIP_TRY(rocprim::exclusive_scan(tmp, scan_tmp, (const int64_t*)row_count,
                                  row_out, (int64_t)0, (size_t)(R + 1),
                                  rocprim::plus<int64_t>(), st));
  HIP_TRY(hipMemcpyAsync(&c->h_small[0], c->d_err, sizeof(int),
                         hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(&c->h_small[1], row_out + R, 8, hipMemcpyDeviceToHost,
                         st));
  HIP_TRY(hipStreamSynchronize(st));
  if (c->h_small[0] & ERR_CORRUPT_CELL)
    return fail(OTSDB_E_ILLEGAL_DATA,
                "Corrupted value: couldn't break down into individual values");
  const int64_t N = c->h_small[1];
  const size_t qo = ((size_t)(R + 1) * 8 + 255) & ~(size_t)255;
  rc = c->cells_col.ensure(qo + 4 * (size_t)N + 64);
  if (rc) return rc;
  int64_t* qoff = (int64_t*)c->cells_col.p;
  uint8_t* qual = (uint8_t*)c->cells_col.p + qo;
  if (R > 0)
    hipLaunchKernelGGL(k_requal<1>, dim3(blocks_for(R, 4 * OTSDB_RQ_RPW)), dim3(256), 0, st,
                       C, row_count, (const int64_t*)row_out, qoff, qual,
                       c->d_err);
  else
    HIP_TRY(hipMemsetAsync(qoff, 0, 8, st));
  HIP_TRY(hipGetLastError());
  *out = CellsDev{R, C.row_series, C.row_base_s, qoff, qual, C.val_off, C.val};
  return OTSDB_OK;
}

// The compacted columns decoded into the context's own columnar buffer: *cb
// is b over them (the fallback of the fused cells queries).
otsdb_status cells_columnar(otsdb_ctx* c, const otsdb_cells* cells,
                            const otsdb_batch* b, otsdb_batch* cb_out) {
  hipStream_t st = c->stream;
  const int64_t S = b->n_series;
  otsdb_status rc =
      c->cells_ws.ensure((size_t)(S + 1) * 8 + 64);
  if (rc) return rc;
  int64_t* offs = (int64_t*)c->cells_ws.p;
  // the generic decode (its own stage; released before the pipeline)
  std::unique_ptr<StageTimer> dec_tm(new StageTimer(c, 7));
  rc = decode_impl(c, cells, S, offs, nullptr, nullptr, nullptr, 0, st);
  if (rc) return rc;
  int64_t N = 0;
  HIP_TRY(hipMemcpyAsync(&N, offs + S, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  const size_t col = ((size_t)std::max<int64_t>(N, 2) * 8 + 255) & ~(size_t)255;
  rc = c->cells_col.ensure(2 * col + (size_t)std::max<int64_t>(N, 2) + 256);
  if (rc) return rc;
  int64_t* ts = (int64_t*)c->cells_col.p;
  int64_t* vv = (int64_t*)((char*)c->cells_col.p + col);
  uint8_t* isf = (uint8_t*)((char*)c->cells_col.p + 2 * col);
  rc = decode_impl(c, cells, S, offs, ts, vv, isf, N, st, true);
  dec_tm.reset();
  if (rc) return rc;
  otsdb_batch cb = *b;
  cb.n_points = N;
  cb.offsets = offs;
  cb.ts_ms = ts;
  cb.val = vv;
  cb.is_float = isf;
  cb.series_float = nullptr;
  *cb_out = cb;
  return OTSDB_OK;
}

// The fused cells path with its retries, for every cells query.  pass(CQ,
// series_row): one attempt's launches over the columns CQ; finish(): the
// rest of the query, once the attempt's error word is clean.
// A column the fused path does not take (ERR_CELLS_GENERIC) — widths mixed
// inside a row or across a series' rows — is rewritten with 4-byte
// qualifiers (k_requal) and the fused path runs again; what it still does
// not take re-runs through the caller's decode.  A uniform fold that meets a
// qualifier of other flags is run again with the general kernel
// (ERR_CELLS_NONUNI, one more attempt).
// *end: whether the status is the query's (CELLS_CORRUPT: of a corrupt
// column) or the caller decodes (CELLS_DECODE).
enum CellsEnd { CELLS_DONE, CELLS_CORRUPT, CELLS_DECODE };

template <class Pass, class Finish>
otsdb_status cells_attempts(otsdb_ctx* c, const otsdb_cells* cells, int64_t S,
                            Params& P, CellsEnd* end, Pass pass,
                            Finish finish) {
  hipStream_t st = c->stream;
  const int64_t R = cells->n_rows;
  *end = CELLS_DONE;
  otsdb_status rc = c->cells_ws.ensure((size_t)(S + 1) * 8);
  if (rc) return rc;
  int64_t* series_row = (int64_t*)c->cells_ws.p;
  hipLaunchKernelGGL(k_series_rows, dim3(blocks_for(R + 1, 256)), dim3(256),
                     0, st, R, S, cells->row_series, series_row);
  P.check_order = c->verbatim ? 1 : 0;
  const CellsDev C{R, cells->row_series, cells->row_base_s, cells->qual_off,
                   cells->qual, cells->val_off, cells->val};
  CellsDev CQ = C;
  c->cells_no_uni = false;
  bool requaled = false;
  for (int attempt = 0; attempt < 4; ++attempt) {
    rc = pass(CQ, series_row);
    if (rc) return rc;
    int e;
    if ((rc = read_err(c, &e))) return rc;
    if ((e & ERR_CELLS_NONUNI) && !c->cells_no_uni) {
      ++c->n_cells_uni_miss;
      c->cells_no_uni = true;
      continue;
    }
    if (c->verbatim && (e & (ERR_CORRUPT_CELL | ERR_CELLS_GENERIC |
                             ERR_NOT_SORTED | ERR_SPEC_MISS)))
      return spec_miss(c);
    if (e & ERR_CORRUPT_CELL) {
      *end = CELLS_CORRUPT;
      return fail(OTSDB_E_ILLEGAL_DATA,
                  "Corrupted value: couldn't break down into individual values");
    }
    if (!(e & ERR_CELLS_GENERIC)) return finish();
    if (requaled) break;
    requaled = true;
    c->cells_no_uni = false;
    {
      StageTimer rq_tm(c, 7);
      rc = requal_impl(c, C, &CQ, st);
      if (rc) return rc;
    }
  }
  c->cells_no_uni = false;
  if (c->verbatim) return spec_miss(c);  // (they have no decode to fall back to)
  *end = CELLS_DECODE;
  return OTSDB_OK;
}

// One cells call for a request without downsampling functions: the single
// query, unchanged, for one output, else the cells multi call.
otsdb_status run_cells_req(otsdb_ctx* c, const otsdb_query_spec* spec,
                           const Req& q, const otsdb_cells* cells,
                           const otsdb_batch* b, std::vector<int64_t>& goff) {
  const otsdb_query_spec s0 = req_spec(spec, q, 0);
  c->multi_failed = -1;
  if (q.n > 1) return run_cells_impl(c, &s0, cells, b, nullptr, goff, &q);
  multi_counters(c, 1, 1);
  const otsdb_status rc = run_cells_impl(c, &s0, cells, b, &q.outs[0], goff);
  if (!rc) c->multi_total[0] = c->h_small[1];
  return rc;
}

// One attempt of the shared cells pass: the functions' buffers, the state
// matrices cleared (multi_build, sentinel = 0), k_bucketize_panel_cells once
// into the D matrices.  The caller reads the error word before it aggregates.
otsdb_status cells_panel_rows(otsdb_ctx* c, PanelPass& X,
                              std::vector<PanelFunc*>& E, const BatchDev& B,
                              const int64_t* d_members,
                              std::vector<int64_t>& goff, const Params& P,
                              const CellsDev& C, const int64_t* series_row) {
  const int D = (int)E.size();
  std::vector<MultiState>& MS = X.MS;
  otsdb_status rc = panel_build(c, X, B, d_members, goff, P, &C);
  if (rc) return rc;
  // keep, lo, hi, kf, kl, of_has and of_ts do not depend on the function:
  // one set of arrays; every function its own of_val (NONE fill: what its
  // rows interpolate toward)
  PanelCellsRows R{};
  for (int d = 0; d < D; ++d) {
    Work& W = MS[d].W;
    double* const ov = W.SM.of_val;
    W.SM = MS[0].W.SM;
    W.SM.of_val = ov;
    switch (E[d]->fn) {
      case PF_SUM: R.sum = W.R.val, R.st_sum = W.R.state, R.of_sum = ov; break;
      case PF_AVG: R.avg = W.R.val, R.st_avg = W.R.state, R.of_avg = ov; break;
      case PF_CNT: R.cnt = W.R.val, R.st_cnt = W.R.state, R.of_cnt = ov; break;
      case PF_MIN: R.min = W.R.val, R.st_min = W.R.state, R.of_min = ov; break;
      default: R.max = W.R.val, R.st_max = W.R.state, R.of_max = ov; break;
    }
    R.fn |= E[d]->fn;
  }
  {
    StageTimer tm(c, 0);
    launch_panel_cells(c->stream, MS[0].P, C, series_row, B.S, MS[0].W.SM, R,
                       c->d_err);
  }
  HIP_TRY(hipGetLastError());
  ++c->n_multi_ds;
  ++c->n_panel_passes;  // (one per attempt; the matrices are the last one's)
  c->n_panel_mats = D;
  return OTSDB_OK;
}

// otsdb_agg_run_cells_panel_device: run_cells_impl's routing for a panel
// request.  Two or more envelope functions of a query the fused cells path
// takes share one pass over the compacted columns (the decode runs once for
// all of them), inside the attempt loop of every cells query
// (cells_attempts): a column of mixed qualifier widths is rewritten once and
// the pass runs again, a corrupt one fails every output.  The other
// functions of such a request then run one cells call each.  One distinct
// function is the cells multi call.  What the
// fused path does not take (`all`, anchored calendars, rate, raw group-by,
// grids past the limits, columns still generic after the rewrite) is decoded
// once into the context's columnar buffer and runs as the columnar panel
// call.
otsdb_status run_cells_panel_impl(otsdb_ctx* c, const otsdb_query_spec* spec,
                                  const Req& q, const otsdb_cells* cells,
                                  const otsdb_batch* b,
                                  std::vector<int64_t>& goff) {
  const int64_t S = b->n_series, R = cells->n_rows;
  if (S < 0 || R < 0) return fail(OTSDB_E_ILLEGAL_ARGUMENT, "negative sizes");
  c->multi_failed = -1;
  c->n_panel_passes = c->n_panel_mats = 0;
  std::vector<PanelFunc> F = panel_funcs(spec, q);
  PanelOutcome O;
  // one cells call for function f's outputs (the single query for one)
  auto run_func = [&](PanelFunc& f) {
    otsdb_query_spec sf = *spec;
    sf.ds_agg_id = f.ds;
    // (OTSDB_SPEC_CELLS_MULTI_FOLD: only a panel of one distinct function is
    // the cells multi call and inherits the bit)
    if (F.size() != 1) sf.flags &= ~OTSDB_SPEC_CELLS_MULTI_FOLD;
    c->result_short = false;
    O.record(c, f, run_cells_req(c, &sf, f.req(q, 0), cells, b, goff));
  };
  std::vector<PanelFunc*> E = panel_envelope(F);
  const bool ds = spec->ds_interval_ms > 0 || spec->run_all;
  Params P;
  const bool shared = ds && !spec->run_all &&
                      panel_shares_rows(c, spec, q, E, S, goff, &P) &&
                      !P.ds_sel && !P.run_all;
  if (shared) {
    const BatchDev B{S, nullptr, nullptr, nullptr, nullptr, nullptr};
    PanelPass X(spec, q, E);
    CellsEnd end;
    // cells_attempts (the row kernel raises no ERR_CELLS_NONUNI: at most the
    // pass, the rewrite, the pass again)
    const otsdb_status rc = cells_attempts(
        c, cells, S, P, &end,
        [&](const CellsDev& CQ, const int64_t* series_row) {
          return cells_panel_rows(c, X, E, B, b->group_members, goff, P, CQ,
                                  series_row);
        },
        [&]() { return panel_finish(c, X, O); });
    // the columns are every output's: all fail, the lowest index reports
    if (end == CELLS_CORRUPT) c->multi_failed = 0;
    if (rc) return rc;
    if (end == CELLS_DONE) {
      for (PanelFunc& f : F)
        if (!f.fn) run_func(f);
      return O.publish(c, q.n);
    }
    c->n_panel_passes = c->n_panel_mats = 0;
  } else if (F.size() == 1) {
    run_func(F[0]);
    return O.publish(c, q.n);
  }
  // one decode for the whole panel, then the columnar panel call
  otsdb_batch cb;
  const otsdb_status rc = cells_columnar(c, cells, b, &cb);
  if (rc) return rc;
  return run_panel_impl(c, spec, q, &cb, goff);
}

// what no partials entry takes: the grid of a query the ranks cannot merge
otsdb_status partials_grid(otsdb_ctx* c, const otsdb_query_spec* spec,
                           const otsdb_batch* b, Params* P) {
  otsdb_status rc = check_spec(spec);
  if (!rc) rc = make_params(spec, P, c);
  if (!rc && !(spec->ds_interval_ms > 0 || spec->run_all))
    rc = fail(OTSDB_E_UNSUPPORTED,
              "raw group-by across ranks (union timestamps need an all-gather)");
  if (!rc && !P->run_all && !P->fill &&
      (double)b->n_series * (double)P->nb > 4.0e9)
    rc = fail(OTSDB_E_UNSUPPORTED, "grid trimming is not supported across ranks");
  return rc;
}

// one aggregator's partials (the context locked, the stream bound)
otsdb_status partials_locked(otsdb_ctx* c, const otsdb_query_spec* spec,
                             const otsdb_batch* b, std::vector<int64_t>& goff,
                             const otsdb_partial* init,
                             const uint8_t* init_emit, otsdb_partial* partials,
                             uint8_t* emit) {
  Params P;
  otsdb_status rc = partials_grid(c, spec, b, &P);
  if (!rc) {
    const BatchDev B = batch_dev(b);
    Work W;
    const int64_t G = (int64_t)goff.size() - 1;
    if (G * P.nb > 0 && init) {
      // groups with no member here pass their state on unchanged
      if (init != partials)
        HIP_TRY(hipMemcpyAsync(partials, init,
                               sizeof(otsdb_partial) * (size_t)G * P.nb,
                               hipMemcpyDeviceToDevice, c->stream));
      if (init_emit != emit)
        HIP_TRY(hipMemcpyAsync(emit, init_emit, (size_t)G * P.nb,
                               hipMemcpyDeviceToDevice, c->stream));
    } else if (G * P.nb > 0) {
      hipMemsetAsync(emit, 0, (size_t)G * P.nb, c->stream);
      hipMemsetAsync(partials, 0, sizeof(otsdb_partial) * (size_t)G * P.nb,
                     c->stream);
    }
    rc = run_pipeline(c, spec, B, b->group_members, goff, P, W, 1,
                      (Packed*)partials, emit, nullptr, nullptr,
                      (const Packed*)init, init_emit);
    int err = 0;
    if (!rc) rc = read_err(c, &err);
    if (!rc && (err & ERR_RATE_TS)) rc = rate_ts_error();
  }
  return rc;
}

otsdb_status partials_impl(otsdb_ctx* c, const otsdb_query_spec* spec,
                           const otsdb_batch* b, const otsdb_partial* init,
                           const uint8_t* init_emit, otsdb_partial* partials,
                           uint8_t* emit, void* hip_stream) {
  if (!c || !spec || !b || !partials || !emit || (!init != !init_emit))
    return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null");
  DeviceCall dc(c, b, hip_stream);
  return dc.rc ? dc.rc
               : partials_locked(c, spec, b, dc.goff, init, init_emit, partials,
                                 emit);
}

// the multi_request checks of the entries that exchange partials: the
// selections take the otsdb_sel_* protocol
otsdb_status check_multi_partials(const otsdb_query_spec* spec,
                                  const Req& q) {
  const otsdb_status rc = check_req(spec, q);
  if (rc) return rc;
  for (int i = 0; i < q.n; ++i)
    if (is_selection(q.aggs[i]))
      return fail(OTSDB_E_ILLEGAL_ARGUMENT,
                  "percentiles across ranks: use the otsdb_sel_* protocol "
                  "(otsdb_sel_retarget for several)");
  return OTSDB_OK;
}

// the protocol's device words, after the error word (d_err + 128 .. 160):
// per-pass flags, the scans' "broken" mark
uint32_t* xs_flags(otsdb_ctx* c) { return (uint32_t*)((char*)c->d_err + 128); }
uint32_t* xs_broken(otsdb_ctx* c) { return (uint32_t*)((char*)c->d_err + 152); }

int64_t* xs_bnd(otsdb_ctx* c) { return (int64_t*)c->sel.segmem.p; }
int64_t* xs_off(otsdb_ctx* c) {
  return (int64_t*)c->sel.segmem.p + (c->sel.G * c->sel.NB + 1);
}
uint32_t* xs_segfill(otsdb_ctx* c) {
  return (uint32_t*)(xs_off(c) + (c->sel.G * c->sel.NB + 1));
}
void* xs_scan_tmp(otsdb_ctx* c) {
  const int64_t GB = c->sel.G * c->sel.NB;
  return (char*)c->sel.segmem.p + (((size_t)(GB + 1) * 16 + (size_t)GB * 4 + 255) & ~(size_t)255);
}

XPool xs_pool(otsdb_ctx* c) {
  auto& S = c->sel;
  XPool p;
  p.key = (uint64_t*)S.pool.p;
  p.seg = S.pool.p ? (int64_t*)((char*)S.pool.p + (size_t)S.pool_cap * 8) : nullptr;
  p.off = xs_off(c);
  p.fill = xs_segfill(c);
  p.cap = S.pool_cap;
  p.flags = xs_broken(c);
  return p;
}

}  // namespace

// ------------------- the query implementations other units call (engine_int.h)
namespace otsdb {
namespace eng {

// Grid of buckets every series row is laid out on.
otsdb_status make_params(const otsdb_query_spec* s, Params* P,
                         otsdb_ctx* c) {
  memset(P, 0, sizeof(*P));
  P->start_ms = s->start_ms;
  P->end_ms = s->end_ms;
  P->run_all = s->run_all;
  P->fill = s->run_all ? 0 : s->fill;
  P->rate = s->rate;
  P->counter = s->counter;
  P->drop_resets = s->drop_resets;
  P->counter_max = s->counter_max;
  P->reset_value = s->reset_value;
  agg_params(P, s->agg_id, s->interp);
  P->fill_value = (P->fill == OTSDB_FILL_ZERO) ? 0.0 : NAN;
  if (!(s->ds_interval_ms > 0 || s->run_all)) return OTSDB_OK;  // raw
  if (is_selection(s->ds_agg_id)) {
    P->ds_sel = s->ds_agg_id == OTSDB_AGG_MEDIAN ? 1 : 2;
    P->ds_pct = s->ds_agg_id >= OTSDB_AGG_P999 ? pct_of(s->ds_agg_id) : 0.0;
  }
  P->rate_origin_ts = 0;
  P->rate_origin_val = 0.0;
  if (s->run_all) {
    // Downsampler "all": one point at query_start holding the points of
    // [query_start, query_end) after seek(start) (Downsampler.java:354-379)
    P->interval = 1;
    P->inv_interval = 1.0;
    P->gbase = s->query_start_ms;
    P->out_ts0 = s->query_start_ms;
    P->seek_ts = std::max(s->start_ms, s->query_start_ms);
    P->stop_ts = s->query_end_ms;
    P->nb = (s->query_start_ms >= s->start_ms &&
             s->query_start_ms <= s->end_ms) ? 1 : 0;
    P->narrow = 1;  // every point is bucket 0
    return OTSDB_OK;
  }
  const int64_t iv = s->ds_interval_ms;
  P->interval = iv;
  P->inv_interval = 1.0 / (double)iv;
  if (s->use_calendar && s->n_cal_anchors > 0)  // callers derive stage B
    return fail(OTSDB_E_UNSUPPORTED,
                "per-series calendar grids on this entry point");
  if (s->use_calendar) return make_cal_params(s, P, c);
  const int64_t grid0 = align_down(s->start_ms + iv - 1, iv);
  P->gbase = grid0;
  P->seek_ts = grid0;
  if (P->fill) {
    // FillingDownsampler: every bucket of [align(start), align(end)); the
    // aggregation iterator skips those before start (FillingDownsampler.java
    // :136-142, AggregationIterator.java:425-447)
    const int64_t aend = align_down(s->end_ms, iv);
    P->nb = aend > grid0 ? (aend - grid0) / iv : 0;
    P->stop_ts = grid0 + P->nb * iv;
    const int64_t astart = align_down(s->start_ms, iv);
    if (astart < grid0) {
      P->rate_origin_ts = astart;
      P->rate_origin_val = P->fill_value;
    }
  } else {
    P->nb = s->end_ms >= grid0 ? (s->end_ms - grid0) / iv + 1 : 0;
    P->stop_ts = grid0 + P->nb * iv;
  }
  // points fed to the bucket fold lie in [gbase, stop_ts): 32-bit offsets
  P->narrow = iv < (int64_t(1) << 31) && P->nb < (int64_t(1) << 32) / iv;
  return OTSDB_OK;
}

otsdb_status run_device_impl(otsdb_ctx* c, const otsdb_query_spec* spec,
                             const otsdb_batch* b, otsdb_result* out,
                             std::vector<int64_t>& goff) {
  otsdb_status rc = check_spec(spec);
  if (rc) return rc;
  if (anchored(spec)) return run_anchored(c, spec, b, out, goff);
  Params P;
  rc = make_params(spec, &P, c);
  if (rc) return rc;
  if (misaligned(b))
    return fail(OTSDB_E_ILLEGAL_ARGUMENT,
                "ts_ms/val must be 16-byte aligned (16-B streaming loads)");
  const BatchDev B = batch_dev(b);
  if (!(spec->ds_interval_ms > 0 || spec->run_all))
    return run_raw(c, spec, b, B, goff, P, out);
  Work W;
  rc = run_pipeline(c, spec, B, b->group_members, goff, P, W, 0, nullptr,
                    nullptr);
  if (rc) return rc;
  const int64_t G = (int64_t)goff.size() - 1;
  rc = compact(c, P, G, W.out_val, W.out_emit, W.counts, out);
  if (rc) return rc;
  return finish(c, G, out);
}

// ------------------------------------------------------- rollup queries
// otsdb_agg_run_rollup*: the points are a rollup table's cells; R (the
// rollup aggregator) and the downsampling function F pick how a bucket is
// computed (Downsampler.java:162-228, FillingDownsampler.java:196-252;
// DESIGN.md §4.3).

// The checks that need no device, and the state the rows are built with
// (ROLLUP_NONE: the ordinary F.runDouble — the single query, counts ignored).
otsdb_status check_rollup(const otsdb_query_spec* s, const Rollup& r,
                          RollupKind* kind) {
  if (r.agg < 0 || r.agg >= OTSDB_AGG_COUNT_IDS)
    return fail(OTSDB_E_NO_SUCH_ELEMENT, "No such aggregator: %d", r.agg);
  otsdb_status rc = check_spec(s);
  if (rc) return rc;
  if (r.agg == OTSDB_AGG_DEV)
    return fail(OTSDB_E_UNSUPPORTED,
                "standard deviation over rolled up data is not supported");
  if (!(s->ds_interval_ms > 0 || s->run_all))
    return fail(OTSDB_E_UNSUPPORTED, "a rollup query without a downsampler");
  if (s->n_cal_anchors > 0)
    return fail(OTSDB_E_UNSUPPORTED,
                "rollup queries over per-series calendar anchors");
  *kind = ROLLUP_NONE;
  if (r.agg == OTSDB_AGG_AVG) {
    if (s->ds_agg_id != OTSDB_AGG_AVG)
      return fail(OTSDB_E_UNSUPPORTED,
                  "rollup avg downsampled with another function");
    if (!r.cnt)
      return fail(OTSDB_E_ILLEGAL_ARGUMENT, "rollup avg needs value_count");
    *kind = ROLLUP_AVG;
  } else if (s->ds_agg_id == OTSDB_AGG_COUNT) {
    *kind = ROLLUP_COUNT;
  }
  return OTSDB_OK;
}

// device pointers throughout (r.cnt too)
otsdb_status run_rollup_impl(otsdb_ctx* c, const otsdb_query_spec* spec,
                             const otsdb_batch* b, const Rollup& r,
                             otsdb_result* out, std::vector<int64_t>& goff) {
  RollupKind kind;
  otsdb_status rc = check_rollup(spec, r, &kind);
  if (rc) return rc;
  if (kind == ROLLUP_AVG && (((uintptr_t)r.cnt) & 15) != 0)
    return fail(OTSDB_E_ILLEGAL_ARGUMENT,
                "value_count must be 16-byte aligned (16-B streaming loads)");
  RollupScope scope(c, kind, r.cnt);
  return run_device_impl(c, spec, b, out, goff);
}

// Query straight from compacted columns: the fused decode + downsample when
// the query and the columns allow it, else decode -> columnar -> pipeline.
// mq: several aggregators (otsdb_agg_run_cells_multi_device; `spec` carries
// output 0's, `out` is unused): the same routing, with the shared-rows
// pipeline in place of run_pipeline where the outputs can share them (with
// OTSDB_SPEC_CELLS_MULTI_FOLD on an eligible request: the cells fold over
// the envelope state in its place, multi_fold_pass), and run_multi_impl over
// the decoded columns otherwise (never folded).
otsdb_status run_cells_impl(otsdb_ctx* c, const otsdb_query_spec* spec,
                            const otsdb_cells* cells, const otsdb_batch* b,
                            otsdb_result* out, std::vector<int64_t>& goff,
                            const Req* mq) {
  otsdb_status rc = check_spec(spec);
  if (rc) return rc;
  const int64_t S = b->n_series, R = cells->n_rows;
  if (S < 0 || R < 0) return fail(OTSDB_E_ILLEGAL_ARGUMENT, "negative sizes");
  const bool ds = spec->ds_interval_ms > 0 || spec->run_all;
  Params P;
  // per-series calendar grids rewrite columnar timestamps: decode first
  const bool fused = ds && !anchored(spec);
  if (fused) {
    rc = make_params(spec, &P, c);
    if (rc) return rc;
  }
  if (fused && !P.ds_sel && !P.run_all &&
      (!mq || multi_shares_rows(spec, *mq, P, S, goff))) {
    const BatchDev B{S, nullptr, nullptr, nullptr, nullptr, nullptr};
    Work W;
    MultiState MS;
    MultiFoldRun MF;
    CellsEnd end;
    // OTSDB_SPEC_CELLS_MULTI_FOLD: the cells fold over the envelope state in
    // the row pass's place (narrow grids, as the single cells fold; calendar
    // grids from cells keep the rows)
    const bool mfold = mq && !c->verbatim && P.narrow &&
                       multi_folds(spec, *mq, P, OTSDB_SPEC_CELLS_MULTI_FOLD);
    if (mq) c->n_multi_fold = 0;
    rc = cells_attempts(
        c, cells, S, P, &end,
        [&](const CellsDev& CQ, const int64_t* series_row) {
          if (mfold)
            return multi_fold_pass(c, spec, *mq, B, b->group_members, goff, P,
                                   &CQ, series_row, MF);
          if (mq) {  // (every attempt its own work set)
            MS = MultiState();
            return multi_build(c, spec, *mq, B, b->group_members, goff, P, &CQ,
                               series_row, MS);
          }
          W = Work();
          return run_pipeline(c, spec, B, b->group_members, goff, P, W, 0,
                              nullptr, nullptr, &CQ, series_row);
        },
        [&]() {
          if (mfold) return multi_fold_finish(c, *mq, MF);
          if (mq) return multi_aggregate(c, MS);
          const int64_t G = (int64_t)goff.size() - 1;
          const otsdb_status rf =
              compact(c, P, G, W.out_val, W.out_emit, W.counts, out);
          return rf ? rf : finish(c, G, out);
        });
    if (rc || end != CELLS_DECODE) return rc;
  }
  // (verbatim storage rows take only the cells fold)
  if (c->verbatim) return spec_miss(c);
  // decode to a columnar batch in the context's own buffer, then the
  // columnar pipeline (raw group-by, median/percentile or "all" downsampling,
  // mixed-width columns)
  otsdb_batch cb;
  rc = cells_columnar(c, cells, b, &cb);
  if (rc) return rc;
  if (mq) return run_multi_impl(c, spec, *mq, &cb, goff, /*may_fold=*/false);
  return run_device_impl(c, spec, &cb, out, goff);
}

}  // namespace eng
}  // namespace otsdb

// =========================================================================
// Top-N over query results (topn.hip): highestMax / highestCurrent
// =========================================================================
namespace {

otsdb_status check_topn(const otsdb_topn_spec* ts, int32_t n_results,
                        const otsdb_result* results, const int64_t* n_groups,
                        int64_t* n_series) {
  if (ts->function != OTSDB_TOPN_HIGHEST_MAX &&
      ts->function != OTSDB_TOPN_HIGHEST_CURRENT)
    return fail(OTSDB_E_ILLEGAL_ARGUMENT, "no top-N function %d", ts->function);
  if (ts->topn < 1)
    return fail(OTSDB_E_ILLEGAL_ARGUMENT,
                "Top n value must be greater than zero: %d", ts->topn);
  if (ts->start_ms < 0) return fail(OTSDB_E_ILLEGAL_ARGUMENT, "negative start");
  if (ts->grid_interval_ms < 0)
    return fail(OTSDB_E_ILLEGAL_ARGUMENT, "negative grid interval");
  if (n_results < 0 || (n_results > 0 && (!results || !n_groups)))
    return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null results");
  int64_t S = 0;
  for (int32_t r = 0; r < n_results; ++r) {
    if (n_groups[r] < 0) return fail(OTSDB_E_ILLEGAL_ARGUMENT, "n_groups < 0");
    if (n_groups[r] > 0 && !results[r].offsets)
      return fail(OTSDB_E_ILLEGAL_ARGUMENT, "result %d without offsets", r);
    S += n_groups[r];
  }
  if (S >= ((int64_t)1 << 31))
    return fail(OTSDB_E_UNSUPPORTED, "top-N over %lld series", (long long)S);
  // emission keys carry the timestamp in 47 bits (raw.hip)
  if (ts->end_ms >= kRawTsMax)
    return fail(OTSDB_E_UNSUPPORTED, "top-N window past 2^47 ms");
  *n_series = S;
  return OTSDB_OK;
}

otsdb_status topn_status(int err) {
  if (err & ERR_RAW_DUP)
    return fail(OTSDB_E_UNSUPPORTED,
                "top-N: a series' timestamps do not increase strictly (or a "
                "window point lies past 2^47 ms)");
  if (err & ERR_X1_MASK)
    return fail(OTSDB_E_ILLEGAL_STATE, "x1 beyond the millisecond mask");
  return OTSDB_OK;
}

// the mapped host block a top-N call reports through (topn.hip, TOPN_H_*)
otsdb_status topn_host_block(otsdb_ctx* c, int64_t n_out) {
  const size_t need = sizeof(int64_t) * (size_t)(TOPN_HDR + 2 * n_out);
  if (need > c->topn_host_cap) {
    if (c->h_topn) hipHostFree(c->h_topn);
    c->h_topn = c->d_topn = nullptr;
    c->topn_host_cap = 0;
    const size_t cap = std::max(need, (size_t)4096);
    HIP_TRY(hipHostMalloc(&c->h_topn, cap,
                          hipHostMallocMapped | hipHostMallocCoherent));
    HIP_TRY(hipHostGetDevicePointer((void**)&c->d_topn, c->h_topn, 0));
    c->topn_host_cap = cap;
  }
  for (int i = 0; i < TOPN_HDR; ++i) c->h_topn[i] = 0;
  return OTSDB_OK;
}

// the per-series arrays both paths use (carved from c->ws)
struct TopnWork {
  TopnSrc* src;
  int32_t *sres, *slot_in, *slot_out, *fb, *lb;
  int64_t *sp0, *slen, *soff, *numbered, *nrank, *members, *lo, *hi, *keybits,
      *picked, *pcount, *ccount, *coff;
  long long *maxl, *marks;
  unsigned long long* maxd;
  uint64_t *sk_in, *sk_out;
  int* flags;
  size_t carve(char* base, int R, int64_t S) {
    Carve cv{base};
    src = cv.take<TopnSrc>(R);
    sres = cv.take<int32_t>(S);
    sp0 = cv.take<int64_t>(S);
    slen = cv.take<int64_t>(S + 1);
    soff = cv.take<int64_t>(S + 1);
    numbered = cv.take<int64_t>(S + 1);
    nrank = cv.take<int64_t>(S + 1);
    members = cv.take<int64_t>(S);
    lo = cv.take<int64_t>(S + 1);
    hi = cv.take<int64_t>(S + 1);
    fb = cv.take<int32_t>(S);
    lb = cv.take<int32_t>(S);
    maxl = cv.take<long long>(S);
    maxd = cv.take<unsigned long long>(S);
    marks = cv.take<long long>(TOPN_MARKS);
    flags = cv.take<int>(4);
    sk_in = cv.take<uint64_t>(S);
    sk_out = cv.take<uint64_t>(S);
    slot_in = cv.take<int32_t>(S);
    slot_out = cv.take<int32_t>(S);
    keybits = cv.take<int64_t>(S);
    picked = cv.take<int64_t>(S);
    pcount = cv.take<int64_t>(S + 1);
    ccount = cv.take<int64_t>(S + 1);
    coff = cv.take<int64_t>(S + 1);
    return cv.off + 256;
  }
};

// numbering: per series its result, place and count; the numbered series
otsdb_status topn_number(otsdb_ctx* c, const otsdb_topn_spec* ts, int32_t R,
                         const otsdb_result* res, const int64_t* n_groups,
                         int64_t S, TopnWork& W) {
  hipStream_t st = c->stream;
  std::vector<TopnSrc> hs((size_t)R);
  int64_t s0 = 0;
  for (int32_t r = 0; r < R; ++r) {
    hs[r] = TopnSrc{res[r].offsets, res[r].ts, res[r].val, res[r].is_int, s0};
    s0 += n_groups[r];
  }
  otsdb_status rc = c->ws.ensure(W.carve(nullptr, R, S));
  if (rc) return rc;
  W.carve((char*)c->ws.p, R, S);
  // (pageable source: the copy is staged before the call returns)
  HIP_TRY(hipMemcpyAsync(W.src, hs.data(), sizeof(TopnSrc) * (size_t)R,
                         hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemsetAsync(c->d_err, 0, sizeof(int), st));
  HIP_TRY(hipMemsetAsync(W.flags, 0, sizeof(int) * 4, st));
  hipLaunchKernelGGL(k_topn_series, dim3(blocks_for(S, 256)), dim3(256), 0, st,
                     (int)R, (const TopnSrc*)W.src, S, (int)ts->function, W.sres,
                     W.sp0, W.slen, W.numbered);
  hipLaunchKernelGGL(k_scan, dim3(1), dim3(1024), 0, st, S,
                     (const int64_t*)W.slen, W.soff);
  hipLaunchKernelGGL(k_scan, dim3(1), dim3(1024), 0, st, S,
                     (const int64_t*)W.numbered, W.nrank);
  hipLaunchKernelGGL(k_topn_members, dim3(blocks_for(S, 256)), dim3(256), 0, st,
                     S, (const int64_t*)W.numbered, (const int64_t*)W.nrank,
                     W.members);
  hipLaunchKernelGGL(k_topn_init, dim3(blocks_for(S, 256)), dim3(256), 0, st, S,
                     W.maxl, W.maxd, W.marks);
  HIP_TRY(hipGetLastError());
  return OTSDB_OK;
}

// keys -> stable sort -> pick -> offsets -> report -> gather; ONE
// synchronisation, then picked / key / n_picked from the mapped block.
// Returns with c->h_topn read; the status of the call's end.
otsdb_status topn_select(otsdb_ctx* c, const otsdb_topn_spec* ts, int64_t S,
                         TopnWork& W, bool grid, otsdb_topn_result* out) {
  hipStream_t st = c->stream;
  const int fn = ts->function;
  const int64_t n_out = std::min<int64_t>(ts->topn, S);
  const int64_t* n_dev = W.nrank + S;
  size_t t_pairs = 0;
  HIP_TRY(rocprim::radix_sort_pairs(nullptr, t_pairs, (const uint64_t*)nullptr,
                                    (uint64_t*)nullptr, (const int32_t*)nullptr,
                                    (int32_t*)nullptr, (size_t)S, 0u, 64u, st));
  // (the general path's sorts are done with this buffer: stream order)
  otsdb_status rc = c->dec_ws.ensure(t_pairs + 256);
  if (rc) return rc;
  hipLaunchKernelGGL(k_topn_keys, dim3(blocks_for(S, 256)), dim3(256), 0, st, fn,
                     S, n_dev, (const long long*)W.marks,
                     (const long long*)W.maxl,
                     (const unsigned long long*)W.maxd, W.sk_in, W.keybits,
                     W.slot_in);
  HIP_TRY(rocprim::radix_sort_pairs(c->dec_ws.p, t_pairs,
                                    (const uint64_t*)W.sk_in, W.sk_out,
                                    (const int32_t*)W.slot_in, W.slot_out,
                                    (size_t)S, 0u, 64u, st));
  hipLaunchKernelGGL(k_topn_pick, dim3(blocks_for(n_out, 256)), dim3(256), 0, st,
                     n_out, (int64_t)ts->topn, n_dev,
                     (const int32_t*)W.slot_out, (const int64_t*)W.keybits,
                     (const int64_t*)W.members, (const int64_t*)W.slen,
                     W.picked, W.pcount, c->d_topn);
  hipLaunchKernelGGL(k_scan, dim3(1), dim3(1024), 0, st, n_out,
                     (const int64_t*)W.pcount, out->series.offsets);
  hipLaunchKernelGGL(k_topn_done, dim3(1), dim3(64), 0, st, n_out,
                     (const int64_t*)out->series.offsets, (const int*)c->d_err,
                     (const int*)W.flags, (const long long*)W.marks, c->d_topn);
  // (a series that does not fit the capacity is not copied)
  hipLaunchKernelGGL(k_topn_gather, dim3(blocks_for(n_out, 4)), dim3(256), 0, st,
                     n_out, (const int64_t*)W.picked, (const TopnSrc*)W.src,
                     (const int32_t*)W.sres, (const int64_t*)W.sp0,
                     (const int64_t*)out->series.offsets, out->series.capacity,
                     out->series.ts, out->series.val, out->series.is_int);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(st));
  const int64_t* H = c->h_topn;
  const int flags = (int)__atomic_load_n(&H[TOPN_H_FLAGS], __ATOMIC_ACQUIRE);
  if (grid && (flags & TOPN_F_MISS)) return OTSDB_OK;  // the caller re-runs
  if ((rc = topn_status((int)H[TOPN_H_ERR]))) return rc;
  if (H[TOPN_H_N] == 0) {  // nothing numbered: nothing picked
    out->n_picked = 0;
    return OTSDB_OK;
  }
  if (!(flags & TOPN_F_EMITTED))
    return fail(OTSDB_E_ILLEGAL_STATE,
                "top-N: no data point inside the window (the reference ends "
                "in a NullPointerException, HighestMax.java:139)");
  const int64_t k = H[TOPN_H_NPICK];
  if (out->picked) memcpy(out->picked, H + TOPN_HDR, 8 * (size_t)k);
  if (out->key) memcpy(out->key, H + TOPN_HDR + n_out, 8 * (size_t)k);
  out->n_picked = k;
  c->h_small[1] = H[TOPN_H_TOTAL];
  if (H[TOPN_H_TOTAL] > out->series.capacity) {
    c->result_short = true;
    return fail(OTSDB_E_CAPACITY, "result capacity %lld < %lld points",
                (long long)out->series.capacity, (long long)H[TOPN_H_TOTAL]);
  }
  return OTSDB_OK;
}

// The general path (topn.hip): any input.  Three synchronisations before the
// last (the point count, the candidate count, the emission count).
otsdb_status topn_general(otsdb_ctx* c, const otsdb_topn_spec* ts, int64_t S,
                          TopnWork& W, otsdb_topn_result* out) {
  hipStream_t st = c->stream;
  const int fn = ts->function;
  HIP_TRY(hipMemcpyAsync(&c->h_small[2], W.soff + S, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(&c->h_small[3], W.nrank + S, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  const int64_t N = c->h_small[2], n = c->h_small[3];
  if (N >= ((int64_t)1 << 32))
    return fail(OTSDB_E_UNSUPPORTED, "top-N (general path) over %lld points",
                (long long)N);
  int64_t E = 0;
  if (n > 0) {
    const int end_bit =
        kOccBits +
        std::max(1, 64 - __builtin_clzll((uint64_t)std::max<int64_t>(ts->end_ms, 1)));
    int64_t *cts, *cval;
    uint8_t* cflt;
    uint64_t *kin, *kout, *kuniq;
    unsigned long long* d_cnt;
    auto carve2 = [&](char* base) {
      Carve cv{base};
      cts = cv.take<int64_t>(N + 1);
      cval = cv.take<int64_t>(N + 1);
      cflt = cv.take<uint8_t>(N + 1);
      kin = cv.take<uint64_t>(N + 1);
      kout = cv.take<uint64_t>(N + 1);
      kuniq = cv.take<uint64_t>(N + 1);
      d_cnt = cv.take<unsigned long long>(1);
      return cv.off + 256;
    };
    otsdb_status rc = c->ws2.ensure(carve2(nullptr));
    if (rc) return rc;
    carve2((char*)c->ws2.p);
    hipLaunchKernelGGL(k_topn_concat, dim3(blocks_for(S, 4)), dim3(256), 0, st,
                       S, ts->start_ms, (const TopnSrc*)W.src,
                       (const int32_t*)W.sres, (const int64_t*)W.sp0,
                       (const int64_t*)W.soff, cts, cval, cflt, W.lo, W.hi,
                       W.marks, c->d_err);
    Params P{};
    P.start_ms = ts->start_ms;
    P.end_ms = ts->end_ms;
    P.interp = OTSDB_INTERP_LERP;
    RawView V;
    V.ts = cts;
    V.val = cval;
    V.is_float = cflt;
    V.series_float = nullptr;
    V.all_double = 0;
    V.lo = W.lo;
    V.hi = W.hi;
    hipLaunchKernelGGL(k_raw_cand_count, dim3(blocks_for(n, 256)), dim3(256), 0,
                       st, P, V, n, (const int64_t*)W.members, W.ccount);
    hipLaunchKernelGGL(k_scan, dim3(1), dim3(1024), 0, st, n,
                       (const int64_t*)W.ccount, W.coff);
    HIP_TRY(hipMemcpyAsync(&c->h_small[2], W.coff + n, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const int64_t C = c->h_small[2];
    if (C < 0 || C > N)
      return fail(OTSDB_E_DEVICE, "internal: %lld candidates", (long long)C);
    if (C > 0) {
      // the device sorts' scratch, sized for this call's C candidates
      size_t t_sort = 0, t_uniq = 0;
      HIP_TRY(rocprim::radix_sort_keys(nullptr, t_sort, (const uint64_t*)nullptr,
                                       (uint64_t*)nullptr, (size_t)C, 0u,
                                       (unsigned)end_bit, st));
      HIP_TRY(rocprim::unique(nullptr, t_uniq, (const uint64_t*)nullptr,
                              (uint64_t*)nullptr, (unsigned long long*)nullptr,
                              (size_t)C, rocprim::equal_to<uint64_t>(), st));
      const size_t tmp_bytes = std::max(t_sort, t_uniq) + 256;
      rc = c->dec_ws.ensure(tmp_bytes);
      if (rc) return rc;
      void* tmp = c->dec_ws.p;
      hipLaunchKernelGGL(k_raw_cand_fill, dim3(blocks_for(n, 4)), dim3(256), 0,
                         st, P, V, n, (const int64_t*)W.members,
                         (const int64_t*)W.coff, kin, c->d_err);
      size_t tb = tmp_bytes;
      HIP_TRY(rocprim::radix_sort_keys(tmp, tb, (const uint64_t*)kin, kout,
                                       (size_t)C, 0u, (unsigned)end_bit, st));
      tb = tmp_bytes;
      HIP_TRY(rocprim::unique(tmp, tb, (const uint64_t*)kout, kuniq, d_cnt,
                              (size_t)C, rocprim::equal_to<uint64_t>(), st));
      HIP_TRY(hipMemcpyAsync(&c->h_small[2], d_cnt, 8, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      E = c->h_small[2];
    }
    if (E > 0) {
      hipLaunchKernelGGL(k_topn_eval, dim3(blocks_for(E, 256)), dim3(256), 0, st,
                         P, V, fn, n, (const int64_t*)W.members, E,
                         (const uint64_t*)kuniq, W.maxl, W.maxd, W.marks,
                         c->d_err);
      if (fn == OTSDB_TOPN_HIGHEST_CURRENT)
        hipLaunchKernelGGL(k_topn_current, dim3(2), dim3(kTopnRound), 0, st, P,
                           V, n, (const int64_t*)W.members,
                           (const uint64_t*)kuniq, (const long long*)W.marks,
                           (int64_t*)W.maxl, (int64_t*)W.maxd, c->d_err);
    }
  }
  return topn_select(c, ts, S, W, false, out);
}

// The grid path (topn.hip) applies: a promise, a window of at most
// kTopnGridCap buckets, a count table under 1 GiB.
bool topn_grid_plan(const otsdb_topn_spec* ts, int64_t S, TopnGrid* Q,
                    int64_t* tiles) {
  const int64_t iv = ts->grid_interval_ms;
  if (iv <= 0 || ts->end_ms < ts->start_ms) return false;
  const int64_t r = ts->start_ms % iv;
  if (r && ts->start_ms > INT64_MAX - iv) return false;
  Q->iv = iv;
  Q->start_ms = ts->start_ms;
  Q->gbase = r ? ts->start_ms + (iv - r) : ts->start_ms;
  Q->NB = ts->end_ms >= Q->gbase ? (ts->end_ms - Q->gbase) / iv + 1 : 0;
  if (Q->NB < 1 || Q->NB > kTopnGridCap) return false;
  *tiles = (S + kTopnTile - 1) / kTopnTile;
  return (double)*tiles * (double)(Q->NB + 1) * 4.0 <= (double)(1 << 30);
}

// Enqueues the whole grid path; *missed: the promise did not hold (nothing
// of `out` is to be trusted; the general path runs).  One synchronisation.
otsdb_status topn_grid(otsdb_ctx* c, const otsdb_topn_spec* ts, int64_t S,
                       const TopnGrid& Q, int64_t tiles, TopnWork& W,
                       otsdb_topn_result* out, bool* missed) {
  hipStream_t st = c->stream;
  const bool fmax = ts->function == OTSDB_TOPN_HIGHEST_MAX;
  const int64_t words = (Q.NB + 63) / 64;
  unsigned long long* bitmap;
  int32_t* table = nullptr;
  auto carve = [&](char* base) {
    Carve cv{base};
    bitmap = cv.take<unsigned long long>(words + 1);
    if (fmax) table = cv.take<int32_t>(tiles * (Q.NB + 1));
    return cv.off + 256;
  };
  otsdb_status rc = c->ws2.ensure(carve(nullptr));
  if (rc) return rc;
  const size_t bytes = carve((char*)c->ws2.p) - 256;
  HIP_TRY(hipMemsetAsync(c->ws2.p, 0, bytes, st));
  const int64_t* n_dev = W.nrank + S;
  hipLaunchKernelGGL(k_topn_grid_scan, dim3(blocks_for(S, 4)), dim3(256), 0, st,
                     Q, S, n_dev, (const int64_t*)W.members,
                     (const TopnSrc*)W.src, (const int32_t*)W.sres,
                     (const int64_t*)W.sp0, (const int64_t*)W.slen, bitmap,
                     W.lo, W.fb, W.lb, table, W.flags);
  hipLaunchKernelGGL(k_topn_grid_last, dim3(blocks_for(words, 256)), dim3(256),
                     0, st, words, (const unsigned long long*)bitmap, W.marks);
  if (fmax) {
    hipLaunchKernelGGL(k_topn_grid_tiles, dim3(blocks_for(Q.NB + 1, 256)),
                       dim3(256), 0, st, Q.NB, tiles, table);
    hipLaunchKernelGGL(k_topn_grid_rows, dim3(blocks_for(tiles, 4)), dim3(256),
                       0, st, Q.NB, tiles, table);
    hipLaunchKernelGGL(k_topn_grid_max, dim3(blocks_for(S, 4)), dim3(256), 0, st,
                       Q, S, n_dev, (const int64_t*)W.members,
                       (const TopnSrc*)W.src, (const int32_t*)W.sres,
                       (const int64_t*)W.sp0, (const int64_t*)W.slen,
                       (const unsigned long long*)bitmap, (const int64_t*)W.lo,
                       (const int32_t*)W.fb, (const int32_t*)W.lb,
                       (const int32_t*)table, W.maxd, c->d_err);
  } else {
    hipLaunchKernelGGL(k_topn_grid_current, dim3(1), dim3(kTopnRound), 0, st, Q,
                       n_dev, (const int64_t*)W.members, (const TopnSrc*)W.src,
                       (const int32_t*)W.sres, (const int64_t*)W.sp0,
                       (const int64_t*)W.slen, (const int64_t*)W.lo,
                       (const int32_t*)W.fb, (const int32_t*)W.lb,
                       (const long long*)W.marks, (int64_t*)W.maxd, c->d_err);
  }
  rc = topn_select(c, ts, S, W, true, out);
  *missed = (c->h_topn[TOPN_H_FLAGS] & TOPN_F_MISS) != 0;
  return rc;
}

// `res`: device pointers; out->series: device pointers; out->picked /
// out->key: host.  The grid path where the caller's promise allows it (one
// synchronisation), the general path otherwise or after a missed promise.
otsdb_status run_topn_impl(otsdb_ctx* c, const otsdb_topn_spec* ts, int32_t R,
                           const otsdb_result* res, const int64_t* n_groups,
                           int64_t S, otsdb_topn_result* out) {
  hipStream_t st = c->stream;
  c->n_topn_grid = c->n_topn_general = c->n_topn_miss = 0;
  out->n_picked = 0;
  c->result_short = false;
  c->h_small[1] = 0;  // the picked series' points (the host entry reads it)
  if (S == 0) {  // no series: nothing picked (HighestMax.java:45-47)
    HIP_TRY(hipMemsetAsync(out->series.offsets, 0, sizeof(int64_t), st));
    HIP_TRY(hipStreamSynchronize(st));
    return OTSDB_OK;
  }
  StageTimer tm(c, 13);
  const int64_t n_out = std::min<int64_t>(ts->topn, S);
  otsdb_status rc = topn_host_block(c, n_out);
  if (rc) return rc;
  TopnWork W;
  TopnGrid Q;
  int64_t tiles = 0;
  if (topn_grid_plan(ts, S, &Q, &tiles)) {
    if ((rc = topn_number(c, ts, R, res, n_groups, S, W))) return rc;
    bool missed = false;
    c->n_topn_grid = 1;
    rc = topn_grid(c, ts, S, Q, tiles, W, out, &missed);
    if (rc || !missed) return rc;
    c->n_topn_miss = 1;
    out->n_picked = 0;
    if ((rc = topn_host_block(c, n_out))) return rc;
  }
  c->n_topn_general = 1;
  if ((rc = topn_number(c, ts, R, res, n_groups, S, W))) return rc;
  return topn_general(c, ts, S, W, out);
}

}  // namespace

// =========================================================================
// C-ABI
// =========================================================================
extern "C" {

int otsdb_abi_version(void) { return OTSDB_ABI_VERSION; }

const char* otsdb_last_error(void) { return g_last_error.c_str(); }

otsdb_status otsdb_ctx_create(int device, otsdb_ctx** out) {
  if (!out) return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null out");
  *out = nullptr;
  int n = 0;
  HIP_TRY(hipGetDeviceCount(&n));
  if (device < 0 || device >= n)
    return fail(OTSDB_E_DEVICE, "no HIP device %d (have %d)", device, n);
  HIP_TRY(hipSetDevice(device));
  otsdb_ctx* c = new otsdb_ctx();
  c->device = device;
  // a blocking stream: ordered with the legacy default stream torch uses,
  // so tensors torch writes are complete before this context reads them
  HIP_TRY(hipStreamCreate(&c->stream));
  HIP_TRY(hipMalloc(&c->d_err, 256));
  HIP_TRY(hipMemset(c->d_err, 0, 256));
  c->d_mm = (unsigned long long*)((char*)c->d_err + 64);
  HIP_TRY(hipHostMalloc(&c->h_small, 64));
  HIP_TRY(hipHostMalloc(&c->h_done, 64,
                        hipHostMallocMapped | hipHostMallocCoherent));
  HIP_TRY(hipHostGetDevicePointer((void**)&c->d_done, c->h_done, 0));
  for (int i = 0; i < 8; ++i) c->h_done[i] = 0;
  *out = c;
  return OTSDB_OK;
}

void otsdb_ctx_destroy(otsdb_ctx* c) {
  if (!c) return;
  hipSetDevice(c->device);
  if (c->stream) hipStreamSynchronize(c->stream);
  for (auto e : c->ev_pool) hipEventDestroy(e);
  if (c->d_err) hipFree(c->d_err);
  if (c->d_merr) hipFree(c->d_merr);
  if (c->h_mdone) hipHostFree(c->h_mdone);
  if (c->h_small) hipHostFree(c->h_small);
  if (c->h_done) hipHostFree(c->h_done);
  if (c->h_topn) hipHostFree(c->h_topn);
  if (c->stream) hipStreamDestroy(c->stream);
  delete c;  // the device buffers free themselves (DevBuf)
}

otsdb_status otsdb_agg_lookup(const char* name, int32_t* agg_id) {
  if (!name || !agg_id) return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null");
  for (int i = 0; i < OTSDB_AGG_COUNT_IDS; ++i)
    if (strcmp(kAggs[i].key, name) == 0) {
      *agg_id = i;
      return OTSDB_OK;
    }
  return fail(OTSDB_E_NO_SUCH_ELEMENT, "No such aggregator: %s", name);
}

const char* otsdb_agg_name(int32_t agg_id) {
  if (agg_id < 0 || agg_id >= OTSDB_AGG_COUNT_IDS) return nullptr;
  return kAggs[agg_id].name;
}

int32_t otsdb_agg_interpolation(int32_t agg_id) {
  if (agg_id < 0 || agg_id >= OTSDB_AGG_COUNT_IDS) return -1;
  return kAggs[agg_id].interp;
}

otsdb_status otsdb_agg_plan(otsdb_ctx* c, const otsdb_query_spec* spec,
                            const otsdb_batch* b, otsdb_sizes* out) {
  if (!spec || !b || !out) return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null");
  otsdb_status rc = check_spec(spec);
  if (rc) return rc;
  AnchoredPlan A;
  if (anchored(spec)) {  // stage B's union grid
    rc = plan_anchored(spec, &A);
    if (rc) return rc;
    spec = &A.derived;
  }
  Params P;
  rc = make_params(spec, &P);
  if (rc) return rc;
  if (!(spec->ds_interval_ms > 0 || spec->run_all)) {
    // raw: every emitted timestamp is a point of some member span, so the
    // batch's point count bounds the output when each span is in one group
    out->n_buckets = 0;
    out->max_out_points = b->n_points;
    out->workspace_bytes = b->n_series * 16 + b->n_points * (spec->rate ? 48 : 32);
    return OTSDB_OK;
  }
  out->n_buckets = P.nb;
  out->max_out_points = b->n_groups * P.nb;
  // Under NONE fill a group emits only at buckets its members have points in:
  // at most n_points per group, whatever the grid and however many groups a
  // series is listed in.  The bound holds for every NONE-fill grid; it is
  // applied past 4e9 series x buckets, where groups x buckets of the window
  // as given is no size a caller can allocate (the host entries stage their
  // results by it), and every smaller plan stays as it was.
  if (!P.run_all && !P.fill && (double)b->n_series * (double)P.nb > 4.0e9)
    out->max_out_points =
        std::min(out->max_out_points, b->n_groups * b->n_points);
  out->workspace_bytes =
      b->n_series * (P.nb * 9 + 48) + b->n_groups * (P.nb * 9 + 8);
  return OTSDB_OK;
}

otsdb_status otsdb_agg_run_device(otsdb_ctx* c, const otsdb_query_spec* spec,
                                  const otsdb_batch* b, otsdb_result* out,
                                  void* hip_stream) {
  if (!c || !spec || !b || !out) return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null");
  DeviceCall dc(c, b, hip_stream);
  return dc.rc ? dc.rc : run_device_impl(c, spec, b, out, dc.goff);
}

otsdb_status otsdb_agg_run_cells_device(otsdb_ctx* c,
                                        const otsdb_query_spec* spec,
                                        const otsdb_cells* cells,
                                        const otsdb_batch* b,
                                        otsdb_result* out, void* hip_stream) {
  if (!c || !spec || !cells || !b || !out)
    return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null");
  DeviceCall dc(c, b, hip_stream);
  return dc.rc ? dc.rc : run_cells_impl(c, spec, cells, b, out, dc.goff);
}

// The host-pointer entries: the batch staged in HBM once, n results (q: the
// multi-aggregator or panel request whose results `outs` are, null: one
// single query; roll: that single query over rollup cells, roll->cnt on the
// host and staged beside the batch when its state reads it).
static otsdb_status run_host(otsdb_ctx* c, const otsdb_query_spec* spec,
                             const otsdb_batch* b, int n, otsdb_result* outs,
                             const Req* q, const Rollup* roll = nullptr) {
  CtxLock lk(c);
  HIP_TRY(hipSetDevice(c->device));
  std::vector<int64_t> goff;
  otsdb_status rc = read_goff(c, b, false, goff);
  if (rc) return rc;
  const int64_t S = b->n_series, N = b->n_points, G = b->n_groups;
  const int64_t M = goff.back();
  if (S < 0 || N < 0) return fail(OTSDB_E_ILLEGAL_ARGUMENT, "negative sizes");
  if (S > 0 && b->offsets[S] != N)
    return fail(OTSDB_E_ILLEGAL_ARGUMENT, "offsets[S] != n_points");
  for (int64_t m = 0; m < M; ++m)
    if (b->group_members[m] < 0 || b->group_members[m] >= S)
      return fail(OTSDB_E_ILLEGAL_ARGUMENT, "group member out of range");
  // staging layout in HBM
  auto carve = [&](char* base) {
    Carve cv{base};
    std::vector<void*> p(8 + 4 * (size_t)n);
    p[7 + 4 * n] = roll && roll->cnt ? cv.take<int64_t>(N + 1) : nullptr;
    p[0] = cv.take<int64_t>(S + 1);
    p[1] = cv.take<int64_t>(N + 1);
    p[2] = cv.take<int64_t>(N + 1);
    p[3] = b->is_float ? cv.take<uint8_t>(N + 1) : nullptr;
    p[4] = b->series_float ? cv.take<uint8_t>(S + 1) : nullptr;
    p[5] = cv.take<int64_t>(G + 1);
    p[6] = cv.take<int64_t>(M + 1);
    for (int i = 0; i < n; ++i) {
      const int64_t cap = outs[i].capacity;
      p[7 + 4 * i] = cv.take<int64_t>(G + 1);
      p[8 + 4 * i] = cv.take<int64_t>(cap + 1);
      p[9 + 4 * i] = cv.take<int64_t>(cap + 1);
      p[10 + 4 * i] = cv.take<uint8_t>(cap + 1);
    }
    return std::make_pair(cv.off + 256, p);
  };
  const size_t need = carve(nullptr).first;
  rc = c->stage.ensure(need);
  if (rc) return rc;
  auto pp = carve((char*)c->stage.p).second;
  hipStream_t st = c->stream;
  auto h2d = [&](void* d, const void* h, size_t n) -> otsdb_status {
    if (n && h) HIP_TRY(hipMemcpyAsync(d, h, n, hipMemcpyHostToDevice, st));
    return OTSDB_OK;
  };
  if ((rc = h2d(pp[0], b->offsets, 8 * (S + 1)))) return rc;
  if ((rc = h2d(pp[1], b->ts_ms, 8 * N))) return rc;
  if ((rc = h2d(pp[2], b->val, 8 * N))) return rc;
  if (b->is_float && (rc = h2d(pp[3], b->is_float, N))) return rc;
  if (b->series_float && (rc = h2d(pp[4], b->series_float, S))) return rc;
  if ((rc = h2d(pp[5], b->group_offsets, 8 * (G + 1)))) return rc;
  if ((rc = h2d(pp[6], b->group_members, 8 * M))) return rc;
  if (roll && (rc = h2d(pp[7 + 4 * n], roll->cnt, 8 * N))) return rc;
  otsdb_batch db = *b;
  db.offsets = (const int64_t*)pp[0];
  db.ts_ms = (const int64_t*)pp[1];
  db.val = (const int64_t*)pp[2];
  db.is_float = (const uint8_t*)pp[3];
  db.series_float = (const uint8_t*)pp[4];
  db.group_offsets = (const int64_t*)pp[5];
  db.group_members = (const int64_t*)pp[6];
  std::vector<otsdb_result> dr((size_t)n);
  for (int i = 0; i < n; ++i) {
    dr[i].capacity = outs[i].capacity;
    dr[i].offsets = (int64_t*)pp[7 + 4 * i];
    dr[i].ts = (int64_t*)pp[8 + 4 * i];
    dr[i].val = (int64_t*)pp[9 + 4 * i];
    dr[i].is_int = (uint8_t*)pp[10 + 4 * i];
  }
  c->result_short = false;
  const bool many = q != nullptr;
  if (many) {
    Req dq = *q;
    dq.outs = dr.data();
    rc = dq.ds ? run_panel_impl(c, spec, dq, &db, goff)
               : run_multi_impl(c, spec, dq, &db, goff);
  } else if (roll) {
    const Rollup dro{roll->agg, (const int64_t*)pp[7 + 4 * n]};
    rc = run_rollup_impl(c, spec, &db, dro, &dr[0], goff);
  } else {
    rc = run_device_impl(c, spec, &db, &dr[0], goff);
  }
  if (rc == OTSDB_E_CAPACITY && c->result_short) {
    // the offsets of the result too small (and of those before it) are whole
    const int last = many ? c->multi_failed : 0;
    for (int i = 0; i < last; ++i)
      copy_offsets_back(c, &outs[i], dr[i].offsets, G, rc);
    return copy_offsets_back(c, &outs[last], dr[last].offsets, G, rc);
  }
  if (rc) return rc;
  for (int i = 0; i < n; ++i) {
    const int64_t total = many ? c->multi_total[i] : c->h_small[1];
    otsdb_result* out = &outs[i];
    HIP_TRY(hipMemcpyAsync(out->offsets, dr[i].offsets, 8 * (G + 1),
                           hipMemcpyDeviceToHost, st));
    if (total > 0) {
      HIP_TRY(hipMemcpyAsync(out->ts, dr[i].ts, 8 * total, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipMemcpyAsync(out->val, dr[i].val, 8 * total, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipMemcpyAsync(out->is_int, dr[i].is_int, total, hipMemcpyDeviceToHost, st));
    }
  }
  HIP_TRY(hipStreamSynchronize(st));
  return OTSDB_OK;
}

otsdb_status otsdb_agg_run(otsdb_ctx* c, const otsdb_query_spec* spec,
                           const otsdb_batch* b, otsdb_result* out) {
  if (!c || !spec || !b || !out) return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null");
  return run_host(c, spec, b, 1, out, nullptr);
}

otsdb_status otsdb_agg_run_rollup_device(otsdb_ctx* c,
                                         const otsdb_query_spec* spec,
                                         const otsdb_batch* b,
                                         int32_t rollup_agg_id,
                                         const int64_t* value_count,
                                         otsdb_result* out, void* hip_stream) {
  if (!c || !spec || !b || !out) return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null");
  const Rollup r{rollup_agg_id, value_count};
  RollupKind kind;
  const otsdb_status rc = check_rollup(spec, r, &kind);
  if (rc) return rc;
  DeviceCall dc(c, b, hip_stream);
  return dc.rc ? dc.rc : run_rollup_impl(c, spec, b, r, out, dc.goff);
}

otsdb_status otsdb_agg_run_rollup(otsdb_ctx* c, const otsdb_query_spec* spec,
                                  const otsdb_batch* b, int32_t rollup_agg_id,
                                  const int64_t* value_count,
                                  otsdb_result* out) {
  if (!c || !spec || !b || !out) return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null");
  Rollup r{rollup_agg_id, value_count};
  RollupKind kind;
  const otsdb_status rc = check_rollup(spec, r, &kind);
  if (rc) return rc;
  if (kind != ROLLUP_AVG) r.cnt = nullptr;  // ignored: nothing to stage
  return run_host(c, spec, b, 1, out, nullptr, &r);
}

// otsdb_agg_plan_multi's bound of a call's workspace: the downsampler's rows
// and one class matrix, every output's dense results and one tile partial
// per distinct reduction state
static int64_t multi_workspace_bytes(const otsdb_batch* b, int64_t nb,
                                     int64_t n_out) {
  return b->n_series * (nb * 18 + 48) +
         (n_out + 1) * b->n_groups * (nb * 9 + 8) +
         (int64_t)kMultiSlots * (b->n_series / kChunk + b->n_groups) * nb * 33;
}

otsdb_status otsdb_agg_plan_multi(otsdb_ctx* c, const otsdb_query_spec* spec,
                                  int32_t n_out, const int32_t* agg_ids,
                                  const int32_t* interps, const otsdb_batch* b,
                                  otsdb_sizes* out) {
  if (!spec || !b || !out) return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null");
  const Req q{n_out, nullptr, agg_ids, interps, nullptr};
  otsdb_status rc = check_req(spec, q);
  if (rc) return rc;
  const otsdb_query_spec s0 = req_spec(spec, q, 0);
  rc = otsdb_agg_plan(c, &s0, b, out);
  if (rc) return rc;
  // the bound of the point count holds for each output
  if (s0.ds_interval_ms > 0 || s0.run_all)
    out->workspace_bytes = multi_workspace_bytes(b, out->n_buckets, n_out);
  return OTSDB_OK;
}

otsdb_status otsdb_agg_run_multi_device(otsdb_ctx* c,
                                        const otsdb_query_spec* spec,
                                        int32_t n_out, const int32_t* agg_ids,
                                        const int32_t* interps,
                                        const otsdb_batch* b,
                                        otsdb_result* outs, void* hip_stream) {
  if (!c || !spec || !b || !outs) return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null");
  const Req q{n_out, nullptr, agg_ids, interps, outs};
  otsdb_status rc = check_req(spec, q);
  if (rc) return rc;
  DeviceCall dc(c, b, hip_stream);
  return dc.rc ? dc.rc : run_multi_impl(c, spec, q, b, dc.goff);
}

otsdb_status otsdb_agg_run_multi(otsdb_ctx* c, const otsdb_query_spec* spec,
                                 int32_t n_out, const int32_t* agg_ids,
                                 const int32_t* interps, const otsdb_batch* b,
                                 otsdb_result* outs) {
  if (!c || !spec || !b || !outs) return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null");
  const Req q{n_out, nullptr, agg_ids, interps, outs};
  const otsdb_status rc = check_req(spec, q);
  if (rc) return rc;
  return run_host(c, spec, b, n_out, outs, &q);
}

otsdb_status otsdb_agg_plan_panel(otsdb_ctx* c, const otsdb_query_spec* spec,
                                  int32_t n_out, const int32_t* ds_agg_ids,
                                  const int32_t* agg_ids,
                                  const int32_t* interps, const otsdb_batch* b,
                                  otsdb_sizes* out) {
  if (!spec || !b || !out) return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null");
  const Req q{n_out, ds_agg_ids, agg_ids, interps, nullptr};
  otsdb_status rc = check_req(spec, q, /*panel=*/true);
  if (rc) return rc;
  const otsdb_query_spec s0 = req_spec(spec, q, 0);
  rc = otsdb_agg_plan(c, &s0, b, out);
  if (rc) return rc;
  // the bound of the point count holds for each output; the workspace: per
  // distinct function what plan_multi counts for its outputs (at most n_out
  // functions of one output each)
  if (s0.ds_interval_ms > 0 || s0.run_all)
    out->workspace_bytes = n_out * multi_workspace_bytes(b, out->n_buckets, 1);
  return OTSDB_OK;
}

otsdb_status otsdb_agg_run_panel_device(otsdb_ctx* c,
                                        const otsdb_query_spec* spec,
                                        int32_t n_out,
                                        const int32_t* ds_agg_ids,
                                        const int32_t* agg_ids,
                                        const int32_t* interps,
                                        const otsdb_batch* b,
                                        otsdb_result* outs, void* hip_stream) {
  if (!c || !spec || !b || !outs) return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null");
  const Req q{n_out, ds_agg_ids, agg_ids, interps, outs};
  otsdb_status rc = check_req(spec, q, /*panel=*/true);
  if (rc) return rc;
  DeviceCall dc(c, b, hip_stream);
  return dc.rc ? dc.rc : run_panel_impl(c, spec, q, b, dc.goff);
}

otsdb_status otsdb_agg_run_panel(otsdb_ctx* c, const otsdb_query_spec* spec,
                                 int32_t n_out, const int32_t* ds_agg_ids,
                                 const int32_t* agg_ids, const int32_t* interps,
                                 const otsdb_batch* b, otsdb_result* outs) {
  if (!c || !spec || !b || !outs) return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null");
  const Req q{n_out, ds_agg_ids, agg_ids, interps, outs};
  const otsdb_status rc = check_req(spec, q, /*panel=*/true);
  if (rc) return rc;
  return run_host(c, spec, b, n_out, outs, &q);
}

otsdb_status otsdb_agg_run_cells_multi_device(
    otsdb_ctx* c, const otsdb_query_spec* spec, int32_t n_out,
    const int32_t* agg_ids, const int32_t* interps, const otsdb_cells* cells,
    const otsdb_batch* b, otsdb_result* outs, void* hip_stream) {
  if (!c || !spec || !cells || !b || !outs)
    return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null");
  const Req q{n_out, nullptr, agg_ids, interps, outs};
  otsdb_status rc = check_req(spec, q);
  if (rc) return rc;
  DeviceCall dc(c, b, hip_stream);
  return dc.rc ? dc.rc : run_cells_req(c, spec, q, cells, b, dc.goff);
}

otsdb_status otsdb_agg_run_cells_panel_device(
    otsdb_ctx* c, const otsdb_query_spec* spec, int32_t n_out,
    const int32_t* ds_agg_ids, const int32_t* agg_ids, const int32_t* interps,
    const otsdb_cells* cells, const otsdb_batch* b, otsdb_result* outs,
    void* hip_stream) {
  if (!c || !spec || !cells || !b || !outs)
    return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null");
  const Req q{n_out, ds_agg_ids, agg_ids, interps, outs};
  otsdb_status rc = check_req(spec, q, /*panel=*/true);
  if (rc) return rc;
  DeviceCall dc(c, b, hip_stream);
  return dc.rc ? dc.rc : run_cells_panel_impl(c, spec, q, cells, b, dc.goff);
}

otsdb_status otsdb_agg_partials_multi_device(
    otsdb_ctx* c, const otsdb_query_spec* spec, int32_t n_out,
    const int32_t* agg_ids, const int32_t* interps, const otsdb_batch* b,
    otsdb_partial* partials, uint8_t* emit, void* hip_stream) {
  if (!c || !spec || !b || !partials || !emit)
    return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null");
  const Req q{n_out, nullptr, agg_ids, interps, nullptr};
  otsdb_status rc = check_multi_partials(spec, q);
  if (rc) return rc;
  DeviceCall dc(c, b, hip_stream);
  if (dc.rc) return dc.rc;
  std::vector<int64_t>& goff = dc.goff;
  const otsdb_query_spec s0 = req_spec(spec, q, 0);
  Params P;
  rc = partials_grid(c, &s0, b, &P);
  if (rc) return rc;
  c->multi_failed = -1;
  multi_counters(c, 0, 0);
  const int64_t G = (int64_t)goff.size() - 1;
  const size_t GB = (size_t)G * P.nb;
  // (a misaligned batch: the single path reports it)
  if (misaligned(b) || !multi_shares_rows(spec, q, P, b->n_series, goff)) {
    // the outputs one after another through the single entry's path: every
    // one writes the same emit mask
    for (int i = 0; i < q.n; ++i) {
      const otsdb_query_spec si = req_spec(spec, q, i);
      rc = partials_locked(c, &si, b, goff, nullptr, nullptr,
                           partials + (size_t)i * GB, emit);
      if (rc) {
        c->multi_failed = i;
        return rc;
      }
      ++c->n_multi_ds;
      ++c->n_multi_group;
    }
    return OTSDB_OK;
  }
  for (int i = 0; i < q.n; ++i)
    if (multi_kind(q.aggs[i]) == MK_ORDERED &&
        (spec->flags & OTSDB_SPEC_EXACT_ORDER))
      return fail(OTSDB_E_UNSUPPORTED,
                  "exact-order dev across ranks: hand the chains on "
                  "(otsdb_agg_partials_chained_device)");
  const BatchDev B = batch_dev(b);
  MultiState M;
  rc = multi_build(c, &s0, q, B, b->group_members, goff, P, nullptr, nullptr, M,
                   /*partial=*/true);
  if (!rc) rc = multi_partials(c, M, (Packed*)partials, emit);
  if (rc) return rc;
  int err;
  if ((rc = read_err(c, &err))) return rc;
  return (err & ERR_RATE_TS) ? rate_ts_error() : OTSDB_OK;
}

otsdb_status otsdb_agg_finalize_multi_device(
    otsdb_ctx* c, const otsdb_query_spec* spec, int32_t n_out,
    const int32_t* agg_ids, const int32_t* interps, int64_t n_groups,
    int64_t n_buckets, int32_t n_ranks, const otsdb_partial* partials,
    const uint8_t* emit, otsdb_result* outs, void* hip_stream) {
  if (!c || !spec || !outs) return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null");
  const Req q{n_out, nullptr, agg_ids, interps, outs};
  otsdb_status rc = check_multi_partials(spec, q);
  if (rc) return rc;
  if (n_groups < 0 || n_ranks < 1)
    return fail(OTSDB_E_ILLEGAL_ARGUMENT, "%lld groups of %d ranks",
                (long long)n_groups, (int)n_ranks);
  CtxLock lk(c);
  HIP_TRY(hipSetDevice(c->device));
  StreamBinding bind(c, hip_stream);
  const otsdb_query_spec s0 = req_spec(spec, q, 0);
  Params P;
  rc = make_params(&s0, &P, c);
  if (!rc && P.nb != n_buckets)
    rc = fail(OTSDB_E_ILLEGAL_ARGUMENT, "n_buckets %lld != plan %lld",
              (long long)n_buckets, (long long)P.nb);
  if (!rc && n_groups * P.nb > 0 && (!partials || !emit))
    rc = fail(OTSDB_E_ILLEGAL_ARGUMENT, "null partials");
  if (!rc) rc = multi_buffers(c);
  if (rc) return rc;
  c->multi_failed = -1;
  const int64_t G = n_groups, GB = G * P.nb;
  FinalizeArgs A{};
  A.n_out = q.n;
  double* out_val[OTSDB_MULTI_MAX];
  uint8_t* out_emit[OTSDB_MULTI_MAX];
  auto carve = [&](char* base) {
    Carve cv{base};
    for (int i = 0; i < q.n; ++i) {
      out_val[i] = cv.take<double>(GB + 1);
      out_emit[i] = cv.take<uint8_t>(GB + 1);
    }
    return cv.off + 256;
  };
  rc = c->ws.ensure(carve(nullptr));
  if (rc) return rc;
  carve((char*)c->ws.p);
  for (int i = 0; i < q.n; ++i) {
    A.slot[i] = kMultiSlotDev;  // (ordered: dev)
    with_monoid(q.aggs[i], [&](auto tag) {
      constexpr int k = MultiSlot<decltype(tag)>::value;
      if (k >= 0) A.slot[i] = k;
    });
    A.out[i] = MultiOut{out_val[i], out_emit[i], c->d_merr + i, nullptr};
  }
  HIP_TRY(hipMemsetAsync(c->d_err, 0, 2 * sizeof(int), c->stream));
  HIP_TRY(hipMemsetAsync(c->d_merr, 0, OTSDB_MULTI_MAX * sizeof(int), c->stream));
  if (GB == 0) {  // no group or no bucket: empty results (compact's zeroes)
    for (int i = 0; i < q.n && !rc; ++i)
      rc = compact(c, P, G, out_val[i], out_emit[i], nullptr, &q.outs[i]);
    c->small_ready = false;
    if (!rc) HIP_TRY(hipStreamSynchronize(c->stream));
    return rc;
  }
  hipLaunchKernelGGL(k_finalize_ranks_multi, dim3(blocks_for(GB, 256)),
                     dim3(256), 0, c->stream, GB, (int)n_ranks,
                     (const Packed*)partials, emit, A);
  HIP_TRY(hipGetLastError());
  return multi_compact_outputs(c, q, P, G, out_val, out_emit);
}

otsdb_status otsdb_agg_partials_device(otsdb_ctx* c,
                                       const otsdb_query_spec* spec,
                                       const otsdb_batch* b,
                                       otsdb_partial* partials, uint8_t* emit,
                                       void* hip_stream) {
  return partials_impl(c, spec, b, nullptr, nullptr, partials, emit,
                       hip_stream);
}

otsdb_status otsdb_agg_partials_chained_device(
    otsdb_ctx* c, const otsdb_query_spec* spec, const otsdb_batch* b,
    const otsdb_partial* init, const uint8_t* init_emit,
    otsdb_partial* partials, uint8_t* emit, void* hip_stream) {
  if (!init || !init_emit) return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null init");
  return partials_impl(c, spec, b, init, init_emit, partials, emit,
                       hip_stream);
}

otsdb_status otsdb_agg_finalize_device(otsdb_ctx* c,
                                       const otsdb_query_spec* spec,
                                       int64_t n_groups, int64_t n_buckets,
                                       int32_t n_ranks,
                                       const otsdb_partial* partials,
                                       const uint8_t* emit, otsdb_result* out,
                                       void* hip_stream) {
  if (!c || !spec || !out) return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null");
  CtxLock lk(c);
  HIP_TRY(hipSetDevice(c->device));
  StreamBinding bind(c, hip_stream);
  otsdb_status rc = check_spec(spec);
  Params P;
  if (!rc) rc = make_params(spec, &P, c);
  if (!rc && P.nb != n_buckets)
    rc = fail(OTSDB_E_ILLEGAL_ARGUMENT, "n_buckets %lld != plan %lld",
              (long long)n_buckets, (long long)P.nb);
  if (!rc) {
    const int64_t G = n_groups, GB = G * P.nb;
    double* ov;
    uint8_t* oe;
    int64_t* cnt;
    auto carve = [&](char* base) {
      Carve cv{base};
      ov = cv.take<double>(GB + 1);
      oe = cv.take<uint8_t>(GB + 1);
      cnt = cv.take<int64_t>(G + 1);
      return cv.off + 256;
    };
    rc = c->ws.ensure(carve(nullptr));
    if (!rc) {
      carve((char*)c->ws.p);
      hipMemsetAsync(c->d_err, 0, sizeof(int), c->stream);
      bool ok = true;
      if (GB > 0)
        ok = with_monoid(spec->agg_id, [&](auto tag) {
          using M = decltype(tag);
          hipLaunchKernelGGL(k_finalize_ranks<M>, dim3(blocks_for(GB, 256)),
                             dim3(256), 0, c->stream, GB, n_ranks,
                             (const Packed*)partials, emit, ov, oe, c->d_err);
        });
      if (!ok) rc = fail(OTSDB_E_UNSUPPORTED, "aggregator %d across ranks",
                         spec->agg_id);
      if (!rc) rc = compact(c, P, G, ov, oe, cnt, out);
      if (!rc) rc = finish(c, G, out);
    }
  }
  return rc;
}

// ---- cross-rank median / percentile -------------------------
otsdb_status otsdb_sel_prepare_device(otsdb_ctx* c, const otsdb_query_spec* spec,
                                      const otsdb_batch* b, int64_t* counts,
                                      uint8_t* emit, int64_t* krange,
                                      void* hip_stream) {
  if (!c || !spec || !b || !counts || !emit || !krange)
    return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null");
  DeviceCall dc(c, b, hip_stream);  // (the lock ends an earlier session)
  std::vector<int64_t>& goff = dc.goff;
  otsdb_status rc = dc.rc;
  Params P;
  if (!rc) rc = check_spec(spec);
  if (!rc && !is_selection(spec->agg_id))
    rc = fail(OTSDB_E_ILLEGAL_ARGUMENT, "otsdb_sel_* needs median/percentile");
  if (!rc && !(spec->ds_interval_ms > 0 || spec->run_all))
    rc = fail(OTSDB_E_UNSUPPORTED, "raw group-by across ranks");
  if (!rc) rc = make_params(spec, &P, c);
  if (!rc && !P.run_all && !P.fill && (double)b->n_series * (double)P.nb > 4.0e9)
    rc = fail(OTSDB_E_UNSUPPORTED, "grid trimming is not supported across ranks");
  if (!rc) {
    const BatchDev B = batch_dev(b);
    Work W;
    rc = run_pipeline(c, spec, B, b->group_members, goff, P, W, 2, nullptr,
                      nullptr);
    const int64_t G = (int64_t)goff.size() - 1, GB = G * P.nb;
    const Tiles T = tiles_of(c, G);
    if (!rc && T.LG != G)  // build_tiles(sel_all): segment = (group, bucket)
      rc = fail(OTSDB_E_DEVICE, "selection segments: %lld of %lld groups",
                (long long)T.LG, (long long)G);
    if (!rc && GB > 0) {
      if (!W.sel_fused)
        hipLaunchKernelGGL(k_dense_to_counts, dim3(blocks_for(GB, 256)),
                           dim3(256), 0, c->stream, GB, (const double*)W.out_val,
                           (const uint8_t*)W.out_emit, counts, emit);
      hipLaunchKernelGGL(k_xsel_range, dim3((unsigned)GB), dim3(256), 0,
                         c->stream, P.nb, goff.back(), T.LG, T.lg_off, T.lg_k,
                         (const uint64_t*)W.keys, (const uint64_t*)W.key_mm,
                         krange,
                         W.sel_fused ? (const uint32_t*)W.key_cnt : nullptr,
                         (const uint32_t*)W.lg_kept, counts, emit);
      HIP_TRY(hipGetLastError());
    }
    if (!rc) {
      HIP_TRY(hipMemsetAsync((char*)c->d_err + 128, 0, 32, c->stream));
      int err = 0;
      rc = read_err(c, &err);
      if (!rc && (err & ERR_RATE_TS)) rc = rate_ts_error();
    }
    if (!rc) {
      auto& S = c->sel;
      S.active = true;
      S.P = P;
      S.spec = *spec;
      S.W = W;
      S.G = G;
      S.NB = P.nb;
      S.M = goff.back();
      S.median = spec->agg_id == OTSDB_AGG_MEDIAN ? 1 : 0;
      S.next_pass = 0;
      S.more = false;
      S.pool_built = false;
      S.need_pick = false;
      S.key_reads = 0;
      S.passes = 0;
      ++S.sessions;
    }
  }
  return rc;
}

// Re-aims the session at another selection aggregator.  What the passes
// consume is rebuilt by the next pass loop itself: pass 0 rewrites the dense
// counts (W.out_val, which finish overwrote with values) from the caller's
// all-reduced counts, the XSel states and the pool bounds; pass 1 the
// candidate pool.  The keys, their per-tile min / max and W.out_emit are
// read-only after prepare and stay.
otsdb_status otsdb_sel_retarget(otsdb_ctx* c, int32_t agg_id) {
  if (!c) return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null");
  if (agg_id < 0 || agg_id >= OTSDB_AGG_COUNT_IDS || !is_selection(agg_id))
    return fail(OTSDB_E_ILLEGAL_ARGUMENT,
                "otsdb_sel_retarget needs median/percentile, not %d",
                (int)agg_id);
  CtxLock lk(c, /*keep_session=*/true);
  auto& S = c->sel;
  if (!S.active) return fail(OTSDB_E_ILLEGAL_STATE, "no selection session");
  if (S.spec.interp == OTSDB_INTERP_DEFAULT && S.spec.fill == OTSDB_FILL_NONE &&
      kAggs[agg_id].interp != kAggs[S.spec.agg_id].interp)
    return fail(OTSDB_E_ILLEGAL_ARGUMENT,
                "aggregator %d interpolates unlike the prepared %d",
                (int)agg_id, (int)S.spec.agg_id);
  S.spec.agg_id = agg_id;
  agg_params(&S.P, agg_id, S.spec.interp);
  S.median = agg_id == OTSDB_AGG_MEDIAN ? 1 : 0;
  S.next_pass = 0;
  S.more = false;
  S.pool_built = false;
  S.need_pick = false;
  S.key_reads = 0;
  S.passes = 0;
  return OTSDB_OK;
}

otsdb_status otsdb_sel_hist_device(otsdb_ctx* c, int32_t pass,
                                   const int64_t* counts, const uint8_t* emit,
                                   const int64_t* krange, uint32_t* hist_prev,
                                   uint32_t* hist_out, int32_t* more,
                                   void* hip_stream) {
  if (!c || !hist_out || !more) return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null");
  CtxLock lk(c, /*keep_session=*/true);
  auto& S = c->sel;
  if (!S.active) return fail(OTSDB_E_ILLEGAL_STATE, "no selection session");
  if (pass < 0 || pass != S.next_pass)
    return fail(OTSDB_E_ILLEGAL_STATE, "pass %d, expected %d", pass, S.next_pass);
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
  const int64_t G = S.G, NB = S.NB, GB = G * NB;
  const Tiles T = tiles_of(c, G);
  // (pass 0: every protocol word, as prepare left them — a retargeted
  // session starts from the same zeroes)
  HIP_TRY(hipMemsetAsync(xs_flags(c), 0, pass == 0 ? 32 : 4, st));
  if (pass == 0) {
    if (!counts || !emit || !krange)
      return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null counts / krange");
    if (GB > 0) {
      // the per-segment pool bookkeeping (bounds: the trailing one stays 0,
      // so the scan's last offset is the pool's size)
      size_t tmp = 0;
      HIP_TRY(rocprim::exclusive_scan(nullptr, tmp, (const int64_t*)nullptr,
                                      (int64_t*)nullptr, (int64_t)0,
                                      (size_t)(GB + 1), rocprim::plus<int64_t>(),
                                      st));
      S.scan_tmp = tmp;
      const size_t need =
          (((size_t)(GB + 1) * 16 + (size_t)GB * 4 + 255) & ~(size_t)255) + tmp;
      otsdb_status rc = S.segmem.ensure(need);
      if (rc) return rc;
      HIP_TRY(hipMemsetAsync(xs_bnd(c), 0, (size_t)(GB + 1) * 8, st));
      hipLaunchKernelGGL(k_counts_to_dense, dim3(blocks_for(GB, 256)), dim3(256),
                         0, st, GB, counts, emit, S.W.out_val, S.W.out_emit);
      hipLaunchKernelGGL(k_xsel_init, dim3(blocks_for(GB, 256)), dim3(256), 0,
                         st, GB, counts, emit, krange, S.W.xsel, S.median,
                         S.P.pct, xs_flags(c));
    }
  } else {
    if (!hist_prev) return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null hist_prev");
    if (!S.more) return fail(OTSDB_E_ILLEGAL_STATE, "no pass planned");
    if (GB > 0)
      hipLaunchKernelGGL(k_xsel_apply, dim3(blocks_for(GB, 4)), dim3(256), 0,
                         st, GB, T.lg_k, NB, (const uint32_t*)hist_prev,
                         S.W.xsel, xs_flags(c), xs_bnd(c));
    if (pass == 1 && GB > 0) {  // the pool's regions: offsets, size off[GB]
      size_t tmp = S.scan_tmp;
      HIP_TRY(rocprim::exclusive_scan(xs_scan_tmp(c), tmp, (const int64_t*)xs_bnd(c),
                                      xs_off(c), (int64_t)0, (size_t)(GB + 1),
                                      rocprim::plus<int64_t>(), st));
      HIP_TRY(hipMemcpyAsync(&c->h_small[5], xs_off(c) + GB, 8,
                             hipMemcpyDeviceToHost, st));
    }
  }
  HIP_TRY(hipGetLastError());
  // the plan is taken from all-reduced data: every rank reads the same flags
  HIP_TRY(hipMemcpyAsync(&c->h_small[4], xs_flags(c), 4, hipMemcpyDeviceToHost,
                         st));
  HIP_TRY(hipStreamSynchronize(st));
  const uint32_t flags = (uint32_t)(c->h_small[4] & 0xFFFFFFFF);
  const int64_t bound = pass == 1 ? c->h_small[5] : 0;
  if (flags & XS_BROKEN) {
    S.active = false;
    return fail(OTSDB_E_DEVICE, "selection: the ranks' counts and keys disagree");
  }
  S.more = (flags & XS_MORE) != 0;
  S.need_pick = (flags & XS_PICK) != 0;
  S.next_pass = pass + 1;
  *more = S.more ? 1 : 0;
  if (!S.more || GB == 0) return OTSDB_OK;
  HIP_TRY(hipMemsetAsync(hist_out, 0, (size_t)GB * XS_BINS * 4, st));
  if (pass <= 1) {
    int mode = 1;
    if (pass == 1) {  // the candidates: every later pass and the pick read them
      const int64_t cap = bound > 0 ? bound : 1;
      otsdb_status rc = S.pool.ensure((size_t)cap * 16);
      if (rc) return rc;
      S.pool_cap = cap;
      HIP_TRY(hipMemsetAsync((char*)S.pool.p + (size_t)cap * 8, 0xFF,
                             (size_t)cap * 8, st));  // every slot unfilled
      HIP_TRY(hipMemsetAsync(xs_segfill(c), 0, (size_t)GB * 4, st));
      S.pool_built = true;
      mode |= 2;
    }
    if (T.LGCH > 0)
      hipLaunchKernelGGL(k_xsel_scan, dim3((unsigned)(T.LGCH * NB)), dim3(XS_THREADS), 0,
                         st, mode, NB, S.M, T.LG, T.lg_off, T.lg_k, T.lg_ch0,
                         (const uint64_t*)S.W.keys, (const XSel*)S.W.xsel,
                         hist_out, xs_pool(c), (int64_t*)nullptr);
    ++S.key_reads;
  } else {
    const int64_t nblk = std::min<int64_t>(blocks_for(S.pool_cap, 256), 8192);
    hipLaunchKernelGGL(k_xsel_pool, dim3((unsigned)nblk), dim3(256), 0, st, 1,
                       xs_pool(c), (const XSel*)S.W.xsel, hist_out,
                       (int64_t*)nullptr);
  }
  ++S.passes;
  // no host sync: the caller's collective on the same stream consumes
  // hist_out (RCCL enqueues behind it; a gloo staging copy waits for it)
  HIP_TRY(hipGetLastError());
  return OTSDB_OK;
}

otsdb_status otsdb_sel_hist_wait(otsdb_ctx* c, void* hip_stream) {
  if (!c) return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null");
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipStreamSynchronize(hip_stream ? (hipStream_t)hip_stream : c->stream));
  return OTSDB_OK;
}

otsdb_status otsdb_sel_pick_device(otsdb_ctx* c, int64_t* picks,
                                   void* hip_stream) {
  if (!c || !picks) return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null");
  CtxLock lk(c, /*keep_session=*/true);
  auto& S = c->sel;
  if (!S.active) return fail(OTSDB_E_ILLEGAL_STATE, "no selection session");
  if (S.next_pass == 0 || S.next_pass == -2 || S.more)
    return fail(OTSDB_E_ILLEGAL_STATE, "selection not resolved: run its passes");
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
  const int64_t G = S.G, NB = S.NB, GB = G * NB;
  const Tiles T = tiles_of(c, G);
  if (GB > 0) HIP_TRY(hipMemsetAsync(picks, 0, (size_t)GB * 16, st));
  if (S.need_pick && GB > 0) {
    if (S.pool_built) {
      const int64_t nblk = std::min<int64_t>(blocks_for(S.pool_cap, 256), 8192);
      hipLaunchKernelGGL(k_xsel_pool, dim3((unsigned)nblk), dim3(256), 0, st, 4,
                         xs_pool(c), (const XSel*)S.W.xsel, (uint32_t*)nullptr,
                         picks);
    } else if (T.LGCH > 0) {
      hipLaunchKernelGGL(k_xsel_scan, dim3((unsigned)(T.LGCH * NB)), dim3(XS_THREADS), 0,
                         st, 4, NB, S.M, T.LG, T.lg_off, T.lg_k, T.lg_ch0,
                         (const uint64_t*)S.W.keys, (const XSel*)S.W.xsel,
                         (uint32_t*)nullptr, xs_pool(c), picks);
      ++S.key_reads;
    }
  }
  S.next_pass = -1;  // picked
  HIP_TRY(hipGetLastError());
  return OTSDB_OK;
}

otsdb_status otsdb_sel_finish_device(otsdb_ctx* c, const int64_t* picks,
                                     otsdb_result* out, void* hip_stream) {
  if (!c || !picks || !out) return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null");
  CtxLock lk(c, /*keep_session=*/true);
  auto& S = c->sel;
  if (!S.active) return fail(OTSDB_E_ILLEGAL_STATE, "no selection session");
  if (S.next_pass != -1)
    return fail(OTSDB_E_ILLEGAL_STATE, "otsdb_sel_pick_device first");
  HIP_TRY(hipSetDevice(c->device));
  StreamBinding bind(c, hip_stream);
  const int64_t G = S.G, NB = S.NB, GB = G * NB;
  HIP_TRY(hipMemsetAsync(c->d_err, 0, sizeof(int), c->stream));
  if (GB > 0)
    hipLaunchKernelGGL(k_xsel_finish, dim3(blocks_for(GB, 256)), dim3(256), 0,
                       c->stream, GB, (const XSel*)S.W.xsel, picks,
                       (const uint8_t*)S.W.out_emit, S.W.out_val, c->d_err,
                       S.median, S.P.pct, (const uint32_t*)xs_broken(c));
  otsdb_status rc = compact(c, S.P, G, S.W.out_val, S.W.out_emit, S.W.counts, out);
  if (!rc) rc = finish(c, G, out);
  // the session stays for otsdb_sel_retarget (the keys are untouched); any
  // other call of the context ends it
  S.next_pass = -2;  // finished
  return rc;
}

otsdb_status otsdb_decode_cells_device(otsdb_ctx* c, const otsdb_cells* cells,
                                       int64_t n_series, int64_t* offsets,
                                       int64_t* ts_ms, int64_t* val,
                                       uint8_t* is_float, int64_t capacity,
                                       void* hip_stream) {
  if (!c || !cells || !offsets) return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null");
  if (ts_ms && (!val || !is_float))
    return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null output column");
  CtxLock lk(c);
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
  return decode_impl(c, cells, n_series, offsets, ts_ms, val, is_float,
                     capacity, st);
}

otsdb_status otsdb_encode_cells_device(otsdb_ctx* c, const otsdb_batch* b,
                                       int64_t* series_rows,
                                       int64_t* series_qbytes,
                                       int64_t* series_vbytes,
                                       const otsdb_cells_out* o,
                                       void* hip_stream) {
  if (!c || !b || !series_rows || !series_qbytes || !series_vbytes)
    return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null");
  if (b->is_float)
    return fail(OTSDB_E_UNSUPPORTED, "per-point value types: use series_float");
  CtxLock lk(c);
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
  const int64_t S = b->n_series;
  if (S > 0)
    hipLaunchKernelGGL(k_encode, dim3(blocks_for(S, 4)), dim3(256), 0, st, S,
                       b->offsets, b->ts_ms, b->val, b->series_float,
                       o ? 1 : 0, series_rows, series_qbytes, series_vbytes,
                       o ? o->row_series : nullptr, o ? o->row_base_s : nullptr,
                       o ? o->qual_off : nullptr, o ? o->val_off : nullptr,
                       o ? o->qual : nullptr, o ? o->val : nullptr);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(st));
  return OTSDB_OK;
}

otsdb_status otsdb_agg_run_cells(otsdb_ctx* c, const otsdb_query_spec* spec,
                                 const otsdb_cells* cells, const otsdb_batch* b,
                                 otsdb_result* out) {
  if (!c || !spec || !cells || !b || !out)
    return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null");
  CtxLock lk(c);
  HIP_TRY(hipSetDevice(c->device));
  otsdb_status rc = check_spec(spec);
  if (rc) return rc;
  std::vector<int64_t> goff;
  if ((rc = read_goff(c, b, false, goff))) return rc;
  const int64_t R = cells->n_rows, S = b->n_series, G = b->n_groups;
  if (R < 0 || S < 0) return fail(OTSDB_E_ILLEGAL_ARGUMENT, "negative sizes");
  if (R > 0 && (!cells->row_series || !cells->row_base_s || !cells->qual_off ||
                !cells->val_off || !cells->qual || !cells->val))
    return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null cells array");
  for (int64_t r = 0; r < R; ++r)
    if (cells->row_series[r] < 0 || cells->row_series[r] >= S ||
        (r && cells->row_series[r] < cells->row_series[r - 1]))
      return fail(OTSDB_E_ILLEGAL_ARGUMENT,
                  "row_series must be nondecreasing series indices");
  const int64_t M = goff.back();
  for (int64_t m = 0; m < M; ++m)
    if (b->group_members[m] < 0 || b->group_members[m] >= S)
      return fail(OTSDB_E_ILLEGAL_ARGUMENT, "group member out of range");
  // the pooled byte offsets set the H2D copy sizes: exclusive prefix sums
  // from 0, never decreasing
  if (R > 0 && (cells->qual_off[0] != 0 || cells->val_off[0] != 0))
    return fail(OTSDB_E_ILLEGAL_ARGUMENT, "qual_off / val_off must start at 0");
  for (int64_t r = 0; r < R; ++r)
    if (cells->qual_off[r + 1] < cells->qual_off[r] ||
        cells->val_off[r + 1] < cells->val_off[r])
      return fail(OTSDB_E_ILLEGAL_ARGUMENT,
                  "qual_off / val_off must be nondecreasing");
  const int64_t QB = R ? cells->qual_off[R] : 0, VB = R ? cells->val_off[R] : 0;
  const int64_t cap = out->capacity;
  auto carve = [&](char* base) {
    Carve cv{base};
    void* p[11];
    p[0] = cv.take<int64_t>(R + 1);
    p[1] = cv.take<int64_t>(R + 1);
    p[2] = cv.take<int64_t>(R + 1);
    p[3] = cv.take<uint8_t>(QB + 32);
    p[4] = cv.take<int64_t>(R + 1);
    p[5] = cv.take<uint8_t>(VB + 32);
    p[6] = cv.take<int64_t>(G + 1);
    p[7] = cv.take<int64_t>(M + 1);
    p[8] = cv.take<int64_t>(G + 1);
    p[9] = cv.take<int64_t>(2 * (cap + 1));
    p[10] = cv.take<uint8_t>(cap + 1);
    return std::make_pair(cv.off + 256, std::vector<void*>(p, p + 11));
  };
  rc = c->raw_stage.ensure(carve(nullptr).first);
  if (rc) return rc;
  auto pp = carve((char*)c->raw_stage.p).second;
  hipStream_t st = c->stream;
  auto h2d = [&](void* d, const void* h, size_t n) -> otsdb_status {
    if (n && h) HIP_TRY(hipMemcpyAsync(d, h, n, hipMemcpyHostToDevice, st));
    return OTSDB_OK;
  };
  if ((rc = h2d(pp[0], cells->row_series, 8 * R)) ||
      (rc = h2d(pp[1], cells->row_base_s, 8 * R)) ||
      (rc = h2d(pp[2], cells->qual_off, 8 * (R + 1))) ||
      (rc = h2d(pp[3], cells->qual, QB)) ||
      (rc = h2d(pp[4], cells->val_off, 8 * (R + 1))) ||
      (rc = h2d(pp[5], cells->val, VB)) ||
      (rc = h2d(pp[6], b->group_offsets, 8 * (G + 1))) ||
      (rc = h2d(pp[7], b->group_members, 8 * M)))
    return rc;
  if (R == 0) HIP_TRY(hipMemsetAsync(pp[2], 0, 8, st));
  if (R == 0) HIP_TRY(hipMemsetAsync(pp[4], 0, 8, st));
  otsdb_cells dc{R,
                 (const int64_t*)pp[0],
                 (const int64_t*)pp[1],
                 (const int64_t*)pp[2],
                 (const uint8_t*)pp[3],
                 (const int64_t*)pp[4],
                 (const uint8_t*)pp[5]};
  otsdb_batch db = *b;
  db.n_points = 0;
  db.offsets = nullptr;
  db.ts_ms = nullptr;
  db.val = nullptr;
  db.is_float = nullptr;
  db.series_float = nullptr;
  db.group_offsets = (const int64_t*)pp[6];
  db.group_members = (const int64_t*)pp[7];
  otsdb_result dres;
  dres.capacity = cap;
  dres.offsets = (int64_t*)pp[8];
  dres.ts = (int64_t*)pp[9];
  dres.val = (int64_t*)pp[9] + (cap + 1);
  dres.is_int = (uint8_t*)pp[10];
  c->result_short = false;
  rc = run_cells_impl(c, spec, &dc, &db, &dres, goff);
  if (rc == OTSDB_E_CAPACITY && c->result_short)
    return copy_offsets_back(c, out, dres.offsets, G, rc);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(out->offsets, dres.offsets, 8 * (G + 1),
                         hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  const int64_t total = out->offsets[G];
  if (total > 0) {
    HIP_TRY(hipMemcpyAsync(out->ts, dres.ts, 8 * total, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out->val, dres.val, 8 * total, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out->is_int, dres.is_int, total, hipMemcpyDeviceToHost, st));
  }
  HIP_TRY(hipStreamSynchronize(st));
  return OTSDB_OK;
}

otsdb_status otsdb_topn_plan(otsdb_ctx* c, const otsdb_topn_spec* spec,
                             int32_t n_results, const int64_t* n_groups,
                             const int64_t* n_points, otsdb_sizes* out) {
  if (!spec || !out || (n_results > 0 && !n_points))
    return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null");
  int64_t S = 0, N = 0;
  std::vector<otsdb_result> shape((size_t)std::max(n_results, 0));
  for (auto& r : shape) r.offsets = (int64_t*)n_points;  // (non-null: shape only)
  const otsdb_status rc =
      check_topn(spec, n_results, shape.data(), n_groups, &S);
  if (rc) return rc;
  for (int32_t r = 0; r < n_results; ++r) {
    if (n_points[r] < 0) return fail(OTSDB_E_ILLEGAL_ARGUMENT, "n_points < 0");
    N += n_points[r];
  }
  out->n_buckets = std::min<int64_t>(spec->topn, S);
  out->max_out_points = N;
  // the columnar view (17 B), candidate / sorted / distinct keys (24 B) and
  // the sort's own scratch (~16 B) a point; ~180 B a series
  out->workspace_bytes = N * 57 + S * 180 + (1 << 20);
  return OTSDB_OK;
}

otsdb_status otsdb_topn_run_device(otsdb_ctx* c, const otsdb_topn_spec* spec,
                                   int32_t n_results,
                                   const otsdb_result* results,
                                   const int64_t* n_groups,
                                   otsdb_topn_result* out, void* hip_stream) {
  if (!c || !spec || !out || !out->series.offsets)
    return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null");
  int64_t S = 0;
  otsdb_status rc = check_topn(spec, n_results, results, n_groups, &S);
  if (rc) return rc;
  CtxLock lk(c);
  HIP_TRY(hipSetDevice(c->device));
  StreamBinding bind(c, hip_stream);
  return run_topn_impl(c, spec, n_results, results, n_groups, S, out);
}

otsdb_status otsdb_topn_run(otsdb_ctx* c, const otsdb_topn_spec* spec,
                            int32_t n_results, const otsdb_result* results,
                            const int64_t* n_groups, otsdb_topn_result* out) {
  if (!c || !spec || !out || !out->series.offsets)
    return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null");
  int64_t S = 0;
  otsdb_status rc = check_topn(spec, n_results, results, n_groups, &S);
  if (rc) return rc;
  CtxLock lk(c);
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = c->stream;
  const int R = n_results;
  const int64_t n_out = std::min<int64_t>(spec->topn, S);
  const int64_t cap = std::max<int64_t>(out->series.capacity, 0);
  std::vector<int64_t> np((size_t)R);
  for (int r = 0; r < R; ++r) {
    const int64_t G = n_groups[r];
    np[r] = G > 0 ? results[r].offsets[G] : 0;
    if (np[r] < 0 || (np[r] > 0 && (!results[r].ts || !results[r].val ||
                                     !results[r].is_int)))
      return fail(OTSDB_E_ILLEGAL_ARGUMENT, "result %d: bad point arrays", r);
  }
  // staging layout in HBM: the inputs, then the output
  std::vector<otsdb_result> dr((size_t)R);
  otsdb_topn_result dout = *out;
  auto carve = [&](char* base) {
    Carve cv{base};
    for (int r = 0; r < R; ++r) {
      dr[r].capacity = np[r];
      dr[r].offsets = cv.take<int64_t>(n_groups[r] + 1);
      dr[r].ts = cv.take<int64_t>(np[r] + 1);
      dr[r].val = cv.take<int64_t>(np[r] + 1);
      dr[r].is_int = cv.take<uint8_t>(np[r] + 1);
    }
    dout.series.capacity = cap;
    dout.series.offsets = cv.take<int64_t>(n_out + 1);
    dout.series.ts = cv.take<int64_t>(cap + 1);
    dout.series.val = cv.take<int64_t>(cap + 1);
    dout.series.is_int = cv.take<uint8_t>(cap + 1);
    return cv.off + 256;
  };
  rc = c->stage.ensure(carve(nullptr));
  if (rc) return rc;
  carve((char*)c->stage.p);
  for (int r = 0; r < R; ++r) {
    if (n_groups[r] > 0)
      HIP_TRY(hipMemcpyAsync(dr[r].offsets, results[r].offsets,
                             8 * (n_groups[r] + 1), hipMemcpyHostToDevice, st));
    if (np[r] > 0) {
      HIP_TRY(hipMemcpyAsync(dr[r].ts, results[r].ts, 8 * np[r],
                             hipMemcpyHostToDevice, st));
      HIP_TRY(hipMemcpyAsync(dr[r].val, results[r].val, 8 * np[r],
                             hipMemcpyHostToDevice, st));
      HIP_TRY(hipMemcpyAsync(dr[r].is_int, results[r].is_int, np[r],
                             hipMemcpyHostToDevice, st));
    }
  }
  rc = run_topn_impl(c, spec, R, dr.data(), n_groups, S, &dout);
  out->n_picked = dout.n_picked;
  if (rc && !(rc == OTSDB_E_CAPACITY && c->result_short)) return rc;
  const int64_t k = out->n_picked;
  HIP_TRY(hipMemcpyAsync(out->series.offsets, dout.series.offsets, 8 * (k + 1),
                         hipMemcpyDeviceToHost, st));
  const int64_t total = rc ? 0 : c->h_small[1];
  if (total > 0) {
    HIP_TRY(hipMemcpyAsync(out->series.ts, dout.series.ts, 8 * total,
                           hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out->series.val, dout.series.val, 8 * total,
                           hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out->series.is_int, dout.series.is_int, total,
                           hipMemcpyDeviceToHost, st));
  }
  HIP_TRY(hipStreamSynchronize(st));
  return rc;
}

otsdb_status otsdb_prof_enable(otsdb_ctx* c, int enable) {
  if (!c) return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null");
  CtxLock lk(c, /*keep_session=*/true);
  c->prof = enable != 0;
  return OTSDB_OK;
}

otsdb_status otsdb_prof_read(otsdb_ctx* c, double* ms, int64_t* launches,
                             int n, int reset) {
  if (!c) return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null");
  CtxLock lk(c, /*keep_session=*/true);
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (auto& p : c->ev_pending) {
    float t = 0.f;
    HIP_TRY(hipEventSynchronize(p.second.second));
    HIP_TRY(hipEventElapsedTime(&t, p.second.first, p.second.second));
    c->prof_ms[p.first] += t;
    c->prof_n[p.first] += 1;
  }
  c->ev_pending.clear();
  c->ev_used = 0;
  for (int i = 0; i < n && i < 14; ++i) {
    if (ms) ms[i] = c->prof_ms[i];
    if (launches) launches[i] = c->prof_n[i];
  }
  if (reset)
    for (int i = 0; i < 14; ++i) {
      c->prof_ms[i] = 0;
      c->prof_n[i] = 0;
    }
  return OTSDB_OK;
}

otsdb_status otsdb_ctx_counters(otsdb_ctx* c, int64_t* out, int n) {
  if (!c || (n > 0 && !out)) return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null");
  CtxLock lk(c, /*keep_session=*/true);
  const int64_t v[21] = {c->n_cells_uniform, c->n_cells_general,
                         c->n_cells_uni_miss, c->sel.key_reads, c->sel.passes,
                         c->n_multi_ds,       c->n_multi_group, c->n_multi_kt,
                         c->n_multi_tf,       c->sel.sessions,
                         c->n_panel_passes,   c->n_panel_mats,
                         c->n_multi_fold,     c->n_hist_fold,
                         c->n_hist_pct,       c->n_hr_decoded,
                         c->n_hr_skipped,     c->n_hr_dropped,
                         c->n_topn_grid,      c->n_topn_general,
                         c->n_topn_miss};
  for (int i = 0; i < n && i < 21; ++i) out[i] = v[i];
  return OTSDB_OK;
}

otsdb_status otsdb_test_set_compact_epoch(otsdb_ctx* c, uint32_t epoch) {
  if (!c || epoch == 0 || epoch >= (1u << 24))
    return fail(OTSDB_E_ILLEGAL_ARGUMENT, "epoch %u", epoch);
  CtxLock lk(c, /*keep_session=*/true);
  // forward only: every granule then carries an epoch below the new one
  // until the wrap (a step back would reuse epochs of live granules)
  if (epoch < c->cmp_epoch)
    return fail(OTSDB_E_ILLEGAL_ARGUMENT, "epoch %u < %u", epoch, c->cmp_epoch);
  // and by whole ticket-slot rotations: the next call's slot is the one the
  // last call's final block cleared (k_compact1)
  if ((epoch - c->cmp_epoch) % kCmpSlots)
    return fail(OTSDB_E_ILLEGAL_ARGUMENT, "epoch %u: not %u + k x %d", epoch,
                c->cmp_epoch, kCmpSlots);
  c->cmp_epoch = epoch;
  return OTSDB_OK;
}

otsdb_status otsdb_gen_counts_device(otsdb_ctx* c, const otsdb_gen_spec* g,
                                     int64_t series0, int64_t n_series,
                                     int64_t* counts, void* hip_stream) {
  if (!c || !g || !counts) return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null");
  if (g->cadence_ms <= 0) return fail(OTSDB_E_ILLEGAL_ARGUMENT, "cadence");
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
  GenP gp{g->seed, g->t0_ms, g->duration_ms, g->cadence_ms, g->kind, g->flags};
  if (n_series > 0)
    hipLaunchKernelGGL(k_gen_counts, dim3(blocks_for(n_series, 4)), dim3(256),
                       0, st, gp, series0, n_series, counts);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(st));
  return OTSDB_OK;
}

otsdb_status otsdb_gen_fill_device(otsdb_ctx* c, const otsdb_gen_spec* g,
                                   int64_t series0, int64_t n_series,
                                   const int64_t* offsets, int64_t* ts_ms,
                                   int64_t* val, void* hip_stream) {
  if (!c || !g || !offsets || !ts_ms || !val)
    return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null");
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
  GenP gp{g->seed, g->t0_ms, g->duration_ms, g->cadence_ms, g->kind, g->flags};
  if (n_series > 0)
    hipLaunchKernelGGL(k_gen_fill, dim3(blocks_for(n_series, 4)), dim3(256),
                       0, st, gp, series0, n_series, offsets, ts_ms, val);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(st));
  return OTSDB_OK;
}

}  // extern "C"
