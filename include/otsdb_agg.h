/*
 * otsdb_agg.h — C-ABI of the MI355X-native OpenTSDB query-time aggregation
 * engine (libotsdb_agg.so).
 *
 * This is the drop-in boundary for ONE path of OpenTSDB: the query-time
 * aggregation that today runs as a chain of Java iterators
 *
 *   Span/RowSeq points -> Downsampler | FillingDownsampler -> RateSpan
 *                      -> AggregationIterator (cross-series group-by)
 *
 * created by SpanGroup.iterator() (src/core/SpanGroup.java:525-530) for every
 * group that TsdbQuery.GroupByAndAggregateCB.call builds
 * (src/core/TsdbQuery.java:992-1113).  A JNI shim replaces
 * the per-group lazy iterators with ONE batched call per query: every group of
 * the query is evaluated on the GPU and handed back as arrays, which a Java
 * array-backed SeekableView/DataPoints then serves to the unchanged callers
 * (HttpJsonSerializer.java:821-869, CliQuery.java:126).
 *
 * Conventions: plain C types only, no torch/HIP types in the signatures.
 * Every entry point returns an otsdb_status; on failure the thread-local
 * message is available from otsdb_last_error().  Status codes map 1:1 onto the
 * Java exceptions the reference path throws (see otsdb_status).
 */
#ifndef OTSDB_AGG_H
#define OTSDB_AGG_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OTSDB_ABI_VERSION 6

/* ------------------------------------------------------------------------ */
/* Status codes — 1:1 with the exceptions of the reference path.             */
/* ------------------------------------------------------------------------ */
typedef enum {
  OTSDB_OK = 0,
  /* IllegalDataException: corrupted cell (Internal.java:307-321), `none`
   * aggregator fed more than one value (Aggregators.java:446-460).          */
  OTSDB_E_ILLEGAL_DATA = 1,
  /* IllegalStateException: "Got Infinity" (AggregationIterator.java:640-643),
   * non-increasing timestamps in a rate (RateSpan.java:129-134), empty long
   * median (Aggregators.java:408-410).                                      */
  OTSDB_E_ILLEGAL_STATE = 2,
  /* IllegalArgumentException: bad spec (DownsamplingSpecification.java:116+,
   * Downsampler "cannot use the NONE aggregator for downsampling").        */
  OTSDB_E_ILLEGAL_ARGUMENT = 3,
  /* NoSuchElementException: unknown aggregator (Aggregators.java:222-228). */
  OTSDB_E_NO_SUCH_ELEMENT = 4,
  /* Valid in the reference but not implemented by this engine (scalar fill,
   * rollup avg downsampled with another function, rollup queries without a
   * downsampler or over per-series calendar anchors; histogram queries
   * without a downsampler, with "0all" or a calendar interval, over rollup
   * tables, or past the limits of otsdb_hist_*): the Java side keeps its own
   * iterators for such queries.  Also what the reference itself refuses with
   * UnsupportedOperationException (a rollup table's dev).                   */
  OTSDB_E_UNSUPPORTED = 5,
  /* HIP runtime failure / out of device memory.                            */
  OTSDB_E_DEVICE = 6,
  /* Caller-provided output capacity too small (otsdb_result.capacity).  The
   * host entries (otsdb_agg_run, otsdb_agg_run_cells, otsdb_agg_run_raw)
   * still fill result.offsets with the whole result's offsets, so
   * offsets[n_groups] is the capacity a retry needs; nothing else written. */
  OTSDB_E_CAPACITY = 7
} otsdb_status;

/* ------------------------------------------------------------------------ */
/* Aggregators registry (Aggregators.java:175-203).  Ids are stable.         */
/* ------------------------------------------------------------------------ */
typedef enum {
  OTSDB_AGG_SUM = 0,        /* "sum"       Sum(LERP)                 */
  OTSDB_AGG_PFSUM = 1,      /* "pfsum"     Sum(PREV)                 */
  OTSDB_AGG_MIN = 2,        /* "min"       Min(LERP)                 */
  OTSDB_AGG_MAX = 3,        /* "max"       Max(LERP)                 */
  OTSDB_AGG_AVG = 4,        /* "avg"       Avg(LERP)                 */
  OTSDB_AGG_MEDIAN = 5,     /* "median"    Median(LERP)              */
  OTSDB_AGG_NONE = 6,       /* "none"      None(ZIM), toString "raw" */
  OTSDB_AGG_MULT = 7,       /* "mult"      Multiply(LERP)            */
  OTSDB_AGG_DEV = 8,        /* "dev"       StdDev(LERP)              */
  OTSDB_AGG_DIFF = 9,       /* "diff"      Diff(LERP)                */
  OTSDB_AGG_ZIMSUM = 10,    /* "zimsum"    Sum(ZIM)                  */
  OTSDB_AGG_MIMMIN = 11,    /* "mimmin"    Min(MAX)                  */
  OTSDB_AGG_MIMMAX = 12,    /* "mimmax"    Max(MIN)                  */
  OTSDB_AGG_SQUARESUM = 13, /* "squareSum" SquareSum(ZIM)            */
  OTSDB_AGG_COUNT = 14,     /* "count"     Count(ZIM)                */
  OTSDB_AGG_FIRST = 15,     /* "first"     First(ZIM)                */
  OTSDB_AGG_LAST = 16,      /* "last"      Last(ZIM)                 */
  /* PercentileAgg(LERP), commons-math3 3.4.1 Percentile
   * (Aggregators.java:125-173, :657-708).  LEGACY estimation: */
  OTSDB_AGG_P999 = 17, OTSDB_AGG_P99 = 18, OTSDB_AGG_P95 = 19,
  OTSDB_AGG_P90 = 20, OTSDB_AGG_P75 = 21, OTSDB_AGG_P50 = 22,
  /* R_3 estimation (honoured by runLong only, Aggregators.java:690): */
  OTSDB_AGG_EP999R3 = 23, OTSDB_AGG_EP99R3 = 24, OTSDB_AGG_EP95R3 = 25,
  OTSDB_AGG_EP90R3 = 26, OTSDB_AGG_EP75R3 = 27, OTSDB_AGG_EP50R3 = 28,
  /* R_7 estimation (honoured by runLong only): */
  OTSDB_AGG_EP999R7 = 29, OTSDB_AGG_EP99R7 = 30, OTSDB_AGG_EP95R7 = 31,
  OTSDB_AGG_EP90R7 = 32, OTSDB_AGG_EP75R7 = 33, OTSDB_AGG_EP50R7 = 34,
  OTSDB_AGG_COUNT_IDS = 35
} otsdb_agg_id;

/* Aggregators.Interpolation (Aggregators.java:38-44), Java ordinal order. */
typedef enum {
  OTSDB_INTERP_DEFAULT = -1, /* use the aggregator's own method */
  OTSDB_INTERP_LERP = 0,
  OTSDB_INTERP_ZIM = 1,
  OTSDB_INTERP_MAX = 2,
  OTSDB_INTERP_MIN = 3,
  OTSDB_INTERP_PREV = 4
} otsdb_interp;

/* FillPolicy (FillPolicy.java:22-28), Java ordinal order. */
typedef enum {
  OTSDB_FILL_NONE = 0,
  OTSDB_FILL_ZERO = 1,
  OTSDB_FILL_NAN = 2,
  OTSDB_FILL_NULL = 3,
  OTSDB_FILL_SCALAR = 4 /* FillingDownsampler throws "unhandled fill policy" */
} otsdb_fill;

/* ------------------------------------------------------------------------ */
/* Query spec: one per query (all groups share it).                          */
/* ------------------------------------------------------------------------ */
#define OTSDB_SPEC_EXACT_ORDER 1
#define OTSDB_SPEC_MULTI_FOLD 2 /* otsdb_agg_run_multi*: see there */
#define OTSDB_SPEC_CELLS_MULTI_FOLD 4 /* otsdb_agg_run_cells_multi_device */
typedef struct {
  /* AggregationIterator window, ms, inclusive on both ends
   * (SpanGroup ctor normalises the scan bounds to ms, SpanGroup.java:267-270;
   * TsdbQuery passes getScanStartTimeSeconds/getScanEndTimeSeconds,
   * TsdbQuery.java:1092-1093).                                               */
  int64_t start_ms;
  int64_t end_ms;
  /* Raw query bounds (TsdbQuery.getStartTime/getEndTime, ms): used by the
   * "all" downsampler (Downsampler.java:354-379).                            */
  int64_t query_start_ms;
  int64_t query_end_ms;
  int32_t agg_id;          /* otsdb_agg_id — cross-series aggregator       */
  int32_t interp;          /* otsdb_interp, OTSDB_INTERP_DEFAULT normally  */
  int64_t ds_interval_ms;  /* 0 = no downsampling (raw path)               */
  int32_t ds_agg_id;       /* downsampling function (not NONE)             */
  int32_t fill;            /* otsdb_fill                                   */
  int32_t run_all;         /* "0all-<agg>" downsampling                    */
  int32_t use_calendar;    /* "<n><u>c-" downsampling: needs cal_edges     */
  int32_t rate;            /* RateSpan applied after downsampling          */
  int32_t counter;         /* RateOptions.counter                          */
  int32_t drop_resets;     /* RateOptions.drop_resets                      */
  /* OTSDB_SPEC_* bits (ABI 5; the padding word before, callers pass 0).
   * OTSDB_SPEC_EXACT_ORDER: an order-sensitive aggregator (dev) reduces
   * every (group, timestamp) in ONE sequential chain over the group's
   * members in SpanCmp order, whatever the group's size — StdDev.runDouble's
   * one Welford loop (Aggregators.java:547-568) bit for bit.  Without it a
   * group of more than 65,536 members on one device merges in-order chunk
   * states with Chan's formula: on well-conditioned contributions (counter
   * rates, C4) within 1e-12 of the loop, on offset gauges (~3e9 +- 1e4,
   * where the loop itself lies ~1e-11 from the exact sigma) measured
   * ~1e-11 off (tests/test_gpu_dev_large.py); the chain costs ~100-180 ns a
   * member per bucket (tools/chain_probe.hip: a 500k-member group ~50-90 ms).
   * A chain whose bucket rows (9 B per member and bucket) pass the engine's
   * fixed row budget is OTSDB_E_CAPACITY with the flag, merged without.    */
  int32_t flags;
  int64_t counter_max;     /* RateOptions.counter_max (default Long.MAX)   */
  int64_t reset_value;     /* RateOptions.reset_value (default 0)          */
  /* Calendar downsampling (use_calendar = 1): the bucket edges, ms, strictly
   * ascending, HOST memory (copied during the call).  cal_edges[0] =
   * DateTime.previousInterval(start_ms, n, unit, tz) (DateTime.java:450-610)
   * and cal_edges[k+1] = cal_edges[k] stepped once the way the Downsampler
   * steps its calendars (Calendar.add(unit, n), or 7n days for weeks,
   * Downsampler.java:387-394), continued until two edges lie past end_ms
   * (past the batch's last point if spans hold points beyond the window).
   * Bucket k is [cal_edges[k], cal_edges[k+1]) with timestamp cal_edges[k]
   * (ValuesInInterval.getIntervalTimestamp, :437-449).  The reference
   * anchors each series at previousInterval(its first point): when every
   * such anchor in the window is an edge of this one table (the grid does
   * not depend on the series: 1dc, 1hc, 1nc, 30mc, ... in any zone) the
   * caller passes it alone (n_cal_anchors = 0).  A point past the window
   * whose bucket end is not in the table is OTSDB_E_UNSUPPORTED.  NULL with
   * use_calendar = 1 -> OTSDB_E_UNSUPPORTED.  ds_interval_ms stays
   * DownsamplingSpecification's nominal interval (parseDuration), which the
   * scan bounds use.                                                       */
  const int64_t* cal_edges;
  int64_t n_cal_edges;
  /* Per-series calendar anchors (n_cal_anchors > 0; 7mc, 2wc, 6hc across a
   * DST change, ...): cal_edges then holds CHAINS, each the Downsampler's
   * calendar stepped from one anchor (Downsampler.java:330-345, :383-397)
   * until two edges lie past the window / the batch's last point, strictly
   * ascending and ended by INT64_MAX.  cal_anchors[j] (ascending) are
   * DateTime.previousInterval values and cal_anchor_edge[j] the index in
   * cal_edges of the chain edge equal to cal_anchors[j]; for every series'
   * first point f after the seek, previousInterval(f) must be the largest
   * anchor <= f (true when the anchors hold every previousInterval value of
   * the window, or just the ones the batch's series take), and so must
   * previousInterval(start_ms) (the seek, Downsampler.java:419-429).  Series
   * grids then differ, and the output timestamps are the union of the
   * series' bucket starts (AggregationIterator.next).  With fill != NONE
   * the FillingDownsampler's own grid is the chain from previousInterval(
   * start_ms) to previousInterval(end_ms) (FillingDownsampler.java:113-135):
   * previousInterval(end_ms) must then be the largest anchor <= end_ms too.
   * A point past its chain's last edge is OTSDB_E_UNSUPPORTED only when a
   * query reads it (rate queries; the first bucket past the window).  The
   * multi-GPU partial / selection entry points -> OTSDB_E_UNSUPPORTED.
   * HOST memory.                                                          */
  const int64_t* cal_anchors;
  const int64_t* cal_anchor_edge;
  int64_t n_cal_anchors;
} otsdb_query_spec;

/* ------------------------------------------------------------------------ */
/* Columnar batch.  Series are given in SpanCmp order (TsdbQuery.java:      */
/* 1862-1892); each group lists its member series in that order.            */
/* Within a series points must be sorted by timestamp (Span/RowSeq order).  */
/* Pointers are HOST pointers for otsdb_agg_run and DEVICE pointers for     */
/* otsdb_agg_run_device.                                                    */
/* ------------------------------------------------------------------------ */
typedef struct {
  int64_t n_series;             /* S                                       */
  int64_t n_points;             /* N = offsets[S]                          */
  const int64_t* offsets;       /* [S+1] CSR point offsets                 */
  const int64_t* ts_ms;         /* [N] timestamps, ms                      */
  const int64_t* val;           /* [N] raw value bits: int64 or IEEE f64   */
  /* Value type.  Exactly one of the following conventions:
   *  - is_float != NULL: per point, 1 = double, 0 = long;
   *  - else series_float != NULL: per series, 1 = double, 0 = long;
   *  - else all values are doubles.                                       */
  const uint8_t* is_float;      /* [N] or NULL                             */
  const uint8_t* series_float;  /* [S] or NULL                             */
  int64_t n_groups;             /* G                                       */
  const int64_t* group_offsets; /* [G+1] CSR into group_members            */
  const int64_t* group_members; /* [M] series indices, SpanCmp order       */
  /* Optional HOST copy of group_offsets (the same G+1 values) for the
   * device entries: the engine plans its tiles from it instead of reading
   * group_offsets back from the device (one copy + stream sync per call).
   * NULL = read it back.  Ignored by the host entries.  The engine plans
   * its tiles from this copy and trusts it: it must equal the device array
   * at the call (a stale copy makes the kernels read members past a group;
   * debug builds, -DOTSDB_DEBUG_SYNC, compare the last offset).            */
  const int64_t* group_offsets_host;
} otsdb_batch;

/* ------------------------------------------------------------------------ */
/* Result: caller-allocated (sizes from otsdb_agg_plan).  Group g's points   */
/* are [offsets[g], offsets[g+1]).  Value bits are a long when is_int=1,     */
/* else an IEEE double (AggregationIterator.isInteger, :612-625).            */
/* ------------------------------------------------------------------------ */
typedef struct {
  int64_t capacity;   /* max points the ts/val/is_int arrays can hold      */
  int64_t* offsets;   /* [G+1]                                              */
  int64_t* ts;        /* [capacity]                                         */
  int64_t* val;       /* [capacity] raw bits                                */
  uint8_t* is_int;    /* [capacity]                                         */
} otsdb_result;

typedef struct {
  int64_t n_buckets;        /* grid buckets per series (downsampled path)  */
  int64_t max_out_points;   /* upper bound of total output points: groups x
                             * buckets; n_points on the raw path (each span
                             * in one group); groups x n_points for a
                             * NONE-fill window past 4e9 series x buckets    */
  int64_t workspace_bytes;  /* device scratch this query needs              */
} otsdb_sizes;

typedef struct otsdb_ctx otsdb_ctx;

/* ---- context ------------------------------------------------------------ */
int otsdb_abi_version(void);
/* Creates a context bound to HIP device `device` (one process per GPU).     */
otsdb_status otsdb_ctx_create(int device, otsdb_ctx** out);
void otsdb_ctx_destroy(otsdb_ctx* ctx);
/* Thread-local message of the last failing call on this thread.            */
const char* otsdb_last_error(void);

/* ---- registry (Aggregators.get / toString / interpolationMethod) -------- */
/* Aggregators.get(name): OTSDB_E_NO_SUCH_ELEMENT for unknown names.         */
otsdb_status otsdb_agg_lookup(const char* name, int32_t* agg_id);
const char* otsdb_agg_name(int32_t agg_id);         /* toString()          */
int32_t otsdb_agg_interpolation(int32_t agg_id);    /* otsdb_interp        */

/* ---- query -------------------------------------------------------------- */
/* Validates spec+batch shape and returns output/workspace sizes.            */
otsdb_status otsdb_agg_plan(otsdb_ctx* ctx, const otsdb_query_spec* spec,
                            const otsdb_batch* batch, otsdb_sizes* out);
/* Host-pointer entry (the JNI shim): copies the batch to HBM, runs, copies
 * the result back.  Synchronous.                                            */
otsdb_status otsdb_agg_run(otsdb_ctx* ctx, const otsdb_query_spec* spec,
                           const otsdb_batch* batch, otsdb_result* out);
/* Device-pointer entry: batch and result live in HBM; runs on `hip_stream`
 * (a hipStream_t passed as void*, NULL = the context's stream).  Returns
 * after the result is complete on the device (the status needs the device
 * error word).                                                               */
otsdb_status otsdb_agg_run_device(otsdb_ctx* ctx, const otsdb_query_spec* spec,
                                  const otsdb_batch* batch, otsdb_result* out,
                                  void* hip_stream);

/* ---- rollup queries ------------------------------------------------------ */
/* The single query over the points of a ROLLUP table (pre-aggregated cells):
 * the reference hands Downsampler / FillingDownsampler a RollupQuery and
 * computes two downsampling functions differently (Downsampler.java:162-228,
 * FillingDownsampler.java:196-252).  With R = rollup_agg_id
 * (RollupQuery.getRollupAgg()) and F = spec->ds_agg_id, a bucket's value over
 * its points in time order is
 *   R = avg, F = avg             sum of the values / sum of value_count (a
 *                                Java long: it wraps); NaN is NOT skipped; a
 *                                total count of 0 gives a present 0.0
 *   R not avg / dev, F = count   the sum of the values (they are counts),
 *                                NaN not skipped
 *   R not avg / dev, other F     F as in otsdb_agg_run: the result is that
 *                                call's, value_count is ignored
 *   R = dev                      OTSDB_E_UNSUPPORTED (the reference throws)
 *   R = avg, F not avg           OTSDB_E_UNSUPPORTED (not built; TsdbQuery
 *                                always makes R = F, TsdbQuery.java:1746-1748)
 * Output points are doubles; bucket timestamps, seek, "all", the filling
 * grid, rate, interpolation, every aggregator and the compaction are the
 * single query's over these bucket values.
 * value_count[i] is point i's valueCount() (RollupSeq.java:659-679) — the
 * (sum, count) pairs RollupSeq's iterator yields after its sync(): pairing
 * sum and count cells stays with the caller here (otsdb_agg_run_rollup_rows*
 * below takes the cells themselves).  Required when R = avg (NULL:
 * OTSDB_E_ILLEGAL_ARGUMENT; 16-byte aligned like ts_ms / val on the device
 * entry), otherwise ignored and may be NULL.
 * A spec without a downsampler (ds_interval_ms == 0 and no run_all) or with
 * per-series calendar anchors (n_cal_anchors > 0): OTSDB_E_UNSUPPORTED; an
 * unknown rollup_agg_id: OTSDB_E_NO_SUCH_ELEMENT.  otsdb_agg_plan's n_buckets
 * and max_out_points hold for these calls unchanged.                        */
otsdb_status otsdb_agg_run_rollup_device(otsdb_ctx* ctx,
                                         const otsdb_query_spec* spec,
                                         const otsdb_batch* batch,
                                         int32_t rollup_agg_id,
                                         const int64_t* value_count,
                                         otsdb_result* out, void* hip_stream);
/* Host pointers throughout (value_count too); otsdb_agg_run's
 * OTSDB_E_CAPACITY contract holds.                                          */
otsdb_status otsdb_agg_run_rollup(otsdb_ctx* ctx, const otsdb_query_spec* spec,
                                  const otsdb_batch* batch,
                                  int32_t rollup_agg_id,
                                  const int64_t* value_count,
                                  otsdb_result* out);

/* ---- several aggregators over one downsample pass ----------------------- */
/* The sub-queries of one panel that differ only in the cross-series
 * aggregator (min / avg / max / p99 of the same metric, tags, range and
 * downsampling): agg_ids[i] / interps[i] take the place of spec->agg_id /
 * spec->interp (OTSDB_INTERP_DEFAULT: the aggregator's own), everything else
 * in `spec` is shared.  The point stream is downsampled ONCE into the
 * per-series bucket rows; the scalar aggregators read the rows in one group
 * pass, dev and the selections run their own group stage over the same rows
 * (DESIGN.md §4).  Output i obeys exactly the contract of the single query
 * with that aggregator; duplicates are allowed.  n_out outside
 * [1, OTSDB_MULTI_MAX]: OTSDB_E_ILLEGAL_ARGUMENT; an unknown id:
 * OTSDB_E_NO_SUCH_ELEMENT; when single queries of several outputs would fail
 * the call fails with the status of the lowest-index one.  n_out == 1 is the
 * single query.  Queries that cannot share the rows (raw group-by,
 * per-series calendar anchors, OTSDB_SPEC_EXACT_ORDER dev past the row
 * budget) run their outputs one after another: same results, nothing shared.
 * spec->flags & OTSDB_SPEC_MULTI_FOLD (opt-in): a call whose outputs are all
 * of sum / zimsum / pfsum / avg / count / min / mimmin / max / mimmax and
 * share ONE interpolation (the same default or override for every output, or
 * any fill policy), on a query the single path runs through the ordered fold
 * (downsampled, no rate, no "all", no median / percentile downsampling),
 * through the columnar entries (otsdb_agg_run_multi, _run_multi_device and a
 * panel call of one distinct downsampling function), takes ONE ordered fold
 * over a combined {sum, count, min, max} state: no row matrix, no transform
 * and no group pass (otsdb_ctx_counters [5..8] = 1, 0, 0, 0 and [12] = 1).
 * Output i is reduced over the single query's tiles in the single query's
 * order: bit for bit otsdb_agg_run's for an order-free downsampling function
 * (min, max, count, first, last ...) and on grids of up to 128 buckets,
 * within 1e-12 of it otherwise (sum / avg downsampling on wider grids: the
 * fold's windows differ).  Every other request ignores the
 * flag and runs exactly as without it ([12] = 0); the cells and partials
 * entries never read it (the cells entry has a bit of its own,
 * OTSDB_SPEC_CELLS_MULTI_FOLD).
 * plan_multi: max_out_points bounds EACH output, workspace_bytes the call.  */
#define OTSDB_MULTI_MAX 32
otsdb_status otsdb_agg_plan_multi(otsdb_ctx* ctx, const otsdb_query_spec* spec,
                                  int32_t n_out, const int32_t* agg_ids,
                                  const int32_t* interps,
                                  const otsdb_batch* batch, otsdb_sizes* out);
/* outs: n_out results (HOST array of structs; DEVICE pointers inside).      */
otsdb_status otsdb_agg_run_multi_device(otsdb_ctx* ctx,
                                        const otsdb_query_spec* spec,
                                        int32_t n_out, const int32_t* agg_ids,
                                        const int32_t* interps,
                                        const otsdb_batch* batch,
                                        otsdb_result* outs, void* hip_stream);
/* Host pointers throughout; otsdb_agg_run's OTSDB_E_CAPACITY contract holds
 * per result (the offsets of a result too small are still whole).           */
otsdb_status otsdb_agg_run_multi(otsdb_ctx* ctx, const otsdb_query_spec* spec,
                                 int32_t n_out, const int32_t* agg_ids,
                                 const int32_t* interps,
                                 const otsdb_batch* batch, otsdb_result* outs);

/* ---- several downsampling functions over one point-stream pass ---------- */
/* The sub-queries of one panel that share spans, window, interval, fill
 * policy and groups and differ in the DOWNSAMPLING function as well as in
 * the aggregator — the envelope panel min:5m-min / avg:5m-avg / max:5m-max
 * (one TSQuery carries several TSSubQuerys over the same data,
 * TSQuery.java:172-214; each becomes its own TsdbQuery run,
 * TsdbQuery.java:992-1113).  Output i is the single query with
 * ds_agg_ids[i] / agg_ids[i] / interps[i] in place of spec->ds_agg_id /
 * spec->agg_id / spec->interp, which are ignored; duplicates are allowed.
 * Functions of the envelope set — sum (zimsum, pfsum), avg, count, min
 * (mimmin), max (mimmax) — are reduced from ONE pass over the point stream
 * into one row matrix per distinct function, bit for bit the rows of the
 * single function's pass; each matrix then goes through the multi-aggregator
 * group stage for the outputs that use it.  Everything else
 * runs function by function, one multi-aggregator call per distinct
 * function: a function outside the set, rate, per-series calendar anchors,
 * raw group-by (no downsampler: ds_agg_ids is ignored), grids past the row
 * limits, a single distinct function.  Same results either way.
 * n_out outside [1, OTSDB_MULTI_MAX] or a null id array:
 * OTSDB_E_ILLEGAL_ARGUMENT; an unknown aggregator or downsampler id:
 * OTSDB_E_NO_SUCH_ELEMENT; `none` as a downsampler:
 * OTSDB_E_ILLEGAL_ARGUMENT.  When several outputs fail the call returns the
 * status of the lowest-index one; the outputs before it are complete.
 * otsdb_ctx_counters [10] / [11]: passes over the point stream / row
 * matrices built by the last panel call.
 * plan_panel: max_out_points bounds EACH output, workspace_bytes the call.  */
otsdb_status otsdb_agg_plan_panel(otsdb_ctx* ctx, const otsdb_query_spec* spec,
                                  int32_t n_out, const int32_t* ds_agg_ids,
                                  const int32_t* agg_ids,
                                  const int32_t* interps,
                                  const otsdb_batch* batch, otsdb_sizes* out);
/* outs: n_out results (HOST array of structs; DEVICE pointers inside).
 * TSQuery.java:172-214 / TsdbQuery.java:992-1113.                           */
otsdb_status otsdb_agg_run_panel_device(otsdb_ctx* ctx,
                                        const otsdb_query_spec* spec,
                                        int32_t n_out,
                                        const int32_t* ds_agg_ids,
                                        const int32_t* agg_ids,
                                        const int32_t* interps,
                                        const otsdb_batch* batch,
                                        otsdb_result* outs, void* hip_stream);
/* Host pointers throughout (TSQuery.java:172-214 / TsdbQuery.java:992-1113);
 * otsdb_agg_run's OTSDB_E_CAPACITY contract holds per result (the offsets of
 * a result too small are still whole).                                      */
otsdb_status otsdb_agg_run_panel(otsdb_ctx* ctx, const otsdb_query_spec* spec,
                                 int32_t n_out, const int32_t* ds_agg_ids,
                                 const int32_t* agg_ids, const int32_t* interps,
                                 const otsdb_batch* batch, otsdb_result* outs);

/* ---- multi-GPU (series-sharded) ----------------------------------------- */
/* Partial per-(group, bucket) reduction state, the unit exchanged between
 * ranks over RCCL.  32 bytes, see DESIGN.md §Multi-GPU.                     */
typedef struct {
  double x, y, z;
  int64_t w;
} otsdb_partial;

/* Runs the local shard (downsample/rate/interpolate + chunked group reduce)
 * and writes one partial per (group, bucket) plus the emit mask into DEVICE
 * buffers partials[G*n_buckets], emit[G*n_buckets].  n_buckets from plan.   */
otsdb_status otsdb_agg_partials_device(otsdb_ctx* ctx,
                                       const otsdb_query_spec* spec,
                                       const otsdb_batch* batch,
                                       otsdb_partial* partials,
                                       uint8_t* emit, void* hip_stream);
/* The same, each (group, bucket) continuing from `init`/`init_emit` (DEVICE,
 * [G*n_buckets]): the state of the group's members on the ranks before this
 * one.  Handed from rank to rank in series order, the last rank's output is
 * the state ONE pass over every member in SpanCmp order reaches — for `dev`
 * the reference's single Welford loop (StdDev.runDouble,
 * src/core/Aggregators.java:547-568, fed by AggregationIterator.java:735-797)
 * bit for bit while each rank's share of a group is one chain
 * (<= 65,536 members), where merging per-rank partials (Chan's formula)
 * lands ~1e-11 from it on offset data.  Groups with no member on this rank
 * pass their state on unchanged; init may alias partials.  Finalise the last
 * rank's output with otsdb_agg_finalize_device(n_ranks = 1).              */
otsdb_status otsdb_agg_partials_chained_device(otsdb_ctx* ctx,
                                               const otsdb_query_spec* spec,
                                               const otsdb_batch* batch,
                                               const otsdb_partial* init,
                                               const uint8_t* init_emit,
                                               otsdb_partial* partials,
                                               uint8_t* emit, void* hip_stream);
/* Combines `n_ranks` partial sets laid out rank-major in DEVICE memory
 * ([n_ranks][G*n_buckets], combined in rank order = series order) and
 * writes the final result (DEVICE pointers).                                */
otsdb_status otsdb_agg_finalize_device(otsdb_ctx* ctx,
                                       const otsdb_query_spec* spec,
                                       int64_t n_groups, int64_t n_buckets,
                                       int32_t n_ranks,
                                       const otsdb_partial* partials,
                                       const uint8_t* emit,
                                       otsdb_result* out, void* hip_stream);

/* ---- several aggregators across ranks: shared partials ------------------ */
/* The multi-aggregator call (otsdb_agg_run_multi*) over series-sharded
 * ranks: the spans of one group (TsdbQuery.java:992-1113 builds one
 * SpanGroup per aggregator of a panel over the same spans) are spread over
 * GPUs.  Each rank downsamples its shard ONCE and writes, for every output
 * i, one partial per (group, bucket) into partials[i][G*n_buckets] (DEVICE,
 * output-major) plus ONE emit mask for all outputs: a (group, bucket) is
 * emitted iff some member has a real point in it
 * (AggregationIterator.java:514-567), whatever the aggregator, so the mask
 * does not depend on the output.  agg_ids / interps and their checks are
 * otsdb_agg_run_multi_device's.  Slice i of `partials` with `emit` is what
 * otsdb_agg_partials_device writes for aggregator i up to the order of the
 * local reduction (and a valid input of otsdb_agg_finalize_device).  Scalar
 * aggregators share one group pass; `dev` takes its own pass over the shared
 * rows and its per-rank states are merged by Chan's formula (handing states
 * on from rank to rank stays with otsdb_agg_partials_chained_device).
 * Median / p* / ep* are refused with OTSDB_E_ILLEGAL_ARGUMENT: they take the
 * otsdb_sel_* protocol (otsdb_sel_retarget for several of them).  What
 * otsdb_agg_partials_device refuses (raw group-by, per-series calendar
 * anchors, grids past 4e9 cells): OTSDB_E_UNSUPPORTED.  n_out == 1 and
 * queries whose outputs cannot share the rows run the outputs one after
 * another: same results, otsdb_ctx_counters [5] == n_out.                   */
otsdb_status otsdb_agg_partials_multi_device(otsdb_ctx* ctx,
                                             const otsdb_query_spec* spec,
                                             int32_t n_out,
                                             const int32_t* agg_ids,
                                             const int32_t* interps,
                                             const otsdb_batch* batch,
                                             otsdb_partial* partials,
                                             uint8_t* emit, void* hip_stream);
/* Combines the ranks' partial sets, DEVICE [n_ranks][n_out][G*n_buckets]
 * with emit [n_ranks][G*n_buckets], in rank order (= series order) and
 * writes output i into outs[i] (HOST array of n_out structs, DEVICE pointers
 * inside): bit for bit what otsdb_agg_finalize_device gives for slice i.
 * Returns the status of the lowest-index failing output.                    */
otsdb_status otsdb_agg_finalize_multi_device(otsdb_ctx* ctx,
                                             const otsdb_query_spec* spec,
                                             int32_t n_out,
                                             const int32_t* agg_ids,
                                             const int32_t* interps,
                                             int64_t n_groups,
                                             int64_t n_buckets,
                                             int32_t n_ranks,
                                             const otsdb_partial* partials,
                                             const uint8_t* emit,
                                             otsdb_result* outs,
                                             void* hip_stream);

/* ---- multi-GPU median / percentiles (series-sharded) -------------------- */
/* Exact selection across ranks: digit histograms summed over
 * the ranks, at most two passes over each rank's local keys.  The protocol,
 * every rank in step:
 *
 *   otsdb_sel_prepare_device(ctx, spec, batch, counts, emit, krange)
 *       local shard -> per-(group, bucket) non-NaN contribution counts
 *       (int64 [G*n_buckets]), emit flags (u8) and key range (int64
 *       [G*n_buckets][2]) in DEVICE memory
 *   all-reduce counts (sum), emit (max), krange (min)
 *   for pass = 0, 1, ...:
 *       otsdb_sel_hist_device(ctx, pass, counts, emit, krange, hist_prev,
 *                             hist, &more)
 *           pass 0 reads the global counts / emit / krange; a later pass
 *           applies hist_prev, the global histogram of the pass before (it
 *           may be `hist` itself).  more == 0: the selection is resolved,
 *           leave the loop.  more == 1: `hist` holds this rank's histogram
 *           of the pass, u32 [G*n_buckets][OTSDB_SEL_BINS]; all-reduce it
 *           (sum)
 *   otsdb_sel_pick_device(ctx, picks)
 *       int64 [G*n_buckets][2]: the key of an order statistic whose bin
 *       holds one key over all ranks, from the rank holding it, else 0
 *   all-reduce picks (sum)
 *   otsdb_sel_finish_device(ctx, picks, result)
 *
 * Pass 0 bins an offset digit, (key >> s) - (min >> s) over the global key
 * range (2,048 bins); pass 1 the next 11 bits (2 x 10 when the estimator's
 * two order statistics sit in different bins) and compacts the local keys
 * still in play into a candidate pool; later passes and the pick read the
 * pool only.  Local key-matrix reads: two at most (otsdb_ctx_counters [3]).
 * otsdb_sel_hist_device reads its plan back (one stream sync) but returns
 * without waiting for the histogram kernels: the caller's collective must be
 * ordered after them on hip_stream (an RCCL all-reduce enqueued there is); a
 * binding that reads `hist` from the host or from another stream calls
 * otsdb_sel_hist_wait(ctx, hip_stream) first; the same holds for `picks`.
 * Every rank ends with the full result.  The batch's group_offsets span all
 * G global groups (empty where the rank holds no member).  Between prepare
 * and finish the context must not run other queries (the session lives in
 * its workspace): every other entry that takes the context (run*,
 * partials*, finalize*, decode, ...; not plan, the counters or the
 * profiling reads) ENDS the session, and the next otsdb_sel_* call other
 * than prepare returns OTSDB_E_ILLEGAL_STATE instead of reading overwritten
 * keys.  Replaces PercentileAgg/Median.runDouble over the spans of
 * a group (Aggregators.java:397-431, :657-708) when the spans are spread
 * over GPUs.
 *
 * Several percentiles of one panel (p99 + p999: one PercentileAgg per
 * sub-query over the same spans, Aggregators.java:657-708):
 *
 *   otsdb_sel_retarget(ctx, agg_id)
 *       legal while a session exists: after a successful prepare, also after
 *       finish.  Re-aims the session at another median / p* / ep* and resets
 *       its pass state; the caller runs hist (pass 0 with the SAME already
 *       all-reduced counts / emit / krange), pick and finish again.  No new
 *       prepare, downsample or key transpose and no new all-reduce of counts
 *       / emit / krange: the local keys and those three do not depend on the
 *       percentile.  Not a selection, or one whose own interpolation differs
 *       from the prepared aggregator's while the spec leaves the
 *       interpolation to the aggregator and has no fill policy (the prepared
 *       contributions would differ): OTSDB_E_ILLEGAL_ARGUMENT; no session:
 *       OTSDB_E_ILLEGAL_STATE.                                              */
#define OTSDB_SEL_BINS 2048
otsdb_status otsdb_sel_prepare_device(otsdb_ctx* ctx,
                                      const otsdb_query_spec* spec,
                                      const otsdb_batch* batch,
                                      int64_t* counts, uint8_t* emit,
                                      int64_t* krange, void* hip_stream);
otsdb_status otsdb_sel_hist_device(otsdb_ctx* ctx, int32_t pass,
                                   const int64_t* counts, const uint8_t* emit,
                                   const int64_t* krange, uint32_t* hist_prev,
                                   uint32_t* hist, int32_t* more,
                                   void* hip_stream);
otsdb_status otsdb_sel_pick_device(otsdb_ctx* ctx, int64_t* picks,
                                   void* hip_stream);
otsdb_status otsdb_sel_finish_device(otsdb_ctx* ctx, const int64_t* picks,
                                     otsdb_result* out, void* hip_stream);
otsdb_status otsdb_sel_retarget(otsdb_ctx* ctx, int32_t agg_id);
/* Blocks until the kernels otsdb_sel_hist_device / _pick_device enqueued on
 * hip_stream (NULL: the context's stream) are done.                         */
otsdb_status otsdb_sel_hist_wait(otsdb_ctx* ctx, void* hip_stream);

/* ---- compacted-cell decode (RowSeq) ------------------- */
/* The storage rows of a query as the scanner hands them to Span.addRow
 * (Span.java:177-220): one compacted column per (series, hour) row —
 * concatenated 2-byte (seconds) / 4-byte (ms) qualifiers and concatenated
 * big-endian values, plus the trailing meta byte of multi-value columns
 * (CompactionQueue.buildCompactedColumn, CompactionQueue.java:594-616).
 * Rows sorted by (series, base time).  DEVICE pointers.                     */
typedef struct {
  int64_t n_rows;            /* R                                          */
  const int64_t* row_series; /* [R] series index, nondecreasing            */
  const int64_t* row_base_s; /* [R] row base time, seconds                 */
  const int64_t* qual_off;   /* [R+1] offsets into qual                    */
  const uint8_t* qual;       /* qualifier bytes                            */
  const int64_t* val_off;    /* [R+1] offsets into val                     */
  const uint8_t* val;        /* value bytes                                */
} otsdb_cells;

/* Decodes the rows into a columnar batch (RowSeq.Iterator semantics,
 * RowSeq.java:552-643): offsets[S+1] (series point CSR), ts_ms/val/is_float
 * [capacity].  Pass ts_ms=NULL to only count (offsets filled, offsets[S] =
 * points).  A column whose value bytes do not match its qualifiers is
 * OTSDB_E_ILLEGAL_DATA (Internal.extractDataPoints, Internal.java:307-321). */
otsdb_status otsdb_decode_cells_device(otsdb_ctx* ctx, const otsdb_cells* cells,
                                       int64_t n_series, int64_t* offsets,
                                       int64_t* ts_ms, int64_t* val,
                                       uint8_t* is_float, int64_t capacity,
                                       void* hip_stream);

/* Test / bench infrastructure (not the query path): encodes a columnar
 * DEVICE batch into compacted RowSeq columns, the layout the write path and
 * compaction produce and otsdb_decode_cells_device reads (one row per
 * (series, hour); 2-byte qualifiers for whole seconds, 4-byte ms qualifiers
 * otherwise; doubles in 8 bytes, longs in the smallest of 1/2/4/8; the meta
 * byte on multi-value columns; Internal.java:848-863, TSDB.java:1051-1147,
 * CompactionQueue.java:594-616).  Two calls: with cells == NULL it writes
 * per-series counts (rows, qualifier bytes, value bytes) into series_rows /
 * series_qbytes / series_vbytes [S]; then, with those arrays turned into
 * exclusive prefix sums by the caller, it writes the cells (qual_off[R] and
 * val_off[R] are the caller's totals).  Values are typed by
 * batch->series_float (NULL = doubles).                                    */
typedef struct {
  int64_t* row_series;  /* [R] */
  int64_t* row_base_s;  /* [R] */
  int64_t* qual_off;    /* [R+1] */
  uint8_t* qual;
  int64_t* val_off;     /* [R+1] */
  uint8_t* val;
} otsdb_cells_out;

otsdb_status otsdb_encode_cells_device(otsdb_ctx* ctx, const otsdb_batch* batch,
                                       int64_t* series_rows,
                                       int64_t* series_qbytes,
                                       int64_t* series_vbytes,
                                       const otsdb_cells_out* cells,
                                       void* hip_stream);

/* The query straight from compacted columns (DEVICE pointers): the decode
 * runs fused into the downsample (no columnar copy).
 * `batch` supplies n_series and the groups only (its point arrays are not
 * read); series s owns the rows with row_series == s.  A corrupt column is
 * OTSDB_E_ILLEGAL_DATA.  Queries the fused path does not cover (raw
 * group-by, median / percentile or "all" downsampling, columns mixing 2-
 * and 4-byte qualifiers) are decoded into a context-owned columnar buffer
 * first and run through the columnar pipeline — same results.           */
otsdb_status otsdb_agg_run_cells_device(otsdb_ctx* ctx,
                                        const otsdb_query_spec* spec,
                                        const otsdb_cells* cells,
                                        const otsdb_batch* batch,
                                        otsdb_result* out, void* hip_stream);
/* Several aggregators over one decode + downsample of the columns
 * (otsdb_agg_run_multi_device's contract; the routing between the fused
 * decode and the columnar buffer is otsdb_agg_run_cells_device's).
 * spec->flags & OTSDB_SPEC_CELLS_MULTI_FOLD (opt-in, read by this entry and
 * by otsdb_agg_run_cells_panel_device for a request of one distinct
 * downsampling function, by no other): a request OTSDB_SPEC_MULTI_FOLD would
 * fold from columns — envelope aggregators of one interpolation class on a
 * downsampled, non-rate query — over a narrow (fixed-interval) grid takes ONE
 * cells fold over the {sum, count, min, max} state: the columns are decoded
 * once, no row matrix, no transform, no group pass (otsdb_ctx_counters
 * [5..8] = 1, 0, 0, 0; [12] = the folds launched: 1, or 2 when the uniform
 * kernel missed and the general one ran again).  Output i is what
 * otsdb_agg_run_cells_device gives for aggregator i: bit for bit for an
 * order-free downsampling function and on grids of up to 128 buckets, within
 * 1e-12 otherwise.  Columns the cells fold does not take are decoded and run
 * as without the flag; every other request ignores it ([12] = 0).          */
otsdb_status otsdb_agg_run_cells_multi_device(otsdb_ctx* ctx,
                                              const otsdb_query_spec* spec,
                                              int32_t n_out,
                                              const int32_t* agg_ids,
                                              const int32_t* interps,
                                              const otsdb_cells* cells,
                                              const otsdb_batch* batch,
                                              otsdb_result* outs,
                                              void* hip_stream);
/* A panel request from the columns (otsdb_agg_run_panel_device's contract and
 * argument checks; the routing is otsdb_agg_run_cells_device's): output i is
 * what otsdb_agg_run_cells_device gives for ds_agg_ids[i] / agg_ids[i] /
 * interps[i].  Two or more distinct functions of the envelope set are reduced
 * from ONE decode of each series' columns into one row matrix per function,
 * bit for bit the rows of the single function's cells pass (DESIGN.md
 * §4.2.1) — in place of one cells query per function, each decoding the same
 * ≈10 B / point again, or a caller-side decode to 16 B / point columns before
 * otsdb_agg_run_panel_device.  A column mixing qualifier widths is rewritten
 * once and the pass runs again; a corrupt column is OTSDB_E_ILLEGAL_DATA for
 * every output.  The other functions of such a request run one cells call
 * each; one distinct function is otsdb_agg_run_cells_multi_device.  What the
 * fused path does not take ("all" downsampling, rate, per-series calendar
 * anchors, raw group-by, grids past the row limits) is decoded once into the
 * context-owned columnar buffer and runs as otsdb_agg_run_panel_device.
 * Same results either way; otsdb_ctx_counters [10] / [11] as for the columnar
 * entry (a pass run again after the rewrite counts again).                  */
otsdb_status otsdb_agg_run_cells_panel_device(otsdb_ctx* ctx,
                                              const otsdb_query_spec* spec,
                                              int32_t n_out,
                                              const int32_t* ds_agg_ids,
                                              const int32_t* agg_ids,
                                              const int32_t* interps,
                                              const otsdb_cells* cells,
                                              const otsdb_batch* batch,
                                              otsdb_result* outs,
                                              void* hip_stream);
/* otsdb_agg_run_cells_device with HOST pointers (the JNI entry at the
 * TsdbQuery seam: the Spans' RowSeq bytes, SpanGroup members); copies in, runs, copies the
 * result out.  Synchronous.  row_series must be nondecreasing.            */
otsdb_status otsdb_agg_run_cells(otsdb_ctx* ctx, const otsdb_query_spec* spec,
                                 const otsdb_cells* cells,
                                 const otsdb_batch* batch, otsdb_result* out);

/* ---- storage rows: query-time compaction + span assembly (§8a a3, a4) -- */
/* The storage rows of a query exactly as the scanner returns them, before
 * TSDB.compact (SaltScanner.java:849-881): each row (one series, one base
 * hour) is a list of columns — single-point cells, compacted columns, append
 * columns (qualifier {0x05,0,0}), annotations / histograms (skipped).        */
typedef struct {
  int64_t n_rows;               /* R                                        */
  const int64_t* row_series;    /* [R] series index, nondecreasing; a series'
                                 * rows in the order the scanner delivers them
                                 * (the Span.addRow call order)            */
  const int64_t* row_base_s;    /* [R] row base time, seconds (row key)     */
  const int64_t* row_col_off;   /* [R+1] CSR into the columns               */
  const int64_t* col_qual_off;  /* [C+1] offsets into qual                  */
  const uint8_t* qual;          /* column qualifiers                        */
  const int64_t* col_val_off;   /* [C+1] offsets into val                   */
  const uint8_t* val;           /* column values                            */
  const int64_t* col_ts;        /* [C] HBase cell timestamps (newest wins a
                                 * duplicate); NULL = ascending column order */
} otsdb_raw_rows;

/* CompactionQueue.compact of every row (CompactionQueue.java:340-616, with
 * ColumnDatapointIterator fix-ups :73-87 / Internal.java:535-591 and
 * AppendDataPoints.parseKeyValue :118-236): one compacted column per row,
 * rows without a data point dropped (as the scanner drops a null
 * compaction), kept rows packed in input order into `out` (DEVICE pointers,
 * caller-allocated: qual_capacity >= the input's qualifier + value bytes and
 * val_capacity >= its value bytes + n_rows always suffice).  *n_out_rows =
 * kept rows; out->qual_off[n] / val_off[n] hold the totals; out->row_series
 * may be NULL.  out == NULL: sizes only.  Duplicate offsets with different
 * values: OTSDB_E_ILLEGAL_DATA unless fix_duplicates
 * (tsd.storage.fix_duplicates); corrupt cells / appends: OTSDB_E_ILLEGAL_DATA;
 * an odd qualifier starting 0x05 that is not 3 bytes:
 * OTSDB_E_ILLEGAL_ARGUMENT; a row needing a merge of more than 8192 points
 * or 4096 data columns: OTSDB_E_UNSUPPORTED.  The first failing row (in row
 * order) decides the status.                                               */
otsdb_status otsdb_compact_rows_device(otsdb_ctx* ctx, const otsdb_raw_rows* raw,
                                       int32_t fix_duplicates,
                                       const otsdb_cells_out* out,
                                       int64_t qual_capacity,
                                       int64_t val_capacity,
                                       int64_t* n_out_rows, void* hip_stream);

/* Span.addRow of every series' compacted rows in arrival order
 * (Span.java:177-220, RowSeq.addRow RowSeq.java:91-222, checkRowOrder
 * :387-392): rows of the same key merge, rows end up sorted by base time.
 * `cells` rows carry nondecreasing row_series; out (DEVICE, caller-allocated,
 * capacities >= the input's bytes + n_rows) receives the span rows; NULL =
 * sizes only.  A row without a qualifier is OTSDB_E_ILLEGAL_ARGUMENT.       */
otsdb_status otsdb_span_assemble_device(otsdb_ctx* ctx, const otsdb_cells* cells,
                                        int64_t n_series,
                                        const otsdb_cells_out* out,
                                        int64_t qual_capacity,
                                        int64_t val_capacity,
                                        int64_t* n_out_rows, void* hip_stream);

/* The whole query from storage rows: compaction -> span assembly -> the
 * fused decode + aggregation of otsdb_agg_run_cells_device.  `batch`
 * supplies n_series and the groups.  _device: DEVICE pointers;
 * otsdb_agg_run_raw: HOST pointers (the JNI entry), synchronous.            */
otsdb_status otsdb_agg_run_raw_device(otsdb_ctx* ctx,
                                      const otsdb_query_spec* spec,
                                      const otsdb_raw_rows* raw,
                                      int32_t fix_duplicates,
                                      const otsdb_batch* batch,
                                      otsdb_result* out, void* hip_stream);
otsdb_status otsdb_agg_run_raw(otsdb_ctx* ctx, const otsdb_query_spec* spec,
                               const otsdb_raw_rows* raw, int32_t fix_duplicates,
                               const otsdb_batch* batch, otsdb_result* out);

/* ---- rollup queries from storage rows ----------------------------------- */
/* The rows of a ROLLUP table as the scanner delivers them (otsdb_raw_rows:
 * one entry per (series, rollup row); rollup cells are never compacted,
 * SaltScanner.java:765-809, so a column is one cell), paired and decoded on
 * the device in place of RollupSpan.addRow (RollupSpan.java:55-72),
 * RollupSeq.setRow / addRow / append (RollupSeq.java:126-322) and
 * RollupIterator's sync() / seek() / value / valueCount() decode (:515-745)
 * under Span.seekRow / Span.Iterator (Span.java:360-471).                    */
typedef struct {
  int32_t interval_s;     /* RollupInterval.getIntervalSeconds()              */
  int32_t value_id;       /* RollupConfig id of the value cells' aggregator
                             ("sum" when R = avg), 0..127                     */
  int32_t count_id;       /* id of "count"; read only when R = avg            */
  int32_t fix_duplicates; /* tsd.storage.fix_duplicates                       */
} otsdb_rollup_table;

/* Decode only, otsdb_decode_cells_device's contract (DEVICE pointers;
 * ts_ms = NULL only counts: offsets filled, offsets[S] = points).  With
 * R = rollup_agg_id:
 *  - R = avg, the tests in this order: qual[0] & 0x7F == value_id: a value
 *    cell; == count_id: a count cell; a qualifier starting with the 3 bytes
 *    "sum": a value cell, old style, 4 bytes stripped; with the 5 bytes
 *    "count": a count cell, 6 stripped (the byte after the name is not
 *    compared, as in the reference: "sumX" passes for "sum:").  Otherwise:
 *    the id, or a qualifier starting with "<R>:" (R's name in lowercase, the
 *    colon compared), stripped.  The 2 bytes after the id / stripped bytes
 *    are offset << 4 | flags.  Any other cell, or one too short:
 *    OTSDB_E_ILLEGAL_DATA (RollupSeq.java:136-161);
 *  - consecutive rows of one series and base time are one RollupSeq; base
 *    times that do not otherwise increase strictly inside a series:
 *    OTSDB_E_UNSUPPORTED (the scanner delivers key order);
 *  - per kind, an offset below the last accepted one, or equal to it without
 *    fix_duplicates: OTSDB_E_ILLEGAL_DATA for a value cell,
 *    OTSDB_E_ILLEGAL_ARGUMENT for a count cell; with fix_duplicates a cell
 *    whose col_ts is older than the last accepted one's is skipped, any other
 *    replaces it (col_ts = NULL: each later duplicate replaces)
 *    (RollupSeq.java:217-322);
 *  - ts_ms = base_s * 1000 + offset * interval_s * 1000; val / is_float as
 *    Internal.extractIntegerValue / extractFloatingPointValue;
 *  - R = avg: the points are the value cells that have a count cell of the
 *    same offset, value_count that cell's value ((long) of a float one: NaN
 *    is 0, saturating); otherwise every accepted value cell is a point and
 *    value_count is not written (may be NULL);
 *  - seek_ms (R = avg; INT64_MIN: none; always milliseconds): the timestamp
 *    the query's downsampler hands its source.  In the row Span.seekRow picks
 *    (the first whose last paired point is >= seek_ms, else the series' last)
 *    the points from seek_ms on are what RollupIterator.seek leaves: value
 *    cells [i0 + k:] paired with count cells [j0 + k:], (i0, j0) the row's
 *    first pair and k its value cells from i0 on before seek_ms — unpaired
 *    cells before the seek point can drop later pairs.  The pairs before
 *    seek_ms are emitted unchanged.
 * Deviations: an offset field >= 3840 (first qualifier byte 0xF0..0xFF) is
 * the millisecond form, which the reference reads past the 2 bytes
 * (RollupUtils.java:213-215): OTSDB_E_UNSUPPORTED.  Value bytes whose length
 * is not the qualifier's, or is none of 1/2/4/8 (a float's 4/8), which the
 * reference appends unchecked and reads misaligned: OTSDB_E_ILLEGAL_DATA.  A
 * row of more than 8,192 columns, or a RollupSeq of more than 65,535:
 * OTSDB_E_UNSUPPORTED.  The first failing row in row order, and the first
 * failing column in it, decides the status.  raw / table NULL or
 * interval_s <= 0: OTSDB_E_ILLEGAL_ARGUMENT; an unknown rollup_agg_id:
 * OTSDB_E_NO_SUCH_ELEMENT; dev: OTSDB_E_UNSUPPORTED.                         */
otsdb_status otsdb_rollup_decode_rows_device(
    otsdb_ctx* ctx, const otsdb_raw_rows* raw, const otsdb_rollup_table* table,
    int32_t rollup_agg_id, int64_t n_series, int64_t seek_ms, int64_t* offsets,
    int64_t* ts_ms, int64_t* val, uint8_t* is_float, int64_t* value_count,
    int64_t capacity, void* hip_stream);

/* The rollup query from the rows: the decode above into a context-owned
 * buffer, then exactly what otsdb_agg_run_rollup_device runs on those columns
 * (the same refusals: R = dev, R = avg with F != avg, no downsampler,
 * per-series calendar anchors).  `batch` supplies n_series and the groups
 * only.  seek_ms is derived from the spec as Downsampler.seekInterval does
 * (Downsampler.java:412-434): start_ms for "all", the first calendar edge at
 * or after start_ms, else start_ms rounded up to a multiple of the interval.
 * _device: DEVICE pointers; otsdb_agg_run_rollup_rows: HOST pointers,
 * synchronous, otsdb_agg_run's OTSDB_E_CAPACITY contract.                    */
otsdb_status otsdb_agg_run_rollup_rows_device(
    otsdb_ctx* ctx, const otsdb_query_spec* spec, const otsdb_raw_rows* raw,
    const otsdb_rollup_table* table, int32_t rollup_agg_id,
    const otsdb_batch* batch, otsdb_result* out, void* hip_stream);
otsdb_status otsdb_agg_run_rollup_rows(
    otsdb_ctx* ctx, const otsdb_query_spec* spec, const otsdb_raw_rows* raw,
    const otsdb_rollup_table* table, int32_t rollup_agg_id,
    const otsdb_batch* batch, otsdb_result* out);

/* ---- histogram queries --------------------------------------------------- */
/* The query over histogram data points (2.4): the group's members are
 * downsampled and summed as histograms and the percentiles are read off the
 * sums — HistogramSpanGroup.iterator (HistogramSpanGroup.java:347-350) with
 * one HistogramDataPointsToDataPointsAdaptor per percentile
 * (TsdbQuery.java:1324-1333), aggregated ONCE here for every percentile.
 *
 * Per series (HistogramDownsampler.java:129-149, :195-377): the seek is the
 * first point >= align(start_ms + interval - 1), align(t) = t - t % interval;
 * bucket b holds the points of [align(t), align(t) + interval), its timestamp
 * is the bucket start; no fill policy, no empty bucket (HistogramSpan.java:
 * 554-563 ignores the fill); a bucket is read to its end even past end_ms.
 * With spec->ds_agg_id == OTSDB_AGG_SUM (the function string is "sum",
 * DownsamplingSpecification.java:153-157) the bucket is the sum of its
 * histograms; with any other function the reference's aggregate(x, null)
 * does nothing and the bucket is its FIRST histogram alone — reproduced.
 * Across a group's members (HistogramAggregationIterator.java:240-287): the
 * output timestamps are the union of the members' bucket timestamps <=
 * end_ms, the value at each the SUM of the members with a bucket exactly
 * there; nothing is interpolated.  spec->agg_id, interp, fill and the rate
 * fields are ignored, as the reference ignores them (TsdbQuery.java:1200,
 * :1277).  Sums are Java long additions (they wrap), per (lower, upper) key,
 * underflow and overflow likewise (SimpleHistogram.java:246-261).
 *
 * Percentile p, a float widened to double (SimpleHistogram.java:124-164):
 * p < 1.0 || p > 100.0 gives -1.0; int bucketSum is the wrapping 32-bit sum
 * of every count's intValue(); walking the keys in order, long running +=
 * intValue() and area = running * 100.0 / bucketSum (separate double
 * operations); the first key with area >= p gives (double)((lower + upper) /
 * 2) in float arithmetic; no such key (bucketSum == 0 with NaN areas, a NaN
 * p) gives 0.0.  Underflow and overflow take no part.
 *
 * Columns.  The batch supplies offsets, ts_ms and the groups (val, is_float,
 * series_float are not read and may be NULL).  lower / upper: the query's
 * bucket schema, HOST memory on every entry, n_bins = K keys strictly
 * ascending in TreeMap order — Float.compare on lower, then on upper
 * (HistogramDataPoint.java:147-165); anything else: OTSDB_E_ILLEGAL_ARGUMENT.
 * counts: [n_points][K + 2] int64 row-major, columns K and K + 1 the
 * underflow and overflow; one point is one contiguous record (8-byte aligned;
 * 16-byte loads when K is even and the matrix 16-byte aligned).  A HOST
 * pointer for otsdb_hist_run, a DEVICE pointer for the _device entries.
 * Decoding the stored blobs stays with the caller here (codecs are plugins,
 * HistogramCodecManager; the Java side holds decoded objects);
 * otsdb_hist_run_rows below decodes SimpleHistogramDecoder's.  The schema is
 * the union of the keys of every histogram of the query; a histogram that
 * lacks a key passes 0 there.  A zero-count key can never be the one a
 * percentile picks — its area equals its predecessor's, which did not
 * qualify, or at the start is +-0.0 or NaN, below every valid p — so the
 * padding changes no percentile.  The merged-counts output cannot tell a key
 * absent from every member from one whose counts sum to 0.
 *
 * Result: group g's points are [offsets[g], offsets[g + 1]); ts [capacity];
 * pct_val [n_pct][capacity] doubles, percentile q of point i at
 * pct_val[q * capacity + i] (every percentile shares offsets and ts); counts,
 * optional (NULL skips it), [capacity][K + 2]: the merged histograms
 * (HistogramBucketDataPointsAdaptor, show_histogram_buckets).
 *
 * Limits: K < 1, a NULL schema, n_pct < 0, n_pct == 0 with a NULL
 * result->counts, start_ms < 0: OTSDB_E_ILLEGAL_ARGUMENT.  K + 2 >
 * OTSDB_HIST_MAX_ROW, n_pct > OTSDB_HIST_MAX_PCT, ds_interval_ms == 0 (the
 * raw timestamp union), run_all, use_calendar, a grid whose first bucket is
 * timestamp 0 (the reference's "end reached" mark): OTSDB_E_UNSUPPORTED.  A
 * dense array n_groups x n_buckets x (K + 2) x 8 bytes past
 * OTSDB_HIST_DENSE_BYTES: OTSDB_E_CAPACITY.  All of these are decided before
 * any device work.  A result capacity too small: OTSDB_E_CAPACITY with the
 * offsets whole (otsdb_agg_run's contract).  The cells, multi and panel
 * entries do not take histograms.                                           */
#define OTSDB_HIST_MAX_ROW 256
#define OTSDB_HIST_MAX_PCT 16
#define OTSDB_HIST_DENSE_BYTES (8LL << 30)
typedef struct {
  int32_t n_bins;        /* K                                               */
  const float* lower;    /* [K] HOST                                        */
  const float* upper;    /* [K] HOST                                        */
  const int64_t* counts; /* [n_points][K + 2]                               */
} otsdb_hist_columns;

typedef struct {
  int64_t capacity;
  int64_t* offsets;  /* [G+1]                                               */
  int64_t* ts;       /* [capacity]                                          */
  double* pct_val;   /* [n_pct][capacity]; may be NULL when n_pct == 0      */
  int64_t* counts;   /* [capacity][K + 2] or NULL                           */
} otsdb_hist_result;

/* n_buckets, max_out_points (groups x buckets) and workspace_bytes, as
 * otsdb_agg_plan returns them; the checks above.  ctx is not read.         */
otsdb_status otsdb_hist_plan(otsdb_ctx* ctx, const otsdb_query_spec* spec,
                             const otsdb_batch* batch,
                             const otsdb_hist_columns* hist, otsdb_sizes* out);
/* Host pointers throughout; synchronous.                                   */
otsdb_status otsdb_hist_run(otsdb_ctx* ctx, const otsdb_query_spec* spec,
                            const otsdb_batch* batch,
                            const otsdb_hist_columns* hist,
                            const float* percentiles, int32_t n_pct,
                            otsdb_hist_result* out);
/* Device pointers (schema and percentiles stay HOST); returns after the
 * result is complete on the device.                                        */
otsdb_status otsdb_hist_run_device(otsdb_ctx* ctx, const otsdb_query_spec* spec,
                                   const otsdb_batch* batch,
                                   const otsdb_hist_columns* hist,
                                   const float* percentiles, int32_t n_pct,
                                   otsdb_hist_result* out, void* hip_stream);
/* The two halves of the run, for series-sharded ranks.  partials: the local
 * shard's dense sums, DEVICE int64 [G][n_buckets][K + 2] and uint8 emit
 * [G][n_buckets] (1: some local member has a bucket there), every cell
 * written (0 where nothing was added).  The ranks' arrays combine by plain
 * integer addition (all-reduce SUM on dense, MAX on emit) in any order: the
 * same bits as one rank over every series.  finalize: percentiles and the
 * compacted result from such arrays; hist supplies the schema (counts is not
 * read); n_buckets must be the plan's.                                     */
otsdb_status otsdb_hist_partials_device(otsdb_ctx* ctx,
                                        const otsdb_query_spec* spec,
                                        const otsdb_batch* batch,
                                        const otsdb_hist_columns* hist,
                                        int64_t* dense, uint8_t* emit,
                                        void* hip_stream);
otsdb_status otsdb_hist_finalize_device(otsdb_ctx* ctx,
                                        const otsdb_query_spec* spec,
                                        const otsdb_hist_columns* hist,
                                        int64_t n_groups, int64_t n_buckets,
                                        const int64_t* dense,
                                        const uint8_t* emit,
                                        const float* percentiles,
                                        int32_t n_pct, otsdb_hist_result* out,
                                        void* hip_stream);
/* Host-only planning: the buckets one workgroup of the histogram fold holds
 * for rows of n_bins + 2 counts (0 outside the limits).  Decides speed, not
 * results; tests take the window edges from it.                            */
int32_t otsdb_hist_window(int32_t n_bins);

/* ---- histogram queries from storage rows --------------------------------- */
/* The histogram query from what the scanner delivers: `raw` holds the rows,
 * one entry per (series, base hour), row_series nondecreasing (col_ts is not
 * read); the stored blobs are decoded on the device for the one codec the
 * reference ships, SimpleHistogramDecoder, whose id in
 * tsd.core.histograms.config is simple_codec_id (0..255).
 *
 * A histogram cell is a column whose qualifier has odd length and starts
 * with 0x06 (HistogramDataPoint.PREFIX; CompactionQueue.java:441-452,
 * SaltScanner.java:788-795); every other column — data cells, compacted
 * columns, appends, annotations, an even-length 06 xx — is ignored.
 * Timestamp (Internal.getTimeStampFromNonDP, Internal.java:1059-1074): a
 * 3-byte qualifier gives (base_s + (signed q[1] << 8 | q[2])) * 1000, a
 * 5-byte one base_s * 1000 + int32(q[1..4] big-endian).  Value
 * (Internal.decodeHistogramDataPoint :1095-1104, SimpleHistogram.fromHistogram
 * SimpleHistogram.java:97-122): the id byte, a big-endian signed short
 * bucketCount, bucketCount times {float lower, float upper (big-endian IEEE
 * bits), var-long count}, then var-long underflow and overflow; trailing
 * bytes are ignored, bucketCount <= 0 reads no bucket, a key repeated in one
 * blob keeps the later count, keys are equal when Float.compare is 0 on both
 * bounds (every NaN one key).  The var-long is Kryo 3.0.0's
 * Output.writeLong(v, true): 7 value bits a byte from the least significant
 * group, bit 7 "another byte follows", a ninth byte taken whole (1..9 bytes,
 * a negative long always 9).  The byte format is pinned by the hand-derived
 * vectors of tests/golden/kat_hist_rows.json, not by a run of the reference.
 * What throws in the reference's decode is logged and SKIPPED there
 * (catch Throwable) and here — an empty value or one under 6 bytes, a read
 * past the value's end, a qualifier of odd length other than 3 or 5: the
 * point does not exist, and a row left without one is no row.
 * Span assembly (HistogramSpan.addRow :280-328, HistogramRowSeq.addRow
 * :66-105): a row's points are its surviving cells in column order;
 * consecutive rows of one series and base time are one row sequence, merged
 * by timestamp, the earlier row keeping an equal one.
 *
 * Deviations, all OTSDB_E_UNSUPPORTED: a cell whose id byte is not
 * simple_codec_id (another codec may decode it in the reference; checked
 * after the qualifier's length, before the value's); bucketCount > 254,
 * checked before the walk (the reference would read on); timestamps that do
 * not strictly increase along a row's surviving cells (the reference keeps
 * column order); base times that decrease inside a series in arrival order
 * (the reference's out-of-order replay is not restated); more than 64
 * consecutive rows of one key; an assembled series whose timestamps do not
 * strictly increase from one row sequence to the next (offsets that leave
 * the row's hour).  A decodable cell's key outside the supplied schema:
 * OTSDB_E_ILLEGAL_ARGUMENT.  The first failing row in row order, then the
 * first failing column in it, decides the status (a failure of the row as a
 * whole counts before its columns; the cross-row timestamp check is made
 * when nothing else failed).  NULL raw or arrays, simple_codec_id outside
 * 0..255, and on the decode and query entries a NULL hist / schema or
 * n_bins < 1: OTSDB_E_ILLEGAL_ARGUMENT, before any device work.
 *
 * otsdb_ctx_counters, of the last of these calls: [15] histogram cells
 * decoded into points, [16] cells skipped as undecodable (what the reference
 * logs), [17] points dropped by a same-key merge.                           */

/* The query's bucket schema: the union of the keys of every cell that
 * decodes, sorted in TreeMap order into HOST arrays of OTSDB_HIST_MAX_ROW - 2
 * floats; *n_bins may come back 0.  More than 254 distinct keys:
 * OTSDB_E_UNSUPPORTED.  raw: DEVICE pointers.  Synchronous.                 */
otsdb_status otsdb_hist_rows_schema_device(otsdb_ctx* ctx, const otsdb_raw_rows* raw,
                                           int32_t simple_codec_id,
                                           float* lower, float* upper,
                                           int32_t* n_bins, void* hip_stream);
/* The decode alone, otsdb_rollup_decode_rows_device's contract: hist gives
 * the schema (its counts is not read); offsets [n_series + 1], ts_ms [N] and
 * counts [N][K + 2] are DEVICE pointers; ts_ms == NULL only counts (offsets
 * filled, offsets[n_series] the points).  Keys a blob lacks are 0, columns K
 * and K + 1 the underflow and overflow.  capacity below the points:
 * OTSDB_E_CAPACITY.                                                         */
otsdb_status otsdb_hist_decode_rows_device(otsdb_ctx* ctx, const otsdb_raw_rows* raw,
                                           int32_t simple_codec_id,
                                           int64_t n_series,
                                           const otsdb_hist_columns* hist,
                                           int64_t* offsets, int64_t* ts_ms,
                                           int64_t* counts, int64_t capacity,
                                           void* hip_stream);
/* The query from the rows: the decode above into a context-owned buffer,
 * then exactly what otsdb_hist_run_device runs on those columns (the same
 * refusals, limits and result layout; otsdb_ctx_counters [13], [14] alike).
 * `batch` supplies n_series and the groups only; `hist` the schema, required
 * (otsdb_hist_rows_schema_device finds it).  _device: DEVICE pointers;
 * otsdb_hist_run_rows: HOST pointers, synchronous.                          */
otsdb_status otsdb_hist_run_rows_device(otsdb_ctx* ctx, const otsdb_query_spec* spec,
                                        const otsdb_raw_rows* raw,
                                        int32_t simple_codec_id,
                                        const otsdb_batch* batch,
                                        const otsdb_hist_columns* hist,
                                        const float* percentiles, int32_t n_pct,
                                        otsdb_hist_result* out,
                                        void* hip_stream);
otsdb_status otsdb_hist_run_rows(otsdb_ctx* ctx, const otsdb_query_spec* spec,
                                 const otsdb_raw_rows* raw,
                                 int32_t simple_codec_id,
                                 const otsdb_batch* batch,
                                 const otsdb_hist_columns* hist,
                                 const float* percentiles, int32_t n_pct,
                                 otsdb_hist_result* out);

/* ---- top-N over query results: highestMax / highestCurrent --------------- */
/* The gexp functions highestMax(query, N) and highestCurrent(query, N)
 * (src/query/expression/HighestMax.java:40-148, HighestCurrent.java:40-152)
 * over the results of one or more sub-queries, each an otsdb_result as the
 * query entries above write it: the answer is N series, not every group.
 *
 * The series are numbered in list order, then group order; highestMax numbers
 * every series, highestCurrent drops the series without a point first
 * (HighestCurrent.java:95-102).  n = the count.  Both functions run
 * AggregationIterator(views, start_ms, end_ms, agg, LERP, rate = false) over
 * the series (HighestMax.java:110-112): the seek goes to each series' first
 * point >= start_ms; the emissions are the distinct timestamps <= end_ms of
 * the points from there on; series i contributes at x iff it has a point
 * after the seek and first_i <= x <= last_i, last_i its last point even past
 * end_ms; its value is its own point or LERP between its neighbours
 * (nextLongValue's wrapping, truncating long arithmetic on an integer
 * emission, nextDoubleValue on a double one); an emission is integer iff no
 * current or next slot of any series holds a double (a series not yet started
 * shows its first point; AggregationIterator.java:612-625).
 * The aggregator reads the values with nextLongValue / nextDoubleValue, which
 * skip the series that do not contribute: the k-th CONTRIBUTING series' value
 * lands in slot k, the rest of the n-vector is 0, and slot k's key is later
 * taken as series k's key.  Reproduced.
 *   highestMax (MaxCacheAggregator, HighestMax.java:182-292): max_longs[k]
 *     from Long.MIN_VALUE, max_doubles[k] from Double.MIN_VALUE — the smallest
 *     POSITIVE double, so all-negative double series tie at 4.9e-324; every
 *     integer emission folds the whole vector with Math.max (the zero padding
 *     counts), every double emission likewise (NaN is sticky, +0.0 over -0.0;
 *     the padding never changes a slot there).
 *   highestCurrent (MaxLatestAggregator, HighestCurrent.java:164-282):
 *     latest_ts is never updated, so every emission overwrites: max_longs is
 *     the whole vector (padding included) of the LAST integer emission,
 *     max_doubles that of the LAST double emission.
 * key[k]: both kinds of emission seen: Math.max((double)max_longs[k],
 * max_doubles[k]); only integer ones: (double)max_longs[k]; only double ones:
 * max_doubles[k].  The slots are sorted descending by Double.compare, stably
 * (NaN first, ties in ascending k), and min(topn, n) series are returned:
 * output i is the WHOLE point list of series k_i, points outside the window
 * included, values and is_int untouched.
 *
 * Statuses: topn < 1, an unknown function, start_ms < 0: OTSDB_E_ILLEGAL_
 * ARGUMENT; n == 0: OTSDB_OK, nothing picked; an x1 with millisecond-mask bits
 * during LERP: the raw path's OTSDB_E_ILLEGAL_STATE.  Deviations: n > 0 with
 * no emission in the window ends the reference in a NullPointerException
 * (Arrays.sort over null entries, HighestMax.java:139): OTSDB_E_ILLEGAL_STATE
 * here — a deviation in kind; a series whose timestamps do not strictly
 * increase: OTSDB_E_UNSUPPORTED (the results of the query entries never hold
 * one); end_ms >= 2^47, 2^31 series or 2^32 points: OTSDB_E_UNSUPPORTED.
 *
 * grid_interval_ms: the caller's promise that every timestamp of every input
 * point is a multiple of it (every fixed-interval downsampled result), 0 for
 * no promise.  It selects a path, never a result.  With a promise, a window
 * of at most 65,536 grid timestamps and every point a double the call takes
 * the grid path: no sort, no copy of the points, one synchronisation.  A
 * promise that does not hold (an off-grid timestamp, a long, timestamps that
 * do not increase) is found on the device and the general path runs in the
 * same call — as every call without a promise does (any input; O(emissions x
 * series x log points), four synchronisations).  The two are bit-identical
 * wherever both apply.
 * otsdb_ctx_counters [18..20], of the last top-N call: [18] 1 when the grid
 * path was run, [19] 1 when the general path was run, [20] 1 when the grid
 * path's promise did not hold (then [18] = [19] = 1).                        */
typedef enum {
  OTSDB_TOPN_HIGHEST_MAX = 0,     /* "highestMax"     */
  OTSDB_TOPN_HIGHEST_CURRENT = 1  /* "highestCurrent" */
} otsdb_topn_function;

typedef struct {
  int32_t function;          /* otsdb_topn_function                          */
  int32_t topn;              /* N                                            */
  int64_t start_ms;          /* TSQuery.startTime()                          */
  int64_t end_ms;            /* TSQuery.endTime()                            */
  int64_t grid_interval_ms;  /* see above; 0 = no promise                    */
} otsdb_topn_spec;

/* n_out = min(topn, series of every input).  `series`: the picked series in
 * rank order, offsets [n_out + 1] (series i's points are [offsets[i],
 * offsets[i + 1])), ts / val / is_int [capacity]; DEVICE pointers for
 * otsdb_topn_run_device, HOST pointers for otsdb_topn_run.  picked / key:
 * HOST memory on both entries, [n_out] each (NULL skips one): picked[i] is
 * output i's series number in the input's flat numbering — highestMax's,
 * empty series counted, for both functions — and key[i] its key as double
 * bits, NaN canonical (0x7FF8000000000000).  n_picked: outputs written.      */
typedef struct {
  otsdb_result series;
  int64_t* picked;
  int64_t* key;
  int64_t n_picked;
} otsdb_topn_result;

/* Sizes from the inputs' shapes (HOST arrays of n_results entries; no device
 * work, ctx is not read): n_buckets = n_out above, max_out_points = the points
 * of every input (what the n_out longest series can hold at most),
 * workspace_bytes the general path's device scratch (an upper estimate: 17 B
 * a point of columnar view, 24 B of keys, the sorts' own scratch; ~180 B a
 * series).  The spec's checks.                                               */
otsdb_status otsdb_topn_plan(otsdb_ctx* ctx, const otsdb_topn_spec* spec,
                             int32_t n_results, const int64_t* n_groups,
                             const int64_t* n_points, otsdb_sizes* out);
/* results: HOST array of n_results structs with DEVICE pointers inside (what
 * otsdb_agg_run_device and its kin wrote; capacity is not read), n_groups
 * (HOST) each one's group count.  Runs on hip_stream (NULL: the context's)
 * and returns after the result is complete on the device and picked / key /
 * n_picked on the host (the kernels write them to mapped host memory, the
 * pattern of the compaction's {error word, total}: no read-back copies).  A capacity too small: OTSDB_E_CAPACITY with
 * series.offsets, picked, key and n_picked whole (offsets[n_picked] is the
 * capacity a retry needs).  Replaces HighestMax.evaluate /
 * HighestCurrent.evaluate over the DataPoints[] of the sub-queries.          */
otsdb_status otsdb_topn_run_device(otsdb_ctx* ctx, const otsdb_topn_spec* spec,
                                   int32_t n_results,
                                   const otsdb_result* results,
                                   const int64_t* n_groups,
                                   otsdb_topn_result* out, void* hip_stream);
/* Host pointers throughout (the JNI entry at the gexp seam,
 * HighestMax.java:40-41); synchronous; the same OTSDB_E_CAPACITY contract.   */
otsdb_status otsdb_topn_run(otsdb_ctx* ctx, const otsdb_topn_spec* spec,
                            int32_t n_results, const otsdb_result* results,
                            const int64_t* n_groups, otsdb_topn_result* out);

/* ---- stage timing (bench roofline) ------------------------------------- */
/* When enabled, every query records HIP events around its pipeline stages
 * on the query's stream.  otsdb_prof_read returns, per stage, the summed
 * milliseconds and the number of launches since the last reset:
 * [0] k_bucketize  [1] k_transform  [2] k_group+k_combine  [3] k_prep
 * [4] k_compact+k_scan; [5] query-time compaction, [6] span assembly, [7] the
 * decode into the context's columnar buffer (compacted cells, rollup rows);
 * histogram queries: [8] k_hist_prep + k_hist_fold, [9] k_hist_combine,
 * [10] k_hist_percentiles, [11] their compaction; [12] the decode of
 * histogram storage rows (otsdb_hist_run_rows*); [13] a top-N call
 * (otsdb_topn_run*: numbering to gather) (n up to 14).
 * Synchronises the stream.                                                  */
otsdb_status otsdb_prof_enable(otsdb_ctx* ctx, int enable);
otsdb_status otsdb_prof_read(otsdb_ctx* ctx, double* ms, int64_t* launches,
                             int n, int reset);

/* ---- diagnostics ---------------------------------------------------------
 * Counters since the context was created (no reference counterpart: the
 * operator's view of which cells-fold kernel ran): out[0] cells folds run
 * with the uniform kernel (every kept series one value type and width),
 * out[1] with the general one, out[2] uniform folds that met a qualifier of
 * other flags and were re-run with the general kernel; out[3] passes over
 * the local key matrix and out[4] histogram passes of the last otsdb_sel_*
 * session.  Of the last otsdb_agg_*_multi* call: out[5] downsample
 * (bucketize) passes over the point stream, out[6] group-stage passes over
 * a row matrix, out[7] key transposes, out[8] transform passes (one per
 * interpolation class).  out[9]: otsdb_sel_* sessions prepared since the
 * context was created (otsdb_sel_retarget prepares none).  Of the last
 * otsdb_agg_run_panel* call: out[10] passes over the point stream, out[11]
 * row matrices built (the multi calls inside it still maintain [5..8]).
 * out[12]: multi-aggregator folds launched by the last otsdb_agg_*_multi*
 * call (OTSDB_SPEC_MULTI_FOLD on an eligible request: 1, else 0;
 * OTSDB_SPEC_CELLS_MULTI_FOLD: one per cells fold launched, 2 after a uniform
 * miss).  Of the last otsdb_hist_* call: out[13] k_hist_fold launches (one
 * aggregation, whatever the number of percentiles), out[14] percentile
 * passes over the dense sums (1, or 0 when n_pct == 0).  Of the last
 * otsdb_hist_*rows* call: out[15] histogram cells decoded into points,
 * out[16] cells skipped as undecodable, out[17] points dropped by a same-key
 * merge.  Of the last otsdb_topn_* call: out[18] runs of the grid path,
 * out[19] runs of the general path, out[20] grid promises missed (the general
 * path then ran again).                                                     */
otsdb_status otsdb_ctx_counters(otsdb_ctx* ctx, int64_t* out, int n);
/* Test hook: the one-pass compaction's epoch (1 .. 2^24 - 1, forward only)
 * the context's next call increments, so tests can drive it to its wrap.  */
otsdb_status otsdb_test_set_compact_epoch(otsdb_ctx* ctx, uint32_t epoch);

/* ---- synthetic workload generator (bench / tests) ----------- */
/* Generates the columnar batch of `n_series` series starting at global
 * series index `series0` directly in HBM.  Pass offsets=NULL first to get
 * the per-series point counts (written to `counts`, DEVICE [S]).            */
typedef struct {
  uint64_t seed;          /* 42                                              */
  int64_t t0_ms;          /* 1356998400000                                   */
  int64_t duration_ms;    /* 86400000 / 604800000                            */
  int64_t cadence_ms;     /* 10000                                           */
  int32_t kind;           /* 0 = gauge f64, 1 = gauge int64, 2 = counter int64 */
  int32_t flags;          /* 1 = whole-second phases (2-byte qualifiers)     */
} otsdb_gen_spec;

otsdb_status otsdb_gen_counts_device(otsdb_ctx* ctx, const otsdb_gen_spec* g,
                                     int64_t series0, int64_t n_series,
                                     int64_t* counts, void* hip_stream);
otsdb_status otsdb_gen_fill_device(otsdb_ctx* ctx, const otsdb_gen_spec* g,
                                   int64_t series0, int64_t n_series,
                                   const int64_t* offsets, int64_t* ts_ms,
                                   int64_t* val, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* OTSDB_AGG_H */
