// engine_hist.hip — the histogram family of the engine's host side
// (otsdb_hist_*, hist.hip): the argument checks, the tiles,
// the fold / combine / percentile / compaction launches, the decode of
// storage rows (hist_rows.hip, §4.4.1) and the C-ABI entries.  What it shares
// with engine.hip: engine_int.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

#include "../../include/otsdb_agg.h"
// kernels.hip and compact.hip for their device helpers only (bucket_of,
// lower_bound_interp, compact_count, ...): their non-template kernels are
// engine.hip's
#define OTSDB_DS_TU 1
#include "kernels.hip"
#include "compact.hip"
#include "hist.hip"
#include "hist_rows.hip"
#include "engine_int.h"

using namespace otsdb;
using namespace otsdb::eng;

namespace {

// Float.compare (HistogramBucket.compareTo's order): -0.0 below 0.0, NaN
// above everything and equal to itself
int float_compare(float a, float b) {
  if (a < b) return -1;
  if (a > b) return 1;
  auto bits = [](float f) {
    int32_t i;
    memcpy(&i, &f, 4);
    return f != f ? (int32_t)0x7fc00000 : i;  // floatToIntBits
  };
  const int32_t ia = bits(a), ib = bits(b);
  return ia == ib ? 0 : (ia < ib ? -1 : 1);
}

// the argument checks of every histogram entry and the grid: no device work
otsdb_status hist_check(const otsdb_query_spec* s, const otsdb_hist_columns* h,
                        int32_t n_pct, Params* P) {
  if (h->n_bins < 1)
    return fail(OTSDB_E_ILLEGAL_ARGUMENT, "histogram schema of %d buckets",
                h->n_bins);
  if (h->n_bins + 2 > kHistMaxRow)
    return fail(OTSDB_E_UNSUPPORTED,
                "histogram rows of %d counts (the limit is %d)", h->n_bins + 2,
                kHistMaxRow);
  if (n_pct < 0) return fail(OTSDB_E_ILLEGAL_ARGUMENT, "n_pct < 0");
  if (n_pct > kHistMaxPct)
    return fail(OTSDB_E_UNSUPPORTED, "%d percentiles (the limit is %d)", n_pct,
                kHistMaxPct);
  if (!h->lower || !h->upper)
    return fail(OTSDB_E_ILLEGAL_ARGUMENT, "no histogram bucket schema");
  for (int k = 1; k < h->n_bins; ++k) {
    int cmp = float_compare(h->lower[k - 1], h->lower[k]);
    if (!cmp) cmp = float_compare(h->upper[k - 1], h->upper[k]);
    if (cmp >= 0)
      return fail(OTSDB_E_ILLEGAL_ARGUMENT,
                  "histogram buckets must ascend strictly (index %d)", k);
  }
  if (s->run_all)
    return fail(OTSDB_E_UNSUPPORTED, "histogram queries with 0all");
  if (s->use_calendar)
    return fail(OTSDB_E_UNSUPPORTED,
                "histogram queries over calendar intervals");
  if (s->ds_interval_ms == 0)
    return fail(OTSDB_E_UNSUPPORTED, "histogram queries without a downsampler");
  if (s->ds_interval_ms < 0)
    return fail(OTSDB_E_ILLEGAL_ARGUMENT, "negative interval");
  if (s->start_ms < 0) return fail(OTSDB_E_ILLEGAL_ARGUMENT, "negative start");
  // the grid of the NONE-fill downsampler: every bucket start <= end_ms from
  // align(start + interval - 1) on; nothing else of the spec is read
  otsdb_query_spec g = *s;
  g.agg_id = OTSDB_AGG_SUM;
  g.ds_agg_id = OTSDB_AGG_SUM;
  g.interp = OTSDB_INTERP_DEFAULT;
  g.fill = OTSDB_FILL_NONE;
  g.rate = g.counter = g.drop_resets = 0;
  const otsdb_status rc = make_params(&g, P);
  if (rc) return rc;
  if (P->nb > 0 && P->gbase == 0)
    return fail(OTSDB_E_UNSUPPORTED,
                "a histogram bucket at timestamp 0 (the reference's end mark)");
  return OTSDB_OK;
}

otsdb_status hist_dense_budget(int64_t G, int64_t nb, int R) {
  if ((double)G * (double)nb * (double)R * 8.0 > (double)kHistDenseBudget)
    return fail(OTSDB_E_CAPACITY,
                "dense histogram sums of %lld groups x %lld buckets x %d counts "
                "pass %lld bytes", (long long)G, (long long)nb, R,
                (long long)kHistDenseBudget);
  return OTSDB_OK;
}

// tiles of at most kHistTile members; a group of several tiles gets one
// partial slot per tile (consecutive, in member order)
struct HistTiles {
  std::vector<int64_t> g, m0, m1, slot, mg_g, mg_s0, mg_s1;
  int64_t n_slots = 0;
};

void hist_tiles(const std::vector<int64_t>& goff, HistTiles* T) {
  for (size_t g = 0; g + 1 < goff.size(); ++g) {
    const int64_t a = goff[g], e = goff[g + 1];
    if (e <= a) continue;
    const bool whole = e - a <= kHistTile;
    if (!whole) {
      T->mg_g.push_back((int64_t)g);
      T->mg_s0.push_back(T->n_slots);
    }
    for (int64_t m = a; m < e; m += kHistTile) {
      T->g.push_back((int64_t)g);
      T->m0.push_back(m);
      T->m1.push_back(std::min(m + kHistTile, e));
      T->slot.push_back(whole ? -1 : T->n_slots++);
    }
    if (!whole) T->mg_s1.push_back(T->n_slots);
  }
}

// the tiles' partials take the dense array's byte budget too (checked before
// the workspace is sized)
otsdb_status hist_partial_budget(const HistTiles& T, int64_t nb, int R) {
  if ((double)T.n_slots * (double)nb * (double)R * 8.0 > (double)kHistDenseBudget)
    return fail(OTSDB_E_CAPACITY,
                "partial histogram sums of %lld tiles x %lld buckets x %d "
                "counts pass %lld bytes", (long long)T.n_slots, (long long)nb,
                R, (long long)kHistDenseBudget);
  return OTSDB_OK;
}

// device buffers of one histogram call, carved from the context workspace
struct HistWork {
  int64_t *lo, *hi, *tiles, *partial, *dense, *cnt;
  uint8_t *part_emit, *emit;
  float* schema;
  double* dense_pct;
};

size_t hist_carve(char* base, HistWork* W, int64_t S, const HistTiles* T,
                  int64_t G, int64_t nb, int R, int n_pct, bool own_dense) {
  Carve cv{base};
  const size_t nt = T ? T->g.size() * 4 + T->mg_g.size() * 3 : 0;
  W->lo = cv.take<int64_t>(S + 1);
  W->hi = cv.take<int64_t>(S + 1);
  W->tiles = cv.take<int64_t>(nt + 1);
  W->partial = cv.take<int64_t>((size_t)(T ? T->n_slots : 0) * nb * R + 2);
  W->part_emit = cv.take<uint8_t>((size_t)(T ? T->n_slots : 0) * nb + 16);
  W->dense = cv.take<int64_t>(own_dense ? (size_t)G * nb * R + 2 : 2);
  W->emit = cv.take<uint8_t>(own_dense ? (size_t)G * nb + 16 : 16);
  W->schema = cv.take<float>(2 * (size_t)R);
  W->dense_pct = cv.take<double>((size_t)n_pct * G * nb + 1);
  W->cnt = cv.take<int64_t>(G + 1);
  return cv.off + 256;
}

// the local shard's dense sums: prep, fold, combine.  Every cell of dense /
// emit is written.  T's arrays stay alive until the caller synchronises.
otsdb_status hist_partials(otsdb_ctx* c, const otsdb_query_spec* spec,
                           const Params& P, const otsdb_batch* b,
                           const otsdb_hist_columns* h, const HistTiles& T,
                           const HistWork& W, std::vector<int64_t>& tbuf,
                           int64_t* dense, uint8_t* emit) {
  hipStream_t st = c->stream;
  const int64_t S = b->n_series, G = b->n_groups, nb = P.nb;
  const int R = h->n_bins + 2;
  c->n_hist_fold = 0;
  if (G == 0 || nb == 0) return OTSDB_OK;
  HIP_TRY(hipMemsetAsync(dense, 0, (size_t)G * nb * R * 8, st));
  HIP_TRY(hipMemsetAsync(emit, 0, (size_t)G * nb, st));
  const int64_t nt = (int64_t)T.g.size(), nmg = (int64_t)T.mg_g.size();
  if (nt == 0 || S == 0) return OTSDB_OK;
  // (a batch without points may come without point columns: none is read)
  if (!b->offsets || !b->group_members ||
      (b->n_points > 0 && (!b->ts_ms || !h->counts)))
    return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null batch column");
  if (((uintptr_t)h->counts) & 7)
    return fail(OTSDB_E_ILLEGAL_ARGUMENT, "histogram counts not 8-byte aligned");
  const int Wb = hist_window(R);
  const int64_t NW = (nb + Wb - 1) / Wb;
  if ((double)nt * (double)NW >= 2147483647.0)
    return fail(OTSDB_E_CAPACITY, "histogram fold of %lld tiles x %lld windows",
                (long long)nt, (long long)NW);
  // tile table: g | m0 | m1 | slot [nt], then mg_g | mg_s0 | mg_s1 [nmg]
  tbuf.clear();
  for (auto* v : {&T.g, &T.m0, &T.m1, &T.slot, &T.mg_g, &T.mg_s0, &T.mg_s1})
    tbuf.insert(tbuf.end(), v->begin(), v->end());
  HIP_TRY(hipMemcpyAsync(W.tiles, tbuf.data(), tbuf.size() * 8,
                         hipMemcpyHostToDevice, st));
  const int64_t* d_g = W.tiles;
  const int64_t* d_m0 = d_g + nt;
  const int64_t* d_m1 = d_m0 + nt;
  const int64_t* d_slot = d_m1 + nt;
  const int64_t* d_mg = d_slot + nt;
  {
    StageTimer tm(c, 8);
    hipLaunchKernelGGL(k_hist_prep, dim3(blocks_for(S, 256)), dim3(256), 0, st,
                       P, S, b->offsets, b->ts_ms, W.lo, W.hi);
    const int first_only = spec->ds_agg_id != OTSDB_AGG_SUM;
    const bool vec = (R % 2 == 0) && (((uintptr_t)h->counts) & 15) == 0;
    const int lds = hist_lds_bytes(R, (int)std::min<int64_t>(Wb, nb));
    const dim3 grid((unsigned)(nt * NW)), blk(HIST_THREADS);
    auto launch = [&](auto kern) {
      hipLaunchKernelGGL(kern, grid, blk, lds, st, P, b->ts_ms, h->counts, R, Wb,
                         first_only, (const int64_t*)W.lo, (const int64_t*)W.hi,
                         nt, d_g, d_m0, d_m1, d_slot, b->group_members, dense,
                         emit, W.partial, W.part_emit);
    };
    if (R <= 128) {
      if (vec) launch(k_hist_fold<1, true>);
      else launch(k_hist_fold<1, false>);
    } else {
      if (vec) launch(k_hist_fold<2, true>);
      else launch(k_hist_fold<2, false>);
    }
    c->n_hist_fold = 1;
  }
  HIP_TRY(hipGetLastError());
  if (nmg > 0) {
    StageTimer tm(c, 9);
    for (int64_t k0 = 0; k0 < nmg; k0 += 65535) {
      const int64_t n = std::min<int64_t>(65535, nmg - k0);
      hipLaunchKernelGGL(k_hist_combine,
                         dim3(blocks_for(nb * R, 256), (unsigned)n), dim3(256),
                         0, st, nb, R, d_mg + k0, d_mg + nmg + k0,
                         d_mg + 2 * nmg + k0, (const int64_t*)W.partial,
                         (const uint8_t*)W.part_emit, dense, emit);
    }
    HIP_TRY(hipGetLastError());
  }
  return OTSDB_OK;
}

// percentiles and the compacted result from dense sums; synchronises
otsdb_status hist_finalize(otsdb_ctx* c, const Params& P, int64_t G,
                           const otsdb_hist_columns* h, const HistWork& W,
                           const int64_t* dense, const uint8_t* emit,
                           const float* pcts, int n_pct,
                           otsdb_hist_result* out, int64_t* total) {
  hipStream_t st = c->stream;
  const int64_t nb = P.nb;
  const int K = h->n_bins, R = K + 2;
  c->n_hist_pct = 0;
  *total = 0;
  if (G == 0 || nb == 0) {
    HIP_TRY(hipMemsetAsync(out->offsets, 0, sizeof(int64_t) * (G + 1), st));
    HIP_TRY(hipStreamSynchronize(st));
    return OTSDB_OK;
  }
  const int64_t cells = G * nb;
  if (n_pct > 0) {
    HIP_TRY(hipMemcpyAsync(W.schema, h->lower, 4 * (size_t)K,
                           hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(W.schema + R, h->upper, 4 * (size_t)K,
                           hipMemcpyHostToDevice, st));
    HistPct hp;
    for (int q = 0; q < kHistMaxPct; ++q)
      hp.p[q] = q < n_pct ? (double)pcts[q] : 0.0;  // float widened
    StageTimer tm(c, 10);
    const dim3 grid(blocks_for(cells, 4)), blk(256);
    auto launch = [&](auto kern) {
      hipLaunchKernelGGL(kern, grid, blk, 0, st, cells, R, K, dense, emit,
                         (const float*)W.schema, (const float*)(W.schema + R),
                         hp, n_pct, W.dense_pct);
    };
    switch ((K + 63) / 64) {
      case 1: launch(k_hist_percentiles<1>); break;
      case 2: launch(k_hist_percentiles<2>); break;
      case 3: launch(k_hist_percentiles<3>); break;
      default: launch(k_hist_percentiles<4>); break;
    }
    c->n_hist_pct = 1;
    HIP_TRY(hipGetLastError());
  }
  {
    StageTimer tm(c, 11);
    hipLaunchKernelGGL(k_hist_count, dim3(blocks_for(G, 4)), dim3(256), 0, st,
                       G, nb, emit, W.cnt);
    launch_scan(G, W.cnt, out->offsets, st);
    hipLaunchKernelGGL(k_hist_scatter, dim3(blocks_for(G, 4)), dim3(256), 0, st,
                       P, G, R, n_pct, emit, (const int64_t*)out->offsets,
                       out->capacity, dense, (const double*)W.dense_pct, out->ts,
                       out->pct_val, out->counts);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipMemcpyAsync(&c->h_small[1], out->offsets + G, sizeof(int64_t),
                         hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  *total = c->h_small[1];
  if (*total > out->capacity) {
    c->result_short = true;
    return fail(OTSDB_E_CAPACITY, "result capacity %lld < %lld points",
                (long long)out->capacity, (long long)*total);
  }
  return OTSDB_OK;
}

otsdb_status hist_out_check(const otsdb_hist_result* out, int32_t n_pct) {
  if (n_pct == 0 && !out->counts)
    return fail(OTSDB_E_ILLEGAL_ARGUMENT,
                "no percentile and no counts output asked for");
  if (out->capacity < 0 || !out->offsets || (out->capacity > 0 && !out->ts) ||
      (n_pct > 0 && out->capacity > 0 && !out->pct_val))
    return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null result array");
  return OTSDB_OK;
}

// the whole query on device pointers (the context locked, the stream bound)
otsdb_status hist_run_impl(otsdb_ctx* c, const otsdb_query_spec* spec,
                           const Params& P, const otsdb_batch* b,
                           const otsdb_hist_columns* h,
                           const std::vector<int64_t>& goff, const float* pcts,
                           int n_pct, otsdb_hist_result* out, int64_t* total) {
  const int R = h->n_bins + 2;
  HistTiles T;
  hist_tiles(goff, &T);
  otsdb_status rc = hist_partial_budget(T, P.nb, R);
  if (rc) return rc;
  HistWork W;
  const size_t need =
      hist_carve(nullptr, &W, b->n_series, &T, b->n_groups, P.nb, R, n_pct, true);
  rc = c->ws.ensure(need);
  if (rc) return rc;
  hist_carve((char*)c->ws.p, &W, b->n_series, &T, b->n_groups, P.nb, R, n_pct,
             true);
  std::vector<int64_t> tbuf;
  rc = hist_partials(c, spec, P, b, h, T, W, tbuf, W.dense, W.emit);
  if (!rc)
    rc = hist_finalize(c, P, b->n_groups, h, W, W.dense, W.emit, pcts, n_pct,
                       out, total);
  else
    hipStreamSynchronize(c->stream);
  return rc;
}

// ------------------------------------------ histogram queries from storage rows
// otsdb_hist_rows_schema_device / otsdb_hist_decode_rows_device /
// otsdb_hist_run_rows*: the scanner's rows decoded on the device
// (hist_rows.hip).
otsdb_status check_hist_rows(const otsdb_raw_rows* raw, int32_t codec) {
  if (!raw) return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null");
  if (codec < 0 || codec > 255)
    return fail(OTSDB_E_ILLEGAL_ARGUMENT, "histogram codec id %d (0..255)",
                codec);
  if (raw->n_rows < 0) return fail(OTSDB_E_ILLEGAL_ARGUMENT, "negative n_rows");
  if (raw->n_rows >= 2147483647LL)
    return fail(OTSDB_E_CAPACITY, "%lld storage rows", (long long)raw->n_rows);
  if (!raw->row_series || !raw->row_base_s || !raw->row_col_off ||
      !raw->col_qual_off || !raw->col_val_off ||
      (raw->n_rows > 0 && (!raw->qual || !raw->val)))
    return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null raw row array");
  return OTSDB_OK;
}

// the schema checks of hist_check alone (the decode entry has no query)
otsdb_status check_hist_schema(const otsdb_hist_columns* h) {
  if (!h) return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null");
  if (h->n_bins < 1)
    return fail(OTSDB_E_ILLEGAL_ARGUMENT, "histogram schema of %d buckets",
                h->n_bins);
  if (h->n_bins + 2 > kHistMaxRow)
    return fail(OTSDB_E_UNSUPPORTED,
                "histogram rows of %d counts (the limit is %d)", h->n_bins + 2,
                kHistMaxRow);
  if (!h->lower || !h->upper)
    return fail(OTSDB_E_ILLEGAL_ARGUMENT, "no histogram bucket schema");
  for (int k = 1; k < h->n_bins; ++k) {
    int cmp = float_compare(h->lower[k - 1], h->lower[k]);
    if (!cmp) cmp = float_compare(h->upper[k - 1], h->upper[k]);
    if (cmp >= 0)
      return fail(OTSDB_E_ILLEGAL_ARGUMENT,
                  "histogram buckets must ascend strictly (index %d)", k);
  }
  return OTSDB_OK;
}

// hr_ord on the host, and back
uint32_t hr_ord_host(float f) {
  uint32_t b;
  memcpy(&b, &f, 4);
  if ((b & 0x7FFFFFFFu) > 0x7F800000u) b = 0x7FC00000u;
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
float hr_unord_host(uint32_t u) {
  const uint32_t b = (u & 0x80000000u) ? (u ^ 0x80000000u) : ~u;
  float f;
  memcpy(&f, &b, 4);
  return f;
}

// one decode call's device view and what must outlive its launches
struct HrCall {
  HistRowsDev T{};
  std::vector<unsigned long long> keys;  // the schema, ordered keys (host)
  void* scan_tmp = nullptr;
  size_t scan_bytes = 0;
};

// the view over the rows and the work arrays in the context's decode
// workspace; synchronises once (the column count is the rows')
otsdb_status hr_setup(otsdb_ctx* c, const otsdb_raw_rows* raw, int32_t codec,
                      int64_t S, const otsdb_hist_columns* h, hipStream_t st,
                      HrCall* H) {
  HistRowsDev& T = H->T;
  const int64_t R = raw->n_rows;
  int64_t C = 0;
  if (R > 0) {
    HIP_TRY(hipMemcpyAsync(&c->h_small[0], raw->row_col_off + R, 8,
                           hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    C = c->h_small[0];
  }
  if (C < 0) return fail(OTSDB_E_ILLEGAL_ARGUMENT, "negative column count");
  T.R = R;
  T.C = C;
  T.S = S;
  T.row_series = raw->row_series;
  T.row_base_s = raw->row_base_s;
  T.row_col_off = raw->row_col_off;
  T.col_qoff = raw->col_qual_off;
  T.qual = raw->qual;
  T.col_voff = raw->col_val_off;
  T.val = raw->val;
  T.codec = codec;
  T.K = h ? h->n_bins : 0;
  H->scan_bytes = scan_tmp_bytes(R, st);
  auto carve = [&](char* base) {
    Carve cv{base};
    T.rec_ts = cv.take<int64_t>(C + 1);
    T.rec_state = cv.take<int32_t>(C + 1);
    T.rec_rank = cv.take<int32_t>(C + 1);
    T.rec_row = cv.take<int32_t>(C + 1);
    T.row_cnt = cv.take<int64_t>(R + 1);
    T.row_out = cv.take<int64_t>(R + 1);
    T.row_head = cv.take<int64_t>(R + 1);
    T.row_first = cv.take<int64_t>(R + 1);
    T.row_last = cv.take<int64_t>(R + 1);
    T.small = cv.take<unsigned long long>(8);
    T.set = cv.take<unsigned long long>(kHrSetSlots);
    T.schema = cv.take<unsigned long long>(kHrMaxEntries + 2);
    H->scan_tmp = cv.take<char>(H->scan_bytes + 16);
    return cv.off + 256;
  };
  const otsdb_status rc = c->dec_ws.ensure(carve(nullptr));
  if (rc) return rc;
  carve((char*)c->dec_ws.p);
  if (h) {
    H->keys.resize(h->n_bins);
    for (int k = 0; k < h->n_bins; ++k)
      H->keys[k] = ((unsigned long long)hr_ord_host(h->lower[k]) << 32) |
                   hr_ord_host(h->upper[k]);
    HIP_TRY(hipMemcpyAsync((void*)T.schema, H->keys.data(), 8 * H->keys.size(),
                           hipMemcpyHostToDevice, st));
  }
  // small: the two error words all ones, the counters zero
  HIP_TRY(hipMemsetAsync(T.small, 0xFF, 16, st));
  HIP_TRY(hipMemsetAsync(T.small + 2, 0, 48, st));
  return OTSDB_OK;
}

otsdb_status hr_status(unsigned long long fe, int64_t C, bool second) {
  const long long pos = (long long)(fe >> 8);
  const int code = (int)(fe & 0xFF);
  const otsdb_status st =
      code == HR_ILLEGAL_ARGUMENT ? OTSDB_E_ILLEGAL_ARGUMENT : OTSDB_E_UNSUPPORTED;
  if (second)
    return fail(st, "histogram rows: a series' timestamps do not increase "
                    "from one row to the next (before column %lld)", pos / 2);
  if (pos & 1) {
    if (code == HR_ILLEGAL_ARGUMENT)
      return fail(st, "histogram column %lld: a bucket outside the schema",
                  pos / 2);
    return fail(st, "histogram column %lld: another codec's id, more than %d "
                    "buckets, or a timestamp not after the cell before's",
                pos / 2, kHrMaxEntries);
  }
  if (code == HR_ILLEGAL_ARGUMENT)
    return fail(st, "histogram rows: row_series must be nondecreasing series "
                    "indices (before column %lld)", pos / 2);
  return fail(st, "histogram rows: base times that decrease inside a series, "
                  "or more than %d rows of one key (before column %lld)",
              kHrRunRows, pos / 2);
}

void hr_counters(otsdb_ctx* c) {
  c->n_hr_decoded = c->h_small[HR_W_DECODED];
  c->n_hr_skipped = c->h_small[HR_W_SKIPPED];
  c->n_hr_dropped = c->h_small[HR_W_DROPPED];
}

// The count pass: cells, the scan walk, assembly; offsets [S + 1] filled and
// *total the points.  Synchronises.
otsdb_status hr_count(otsdb_ctx* c, HrCall* H, int64_t* offsets,
                      int64_t* total, hipStream_t st) {
  HistRowsDev& T = H->T;
  const int64_t R = T.R, C = T.C;
  if (C > 0) {
    hipLaunchKernelGGL(k_hr_cells, dim3(blocks_for(C, 256)), dim3(256), 0, st, T);
    hipLaunchKernelGGL(k_hr_walk<1>, dim3(blocks_for(C, kHrWaves)),
                       dim3(64 * kHrWaves), 0, st, T, (int64_t*)nullptr,
                       (int64_t*)nullptr, (int64_t)0);
  }
  HIP_TRY(hipMemsetAsync(T.row_cnt + R, 0, 8, st));
  if (R > 0) {
    hipLaunchKernelGGL(k_hr_rows, dim3(blocks_for(R, 256)), dim3(256), 0, st, T);
    hipLaunchKernelGGL(k_hr_merge, dim3(blocks_for(R, 64)), dim3(64), 0, st, T);
  }
  HIP_TRY(hipGetLastError());
  otsdb_status rc =
      scan_excl(H->scan_tmp, H->scan_bytes, T.row_cnt, T.row_out, R, st);
  if (rc) return rc;
  // the first failure before anything is indexed by a series number
  HIP_TRY(hipMemcpyAsync(&c->h_small[0], T.small, 56, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(&c->h_small[HR_W_TOTAL], T.row_out + R, 8,
                         hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  hr_counters(c);
  unsigned long long fe = (unsigned long long)c->h_small[HR_W_ERR];
  if (fe != ~0ULL) return hr_status(fe, C, false);
  *total = c->h_small[HR_W_TOTAL];
  launch_series_offsets(R, T.S, T.row_series, T.row_out, offsets, st);
  if (R > 0)
    hipLaunchKernelGGL(k_hr_series, dim3(blocks_for(R, 256)), dim3(256), 0, st, T);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(&c->h_small[HR_W_ERR2], T.small + HR_W_ERR2, 8,
                         hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  fe = (unsigned long long)c->h_small[HR_W_ERR2];
  if (fe != ~0ULL) return hr_status(fe, C, true);
  return OTSDB_OK;
}

// the write pass (after hr_count on the same call): queued, not synchronised
otsdb_status hr_write(HrCall* H, int64_t* ts_ms, int64_t* counts, int64_t cap,
                      hipStream_t st) {
  if (H->T.C > 0)
    hipLaunchKernelGGL(k_hr_walk<2>, dim3(blocks_for(H->T.C, kHrWaves)),
                       dim3(64 * kHrWaves), 0, st, H->T, ts_ms, counts, cap);
  HIP_TRY(hipGetLastError());
  return OTSDB_OK;
}

// device pointers throughout: the rows decoded into the context's columnar
// buffer, then otsdb_hist_run_device's pipeline over it
otsdb_status hist_run_rows_impl(otsdb_ctx* c, const otsdb_query_spec* spec,
                                const Params& P, const otsdb_raw_rows* raw,
                                int32_t codec, const otsdb_batch* b,
                                const otsdb_hist_columns* h,
                                const std::vector<int64_t>& goff,
                                const float* pcts, int n_pct,
                                otsdb_hist_result* out, int64_t* total) {
  hipStream_t st = c->stream;
  const int64_t S = b->n_series;
  const int R = h->n_bins + 2;
  if (S < 0) return fail(OTSDB_E_ILLEGAL_ARGUMENT, "negative sizes");
  otsdb_status rc = c->cells_ws.ensure((size_t)(S + 1) * 8 + 64);
  if (rc) return rc;
  int64_t* offs = (int64_t*)c->cells_ws.p;
  HrCall H;
  int64_t N = 0;
  int64_t *ts = nullptr, *cnt = nullptr;
  {
    StageTimer tm(c, 12);  // the rows decode
    if ((rc = hr_setup(c, raw, codec, S, h, st, &H))) return rc;
    if ((rc = hr_count(c, &H, offs, &N, st))) return rc;
    const size_t col = ((size_t)std::max<int64_t>(N, 2) * 8 + 255) & ~(size_t)255;
    rc = c->cells_col.ensure(col + (size_t)std::max<int64_t>(N, 2) * R * 8 + 256);
    if (rc) return rc;
    ts = (int64_t*)c->cells_col.p;
    cnt = (int64_t*)((char*)c->cells_col.p + col);
    if ((rc = hr_write(&H, ts, cnt, N, st))) return rc;
  }
  otsdb_batch cb = *b;
  cb.n_points = N;
  cb.offsets = offs;
  cb.ts_ms = ts;
  cb.val = nullptr;
  cb.is_float = cb.series_float = nullptr;
  otsdb_hist_columns ch = *h;
  ch.counts = cnt;
  // (hist_run_impl synchronises on every path: H outlives the write pass)
  return hist_run_impl(c, spec, P, &cb, &ch, goff, pcts, n_pct, out, total);
}

// the argument checks of the two query entries, before any device work
otsdb_status check_hist_run_rows(const otsdb_query_spec* spec,
                                 const otsdb_raw_rows* raw, int32_t codec,
                                 const otsdb_batch* b,
                                 const otsdb_hist_columns* h, const float* pcts,
                                 int32_t n_pct, const otsdb_hist_result* out,
                                 Params* P) {
  if (!spec || !raw || !b || !h || !out || (n_pct > 0 && !pcts))
    return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null");
  otsdb_status rc = hist_check(spec, h, n_pct, P);
  if (!rc) rc = hist_out_check(out, n_pct);
  if (!rc) rc = hist_dense_budget(b->n_groups, P->nb, h->n_bins + 2);
  if (!rc) rc = check_hist_rows(raw, codec);
  return rc;
}

}  // namespace

extern "C" {

int32_t otsdb_hist_window(int32_t n_bins) {
  if (n_bins < 1 || n_bins + 2 > kHistMaxRow) return 0;
  return hist_window(n_bins + 2);
}

otsdb_status otsdb_hist_plan(otsdb_ctx*, const otsdb_query_spec* spec,
                             const otsdb_batch* b, const otsdb_hist_columns* h,
                             otsdb_sizes* out) {
  if (!spec || !b || !h || !out) return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null");
  Params P;
  otsdb_status rc = hist_check(spec, h, 0, &P);
  if (rc) return rc;
  if (b->n_groups < 0 || b->n_series < 0)
    return fail(OTSDB_E_ILLEGAL_ARGUMENT, "negative sizes");
  const int R = h->n_bins + 2;
  if ((rc = hist_dense_budget(b->n_groups, P.nb, R))) return rc;
  out->n_buckets = P.nb;
  out->max_out_points = b->n_groups * P.nb;
  // the dense sums and percentiles, the series bounds, and one partial slot
  // for each 64-member tile of a group of more than 64 members: counted from
  // the host copy of the group offsets where the batch has one, else bounded
  // for a batch that lists each series in one group (members / 64 slots plus
  // one a group of 65 or more; a batch that lists series in several groups
  // without a host copy takes more)
  int64_t slots = 2 * (b->n_series / kHistTile) + 1;
  if (b->group_offsets_host) {
    slots = 0;
    for (int64_t g = 0; g < b->n_groups; ++g) {
      const int64_t k = b->group_offsets_host[g + 1] - b->group_offsets_host[g];
      if (k > kHistTile) slots += (k + kHistTile - 1) / kHistTile;
    }
  }
  out->workspace_bytes =
      b->n_groups * P.nb * (8 * (int64_t)R + 8 * kHistMaxPct + 1) +
      b->n_series * 16 + slots * P.nb * (8 * (int64_t)R + 1) +
      ((int64_t)1 << 20);
  return OTSDB_OK;
}

otsdb_status otsdb_hist_run_device(otsdb_ctx* c, const otsdb_query_spec* spec,
                                   const otsdb_batch* b,
                                   const otsdb_hist_columns* h,
                                   const float* pcts, int32_t n_pct,
                                   otsdb_hist_result* out, void* hip_stream) {
  if (!spec || !b || !h || !out || (n_pct > 0 && !pcts))
    return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null");
  Params P;
  otsdb_status rc = hist_check(spec, h, n_pct, &P);
  if (!rc) rc = hist_out_check(out, n_pct);
  if (!rc) rc = hist_dense_budget(b->n_groups, P.nb, h->n_bins + 2);
  if (rc) return rc;
  if (!c) return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null context");
  DeviceCall dc(c, b, hip_stream);
  if (dc.rc) return dc.rc;
  int64_t total = 0;
  return hist_run_impl(c, spec, P, b, h, dc.goff, pcts, n_pct, out, &total);
}

otsdb_status otsdb_hist_partials_device(otsdb_ctx* c,
                                        const otsdb_query_spec* spec,
                                        const otsdb_batch* b,
                                        const otsdb_hist_columns* h,
                                        int64_t* dense, uint8_t* emit,
                                        void* hip_stream) {
  if (!spec || !b || !h || !dense || !emit)
    return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null");
  Params P;
  otsdb_status rc = hist_check(spec, h, 0, &P);
  if (!rc) rc = hist_dense_budget(b->n_groups, P.nb, h->n_bins + 2);
  if (rc) return rc;
  if (!c) return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null context");
  DeviceCall dc(c, b, hip_stream);
  if (dc.rc) return dc.rc;
  HistTiles T;
  hist_tiles(dc.goff, &T);
  const int R = h->n_bins + 2;
  if ((rc = hist_partial_budget(T, P.nb, R))) return rc;
  HistWork W;
  const size_t need =
      hist_carve(nullptr, &W, b->n_series, &T, b->n_groups, P.nb, R, 0, false);
  if ((rc = c->ws.ensure(need))) return rc;
  hist_carve((char*)c->ws.p, &W, b->n_series, &T, b->n_groups, P.nb, R, 0, false);
  std::vector<int64_t> tbuf;
  rc = hist_partials(c, spec, P, b, h, T, W, tbuf, dense, emit);
  HIP_TRY(hipStreamSynchronize(c->stream));
  return rc;
}

otsdb_status otsdb_hist_finalize_device(otsdb_ctx* c,
                                        const otsdb_query_spec* spec,
                                        const otsdb_hist_columns* h,
                                        int64_t n_groups, int64_t n_buckets,
                                        const int64_t* dense,
                                        const uint8_t* emit, const float* pcts,
                                        int32_t n_pct, otsdb_hist_result* out,
                                        void* hip_stream) {
  if (!spec || !h || !dense || !emit || !out || (n_pct > 0 && !pcts))
    return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null");
  Params P;
  otsdb_status rc = hist_check(spec, h, n_pct, &P);
  if (!rc) rc = hist_out_check(out, n_pct);
  if (rc) return rc;
  if (n_groups < 0 || n_buckets != P.nb)
    return fail(OTSDB_E_ILLEGAL_ARGUMENT,
                "n_buckets %lld is not the plan's %lld", (long long)n_buckets,
                (long long)P.nb);
  if ((rc = hist_dense_budget(n_groups, P.nb, h->n_bins + 2))) return rc;
  if (!c) return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null context");
  CtxLock lk(c);
  HIP_TRY(hipSetDevice(c->device));
  StreamBinding bind(c, hip_stream);
  HistWork W;
  const int R = h->n_bins + 2;
  const size_t need =
      hist_carve(nullptr, &W, 0, nullptr, n_groups, P.nb, R, n_pct, false);
  if ((rc = c->ws.ensure(need))) return rc;
  hist_carve((char*)c->ws.p, &W, 0, nullptr, n_groups, P.nb, R, n_pct, false);
  int64_t total = 0;
  return hist_finalize(c, P, n_groups, h, W, dense, emit, pcts, n_pct, out,
                       &total);
}

otsdb_status otsdb_hist_run(otsdb_ctx* c, const otsdb_query_spec* spec,
                            const otsdb_batch* b, const otsdb_hist_columns* h,
                            const float* pcts, int32_t n_pct,
                            otsdb_hist_result* out) {
  if (!spec || !b || !h || !out || (n_pct > 0 && !pcts))
    return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null");
  Params P;
  otsdb_status rc = hist_check(spec, h, n_pct, &P);
  if (!rc) rc = hist_out_check(out, n_pct);
  if (!rc) rc = hist_dense_budget(b->n_groups, P.nb, h->n_bins + 2);
  if (rc) return rc;
  if (!c) return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null context");
  CtxLock lk(c);
  HIP_TRY(hipSetDevice(c->device));
  std::vector<int64_t> goff;
  if ((rc = read_goff(c, b, false, goff))) return rc;
  const int64_t S = b->n_series, N = b->n_points, G = b->n_groups;
  const int64_t M = goff.back(), cap = out->capacity;
  const int R = h->n_bins + 2;
  if (S < 0 || N < 0) return fail(OTSDB_E_ILLEGAL_ARGUMENT, "negative sizes");
  if (S > 0 && (!b->offsets || b->offsets[S] != N))
    return fail(OTSDB_E_ILLEGAL_ARGUMENT, "offsets[S] != n_points");
  if (N > 0 && (!b->ts_ms || !h->counts))
    return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null batch column");
  if (M > 0 && !b->group_members)
    return fail(OTSDB_E_ILLEGAL_ARGUMENT, "no group members");
  for (int64_t s = 0; s < S; ++s)
    if (b->offsets[s] < 0 || b->offsets[s + 1] < b->offsets[s])
      return fail(OTSDB_E_ILLEGAL_ARGUMENT, "offsets not monotonic");
  for (int64_t m = 0; m < M; ++m)
    if (b->group_members[m] < 0 || b->group_members[m] >= S)
      return fail(OTSDB_E_ILLEGAL_ARGUMENT, "group member out of range");
  // staging layout in HBM: the batch, then the result
  struct Stage {
    int64_t *off, *ts, *cnt, *goff, *mem, *r_off, *r_ts, *r_cnt;
    double* r_pct;
  } D;
  auto carve = [&](char* base) {
    Carve cv{base};
    D.off = cv.take<int64_t>(S + 1);
    D.ts = cv.take<int64_t>(N + 1);
    D.cnt = cv.take<int64_t>((size_t)N * R + 2);
    D.goff = cv.take<int64_t>(G + 1);
    D.mem = cv.take<int64_t>(M + 1);
    D.r_off = cv.take<int64_t>(G + 1);
    D.r_ts = cv.take<int64_t>(cap + 1);
    D.r_pct = cv.take<double>((size_t)n_pct * cap + 1);
    D.r_cnt = cv.take<int64_t>(out->counts ? (size_t)cap * R + 1 : 1);
    return cv.off + 256;
  };
  if ((rc = c->stage.ensure(carve(nullptr)))) return rc;
  carve((char*)c->stage.p);
  hipStream_t st = c->stream;
  auto h2d = [&](void* d, const void* hsrc, size_t n) -> otsdb_status {
    if (n && hsrc) HIP_TRY(hipMemcpyAsync(d, hsrc, n, hipMemcpyHostToDevice, st));
    return OTSDB_OK;
  };
  if ((rc = h2d(D.off, b->offsets, 8 * (size_t)(S + 1)))) return rc;
  if ((rc = h2d(D.ts, b->ts_ms, 8 * (size_t)N))) return rc;
  if ((rc = h2d(D.cnt, h->counts, 8 * (size_t)N * R))) return rc;
  if ((rc = h2d(D.goff, b->group_offsets, 8 * (size_t)(G + 1)))) return rc;
  if ((rc = h2d(D.mem, b->group_members, 8 * (size_t)M))) return rc;
  otsdb_batch db = *b;
  db.offsets = D.off;
  db.ts_ms = D.ts;
  db.val = nullptr;
  db.is_float = db.series_float = nullptr;
  db.group_offsets = D.goff;
  db.group_members = D.mem;
  otsdb_hist_columns dh = *h;
  dh.counts = D.cnt;
  otsdb_hist_result dr{cap, D.r_off, D.r_ts, n_pct > 0 ? D.r_pct : nullptr,
                       out->counts ? D.r_cnt : nullptr};
  c->result_short = false;
  int64_t total = 0;
  rc = hist_run_impl(c, spec, P, &db, &dh, goff, pcts, n_pct, &dr, &total);
  if (rc == OTSDB_E_CAPACITY && c->result_short) {
    // the offsets the whole result needs, then the status
    hipMemcpyAsync(out->offsets, D.r_off, 8 * (G + 1), hipMemcpyDeviceToHost, st);
    hipStreamSynchronize(st);
    return rc;
  }
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(out->offsets, D.r_off, 8 * (G + 1),
                         hipMemcpyDeviceToHost, st));
  if (total > 0) {
    HIP_TRY(hipMemcpyAsync(out->ts, D.r_ts, 8 * total, hipMemcpyDeviceToHost, st));
    for (int q = 0; q < n_pct; ++q)
      HIP_TRY(hipMemcpyAsync(out->pct_val + (size_t)q * cap,
                             D.r_pct + (size_t)q * cap, 8 * total,
                             hipMemcpyDeviceToHost, st));
    if (out->counts)
      HIP_TRY(hipMemcpyAsync(out->counts, D.r_cnt, 8 * (size_t)total * R,
                             hipMemcpyDeviceToHost, st));
  }
  HIP_TRY(hipStreamSynchronize(st));
  return OTSDB_OK;
}

otsdb_status otsdb_hist_rows_schema_device(otsdb_ctx* c,
                                           const otsdb_raw_rows* raw,
                                           int32_t simple_codec_id,
                                           float* lower, float* upper,
                                           int32_t* n_bins, void* hip_stream) {
  // (the argument checks first: they need no context)
  otsdb_status rc = check_hist_rows(raw, simple_codec_id);
  if (rc) return rc;
  if (!lower || !upper || !n_bins) return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null");
  if (!c) return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null context");
  CtxLock lk(c);
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
  HrCall H;
  if ((rc = hr_setup(c, raw, simple_codec_id, 0, nullptr, st, &H))) return rc;
  const HistRowsDev& T = H.T;
  HIP_TRY(hipMemsetAsync(T.set, 0xFF, 8 * kHrSetSlots, st));
  if (T.C > 0) {
    hipLaunchKernelGGL(k_hr_cells, dim3(blocks_for(T.C, 256)), dim3(256), 0, st,
                       T);
    hipLaunchKernelGGL(k_hr_walk<0>, dim3(blocks_for(T.C, kHrWaves)),
                       dim3(64 * kHrWaves), 0, st, T, (int64_t*)nullptr,
                       (int64_t*)nullptr, (int64_t)0);
  }
  HIP_TRY(hipGetLastError());
  std::vector<unsigned long long> set(kHrSetSlots);
  HIP_TRY(hipMemcpyAsync(&c->h_small[0], T.small, 56, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(set.data(), T.set, 8 * kHrSetSlots,
                         hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  const unsigned long long fe = (unsigned long long)c->h_small[HR_W_ERR];
  if (fe != ~0ULL) return hr_status(fe, T.C, false);
  if (c->h_small[HR_W_FULL] || c->h_small[HR_W_KEYS] > kHrMaxEntries)
    return fail(OTSDB_E_UNSUPPORTED,
                "more than %d distinct histogram buckets in the rows",
                kHrMaxEntries);
  set.erase(std::remove(set.begin(), set.end(), kHrEmpty), set.end());
  std::sort(set.begin(), set.end());
  for (size_t k = 0; k < set.size(); ++k) {
    lower[k] = hr_unord_host((uint32_t)(set[k] >> 32));
    upper[k] = hr_unord_host((uint32_t)set[k]);
  }
  *n_bins = (int32_t)set.size();
  return OTSDB_OK;
}

otsdb_status otsdb_hist_decode_rows_device(otsdb_ctx* c,
                                           const otsdb_raw_rows* raw,
                                           int32_t simple_codec_id,
                                           int64_t n_series,
                                           const otsdb_hist_columns* hist,
                                           int64_t* offsets, int64_t* ts_ms,
                                           int64_t* counts, int64_t capacity,
                                           void* hip_stream) {
  // (the argument checks first: they need no context)
  otsdb_status rc = check_hist_rows(raw, simple_codec_id);
  if (!rc) rc = check_hist_schema(hist);
  if (rc) return rc;
  if (n_series < 0) return fail(OTSDB_E_ILLEGAL_ARGUMENT, "negative sizes");
  if (!offsets) return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null");
  if (ts_ms && !counts) return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null output column");
  if (ts_ms && (((uintptr_t)counts) & 7))
    return fail(OTSDB_E_ILLEGAL_ARGUMENT, "histogram counts not 8-byte aligned");
  if (!c) return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null context");
  CtxLock lk(c);
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
  HrCall H;
  int64_t total = 0;
  if ((rc = hr_setup(c, raw, simple_codec_id, n_series, hist, st, &H))) return rc;
  if ((rc = hr_count(c, &H, offsets, &total, st))) return rc;
  if (!ts_ms) return OTSDB_OK;
  if (total > capacity)
    return fail(OTSDB_E_CAPACITY, "decode capacity %lld < %lld points",
                (long long)capacity, (long long)total);
  if ((rc = hr_write(&H, ts_ms, counts, capacity, st))) return rc;
  HIP_TRY(hipStreamSynchronize(st));
  return OTSDB_OK;
}

otsdb_status otsdb_hist_run_rows_device(otsdb_ctx* c,
                                        const otsdb_query_spec* spec,
                                        const otsdb_raw_rows* raw,
                                        int32_t simple_codec_id,
                                        const otsdb_batch* b,
                                        const otsdb_hist_columns* h,
                                        const float* pcts, int32_t n_pct,
                                        otsdb_hist_result* out,
                                        void* hip_stream) {
  Params P;
  const otsdb_status rc = check_hist_run_rows(spec, raw, simple_codec_id, b, h,
                                              pcts, n_pct, out, &P);
  if (rc) return rc;
  if (!c) return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null context");
  DeviceCall dc(c, b, hip_stream);
  if (dc.rc) return dc.rc;
  int64_t total = 0;
  return hist_run_rows_impl(c, spec, P, raw, simple_codec_id, b, h, dc.goff,
                            pcts, n_pct, out, &total);
}

otsdb_status otsdb_hist_run_rows(otsdb_ctx* c, const otsdb_query_spec* spec,
                                 const otsdb_raw_rows* raw,
                                 int32_t simple_codec_id, const otsdb_batch* b,
                                 const otsdb_hist_columns* h, const float* pcts,
                                 int32_t n_pct, otsdb_hist_result* out) {
  Params P;
  otsdb_status rc = check_hist_run_rows(spec, raw, simple_codec_id, b, h, pcts,
                                        n_pct, out, &P);
  if (rc) return rc;
  if (!c) return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null context");
  CtxLock lk(c);
  HIP_TRY(hipSetDevice(c->device));
  std::vector<int64_t> goff;
  if ((rc = read_goff(c, b, false, goff))) return rc;
  const int64_t NR = raw->n_rows, S = b->n_series, G = b->n_groups;
  const int64_t M = goff.back(), cap = out->capacity;
  const int R = h->n_bins + 2;
  if (S < 0) return fail(OTSDB_E_ILLEGAL_ARGUMENT, "negative sizes");
  if (M > 0 && !b->group_members)
    return fail(OTSDB_E_ILLEGAL_ARGUMENT, "no group members");
  for (int64_t r = 0; r < NR; ++r)
    if (raw->row_series[r] < 0 || raw->row_series[r] >= S ||
        (r && raw->row_series[r] < raw->row_series[r - 1]))
      return fail(OTSDB_E_ILLEGAL_ARGUMENT,
                  "row_series must be nondecreasing series indices");
  for (int64_t r = 0; r < NR; ++r)
    if (raw->row_col_off[r + 1] < raw->row_col_off[r])
      return fail(OTSDB_E_ILLEGAL_ARGUMENT, "row_col_off not monotonic");
  for (int64_t m = 0; m < M; ++m)
    if (b->group_members[m] < 0 || b->group_members[m] >= S)
      return fail(OTSDB_E_ILLEGAL_ARGUMENT, "group member out of range");
  const int64_t C = NR > 0 ? raw->row_col_off[NR] : 0;
  const int64_t QB = raw->col_qual_off[C], VB = raw->col_val_off[C];
  if (C < 0 || QB < 0 || VB < 0)
    return fail(OTSDB_E_ILLEGAL_ARGUMENT, "negative sizes");
  // staging layout in HBM: the rows, the groups, then the result
  struct Stage {
    int64_t *rs, *rb, *rc, *qo, *vo, *goff, *mem, *r_off, *r_ts, *r_cnt;
    uint8_t *q, *v;
    double* r_pct;
  } D;
  auto carve = [&](char* base) {
    Carve cv{base};
    D.rs = cv.take<int64_t>(NR + 1);
    D.rb = cv.take<int64_t>(NR + 1);
    D.rc = cv.take<int64_t>(NR + 1);
    D.qo = cv.take<int64_t>(C + 1);
    D.q = cv.take<uint8_t>(QB + 16);
    D.vo = cv.take<int64_t>(C + 1);
    D.v = cv.take<uint8_t>(VB + 16);
    D.goff = cv.take<int64_t>(G + 1);
    D.mem = cv.take<int64_t>(M + 1);
    D.r_off = cv.take<int64_t>(G + 1);
    D.r_ts = cv.take<int64_t>(cap + 1);
    D.r_pct = cv.take<double>((size_t)n_pct * cap + 1);
    D.r_cnt = cv.take<int64_t>(out->counts ? (size_t)cap * R + 1 : 1);
    return cv.off + 256;
  };
  if ((rc = c->raw_stage.ensure(carve(nullptr)))) return rc;
  carve((char*)c->raw_stage.p);
  hipStream_t st = c->stream;
  auto h2d = [&](void* d, const void* hsrc, size_t n) -> otsdb_status {
    if (n && hsrc) HIP_TRY(hipMemcpyAsync(d, hsrc, n, hipMemcpyHostToDevice, st));
    return OTSDB_OK;
  };
  if ((rc = h2d(D.rs, raw->row_series, 8 * (size_t)NR)) ||
      (rc = h2d(D.rb, raw->row_base_s, 8 * (size_t)NR)) ||
      (rc = h2d(D.rc, raw->row_col_off, 8 * (size_t)(NR + 1))) ||
      (rc = h2d(D.qo, raw->col_qual_off, 8 * (size_t)(C + 1))) ||
      (rc = h2d(D.q, raw->qual, (size_t)QB)) ||
      (rc = h2d(D.vo, raw->col_val_off, 8 * (size_t)(C + 1))) ||
      (rc = h2d(D.v, raw->val, (size_t)VB)) ||
      (rc = h2d(D.goff, b->group_offsets, 8 * (size_t)(G + 1))) ||
      (rc = h2d(D.mem, b->group_members, 8 * (size_t)M)))
    return rc;
  const otsdb_raw_rows dr{NR, D.rs, D.rb, D.rc, D.qo, D.q, D.vo, D.v, nullptr};
  otsdb_batch db = *b;
  db.n_points = 0;
  db.offsets = db.ts_ms = db.val = nullptr;
  db.is_float = db.series_float = nullptr;
  db.group_offsets = D.goff;
  db.group_members = D.mem;
  otsdb_hist_result dres{cap, D.r_off, D.r_ts, n_pct > 0 ? D.r_pct : nullptr,
                         out->counts ? D.r_cnt : nullptr};
  c->result_short = false;
  int64_t total = 0;
  rc = hist_run_rows_impl(c, spec, P, &dr, simple_codec_id, &db, h, goff, pcts,
                          n_pct, &dres, &total);
  if (rc == OTSDB_E_CAPACITY && c->result_short) {
    // the offsets the whole result needs, then the status
    hipMemcpyAsync(out->offsets, D.r_off, 8 * (G + 1), hipMemcpyDeviceToHost, st);
    hipStreamSynchronize(st);
    return rc;
  }
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(out->offsets, D.r_off, 8 * (G + 1),
                         hipMemcpyDeviceToHost, st));
  if (total > 0) {
    HIP_TRY(hipMemcpyAsync(out->ts, D.r_ts, 8 * total, hipMemcpyDeviceToHost, st));
    for (int q = 0; q < n_pct; ++q)
      HIP_TRY(hipMemcpyAsync(out->pct_val + (size_t)q * cap,
                             D.r_pct + (size_t)q * cap, 8 * total,
                             hipMemcpyDeviceToHost, st));
    if (out->counts)
      HIP_TRY(hipMemcpyAsync(out->counts, D.r_cnt, 8 * (size_t)total * R,
                             hipMemcpyDeviceToHost, st));
  }
  HIP_TRY(hipStreamSynchronize(st));
  return OTSDB_OK;
}

}  // extern "C"
