// engine_rows.hip — the storage-row family of the engine's host side:
// compaction of storage rows, span assembly and the query from raw rows
// (rows.hip), the rollup tables' rows paired and decoded (rollup_rows.hip),
// and their C-ABI entries.  What it shares with engine.hip: engine_int.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cctype>
#include <memory>
#include <utility>
#include <vector>

#include <rocprim/device/device_segmented_radix_sort.hpp>

#include "../../include/otsdb_agg.h"
// kernels.hip and decode.hip for their device helpers only (fmap_compose,
// CellsDev, ...): their non-template kernels are engine.hip's (rows.hip and
// rollup_rows.hip guard theirs with the same word, hence the #undef)
#define OTSDB_DS_TU 1
#include "kernels.hip"
#include "decode.hip"
#undef OTSDB_DS_TU
#include "rows.hip"
#include "rollup_rows.hip"
#include "engine_int.h"

using namespace otsdb;
using namespace otsdb::eng;

namespace {

// ----------------------------------------- storage rows -> compacted rows
otsdb_status row_status(otsdb_ctx*, unsigned long long fe, const char* what) {
  if (fe == ~0ULL) return OTSDB_OK;
  const int code = (int)(fe & 0xFF);
  const long long row = (long long)(fe >> 8);
  switch (code) {
    case RS_ILLEGAL_ARGUMENT:
      return fail(OTSDB_E_ILLEGAL_ARGUMENT,
                  "%s row %lld: Can not parse cell, it is not an appended cell",
                  what, row);
    case RS_UNSUPPORTED:
      return fail(OTSDB_E_UNSUPPORTED,
                  "%s row %lld: more than %d points or %d data columns to "
                  "merge, or appended points beside a column out of time order",
                  what, row, kRowCellCap, kRowColCap);
    default:
      return fail(OTSDB_E_ILLEGAL_DATA,
                  "%s row %lld: corrupted value or duplicate timestamp", what,
                  row);
  }
}

// a context-owned cells buffer for R rows, qb / vb bytes
otsdb_status cells_buffer(otsdb_ctx* c, int which, int64_t R, int64_t qb,
                          int64_t vb, otsdb_cells_out* o) {
  const size_t a = ((size_t)(R + 1) * 8 + 255) & ~(size_t)255;
  const size_t q = ((size_t)qb + 256) & ~(size_t)255;
  const size_t v = ((size_t)vb + 256) & ~(size_t)255;
  otsdb_status rc =
      c->raw_cells[which].ensure(4 * a + q + v);
  if (rc) return rc;
  char* p = (char*)c->raw_cells[which].p;
  o->row_series = (int64_t*)p;
  o->row_base_s = (int64_t*)(p + a);
  o->qual_off = (int64_t*)(p + 2 * a);
  o->val_off = (int64_t*)(p + 3 * a);
  o->qual = (uint8_t*)(p + 4 * a);
  o->val = (uint8_t*)(p + 4 * a + q);
  return OTSDB_OK;
}

// CompactionQueue.compact of every storage row (rows.hip).  Output: the kept
// rows' compacted columns packed in row order, *n_out rows; *qbytes / *vbytes
// the bytes written.
// own >= 0: the output goes to the context's cells buffer `own`, returned in
// *owned (o is ignored)
// LARGE rows (rows.hip): rank the columns, record the cells, sort the keys,
// merge — through global memory, one segment per row
otsdb_status compact_large(otsdb_ctx* c, const RawDev& D, int fix,
                           const LargeSlots& LS, int64_t n_large, int64_t NC,
                           int64_t ncell, const int64_t* gen_base,
                           const int64_t* gen_n, CellRec* rec, uint8_t* stq,
                           uint8_t* stv, int64_t* out_q, int64_t* out_v,
                           unsigned long long* first_err, hipStream_t st) {
  if (NC >= (int64_t(1) << 32) || ncell >= (int64_t(1) << 32))
    return fail(OTSDB_E_UNSUPPORTED, "compaction of %lld cells in large rows",
                (long long)ncell);
  size_t t_pairs = 0, t_keys = 0;
  HIP_TRY(rocprim::segmented_radix_sort_pairs(
      nullptr, t_pairs, (const uint64_t*)nullptr, (uint64_t*)nullptr,
      (const int64_t*)nullptr, (int64_t*)nullptr, (unsigned)NC,
      (unsigned)n_large, (const int64_t*)nullptr, (const int64_t*)nullptr, 0,
      64, st));
  HIP_TRY(rocprim::segmented_radix_sort_keys(
      nullptr, t_keys, (const uint64_t*)nullptr, (uint64_t*)nullptr,
      (unsigned)ncell, (unsigned)n_large, (const int64_t*)nullptr,
      (const int64_t*)nullptr, 0, kLargeKeyBits, st));
  const size_t t_scan = scan_tmp_bytes(NC, st);
  const size_t t_sort = std::max(std::max(t_pairs, t_keys), t_scan);
  uint64_t *ckey, *ckey2, *rkey, *rkey2;
  int64_t *cidx, *cidx2, *cslot, *ccount, *cbase, *segb, *sege;
  int* bad;
  void* tmp;
  auto carve = [&](char* base) {
    Carve cv{base};
    ckey = cv.take<uint64_t>(NC);
    ckey2 = cv.take<uint64_t>(NC);
    cidx = cv.take<int64_t>(NC);
    cidx2 = cv.take<int64_t>(NC);
    cslot = cv.take<int64_t>(NC);
    ccount = cv.take<int64_t>(NC + 1);
    cbase = cv.take<int64_t>(NC + 1);
    segb = cv.take<int64_t>(n_large);
    sege = cv.take<int64_t>(n_large);
    bad = cv.take<int>(n_large);
    rkey = cv.take<uint64_t>(ncell);
    rkey2 = cv.take<uint64_t>(ncell);
    tmp = cv.take<char>(t_sort + 1);
    return cv.off + 256;
  };
  otsdb_status rc = c->rows_large.ensure(carve(nullptr));
  if (rc) return rc;
  carve((char*)c->rows_large.p);
  hipLaunchKernelGGL(k_large_cols, dim3(blocks_for(n_large, 4)), dim3(256), 0,
                     st, D, LS, n_large, ckey, cidx, cslot, segb, sege);
  size_t t = t_sort;
  HIP_TRY(rocprim::segmented_radix_sort_pairs(
      tmp, t, (const uint64_t*)ckey, ckey2, (const int64_t*)cidx, cidx2,
      (unsigned)NC, (unsigned)n_large, (const int64_t*)segb,
      (const int64_t*)sege, 0, 64, st));
  HIP_TRY(hipMemsetAsync(ccount + NC, 0, 8, st));
  const unsigned wblocks = blocks_for((NC + 63) / 64, 4);
  hipLaunchKernelGGL(k_large_recs, dim3(wblocks), dim3(256), 0, st, D, LS, NC,
                     (const int64_t*)cidx2, (const int64_t*)cslot, gen_base,
                     ccount, (const int64_t*)nullptr, rec, rkey, bad, 0);
  if ((rc = scan_excl(tmp, t_sort, ccount, cbase, NC, st))) return rc;
  HIP_TRY(hipMemsetAsync(bad, 0, sizeof(int) * n_large, st));
  hipLaunchKernelGGL(k_large_recs, dim3(wblocks), dim3(256), 0, st, D, LS, NC,
                     (const int64_t*)cidx2, (const int64_t*)cslot, gen_base,
                     ccount, (const int64_t*)cbase, rec, rkey, bad, 1);
  hipLaunchKernelGGL(k_large_segs, dim3(blocks_for(n_large, 256)), dim3(256),
                     0, st, LS, n_large, gen_base, gen_n, segb, sege);
  t = t_sort;
  HIP_TRY(rocprim::segmented_radix_sort_keys(
      tmp, t, (const uint64_t*)rkey, rkey2, (unsigned)ncell,
      (unsigned)n_large, (const int64_t*)segb, (const int64_t*)sege, 0,
      kLargeKeyBits, st));
  // (rkey, free after the sort, holds the heap order of rows with unsorted
  // columns)
  hipLaunchKernelGGL(k_large_merge, dim3((unsigned)n_large), dim3(64), 0, st,
                     D, fix, LS, gen_base, gen_n, (const CellRec*)rec,
                     (const uint64_t*)rkey2, (const int*)bad, rkey, stq, stv,
                     out_q, out_v, first_err);
  HIP_TRY(hipGetLastError());
  return OTSDB_OK;
}

otsdb_status compact_impl(otsdb_ctx* c, const otsdb_raw_rows* raw, int fix,
                          const otsdb_cells_out* o, int64_t qcap, int64_t vcap,
                          int64_t* n_out, int64_t* qbytes, int64_t* vbytes,
                          hipStream_t st, int own = -1,
                          otsdb_cells_out* owned = nullptr) {
  const int64_t R = raw->n_rows;
  if (R < 0) return fail(OTSDB_E_ILLEGAL_ARGUMENT, "negative n_rows");
  if (!raw->row_base_s || !raw->row_col_off || !raw->col_qual_off ||
      !raw->col_val_off || (R > 0 && (!raw->qual || !raw->val)))
    return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null raw row array");
  RawDev D{R, raw->row_col_off, raw->col_qual_off, raw->qual, raw->col_val_off,
           raw->val, raw->col_ts};
  const size_t tmpb = scan_tmp_bytes(R, st);
  const size_t A = ((size_t)(R + 1) * 8 + 255) & ~(size_t)255;
  // kind, lone, gen_n, gen_base, out_q, out_v, kept, oq_off, ov_off, k_off,
  // LARGE slots (row, columns, ranked-column base), first_err, counters,
  // scan temp
  const size_t need = 13 * A + 512 + tmpb;
  otsdb_status rc = c->rows_ws.ensure(need);
  if (rc) return rc;
  char* w = (char*)c->rows_ws.p;
  uint8_t* kind = (uint8_t*)w;
  int64_t* lone = (int64_t*)(w + A);
  int64_t* gen_n = (int64_t*)(w + 2 * A);
  int64_t* gen_base = (int64_t*)(w + 3 * A);
  int64_t* out_q = (int64_t*)(w + 4 * A);
  int64_t* out_v = (int64_t*)(w + 5 * A);
  int64_t* kept = (int64_t*)(w + 6 * A);
  int64_t* oq_off = (int64_t*)(w + 7 * A);
  int64_t* ov_off = (int64_t*)(w + 8 * A);
  int64_t* k_off = (int64_t*)(w + 9 * A);
  LargeSlots LS{(unsigned long long*)(w + 13 * A + 256), (int64_t*)(w + 10 * A),
                (int64_t*)(w + 11 * A), (int64_t*)(w + 12 * A)};
  unsigned long long* first_err = (unsigned long long*)(w + 13 * A);
  void* tmp = w + 13 * A + 512;
  HIP_TRY(hipMemsetAsync(first_err, 0xFF, 8, st));
  HIP_TRY(hipMemsetAsync(LS.ctr, 0, 16, st));
  for (int64_t* a : {gen_n, out_q, out_v, kept})
    HIP_TRY(hipMemsetAsync(a + R, 0, 8, st));
  if (R > 0) {
    // the verbatim columns first (64 rows a wavefront), the exact plan only
    // when some row is left (a flag read: one sync)
    int* pend = (int*)(LS.ctr + 8);
    HIP_TRY(hipMemsetAsync(pend, 0, sizeof(int), st));
    hipLaunchKernelGGL(k_rows_uniform, dim3(blocks_for(R, 256)), dim3(256), 0,
                       st, D, kind, lone, gen_n, out_q, out_v, kept, pend);
    int hp = 0;
    HIP_TRY(hipMemcpyAsync(&hp, pend, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (hp)
      hipLaunchKernelGGL(k_rows_plan, dim3(blocks_for(R, 4)), dim3(256), 0, st,
                         D, fix, kind, lone, gen_n, out_q, out_v, kept,
                         first_err, LS);
  }
  HIP_TRY(hipGetLastError());
  if ((rc = scan_excl(tmp, tmpb, gen_n, gen_base, R, st))) return rc;
  HIP_TRY(hipMemcpyAsync(&c->h_small[0], gen_base + R, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(&c->h_small[5], LS.ctr, 16, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  const int64_t ncell = c->h_small[0];
  const int64_t n_large = c->h_small[5], NC = c->h_small[6];
  if (ncell > 0) {
    const size_t recb = ((size_t)ncell * sizeof(CellRec) + 255) & ~(size_t)255;
    const size_t qb = ((size_t)ncell * 4 + 255) & ~(size_t)255;
    rc = c->rows_scr.ensure(recb + qb + (size_t)ncell * 9 + 256);
    if (rc) return rc;
    CellRec* rec = (CellRec*)c->rows_scr.p;
    uint8_t* stq = (uint8_t*)c->rows_scr.p + recb;
    uint8_t* stv = stq + qb;
    hipLaunchKernelGGL(k_rows_general, dim3((unsigned)R), dim3(64), 0, st, D, fix,
                       (const uint8_t*)kind, (const int64_t*)gen_base, rec, stq,
                       stv, out_q, out_v, first_err);
    HIP_TRY(hipGetLastError());
    if (n_large > 0 &&
        (rc = compact_large(c, D, fix, LS, n_large, NC, ncell, gen_base, gen_n,
                            rec, stq, stv, out_q, out_v, first_err, st)))
      return rc;
  }
  HIP_TRY(hipMemcpyAsync(&c->h_small[1], first_err, 8, hipMemcpyDeviceToHost, st));
  if ((rc = scan_excl(tmp, tmpb, out_q, oq_off, R, st))) return rc;
  if ((rc = scan_excl(tmp, tmpb, out_v, ov_off, R, st))) return rc;
  if ((rc = scan_excl(tmp, tmpb, kept, k_off, R, st))) return rc;
  HIP_TRY(hipMemcpyAsync(&c->h_small[2], oq_off + R, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(&c->h_small[3], ov_off + R, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(&c->h_small[4], k_off + R, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  rc = row_status(c, (unsigned long long)c->h_small[1], "storage");
  if (rc) return rc;
  const int64_t tq = c->h_small[2], tv = c->h_small[3], nk = c->h_small[4];
  *n_out = nk;
  if (qbytes) *qbytes = tq;
  if (vbytes) *vbytes = tv;
  int bytes = 1;
  if (own >= 0) {
    if ((rc = cells_buffer(c, own, nk, 0, 0, owned))) return rc;
    // an engine-owned output aliases the input pools when it can
    // (k_rows_alias): the common scan of single compacted columns moves no
    // value bytes
    unsigned long long* acc = LS.ctr + 2;  // 5 words after the counters
    const unsigned long long init[5] = {~0ULL, 0ULL, ~0ULL, 0ULL, 0ULL};
    HIP_TRY(hipMemcpyAsync(acc, init, sizeof(init), hipMemcpyHostToDevice, st));
    if (R > 0)
      hipLaunchKernelGGL(k_rows_alias,
                         dim3((unsigned)std::min<int64_t>(blocks_for(R, 256), 2048)),
                         dim3(256), 0, st, D, (const uint8_t*)kind,
                         (const int64_t*)lone, (const int64_t*)oq_off,
                         (const int64_t*)ov_off, acc);
    HIP_TRY(hipGetLastError());
    unsigned long long h[5];
    HIP_TRY(hipMemcpyAsync(h, acc, sizeof(h), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (nk > 0 && h[4] == 0 && h[0] == h[1] && h[2] == h[3]) {
      bytes = 0;
      owned->qual = const_cast<uint8_t*>(raw->qual) + h[0];
      owned->val = const_cast<uint8_t*>(raw->val) + h[2];
    } else if ((rc = cells_buffer(c, own, nk, tq, tv, owned))) {
      return rc;
    }
    o = owned;
    qcap = tq;
    vcap = tv;
  }
  if (!o) return OTSDB_OK;  // sizes only
  if (tq > qcap || tv > vcap)
    return fail(OTSDB_E_CAPACITY, "compaction output: %lld qualifier / %lld "
                "value bytes, capacity %lld / %lld", (long long)tq,
                (long long)tv, (long long)qcap, (long long)vcap);
  if (!o->row_base_s || !o->qual_off || !o->val_off || !o->qual || !o->val)
    return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null output array");
  CellRec* rec = (CellRec*)c->rows_scr.p;
  const size_t recb = ((size_t)ncell * sizeof(CellRec) + 255) & ~(size_t)255;
  const size_t qb = ((size_t)ncell * 4 + 255) & ~(size_t)255;
  const uint8_t* stq = ncell ? (uint8_t*)c->rows_scr.p + recb : nullptr;
  const uint8_t* stv = ncell ? stq + qb : nullptr;
  (void)rec;
  if (R > 0 && nk > 0 && !bytes) {
    hipLaunchKernelGGL(k_rows_meta, dim3(blocks_for(R, 256)), dim3(256), 0, st,
                       R, raw->row_series, raw->row_base_s, (const uint8_t*)kind,
                       (const int64_t*)oq_off, (const int64_t*)ov_off,
                       (const int64_t*)k_off, o->row_series, o->row_base_s,
                       o->qual_off, o->val_off);
    HIP_TRY(hipGetLastError());
  } else if (R > 0 && nk > 0) {
    // row_series is optional on the output
    hipLaunchKernelGGL(k_rows_write, dim3(blocks_for(R, 4)), dim3(256), 0, st,
                       D, fix, raw->row_series, raw->row_base_s,
                       (const uint8_t*)kind, (const int64_t*)lone,
                       (const int64_t*)gen_base, stq, stv,
                       (const int64_t*)out_q, (const int64_t*)out_v,
                       (const int64_t*)oq_off, (const int64_t*)ov_off,
                       (const int64_t*)k_off, o->row_series, o->row_base_s, o->qual_off, o->qual, o->val_off, o->val);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipMemcpyAsync(o->qual_off + nk, oq_off + R, 8, hipMemcpyDeviceToDevice, st));
  HIP_TRY(hipMemcpyAsync(o->val_off + nk, ov_off + R, 8, hipMemcpyDeviceToDevice, st));
  HIP_TRY(hipStreamSynchronize(st));
  return OTSDB_OK;
}

// Span.addRow over every series' compacted rows (rows.hip).  *identity: no
// series needed the replay (the output then equals the input and, when
// o == nullptr, nothing is written).
otsdb_status span_impl(otsdb_ctx* c, const otsdb_cells* in, int64_t S,
                       const otsdb_cells_out* o, int64_t qcap, int64_t vcap,
                       int64_t* n_out, int64_t* qbytes, int64_t* vbytes,
                       bool* identity, hipStream_t st, int own = -1,
                       otsdb_cells_out* owned = nullptr) {
  const int64_t R = in->n_rows;
  if (R < 0 || S < 0) return fail(OTSDB_E_ILLEGAL_ARGUMENT, "negative sizes");
  CellsDev C{R, in->row_series, in->row_base_s, in->qual_off, in->qual,
             in->val_off, in->val};
  const size_t tmpb = scan_tmp_bytes(S, st);
  const size_t A = ((size_t)(S + 1) * 8 + 255) & ~(size_t)255;
  // series_row, slow, arena_sz, arena_off, o_rows, o_q, o_v, row_off, q_off,
  // v_off, err word, scan temp
  const size_t need = 10 * A + 256 + tmpb;
  otsdb_status rc = c->rows_ws.ensure(need);
  if (rc) return rc;
  char* w = (char*)c->rows_ws.p;
  int64_t* series_row = (int64_t*)w;
  uint8_t* slow = (uint8_t*)(w + A);
  int64_t* arena_sz = (int64_t*)(w + 2 * A);
  int64_t* arena_off = (int64_t*)(w + 3 * A);
  int64_t* o_rows = (int64_t*)(w + 4 * A);
  int64_t* o_q = (int64_t*)(w + 5 * A);
  int64_t* o_v = (int64_t*)(w + 6 * A);
  int64_t* row_off = (int64_t*)(w + 7 * A);
  int64_t* q_off = (int64_t*)(w + 8 * A);
  int64_t* v_off = (int64_t*)(w + 9 * A);
  int* err = (int*)(w + 10 * A);
  void* tmp = w + 10 * A + 256;
  HIP_TRY(hipMemsetAsync(err, 0, 4, st));
  for (int64_t* a : {arena_sz, o_rows, o_q, o_v})
    HIP_TRY(hipMemsetAsync(a + S, 0, 8, st));
  launch_series_rows(R, S, in->row_series, series_row, st);
  if (S > 0)
    hipLaunchKernelGGL(k_span_plan, dim3(blocks_for(S, 4)), dim3(256), 0, st, C,
                       S, (const int64_t*)series_row, slow, arena_sz, o_rows,
                       o_q, o_v, err);
  HIP_TRY(hipGetLastError());
  if ((rc = scan_excl(tmp, tmpb, arena_sz, arena_off, S, st))) return rc;
  HIP_TRY(hipMemcpyAsync(&c->h_small[0], arena_off + S, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(&c->h_small[1], err, 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if ((int)(c->h_small[1] & 0xFFFFFFFF))
    return fail(OTSDB_E_ILLEGAL_ARGUMENT, "a row without a data point");
  const int64_t arena = c->h_small[0];
  *identity = arena == 0;
  if (arena > 0) {
    rc = c->rows_scr.ensure((size_t)arena + 256);
    if (rc) return rc;
    hipLaunchKernelGGL(k_span_replay, dim3((unsigned)S), dim3(64), 0, st, C, S,
                       (const int64_t*)series_row, (const uint8_t*)slow,
                       (const int64_t*)arena_off, (uint8_t*)c->rows_scr.p, o_rows,
                       o_q, o_v);
    HIP_TRY(hipGetLastError());
  }
  if ((rc = scan_excl(tmp, tmpb, o_rows, row_off, S, st))) return rc;
  if ((rc = scan_excl(tmp, tmpb, o_q, q_off, S, st))) return rc;
  if ((rc = scan_excl(tmp, tmpb, o_v, v_off, S, st))) return rc;
  HIP_TRY(hipMemcpyAsync(&c->h_small[2], row_off + S, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(&c->h_small[3], q_off + S, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(&c->h_small[4], v_off + S, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  *n_out = c->h_small[2];
  if (qbytes) *qbytes = c->h_small[3];
  if (vbytes) *vbytes = c->h_small[4];
  if (own >= 0) {
    if (*identity) return OTSDB_OK;  // the input is the span order
    if ((rc = cells_buffer(c, own, *n_out, c->h_small[3], c->h_small[4], owned)))
      return rc;
    o = owned;
    qcap = c->h_small[3];
    vcap = c->h_small[4];
  }
  if (!o) return OTSDB_OK;
  if (c->h_small[3] > qcap || c->h_small[4] > vcap)
    return fail(OTSDB_E_CAPACITY, "span output capacity");
  if (S > 0)
    hipLaunchKernelGGL(k_span_write, dim3(blocks_for(S, 4)), dim3(256), 0, st,
                       C, S, (const int64_t*)series_row, (const uint8_t*)slow,
                       (const int64_t*)arena_off, (const uint8_t*)c->rows_scr.p,
                       (const int64_t*)row_off, (const int64_t*)q_off,
                       (const int64_t*)v_off, o->row_series, o->row_base_s,
                       o->qual_off, o->qual, o->val_off, o->val);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(o->qual_off + *n_out, q_off + S, 8,
                         hipMemcpyDeviceToDevice, st));
  HIP_TRY(hipMemcpyAsync(o->val_off + *n_out, v_off + S, 8,
                         hipMemcpyDeviceToDevice, st));
  HIP_TRY(hipStreamSynchronize(st));
  return OTSDB_OK;
}

// The storage rows taken verbatim, when they can be: every row one
// compacted column (k_rows_shape), the rows of each series in base-time
// order, every series in one group — the rows ARE the compacted, assembled
// spans, viewed in place (qual_off / val_off point into the column offsets).
// The cells fold checks the rest as it streams (Params.check_order).
// Flags spec_miss when the view does not hold or the query would not
// stream every point through the cells fold; the caller then compacts.
otsdb_status run_raw_verbatim(otsdb_ctx* c, const otsdb_query_spec* spec,
                              const otsdb_raw_rows* raw, const otsdb_batch* b,
                              otsdb_result* out, std::vector<int64_t>& goff) {
  hipStream_t st = c->stream;
  const int64_t R = raw->n_rows;
  if (R <= 0 || goff.empty() || goff.back() != b->n_series ||
      !(spec->ds_interval_ms > 0) || spec->run_all || anchored(spec))
    return spec_miss(c);
  RawDev D{R, raw->row_col_off, raw->col_qual_off, raw->qual, raw->col_val_off,
           raw->val, raw->col_ts};
  int* bad = (int*)c->d_mm;
  HIP_TRY(hipMemsetAsync(bad, 0, sizeof(int), st));
  hipLaunchKernelGGL(k_rows_shape, dim3(blocks_for(R, 256)), dim3(256), 0, st,
                     D, raw->row_series, raw->row_base_s, bad);
  HIP_TRY(hipGetLastError());
  int h[3] = {0, 0, 0};
  int64_t c0 = 0;
  HIP_TRY(hipMemcpyAsync(h, bad, sizeof(int), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(&c0, raw->row_col_off, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (h[0]) return spec_miss(c);
  const otsdb_cells cc{R, raw->row_series, raw->row_base_s,
                       raw->col_qual_off + c0, raw->qual,
                       raw->col_val_off + c0, raw->val};
  c->verbatim = true;
  const otsdb_status rc = run_cells_impl(c, spec, &cc, b, out, goff);
  c->verbatim = false;
  return rc;
}

// ------------------------------------------ rollup queries from storage rows
// otsdb_rollup_decode_rows_device / otsdb_agg_run_rollup_rows*: the rows of a
// rollup table paired and decoded on the device (rollup_rows.hip, DESIGN.md
// §4.3.1).
otsdb_status check_rollup_table(const otsdb_raw_rows* raw,
                                const otsdb_rollup_table* t, int32_t agg) {
  if (!raw || !t) return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null");
  if (agg < 0 || agg >= OTSDB_AGG_COUNT_IDS)
    return fail(OTSDB_E_NO_SUCH_ELEMENT, "No such aggregator: %d", agg);
  if (agg == OTSDB_AGG_DEV)
    return fail(OTSDB_E_UNSUPPORTED,
                "standard deviation over rolled up data is not supported");
  if (t->interval_s <= 0)
    return fail(OTSDB_E_ILLEGAL_ARGUMENT, "rollup interval %d s", t->interval_s);
  const bool avg = agg == OTSDB_AGG_AVG;
  if (t->value_id < 0 || t->value_id > 127 ||
      (avg && (t->count_id < 0 || t->count_id > 127)))
    return fail(OTSDB_E_ILLEGAL_ARGUMENT, "rollup aggregator ids are 0..127");
  if (raw->n_rows < 0) return fail(OTSDB_E_ILLEGAL_ARGUMENT, "negative n_rows");
  if (!raw->row_series || !raw->row_base_s || !raw->row_col_off ||
      !raw->col_qual_off || !raw->col_val_off ||
      (raw->n_rows > 0 && (!raw->qual || !raw->val)))
    return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null raw row array");
  return OTSDB_OK;
}

// The decode without the lock (the contract of decode_impl: ts_ms null only
// counts).  cnt may be null (R not avg: never written).
otsdb_status rollup_decode_impl(otsdb_ctx* c, const otsdb_raw_rows* raw,
                                const otsdb_rollup_table* t, int32_t agg,
                                int64_t n_series, int64_t seek_ms,
                                int64_t* offsets, int64_t* ts_ms, int64_t* val,
                                uint8_t* is_float, int64_t* cnt,
                                int64_t capacity, hipStream_t st,
                                bool counted = false) {
  const int64_t R = raw->n_rows, S = n_series;
  if (S < 0) return fail(OTSDB_E_ILLEGAL_ARGUMENT, "negative sizes");
  RollupRowsDev T{};
  T.R = R;
  T.row_series = raw->row_series;
  T.row_base_s = raw->row_base_s;
  T.row_col_off = raw->row_col_off;
  T.col_qoff = raw->col_qual_off;
  T.qual = raw->qual;
  T.col_voff = raw->col_val_off;
  T.val = raw->val;
  T.col_ts = raw->col_ts;
  T.interval_ms = (int64_t)t->interval_s * 1000;
  T.seek_ms = seek_ms;
  T.need_count = agg == OTSDB_AGG_AVG;
  T.value_id = t->value_id;
  T.count_id = t->count_id;
  T.fix = t->fix_duplicates != 0;
  // RollupUtils.getRollupQualifierPrefix(R.toString()): lowercase + ':'
  const char* name = kAggs[agg].name;
  int pl = 0;
  for (; name[pl] && pl < (int)sizeof(T.prefix) - 1; ++pl)
    T.prefix[pl] = (uint8_t)tolower((unsigned char)name[pl]);
  T.prefix[pl++] = ':';
  T.prefix_len = pl;
  const bool seek = T.need_count && seek_ms != INT64_MIN;
  // workspace: row counts, row output offsets, last paired timestamps, the
  // sought marks, the first error, the scan's temporary storage
  const size_t tmpb = scan_tmp_bytes(R, st);
  const size_t A = ((size_t)(R + 1) * 8 + 255) & ~(size_t)255;
  otsdb_status rc = c->dec_ws.ensure(4 * A + 256 + tmpb);
  if (rc) return rc;
  char* w = (char*)c->dec_ws.p;
  int64_t* row_count = (int64_t*)w;
  int64_t* row_out = (int64_t*)(w + A);
  int64_t* row_last = (int64_t*)(w + 2 * A);
  uint8_t* sought = (uint8_t*)(w + 3 * A);
  unsigned long long* first_err = (unsigned long long*)(w + 4 * A);
  void* tmp = w + 4 * A + 256;
  auto pass = [&](int mode) {
    hipLaunchKernelGGL(k_rr_seq, dim3((unsigned)R), dim3(64), 0, st, T, mode,
                       row_count, row_last,
                       (const uint8_t*)(seek ? sought : nullptr),
                       (const int64_t*)row_out, capacity, ts_ms, val, is_float,
                       cnt, first_err);
  };
  // counted: an earlier call on the same rows (ts_ms null) left the row
  // output offsets and the sought marks here: only the write pass runs, and
  // the caller's pipeline follows it on the same stream (no synchronise)
  if (counted) {
    if (R > 0) pass(2);
    HIP_TRY(hipGetLastError());
    return OTSDB_OK;
  }
  HIP_TRY(hipMemsetAsync(first_err, 0xFF, 8, st));
  HIP_TRY(hipMemsetAsync(row_count + R, 0, 8, st));
  if (R > 0) {
    pass(0);
    if (seek) {
      HIP_TRY(hipMemsetAsync(sought, 0, (size_t)R, st));
      hipLaunchKernelGGL(k_rr_sought, dim3(blocks_for(R, 256)), dim3(256), 0,
                         st, T, (const int64_t*)row_count,
                         (const int64_t*)row_last, sought);
      pass(1);
    }
  }
  HIP_TRY(hipGetLastError());
  if ((rc = scan_excl(tmp, tmpb, row_count, row_out, R, st))) return rc;
  launch_series_offsets(R, S, raw->row_series, row_out, offsets, st);
  HIP_TRY(hipMemcpyAsync(&c->h_small[0], first_err, 8, hipMemcpyDeviceToHost,
                         st));
  HIP_TRY(hipMemcpyAsync(&c->h_small[1], row_out + R, 8, hipMemcpyDeviceToHost,
                         st));
  HIP_TRY(hipStreamSynchronize(st));
  const unsigned long long fe = (unsigned long long)c->h_small[0];
  if (fe != ~0ULL) {
    const long long row = (long long)(fe >> 8);
    switch ((int)(fe & 0xFF)) {
      case RR_ILLEGAL_DATA:
        return fail(OTSDB_E_ILLEGAL_DATA,
                    "rollup row %lld: a cell of another aggregator, a value "
                    "offset going back, or value bytes that do not match the "
                    "qualifier", row);
      case RR_ILLEGAL_ARGUMENT:
        return fail(OTSDB_E_ILLEGAL_ARGUMENT,
                    "rollup row %lld: a count offset is <= the last offset",
                    row);
      default:
        return fail(OTSDB_E_UNSUPPORTED,
                    "rollup row %lld: a millisecond qualifier, more than %d "
                    "columns, or base times that do not increase", row,
                    kRrRowCols);
    }
  }
  const int64_t total = c->h_small[1];
  if (!ts_ms) return OTSDB_OK;
  if (total > capacity)
    return fail(OTSDB_E_CAPACITY, "decode capacity %lld < %lld points",
                (long long)capacity, (long long)total);
  if (R > 0) pass(2);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(st));
  return OTSDB_OK;
}

// The timestamp the query's downsampler hands its source
// (Downsampler.seekInterval, Downsampler.java:412-434): "all" seeks to the
// window's start as given, a calendar to the first edge at or after it, a
// fixed interval to the start rounded up to a multiple of it.
int64_t rollup_seek_ms(const otsdb_query_spec* s) {
  if (s->run_all) return s->start_ms;
  if (s->use_calendar && s->cal_edges && s->n_cal_edges > 0) {
    const int64_t* e = s->cal_edges;
    const int64_t* p = std::lower_bound(e, e + s->n_cal_edges, s->start_ms);
    return p == e + s->n_cal_edges ? s->start_ms : *p;
  }
  const int64_t iv = s->ds_interval_ms;
  return align_down(s->start_ms + iv - 1, iv);
}

// device pointers throughout: the rows decoded into the context's columnar
// buffer, then otsdb_agg_run_rollup_device's pipeline over it
otsdb_status run_rollup_rows_impl(otsdb_ctx* c, const otsdb_query_spec* spec,
                                  const otsdb_raw_rows* raw,
                                  const otsdb_rollup_table* t, int32_t agg,
                                  const otsdb_batch* b, otsdb_result* out,
                                  std::vector<int64_t>& goff) {
  hipStream_t st = c->stream;
  const int64_t S = b->n_series;
  otsdb_status rc =
      c->cells_ws.ensure((size_t)(S + 1) * 8 + 64);
  if (rc) return rc;
  int64_t* offs = (int64_t*)c->cells_ws.p;
  const int64_t seek_ms = rollup_seek_ms(spec);
  // the decode (its own stage; released before the pipeline)
  std::unique_ptr<StageTimer> dec_tm(new StageTimer(c, 7));
  rc = rollup_decode_impl(c, raw, t, agg, S, seek_ms, offs, nullptr, nullptr,
                          nullptr, nullptr, 0, st);
  if (rc) return rc;
  const int64_t N = c->h_small[1];
  const size_t col = ((size_t)std::max<int64_t>(N, 2) * 8 + 255) & ~(size_t)255;
  rc = c->cells_col.ensure(4 * col + 256);
  if (rc) return rc;
  int64_t* ts = (int64_t*)c->cells_col.p;
  int64_t* vv = (int64_t*)((char*)c->cells_col.p + col);
  int64_t* cnt = (int64_t*)((char*)c->cells_col.p + 2 * col);
  uint8_t* isf = (uint8_t*)((char*)c->cells_col.p + 3 * col);
  rc = rollup_decode_impl(c, raw, t, agg, S, seek_ms, offs, ts, vv, isf, cnt, N,
                          st, true);
  dec_tm.reset();
  if (rc) return rc;
  otsdb_batch cb = *b;
  cb.n_points = N;
  cb.offsets = offs;
  cb.ts_ms = ts;
  cb.val = vv;
  cb.is_float = isf;
  cb.series_float = nullptr;
  return run_rollup_impl(c, spec, &cb, Rollup{agg, cnt}, out, goff);
}

// The host-pointer entries over storage rows: the rows, the groups and the
// result staged in HBM; check: the entry's argument checks; run: its device
// implementation over the staged copies.
template <class Check, class Run>
otsdb_status run_rows_host(otsdb_ctx* c, const otsdb_raw_rows* raw,
                           const otsdb_batch* b, otsdb_result* out,
                           Check check, Run run) {
  CtxLock lk(c);
  HIP_TRY(hipSetDevice(c->device));
  otsdb_status rc = check();
  if (rc) return rc;
  std::vector<int64_t> goff;
  if ((rc = read_goff(c, b, false, goff))) return rc;
  const int64_t R = raw->n_rows, S = b->n_series, G = b->n_groups;
  if (R < 0 || S < 0) return fail(OTSDB_E_ILLEGAL_ARGUMENT, "negative sizes");
  if (!raw->row_series || !raw->row_base_s || !raw->row_col_off ||
      !raw->col_qual_off || !raw->col_val_off)
    return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null raw row array");
  const int64_t M = goff.back();
  for (int64_t r = 0; r < R; ++r)
    if (raw->row_series[r] < 0 || raw->row_series[r] >= S ||
        (r && raw->row_series[r] < raw->row_series[r - 1]))
      return fail(OTSDB_E_ILLEGAL_ARGUMENT,
                  "row_series must be nondecreasing series indices");
  for (int64_t m = 0; m < M; ++m)
    if (b->group_members[m] < 0 || b->group_members[m] >= S)
      return fail(OTSDB_E_ILLEGAL_ARGUMENT, "group member out of range");
  const int64_t C = raw->row_col_off[R];
  const int64_t QB = raw->col_qual_off[C], VB = raw->col_val_off[C];
  const int64_t cap = out->capacity;
  auto carve = [&](char* base) {
    Carve cv{base};
    void* p[14];
    p[0] = cv.take<int64_t>(R + 1);
    p[1] = cv.take<int64_t>(R + 1);
    p[2] = cv.take<int64_t>(R + 1);
    p[3] = cv.take<int64_t>(C + 1);
    p[4] = cv.take<uint8_t>(QB + 16);
    p[5] = cv.take<int64_t>(C + 1);
    p[6] = cv.take<uint8_t>(VB + 16);
    p[7] = raw->col_ts ? cv.take<int64_t>(C + 1) : nullptr;
    p[8] = cv.take<int64_t>(G + 1);
    p[9] = cv.take<int64_t>(M + 1);
    p[10] = cv.take<int64_t>(G + 1);
    p[11] = cv.take<int64_t>(cap + 1);
    p[12] = cv.take<int64_t>(cap + 1);
    p[13] = cv.take<uint8_t>(cap + 1);
    return std::make_pair(cv.off + 256, std::vector<void*>(p, p + 14));
  };
  rc = c->raw_stage.ensure(carve(nullptr).first);
  if (rc) return rc;
  auto pp = carve((char*)c->raw_stage.p).second;
  hipStream_t st = c->stream;
  auto h2d = [&](void* d, const void* h, size_t n) -> otsdb_status {
    if (n && h) HIP_TRY(hipMemcpyAsync(d, h, n, hipMemcpyHostToDevice, st));
    return OTSDB_OK;
  };
  if ((rc = h2d(pp[0], raw->row_series, 8 * R)) ||
      (rc = h2d(pp[1], raw->row_base_s, 8 * R)) ||
      (rc = h2d(pp[2], raw->row_col_off, 8 * (R + 1))) ||
      (rc = h2d(pp[3], raw->col_qual_off, 8 * (C + 1))) ||
      (rc = h2d(pp[4], raw->qual, QB)) ||
      (rc = h2d(pp[5], raw->col_val_off, 8 * (C + 1))) ||
      (rc = h2d(pp[6], raw->val, VB)) ||
      (rc = h2d(pp[7], raw->col_ts, 8 * C)) ||
      (rc = h2d(pp[8], b->group_offsets, 8 * (G + 1))) ||
      (rc = h2d(pp[9], b->group_members, 8 * M)))
    return rc;
  otsdb_raw_rows dr{R,
                    (const int64_t*)pp[0],
                    (const int64_t*)pp[1],
                    (const int64_t*)pp[2],
                    (const int64_t*)pp[3],
                    (const uint8_t*)pp[4],
                    (const int64_t*)pp[5],
                    (const uint8_t*)pp[6],
                    (const int64_t*)pp[7]};
  otsdb_batch db = *b;
  db.n_points = 0;
  db.offsets = nullptr;
  db.ts_ms = nullptr;
  db.val = nullptr;
  db.is_float = nullptr;
  db.series_float = nullptr;
  db.group_offsets = (const int64_t*)pp[8];
  db.group_members = (const int64_t*)pp[9];
  otsdb_result dres;
  dres.capacity = cap;
  dres.offsets = (int64_t*)pp[10];
  dres.ts = (int64_t*)pp[11];
  dres.val = (int64_t*)pp[12];
  dres.is_int = (uint8_t*)pp[13];
  c->result_short = false;
  rc = run(&dr, &db, &dres, goff);
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

}  // namespace

namespace otsdb {
namespace eng {

// The query from storage rows: compaction -> span assembly -> the cells
// query (DEVICE pointers).
otsdb_status run_raw_impl(otsdb_ctx* c, const otsdb_query_spec* spec,
                          const otsdb_raw_rows* raw, int fix,
                          const otsdb_batch* b, otsdb_result* out,
                          std::vector<int64_t>& goff) {
  hipStream_t st = c->stream;
  if (!raw->row_series) return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null row_series");
  if (!raw->row_base_s || !raw->row_col_off || !raw->col_qual_off ||
      !raw->col_val_off || (raw->n_rows > 0 && (!raw->qual || !raw->val)))
    return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null raw row array");
  {
    c->spec_miss = false;
    const otsdb_status v = run_raw_verbatim(c, spec, raw, b, out, goff);
    if (!c->spec_miss) return v;
    c->spec_miss = false;
  }
  int64_t nk = 0, tq = 0, tv = 0;
  otsdb_cells_out co;
  otsdb_status rc;
  {
    StageTimer tm(c, 5);  // query-time compaction
    rc = compact_impl(c, raw, fix, nullptr, 0, 0, &nk, &tq, &tv, st, 0, &co);
  }
  if (rc) return rc;
  otsdb_cells cc{nk, co.row_series, co.row_base_s, co.qual_off, co.qual,
                 co.val_off, co.val};
  int64_t ns = 0, sq = 0, sv = 0;
  bool identity = true;
  otsdb_cells_out so;
  {
    StageTimer tm(c, 6);  // span assembly
    rc = span_impl(c, &cc, b->n_series, nullptr, 0, 0, &ns, &sq, &sv,
                   &identity, st, 1, &so);
  }
  if (rc) return rc;
  if (!identity)
    cc = otsdb_cells{ns, so.row_series, so.row_base_s, so.qual_off, so.qual,
                     so.val_off, so.val};
  return run_cells_impl(c, spec, &cc, b, out, goff);
}

}  // namespace eng
}  // namespace otsdb

extern "C" {

otsdb_status otsdb_compact_rows_device(otsdb_ctx* c, const otsdb_raw_rows* raw,
                                       int32_t fix_duplicates,
                                       const otsdb_cells_out* out,
                                       int64_t qual_capacity,
                                       int64_t val_capacity, int64_t* n_out_rows,
                                       void* hip_stream) {
  if (!c || !raw || !n_out_rows) return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null");
  CtxLock lk(c);
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
  return compact_impl(c, raw, fix_duplicates != 0, out, qual_capacity,
                      val_capacity, n_out_rows, nullptr, nullptr, st);
}

otsdb_status otsdb_span_assemble_device(otsdb_ctx* c, const otsdb_cells* cells,
                                        int64_t n_series,
                                        const otsdb_cells_out* out,
                                        int64_t qual_capacity,
                                        int64_t val_capacity,
                                        int64_t* n_out_rows, void* hip_stream) {
  if (!c || !cells || !n_out_rows) return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null");
  if (out && !out->row_series)
    return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null output row_series");
  CtxLock lk(c);
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
  bool identity = true;
  return span_impl(c, cells, n_series, out, qual_capacity, val_capacity,
                   n_out_rows, nullptr, nullptr, &identity, st);
}

otsdb_status otsdb_agg_run_raw_device(otsdb_ctx* c, const otsdb_query_spec* spec,
                                      const otsdb_raw_rows* raw,
                                      int32_t fix_duplicates,
                                      const otsdb_batch* b, otsdb_result* out,
                                      void* hip_stream) {
  if (!c || !spec || !raw || !b || !out)
    return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null");
  DeviceCall dc(c, b, hip_stream);
  otsdb_status rc = dc.rc;
  if (!rc) rc = check_spec(spec);
  if (!rc) rc = run_raw_impl(c, spec, raw, fix_duplicates != 0, b, out, dc.goff);
  return rc;
}

otsdb_status otsdb_agg_run_raw(otsdb_ctx* c, const otsdb_query_spec* spec,
                               const otsdb_raw_rows* raw, int32_t fix_duplicates,
                               const otsdb_batch* b, otsdb_result* out) {
  if (!c || !spec || !raw || !b || !out)
    return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null");
  return run_rows_host(
      c, raw, b, out, [&] { return check_spec(spec); },
      [&](const otsdb_raw_rows* dr, const otsdb_batch* db, otsdb_result* dres,
          std::vector<int64_t>& goff) {
        return run_raw_impl(c, spec, dr, fix_duplicates != 0, db, dres, goff);
      });
}

otsdb_status otsdb_rollup_decode_rows_device(
    otsdb_ctx* c, const otsdb_raw_rows* raw, const otsdb_rollup_table* table,
    int32_t rollup_agg_id, int64_t n_series, int64_t seek_ms, int64_t* offsets,
    int64_t* ts_ms, int64_t* val, uint8_t* is_float, int64_t* value_count,
    int64_t capacity, void* hip_stream) {
  // (the argument checks first: they need no context)
  otsdb_status rc = check_rollup_table(raw, table, rollup_agg_id);
  if (rc) return rc;
  if (!c || !offsets) return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null");
  if (ts_ms && (!val || !is_float ||
                (rollup_agg_id == OTSDB_AGG_AVG && !value_count)))
    return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null output column");
  CtxLock lk(c);
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
  return rollup_decode_impl(c, raw, table, rollup_agg_id, n_series, seek_ms,
                            offsets, ts_ms, val, is_float, value_count,
                            capacity, st);
}

// check_rollup's refusals with the counts still to come (the decode writes
// them), then the table's
static otsdb_status check_rollup_rows(const otsdb_query_spec* spec,
                                      const otsdb_raw_rows* raw,
                                      const otsdb_rollup_table* table,
                                      int32_t agg) {
  static const int64_t kPending = 0;
  RollupKind kind;
  const otsdb_status rc = check_rollup(spec, Rollup{agg, &kPending}, &kind);
  return rc ? rc : check_rollup_table(raw, table, agg);
}

otsdb_status otsdb_agg_run_rollup_rows_device(
    otsdb_ctx* c, const otsdb_query_spec* spec, const otsdb_raw_rows* raw,
    const otsdb_rollup_table* table, int32_t rollup_agg_id,
    const otsdb_batch* b, otsdb_result* out, void* hip_stream) {
  if (!spec || !raw || !table || !b || !out)
    return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null");
  // (the argument checks first: they need no context)
  const otsdb_status rc = check_rollup_rows(spec, raw, table, rollup_agg_id);
  if (rc) return rc;
  if (!c) return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null context");
  DeviceCall dc(c, b, hip_stream);
  return dc.rc ? dc.rc
               : run_rollup_rows_impl(c, spec, raw, table, rollup_agg_id, b,
                                      out, dc.goff);
}

otsdb_status otsdb_agg_run_rollup_rows(otsdb_ctx* c,
                                       const otsdb_query_spec* spec,
                                       const otsdb_raw_rows* raw,
                                       const otsdb_rollup_table* table,
                                       int32_t rollup_agg_id,
                                       const otsdb_batch* b,
                                       otsdb_result* out) {
  if (!spec || !raw || !table || !b || !out)
    return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null");
  // (the argument checks first: they need no context)
  const otsdb_status rc = check_rollup_rows(spec, raw, table, rollup_agg_id);
  if (rc) return rc;
  if (!c) return fail(OTSDB_E_ILLEGAL_ARGUMENT, "null context");
  return run_rows_host(
      c, raw, b, out, [] { return OTSDB_OK; },
      [&](const otsdb_raw_rows* dr, const otsdb_batch* db, otsdb_result* dres,
          std::vector<int64_t>& goff) {
        return run_rollup_rows_impl(c, spec, dr, table, rollup_agg_id, db,
                                    dres, goff);
      });
}

}  // extern "C"
