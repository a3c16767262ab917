// rollup_rows.hip — a rollup table's storage rows -> columnar points
// (ts_ms, val, is_float, value_count), DESIGN.md §4.3.1.
//
// The rows are the scanner's (otsdb_raw_rows): rollup cells are never
// compacted (SaltScanner.java:765-809), so a column is one cell.  What the
// reference does with them, restated:
//   * RollupSpan.addRow (RollupSpan.java:55-72): consecutive rows of one key
//     are ONE RollupSeq, their cells appended in arrival order; a row of
//     another base time starts the next RollupSeq.  Base times that do not
//     increase strictly inside a series are refused here (E_UNSUPPORTED: the
//     scanner delivers key order).
//   * RollupSeq.setRow / addRow (RollupSeq.java:126-208): a cell is a value
//     cell or, when the rollup aggregator R is avg, a count cell — by the
//     numeric id in the qualifier's first byte (& 0x7F), else by the old
//     string prefix ("sum:" / "count:" when R = avg, "<R>:" otherwise);
//     anything else is IllegalDataException.  After the prefix: 2 bytes,
//     offset << 4 | flags.
//   * append (:217-322), per kind: an offset below the last accepted one
//     throws (IllegalDataException for a value cell, IllegalArgumentException
//     for a count cell); so does an equal one without fix_duplicates; with it
//     a cell older (HBase timestamp) than the last accepted one is skipped,
//     any other replaces it.
//   * RollupIterator (:515-745): every accepted value cell is a point; with
//     R = avg the points are the value cells that have a count cell of the
//     same offset (sync(), :557-586), valueCount() that cell's value, a float
//     one cast to long the Java way.  seek() (:613-643) resets, syncs to the
//     first pair (i0, j0), advances BOTH cursors once per value cell before
//     the timestamp, and syncs again: with k such cells the row yields value
//     cells [i0 + k:] intersected with count cells [j0 + k:].
//   * Span.seekRow (Span.java:360-380) over RollupSeq.size() / timestamp(i),
//     which count paired points: the sought row is the first whose last
//     paired point is >= the timestamp, else the series' last row.
// The output keeps the plain pairs before seek_ms (the downsampler skips
// them; they keep the span's first timestamp for the SpanGroup range filter)
// and, from seek_ms on, what the iterator yields after the seek.
//
// One wavefront per RollupSeq (a one-wave workgroup on the seq's first row;
// the other rows of the seq exit).  Offsets are below 3,840 (a first
// qualifier byte of 0xF0.. is the millisecond form the reference misreads:
// E_UNSUPPORTED), so each kind is a 60-word bitmap in LDS beside a table of
// the accepted cell per offset; pairing is the AND of the two bitmaps, the
// seek two thresholds applied before it, a point's output rank a popcount
// prefix.  Duplicates arrive only in runs (offsets never go back), so a chunk
// of 64 cells that holds none — the stored form — takes no serial step.
//
// Kernels:
//   k_rr_seq     mode 0: validates, counts the seq's plain points, its last
//                paired timestamp; mode 1: the sought seqs counted again with
//                the seek; mode 2: writes the points at the scanned offsets;
//   k_rr_sought  one thread per series: Span.seekRow.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

namespace otsdb {

#ifndef OTSDB_DS_TU

constexpr int kRrOffsets = 3840;      // offsets a 2-byte qualifier can hold
constexpr int kRrWords = kRrOffsets / 64;
constexpr int kRrRowCols = 8192;      // columns of one input row
constexpr int kRrSeqCells = 65535;    // cells of one RollupSeq (16-bit table)

struct RollupRowsDev {
  int64_t R;
  const int64_t* row_series;
  const int64_t* row_base_s;
  const int64_t* row_col_off;  // [R+1]
  const int64_t* col_qoff;     // [C+1]
  const uint8_t* qual;
  const int64_t* col_voff;     // [C+1]
  const uint8_t* val;
  const int64_t* col_ts;       // [C] or null (= column index)
  int64_t interval_ms;         // RollupInterval.getIntervalSeconds() * 1000
  int64_t seek_ms;             // INT64_MIN: no seek
  int32_t need_count;          // R = avg
  int32_t value_id, count_id;  // RollupConfig ids
  int32_t fix;                 // tsd.storage.fix_duplicates
  int32_t prefix_len;          // R != avg: "<R>:" (old string qualifiers)
  uint8_t prefix[20];
};

// status codes of a failing cell (otsdb_status values)
enum : int { RR_ILLEGAL_DATA = 1, RR_ILLEGAL_ARGUMENT = 3, RR_UNSUPPORTED = 5 };

DEV void rr_error(unsigned long long* first_err, int64_t r, int code) {
  atomicMin(first_err, ((unsigned long long)r << 8) | (unsigned)code);
}

DEV bool rr_starts(const uint8_t* q, int64_t qlen, const uint8_t* p, int n) {
  if (qlen < n) return false;
  for (int i = 0; i < n; ++i)
    if (q[i] != p[i]) return false;
  return true;
}

// RollupSeq.setRow / addRow's tests in their order: kind (0 value, 1 count)
// and the bytes before the 2-byte qualifier; the status of a cell that is
// neither, or too short
DEV int rr_classify(const RollupRowsDev& T, const uint8_t* q, int64_t qlen,
                    int* kind, int* strip) {
  const uint8_t kSum[3] = {'s', 'u', 'm'};
  const uint8_t kCount[5] = {'c', 'o', 'u', 'n', 't'};
  if (qlen < 1) return RR_ILLEGAL_DATA;
  const int id = q[0] & 0x7F;
  if (T.need_count) {
    if (id == T.value_id) { *kind = 0; *strip = 1; }
    else if (id == T.count_id) { *kind = 1; *strip = 1; }
    else if (rr_starts(q, qlen, kSum, 3)) { *kind = 0; *strip = 4; }
    else if (rr_starts(q, qlen, kCount, 5)) { *kind = 1; *strip = 6; }
    else return RR_ILLEGAL_DATA;
  } else {
    if (id == T.value_id) { *kind = 0; *strip = 1; }
    else if (rr_starts(q, qlen, T.prefix, T.prefix_len)) {
      *kind = 0;
      *strip = T.prefix_len;
    } else return RR_ILLEGAL_DATA;
  }
  return qlen < *strip + 2 ? RR_ILLEGAL_DATA : 0;
}

// (long) of a double as Java casts: NaN -> 0, saturating
DEV int64_t rr_java_long(double d) {
  if (d != d) return 0;
  if (d >= 9223372036854775808.0) return INT64_MAX;
  if (d <= -9223372036854775808.0) return INT64_MIN;
  return (int64_t)d;
}

// Internal.extractIntegerValue / extractFloatingPointValue of the vl bytes
// at a (vl already one of 1/2/4/8, a float's 4/8)
DEV int64_t rr_value(const uint8_t* v, int64_t a, int vl, int fl) {
  uint64_t x = 0;
  for (int i = 0; i < vl; ++i) x = (x << 8) | v[a + i];
  if (fl)
    return vl == 4 ? __double_as_longlong((double)__uint_as_float((uint32_t)x))
                   : (int64_t)x;
  switch (vl) {
    case 1: return (int8_t)x;
    case 2: return (int16_t)x;
    case 4: return (int32_t)x;
    default: return (int64_t)x;
  }
}

DEV int rr_wave_sum(int x) {
  for (int s = 32; s; s >>= 1) x += __shfl_xor(x, s);
  return x;
}

DEV int rr_wave_excl_scan(int x, int lane) {
  int incl = x;
  for (int s = 1; s < 64; s <<= 1) {
    const int y = __shfl_up(incl, s);
    if (lane >= s) incl += y;
  }
  return incl - x;
}

// the bits of bitmap word w whose offsets lie below x
DEV uint64_t rr_below(int x, int w) {
  const int lo = w * 64;
  if (x >= lo + 64) return ~0ULL;
  if (x <= lo) return 0;
  return (1ULL << (x - lo)) - 1;
}

// position of the n-th (0-based) set bit of x; popcount(x) > n
DEV int rr_select(uint64_t x, int n) {
  int pos = 0;
  for (int s = 32; s; s >>= 1) {
    const int c = __popcll(x & (((1ULL << s) - 1) << pos));
    if (n >= c) {
      n -= c;
      pos += s;
    }
  }
  return pos;
}

// row r begins a RollupSeq: the first row, or another key than the row before
DEV bool rr_head(const RollupRowsDev& T, int64_t r) {
  return r == 0 || T.row_series[r - 1] != T.row_series[r] ||
         T.row_base_s[r - 1] != T.row_base_s[r];
}

__global__ void __launch_bounds__(64)
k_rr_seq(RollupRowsDev T, int mode, int64_t* __restrict__ row_count,
         int64_t* __restrict__ row_last, const uint8_t* __restrict__ sought,
         const int64_t* __restrict__ row_out, int64_t cap,
         int64_t* __restrict__ ts, int64_t* __restrict__ val,
         uint8_t* __restrict__ isf, int64_t* __restrict__ cnt,
         unsigned long long* first_err) {
  __shared__ uint16_t win[2][kRrOffsets];  // accepted cell + 1 per offset
  __shared__ uint64_t bm[2][kRrWords];     // offsets that hold one
  __shared__ uint64_t fin[kRrWords];       // the seq's points
  __shared__ int pre[kRrWords];            // points in the words before
  const int lane = threadIdx.x;
  const int64_t r = blockIdx.x;
  if (r >= T.R) return;
  const bool head = rr_head(T, r);
  // base times go up inside a series (equal: the same RollupSeq)
  const bool back = r > 0 && T.row_series[r - 1] == T.row_series[r] &&
                    T.row_base_s[r] < T.row_base_s[r - 1];
  if (mode == 0 && lane == 0 && (!head || back)) {
    row_count[r] = 0;
    row_last[r] = INT64_MIN;
    if (back) rr_error(first_err, r, RR_UNSUPPORTED);
  }
  if (!head || back) return;
  const bool is_sought = sought && sought[r];
  if (mode == 1 && !is_sought) return;
  // the seq's rows [r, r_end): the same key in consecutive rows
  int64_t r_end = r + 1;
  for (;;) {
    const int64_t q = r_end + lane;
    const bool same = q < T.R && T.row_series[q] == T.row_series[r] &&
                      T.row_base_s[q] == T.row_base_s[r];
    const uint64_t m = __ballot(same);
    if (m == ~0ULL) {
      r_end += 64;
      continue;
    }
    r_end += __builtin_ctzll(~m);
    break;
  }
  const int64_t c0 = T.row_col_off[r];
  int64_t c1 = T.row_col_off[r_end];
  // a row past the column limit, a seq past the table's: refused after the
  // cells before it
  int64_t late_row = -1;
  for (int64_t q = r; q < r_end; ++q) {
    const int64_t a = T.row_col_off[q], e = T.row_col_off[q + 1];
    if (e - a > kRrRowCols || e - c0 > kRrSeqCells) {
      late_row = q;
      c1 = a;
      break;
    }
  }
  const int64_t n = c1 - c0;
  for (int i = lane; i < 2 * kRrWords; i += 64) (&bm[0][0])[i] = 0;
  __syncthreads();

  // ---- the cells in arrival order, 64 a step
  int c_off[2] = {-1, -1};  // per kind: the last accepted offset,
  int64_t c_ts[2] = {0, 0};  // its HBase timestamp
  for (int64_t b0 = 0; b0 < n; b0 += 64) {
    const int64_t i = b0 + lane;
    const bool valid = i < n;
    int kind = 0, strip = 0, off = 0, code = 0;
    int64_t t = 0;
    if (valid) {
      const int64_t c = c0 + i;
      const int64_t q0 = T.col_qoff[c], qlen = T.col_qoff[c + 1] - q0;
      const int64_t vlen = T.col_voff[c + 1] - T.col_voff[c];
      const uint8_t* q = T.qual + q0;
      code = rr_classify(T, q, qlen, &kind, &strip);
      if (!code) {
        const int b1 = q[strip], b2 = q[strip + 1];
        off = (b1 << 4) | (b2 >> 4);
        const int fl = b2 & 0x8, vl = (b2 & 0x7) + 1;
        if ((b1 & 0xF0) == 0xF0) code = RR_UNSUPPORTED;  // ms qualifier
        // (the order check comes first in append; the length checks after)
        else if (vlen != vl || (fl ? (vl != 4 && vl != 8)
                                   : (vl != 1 && vl != 2 && vl != 4 && vl != 8)))
          code = -RR_ILLEGAL_DATA;
        t = T.col_ts ? T.col_ts[c] : c;
      }
    }
    const bool ok = valid && (code == 0 || code == -RR_ILLEGAL_DATA);
    // the cell of this kind before: in the step, else the carried one
    const uint64_t m0 = __ballot(ok && kind == 0), m1 = __ballot(ok && kind == 1);
    const uint64_t mk = kind ? m1 : m0;
    const uint64_t below = mk & ((1ULL << lane) - 1);
    const int p = below ? 63 - __builtin_clzll(below) : -1;
    const int poff = __shfl(off, p < 0 ? 0 : p);
    const int prev = p >= 0 ? poff : c_off[kind];
    int dup = 0;
    if (ok && prev >= 0 && off <= prev) {
      if (off < prev || !T.fix)
        code = kind ? RR_ILLEGAL_ARGUMENT : RR_ILLEGAL_DATA;
      else
        dup = 1;
    }
    if (code < 0) code = -code;
    const uint64_t em = __ballot(valid && code != 0);
    if (em) {  // the first failing cell in arrival order
      const int fl = __builtin_ctzll(em);
      const int fc = __shfl(code, fl);
      if (mode == 0 && lane == 0) {
        const int64_t c = c0 + b0 + fl;
        int64_t q = r;
        while (q + 1 < r_end && T.row_col_off[q + 1] <= c) ++q;
        rr_error(first_err, q, fc);
        row_count[r] = 0;
      }
      return;
    }
    if (__ballot(dup) == 0) {
      if (valid) {
        win[kind][off] = (uint16_t)(i + 1);
        atomicOr((unsigned long long*)&bm[kind][off >> 6], 1ULL << (off & 63));
      }
      if (m0) {
        const int l = 63 - __builtin_clzll(m0);
        c_off[0] = __shfl(off, l);
        c_ts[0] = __shfl(t, l);
      }
      if (m1) {
        const int l = 63 - __builtin_clzll(m1);
        c_off[1] = __shfl(off, l);
        c_ts[1] = __shfl(t, l);
      }
    } else {
      // a run of equal offsets (fix_duplicates): append, cell by cell
      const uint64_t vm = __ballot(valid);
      for (int j = 0; j < 64 && ((vm >> j) & 1); ++j) {
        const int kj = __shfl(kind, j), oj = __shfl(off, j);
        const int64_t tj = __shfl(t, j);
        if (oj == c_off[kj] && tj < c_ts[kj]) continue;  // older: skipped
        c_off[kj] = oj;
        c_ts[kj] = tj;
        if (lane == j) {
          win[kj][oj] = (uint16_t)(i + 1);
          atomicOr((unsigned long long*)&bm[kj][oj >> 6], 1ULL << (oj & 63));
        }
      }
    }
  }
  if (late_row >= 0) {
    if (mode == 0 && lane == 0) {
      rr_error(first_err, late_row, RR_UNSUPPORTED);
      row_count[r] = 0;
    }
    return;
  }
  __syncthreads();

  // ---- pairing, the seek, ranks
  const int w = lane;
  const uint64_t a = w < kRrWords ? bm[0][w] : 0;
  const uint64_t b = w < kRrWords ? (T.need_count ? bm[1][w] : ~0ULL) : 0;
  const uint64_t P = a & b;
  const uint64_t pm = __ballot(P != 0);
  const int64_t base_ms = T.row_base_s[r] * 1000;
  uint64_t F = P;
  if (mode == 0) {
    if (pm) {
      const int lw = 63 - __builtin_clzll(pm);
      const uint64_t x = __shfl((unsigned long long)P, lw);
      if (lane == 0)
        row_last[r] = base_ms + (int64_t)(lw * 64 + 63 - __builtin_clzll(x)) *
                                    T.interval_ms;
    } else if (lane == 0) {
      row_last[r] = INT64_MIN;
    }
  } else if (is_sought && T.need_count) {
    F = 0;
    if (pm) {
      const int fw = __builtin_ctzll(pm);
      const uint64_t x = __shfl((unsigned long long)P, fw);
      const int p0 = fw * 64 + __builtin_ctzll(x);  // the first pair
      // the first offset at or after seek_ms
      int so = 0;
      if (T.seek_ms > base_ms) {
        const uint64_t d = (uint64_t)T.seek_ms - (uint64_t)base_ms;
        const uint64_t k = (d + (uint64_t)T.interval_ms - 1) /
                           (uint64_t)T.interval_ms;
        so = k > (uint64_t)kRrOffsets ? kRrOffsets : (int)k;
      }
      const int lo = so > p0 ? so : p0;
      // seek(): i0 + k value cells, j0 + k count cells are behind the cursors
      const int j0 = rr_wave_sum(__popcll(b & rr_below(p0, w)));
      const int k = rr_wave_sum(__popcll(a & rr_below(lo, w) & ~rr_below(p0, w)));
      const int m = j0 + k;
      const int pc = __popcll(b);
      const int ex = rr_wave_excl_scan(pc, lane);
      uint64_t cs = b;
      if (ex + pc <= m) cs = 0;
      else if (ex < m)
        for (int d = m - ex; d; --d) cs &= cs - 1;
      F = (P & rr_below(so, w)) | (a & ~rr_below(lo, w) & cs);
    }
  }
  const int fpc = __popcll(F);
  const int fex = rr_wave_excl_scan(fpc, lane);
  const int total = __shfl(fex + fpc, 63);
  if (mode < 2) {
    if (lane == 0) row_count[r] = total;
    return;
  }
  if (w < kRrWords) {
    fin[w] = F;
    pre[w] = fex;
  }
  __syncthreads();

  // ---- the points, 64 a step in time order
  const int64_t out0 = row_out[r];
  for (int p0 = 0; p0 < total; p0 += 64) {
    const int rank = p0 + lane;
    if (rank >= total) break;
    int lo = 0, hi = kRrWords - 1;  // the last word with pre <= rank
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (pre[mid] <= rank) lo = mid;
      else hi = mid - 1;
    }
    const int off = lo * 64 + rr_select(fin[lo], rank - pre[lo]);
    const int64_t pos = out0 + rank;
    if (pos >= cap) continue;
    int kind, strip;
    {
      const int64_t c = c0 + win[0][off] - 1;
      const int64_t q0 = T.col_qoff[c];
      rr_classify(T, T.qual + q0, T.col_qoff[c + 1] - q0, &kind, &strip);
      const int b2 = T.qual[q0 + strip + 1];
      const int fl = (b2 & 0x8) != 0;
      // (streamed out: the pipeline reads the columns from their start, long
      // after these lines would have left the caches)
      __builtin_nontemporal_store(base_ms + (int64_t)off * T.interval_ms,
                                  &ts[pos]);
      __builtin_nontemporal_store(
          rr_value(T.val, T.col_voff[c], (b2 & 0x7) + 1, fl), &val[pos]);
      __builtin_nontemporal_store((uint8_t)fl, &isf[pos]);
    }
    if (T.need_count && cnt) {
      const int64_t c = c0 + win[1][off] - 1;
      const int64_t q0 = T.col_qoff[c];
      rr_classify(T, T.qual + q0, T.col_qoff[c + 1] - q0, &kind, &strip);
      const int b2 = T.qual[q0 + strip + 1];
      const int fl = (b2 & 0x8) != 0;
      const int64_t x = rr_value(T.val, T.col_voff[c], (b2 & 0x7) + 1, fl);
      __builtin_nontemporal_store(
          fl ? rr_java_long(__longlong_as_double(x)) : x, &cnt[pos]);
    }
  }
}

// Span.seekRow per series: the first RollupSeq whose last paired point is at
// or after seek_ms, else the series' last one (seqs without a pair are passed
// over: row_count 0).  One thread per row, at work on a series' first row.
__global__ void k_rr_sought(RollupRowsDev T, const int64_t* __restrict__ row_count,
                            const int64_t* __restrict__ row_last,
                            uint8_t* __restrict__ sought) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= T.R) return;
  const int64_t s = T.row_series[r];
  if (r > 0 && T.row_series[r - 1] == s) return;
  int64_t last_head = r;
  for (int64_t q = r; q < T.R && T.row_series[q] == s; ++q) {
    if (!rr_head(T, q)) continue;
    last_head = q;
    if (row_count[q] >= 1 && row_last[q] >= T.seek_ms) break;
  }
  sought[last_head] = 1;
}

#endif  // OTSDB_DS_TU

}  // namespace otsdb
