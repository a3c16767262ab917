// topn.hip — the gexp top-N functions over query results: highestMax and
// highestCurrent (src/query/expression/HighestMax.java:40-148,
// HighestCurrent.java:40-152).  Both run the reference's core a second time:
// an AggregationIterator (LERP, no rate) over the result series of the
// sub-queries whose "aggregator" (MaxCacheAggregator, HighestMax.java:182-292;
// MaxLatestAggregator, HighestCurrent.java:164-282) does not reduce but
// records one key per series; the series are then sorted by key.
//
// What is restated, quirks included:
//   - the aggregator reads the emission's values with nextLongValue /
//     nextDoubleValue, which skip the series that do not contribute: the k-th
//     CONTRIBUTING series' value lands in slot k, the rest of the vector is 0,
//     and slot k's key is later taken as series k's key;
//   - highestMax: max_longs from Long.MIN_VALUE, max_doubles from
//     Double.MIN_VALUE (4.9e-324, the smallest POSITIVE double); an integer
//     emission folds the whole vector, padding zeros included; Math.max on
//     doubles keeps NaN and puts +0.0 over -0.0;
//   - highestCurrent: latest_ts is never updated, so the vectors are those of
//     the last integer and of the last double emission;
//   - key: both kinds of emission seen: Math.max((double)long, double); else
//     the kind seen; sorted descending by Double.compare, stable.
//
// General path (any input), one query:
//   k_topn_series    per input series: its result, its points, its number
//   k_topn_concat    one wavefront per series: the points into one columnar
//                    view (RawView), the seek (first point >= start), the
//                    strictly-increasing check
//   k_raw_cand_*     (raw.hip) the emission candidates of one group of all
//                    numbered series; device radix sort + unique: emissions
//   k_topn_eval      one thread per emission: isInteger over every series'
//                    slots, then the walk in series order with span_slots /
//                    span_long / span_double, counting positions; highestMax
//                    folds with atomic max on order-preserving keys (NaN on
//                    top), highestCurrent only marks the last emission of
//                    each kind
//   k_topn_current   highestCurrent: the vectors of those two emissions, one
//                    workgroup each (positions by a block scan)
//   k_topn_keys      per slot: the key rule, the sort key
//   (device radix sort of (descending Double.compare key, slot), stable)
//   k_topn_pick      the picked slots' series, keys and point counts
//   k_topn_gather    one wavefront per picked series: its whole point list
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "raw.hip"

namespace otsdb {

enum : int { TOPN_HIGHEST_MAX = 0, TOPN_HIGHEST_CURRENT = 1 };

// one input result (device pointers) and the flat number of its first series
struct TopnSrc {
  const int64_t* off;
  const int64_t* ts;
  const int64_t* val;
  const uint8_t* is_int;
  int64_t s0;
};

// marks written by k_topn_eval (int64 each)
enum : int {
  TOPN_LAST_INT = 0,  // 1 + index of the last integer emission (0: none)
  TOPN_LAST_DBL = 1,  // 1 + index of the last double emission (0: none)
  TOPN_MIN_ACT = 2,   // fewest contributing series of any integer emission
  TOPN_ANY_LONG = 3,  // 1: some input point is a long (k_topn_concat)
  TOPN_MARKS = 4
};

// series per round of k_topn_current (one workgroup): positions carry a
// running base from round to round
constexpr int kTopnRound = 1024;

constexpr uint64_t kTopnNanKey = ~0ULL;  // NaN: above every double's key
constexpr int64_t kCanonNan = 0x7FF8000000000000LL;  // Double.doubleToLongBits

// order-preserving key of a double under Math.max: -0.0 < +0.0, NaN on top
DEV uint64_t topn_dkey(double v) { return is_nan(v) ? kTopnNanKey : raw_dkey(v); }
DEV double topn_key_double(uint64_t k) {
  return k == kTopnNanKey ? __longlong_as_double(kCanonNan) : raw_key_double(k);
}

// Math.max(double, double): NaN if either is, +0.0 over -0.0
DEV double jmax_double(double a, double b) {
  if (is_nan(a) || is_nan(b)) return __longlong_as_double(kCanonNan);
  return topn_dkey(a) >= topn_dkey(b) ? a : b;
}

// ------------------------------------------------------------------------
// k_topn_series: one thread per input series, numbered in list order then
// group order.  highestCurrent drops the series without a point before it
// numbers them (HighestCurrent.java:95-102); highestMax numbers every one.
// ------------------------------------------------------------------------
__global__ void k_topn_series(int R, const TopnSrc* __restrict__ src, int64_t S,
                              int fn, int32_t* __restrict__ sres,
                              int64_t* __restrict__ sp0,
                              int64_t* __restrict__ slen,
                              int64_t* __restrict__ numbered) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= S) return;
  int r = 0;
  while (r + 1 < R && src[r + 1].s0 <= i) ++r;
  const int64_t g = i - src[r].s0;
  const int64_t p0 = src[r].off[g], p1 = src[r].off[g + 1];
  sres[i] = r;
  sp0[i] = p0;
  slen[i] = p1 > p0 ? p1 - p0 : 0;
  numbered[i] = (fn == TOPN_HIGHEST_MAX || p1 > p0) ? 1 : 0;
}

// members[k] = the flat series numbered k
__global__ void k_topn_members(int64_t S, const int64_t* __restrict__ numbered,
                               const int64_t* __restrict__ nrank,
                               int64_t* __restrict__ members) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= S) return;
  if (numbered[i]) members[nrank[i]] = i;
}

// ------------------------------------------------------------------------
// k_topn_concat: one wavefront per series.  Its points go to [soff[i],
// soff[i + 1]) of the view's columns (is_float = !is_int); lo[i] is the
// iterator's seek (the first point >= start, PostAggregatedDataPoints'
// iterator under AggregationIterator.java:414-441; no SpanGroup.add filter
// here: a series past the window still shows its first point to isInteger),
// hi[i] one past its last point.  Timestamps that do not strictly increase
// flag ERR_RAW_DUP — anywhere in the series, points before the seek
// included, which the iterator never sees: stricter than the iterator needs,
// and harmless for results of the query entries, which always increase.
// ------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_topn_concat(
    int64_t S, int64_t start_ms, const TopnSrc* __restrict__ src,
    const int32_t* __restrict__ sres, const int64_t* __restrict__ sp0,
    const int64_t* __restrict__ soff, int64_t* __restrict__ cts,
    int64_t* __restrict__ cval, uint8_t* __restrict__ cflt,
    int64_t* __restrict__ lo, int64_t* __restrict__ hi,
    long long* __restrict__ marks, int* err_word) {
  const int lane = LANE;
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= S) return;
  const TopnSrc R = src[sres[i]];
  const int64_t p0 = sp0[i], o0 = soff[i], n = soff[i + 1] - o0;
  int bad = 0, anyl = 0;
  for (int64_t j = lane; j < n; j += 64) {
    const int64_t t = R.ts[p0 + j];
    if (j > 0 && R.ts[p0 + j - 1] >= t) bad = 1;
    cts[o0 + j] = t;
    cval[o0 + j] = R.val[p0 + j];
    const int li = R.is_int[p0 + j] ? 1 : 0;
    anyl |= li;
    cflt[o0 + j] = li ? 0 : 1;
  }
  if (__ballot(bad) && lane == 0) atomicOr(err_word, ERR_RAW_DUP);
  if (__ballot(anyl) && lane == 0) atomicMax(&marks[TOPN_ANY_LONG], 1LL);
  if (lane == 0) {
    lo[i] = o0 + (lower_bound(R.ts, p0, p0 + n, start_ms) - p0);
    hi[i] = o0 + n;
  }
}

// the slots' start values (MaxCacheAggregator's constructor,
// HighestMax.java:218-221: Long.MIN_VALUE and Double.MIN_VALUE) and the marks
__global__ void k_topn_init(int64_t n, long long* __restrict__ maxl,
                            unsigned long long* __restrict__ maxd,
                            long long* __restrict__ marks) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k < n) {
    maxl[k] = INT64_MIN;
    maxd[k] = raw_dkey(__longlong_as_double(1LL));  // 4.9e-324
  }
  if (k == 0) {
    marks[TOPN_LAST_INT] = 0;
    marks[TOPN_LAST_DBL] = 0;
    marks[TOPN_MIN_ACT] = INT64_MAX;
    marks[TOPN_ANY_LONG] = 0;
  }
}

// ------------------------------------------------------------------------
// k_topn_eval: one thread per emission u (timestamp ukeys[u] >> kOccBits).
// isInteger is decided over every numbered series' slots first
// (AggregationIterator.java:612-625: a series not yet started shows its
// first point), then the series are walked in order and the k-th
// contributing one's value goes to slot k.
//   highestMax: slot k folds the value (atomic max; a plain read first: the
//     slots only grow, so a stale read can only ask for an atomic too many).
//     The zero padding of an integer emission with a contributing series
//     reaches the slots from a on: only the smallest a matters (TOPN_MIN_ACT).
//   highestCurrent: only the marks; k_topn_current writes the vectors.
// ------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_topn_eval(
    Params P, RawView V, int fn, int64_t n, const int64_t* __restrict__ members,
    int64_t E, const uint64_t* __restrict__ ukeys,
    long long* __restrict__ maxl, unsigned long long* __restrict__ maxd,
    long long* __restrict__ marks, int* err_word) {
  const int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= E) return;
  const int64_t x = (int64_t)(ukeys[u] >> kOccBits);
  bool is_int = marks[TOPN_ANY_LONG] != 0;  // all doubles: no slot to ask
  for (int64_t k = 0; k < n && is_int; ++k) {
    const int64_t s = members[k];
    is_int = !slots_float(V, s, span_slots(P, V, s, x, 0));
  }
  atomicMax(&marks[is_int ? TOPN_LAST_INT : TOPN_LAST_DBL], (long long)(u + 1));
  if (fn != TOPN_HIGHEST_MAX) return;
  int err = 0;
  int64_t pos = 0;
  for (int64_t k = 0; k < n; ++k) {
    const int64_t s = members[k];
    const Slots q = span_slots(P, V, s, x, 0);
    if (q.state != 1) continue;
    if (is_int) {
      const long long v = span_long(P, V, q, x, &err);
      if (v > maxl[pos]) atomicMax(&maxl[pos], v);
    } else {
      const unsigned long long key = topn_dkey(span_double(P, V, s, q, x, &err));
      if (key > maxd[pos]) atomicMax(&maxd[pos], key);
    }
    ++pos;
  }
  if (is_int) atomicMin(&marks[TOPN_MIN_ACT], (long long)pos);
  if (err) atomicOr(err_word, err);
}

// ------------------------------------------------------------------------
// k_topn_current: block 0 writes the vector of the last integer emission into
// vecl, block 1 that of the last double emission into vecd (value bits):
// thread per series, its position the count of contributing series before it
// (ballot inside the wavefront, LDS across the 16 of the block, a running
// base across rounds); the slots from the contributing count on are 0.
// ------------------------------------------------------------------------
__global__ __launch_bounds__(kTopnRound) void k_topn_current(
    Params P, RawView V, int64_t n, const int64_t* __restrict__ members,
    const uint64_t* __restrict__ ukeys, const long long* __restrict__ marks,
    int64_t* __restrict__ vecl, int64_t* __restrict__ vecd, int* err_word) {
  __shared__ int wcount[kTopnRound / 64];
  const bool is_int = blockIdx.x == 0;
  const int64_t u = marks[is_int ? TOPN_LAST_INT : TOPN_LAST_DBL] - 1;
  if (u < 0) return;
  const int64_t x = (int64_t)(ukeys[u] >> kOccBits);
  int64_t* vec = is_int ? vecl : vecd;
  const int tid = threadIdx.x, lane = LANE, w = tid >> 6;
  int err = 0;
  int64_t base = 0;
  for (int64_t k0 = 0; k0 < n; k0 += kTopnRound) {
    const int64_t k = k0 + tid;
    bool act = false;
    int64_t bits = 0;
    if (k < n) {
      const int64_t s = members[k];
      const Slots q = span_slots(P, V, s, x, 0);
      if (q.state == 1) {
        act = true;
        bits = is_int ? span_long(P, V, q, x, &err)
                      : __double_as_longlong(span_double(P, V, s, q, x, &err));
      }
    }
    const uint64_t m = __ballot(act);
    if (lane == 0) wcount[w] = __popcll(m);
    __syncthreads();
    int before = 0, total = 0;
    for (int j = 0; j < kTopnRound / 64; ++j) {
      if (j < w) before += wcount[j];
      total += wcount[j];
    }
    if (act) vec[base + before + __popcll(m & ((1ULL << lane) - 1))] = bits;
    base += total;
    __syncthreads();
  }
  for (int64_t k = base + tid; k < n; k += kTopnRound) vec[k] = 0;
  if (err) atomicOr(err_word, err);
}

// ------------------------------------------------------------------------
// k_topn_keys: one thread per slot.  The key rule (HighestMax.java:121-137)
// and the sort key: ascending order of ~key(Double.compare order) is the
// reference's descending sort, NaN (canonical, as Double.compare sees it)
// first; the radix sort is stable, so ties keep ascending slots.
// ------------------------------------------------------------------------
__global__ void k_topn_keys(int fn, int64_t S, const int64_t* __restrict__ n_dev,
                            const long long* __restrict__ marks,
                            const long long* __restrict__ maxl,
                            const unsigned long long* __restrict__ maxd,
                            uint64_t* __restrict__ sortkey,
                            int64_t* __restrict__ keybits,
                            int32_t* __restrict__ slot) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= S) return;
  slot[k] = (int32_t)k;
  if (k >= *n_dev) {  // no slot: behind every key (~key of NaN is the least)
    sortkey[k] = ~0ULL;
    keybits[k] = 0;
    return;
  }
  const bool has_l = marks[TOPN_LAST_INT] > 0, has_d = marks[TOPN_LAST_DBL] > 0;
  long long ml = 0;
  double md = 0.0;
  if (has_l) {
    ml = maxl[k];
    // the padding zeros of the integer emissions (highestMax; the vectors of
    // highestCurrent hold theirs already)
    if (fn == TOPN_HIGHEST_MAX && k >= marks[TOPN_MIN_ACT] && ml < 0) ml = 0;
  }
  if (has_d)
    md = fn == TOPN_HIGHEST_MAX ? topn_key_double(maxd[k])
                                : __longlong_as_double((long long)maxd[k]);
  double key = 0.0;
  if (has_l && has_d) key = jmax_double((double)ml, md);
  else if (has_l) key = (double)ml;
  else if (has_d) key = md;
  if (is_nan(key)) key = __longlong_as_double(kCanonNan);
  sortkey[k] = ~raw_dkey(key);
  keybits[k] = __double_as_longlong(key);
}

// what the call leaves in mapped host memory (the pattern of k_compact1's
// {error word, total}: the entry synchronises once and reads it): a header
// of TOPN_HDR words, then picked [n_out] and key [n_out]
enum : int {
  TOPN_H_ERR = 0,      // the device error word
  TOPN_H_TOTAL = 1,    // points of the picked series
  TOPN_H_NPICK = 2,    // min(topn, n)
  TOPN_H_FLAGS = 3,    // TOPN_F_*
  TOPN_H_N = 4,        // n, the numbered series
  TOPN_HDR = 8
};
enum : int {
  TOPN_F_MISS = 1,     // grid path: the promise does not hold (or a long)
  TOPN_F_EMITTED = 2   // some emission lies in the window
};

// ------------------------------------------------------------------------
// k_topn_pick: output i is the series numbered slot_sorted[i] — the slot's
// key is taken as that series' key, whatever series' values made it.  One
// thread per possible output (n_out = min(topn, S)); those past min(topn, n)
// count no points.  picked / key also go to mapped host memory.
// ------------------------------------------------------------------------
__global__ void k_topn_pick(int64_t n_out, int64_t topn,
                            const int64_t* __restrict__ n_dev,
                            const int32_t* __restrict__ slot_sorted,
                            const int64_t* __restrict__ keybits,
                            const int64_t* __restrict__ members,
                            const int64_t* __restrict__ slen,
                            int64_t* __restrict__ picked,
                            int64_t* __restrict__ pcount,
                            int64_t* __restrict__ host) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_out) return;
  const int64_t n = *n_dev, n_pick = topn < n ? topn : n;
  if (i == 0) {
    host[TOPN_H_NPICK] = n_pick;
    host[TOPN_H_N] = n;
  }
  if (i >= n_pick) {
    picked[i] = -1;
    pcount[i] = 0;
    return;
  }
  const int32_t k = slot_sorted[i];
  const int64_t s = members[k];
  picked[i] = s;
  pcount[i] = slen[s];
  host[TOPN_HDR + i] = s;
  host[TOPN_HDR + n_out + i] = keybits[k];
}

// after the offsets' scan: the error word, the total and the flags
__global__ void k_topn_done(int64_t n_out, const int64_t* __restrict__ ooff,
                            const int* __restrict__ err_word,
                            const int* __restrict__ flags,
                            const long long* __restrict__ marks,
                            int64_t* __restrict__ host) {
  if (threadIdx.x || blockIdx.x) return;
  host[TOPN_H_ERR] = *err_word;
  host[TOPN_H_TOTAL] = ooff[n_out];
  host[TOPN_H_FLAGS] =
      (flags ? *flags : 0) |
      ((marks[TOPN_LAST_INT] > 0 || marks[TOPN_LAST_DBL] > 0) ? TOPN_F_EMITTED : 0);
}

// ------------------------------------------------------------------------
// k_topn_gather: one wavefront per picked series: its whole point list,
// untouched.  Timestamps and values move in 16-byte loads and stores when the
// series starts on the same 16-byte phase in its source and in the output
// (one word peeled in front when that phase is odd), else word by word; the
// is_int bytes likewise in 16-byte pieces when both sides are aligned alike.
// ------------------------------------------------------------------------
DEV void copy_words16(const int64_t* __restrict__ a, int64_t* __restrict__ o,
                      int64_t n, int lane) {
  if ((((uintptr_t)a ^ (uintptr_t)o) & 15) != 0) {
    for (int64_t j = lane; j < n; j += 64) o[j] = a[j];
    return;
  }
  int64_t h = ((uintptr_t)a & 15) ? 1 : 0;
  if (h > n) h = n;
  if (lane == 0 && h) o[0] = a[0];
  const int64_t pairs = (n - h) >> 1;
  const longlong2* a2 = (const longlong2*)(a + h);
  longlong2* o2 = (longlong2*)(o + h);
  for (int64_t j = lane; j < pairs; j += 64) o2[j] = a2[j];
  if (lane == 0 && ((n - h) & 1)) o[n - 1] = a[n - 1];
}

DEV void copy_bytes16(const uint8_t* __restrict__ a, uint8_t* __restrict__ o,
                      int64_t n, int lane) {
  if ((((uintptr_t)a ^ (uintptr_t)o) & 15) != 0) {
    for (int64_t j = lane; j < n; j += 64) o[j] = a[j];
    return;
  }
  int64_t h = (16 - ((uintptr_t)a & 15)) & 15;
  if (h > n) h = n;
  for (int64_t j = lane; j < h; j += 64) o[j] = a[j];
  const int64_t q = (n - h) >> 4;
  const uint4* a4 = (const uint4*)(a + h);
  uint4* o4 = (uint4*)(o + h);
  for (int64_t j = lane; j < q; j += 64) o4[j] = a4[j];
  for (int64_t j = h + (q << 4) + lane; j < n; j += 64) o[j] = a[j];
}

__global__ __launch_bounds__(256) void k_topn_gather(
    int64_t n_out, const int64_t* __restrict__ picked,
    const TopnSrc* __restrict__ src, const int32_t* __restrict__ sres,
    const int64_t* __restrict__ sp0, const int64_t* __restrict__ ooff,
    int64_t cap, int64_t* __restrict__ ots, int64_t* __restrict__ oval,
    uint8_t* __restrict__ oint) {
  const int lane = LANE;
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n_out) return;
  const int64_t s = picked[i];
  if (s < 0) return;
  const TopnSrc R = src[sres[s]];
  const int64_t p0 = sp0[s], o0 = ooff[i], n = ooff[i + 1] - o0;
  if (n <= 0 || o0 + n > cap) return;
  copy_words16(R.ts + p0, ots + o0, n, lane);
  copy_words16(R.val + p0, oval + o0, n, lane);
  copy_bytes16(R.is_int + p0, oint + o0, n, lane);
}

// ========================================================================
// Grid path: every point a double, every timestamp a multiple of the
// caller's grid interval iv, NB = the window's buckets under the cap.
// Bucket b is the timestamp gbase + b * iv, gbase the first multiple of iv
// >= start; the window is b in [0, NB).  No sort, no columnar copy and no
// series x bucket matrix; the whole path is enqueued without reading
// anything back: a promise that does not hold (an off-grid timestamp, a
// long, timestamps that do not increase) raises TOPN_F_MISS, every kernel
// stays inside its arrays whatever the points hold, and the engine runs the
// general path once it has read the flag.
//
//   k_topn_grid_scan   one wavefront per numbered series over ts and is_int
//                      (9 B a point, coalesced): the promise, the emitted-
//                      bucket bitmap, the seek, the series' first and last
//                      bucket [fb, lb] inside the window (it contributes at
//                      b iff fb <= b <= lb: lb is clipped from a last point
//                      that may lie past the window), and +1 / -1 at fb /
//                      lb + 1 of its tile's row of the count table
//   k_topn_grid_last   the last emitted bucket (+ 1) into TOPN_LAST_DBL
//   k_topn_grid_tiles  per bucket: exclusive prefix over the tiles
//   k_topn_grid_rows   per tile: running sum over the buckets — the table
//                      [tiles][NB + 1] of int32 then holds, per bucket, the
//                      contributing series of all tiles before this one
//   k_topn_grid_max    highestMax: one wavefront per series streams ts and
//                      val once (16 B a point); a lane takes a point and the
//                      gap behind it: its own value at its bucket, the LERP
//                      value (span_double's expression) at every emitted
//                      bucket of the gap.  pos(k, b) = table[tile][b] + the
//                      tile's earlier series contributing at b (their fb /
//                      lb are wave-uniform loads); the key folds into slot
//                      pos with a plain read before the atomic max
//   k_topn_grid_current highestCurrent: only the last emitted bucket — one
//                      search per series, positions by ballot and LDS as in
//                      k_topn_current
// ========================================================================
constexpr int kTopnTile = 64;            // series per position tile
constexpr int64_t kTopnGridCap = 1 << 16;  // most buckets of a window

struct TopnGrid {
  int64_t gbase, iv, NB, start_ms;
};

DEV int64_t grid_bucket(const TopnGrid& Q, int64_t t) {
  return t < Q.gbase ? -1 : (t - Q.gbase) / Q.iv;
}

DEV bool grid_emitted(const unsigned long long* bitmap, int64_t b) {
  return (bitmap[b >> 6] >> (b & 63)) & 1ULL;
}

__global__ __launch_bounds__(256) void k_topn_grid_scan(
    TopnGrid Q, int64_t S, const int64_t* __restrict__ n_dev,
    const int64_t* __restrict__ members, const TopnSrc* __restrict__ src,
    const int32_t* __restrict__ sres, const int64_t* __restrict__ sp0,
    const int64_t* __restrict__ slen, unsigned long long* __restrict__ bitmap,
    int64_t* __restrict__ lo, int32_t* __restrict__ fb, int32_t* __restrict__ lb,
    int32_t* __restrict__ table, int* __restrict__ flags) {
  const int lane = LANE;
  const int64_t k = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (k >= S || k >= *n_dev) return;
  const int64_t s = members[k];
  const TopnSrc R = src[sres[s]];
  const int64_t p0 = sp0[s], n = slen[s];
  const int64_t a = lower_bound(R.ts, p0, p0 + n, Q.start_ms) - p0;  // the seek
  int bad = 0;
  for (int64_t j = lane; j < n; j += 64) {
    const int64_t t = R.ts[p0 + j];
    if (R.is_int[p0 + j] || t % Q.iv != 0 || t < 0) bad = 1;
    if (j > 0 && R.ts[p0 + j - 1] >= t) bad = 1;
    if (j >= a) {
      const int64_t b = grid_bucket(Q, t);
      // (a plain read first: after the first few series every bit is set,
      // and 20 M atomics on 32 words would serialise)
      if (b >= 0 && b < Q.NB && !grid_emitted(bitmap, b))
        atomicOr(&bitmap[b >> 6], 1ULL << (b & 63));
    }
  }
  if (__ballot(bad) && lane == 0) atomicOr(flags, TOPN_F_MISS);
  if (lane != 0) return;
  lo[k] = a;
  int64_t f = Q.NB, l = -1;  // no point after the seek: never contributes
  if (a < n) {
    f = grid_bucket(Q, R.ts[p0 + a]);
    l = grid_bucket(Q, R.ts[p0 + n - 1]);
    if (f < 0) f = 0;  // (only when the promise is broken)
    if (f > Q.NB) f = Q.NB;
    if (l >= Q.NB) l = Q.NB - 1;
  }
  fb[k] = (int32_t)f;
  lb[k] = (int32_t)l;
  if (table && f <= l) {
    int32_t* row = table + (k / kTopnTile) * (Q.NB + 1);
    atomicAdd(&row[f], 1);
    atomicAdd(&row[l + 1], -1);
  }
}

__global__ void k_topn_grid_last(int64_t words,
                                 const unsigned long long* __restrict__ bitmap,
                                 long long* __restrict__ marks) {
  const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= words) return;
  const unsigned long long m = bitmap[w];
  if (m) atomicMax(&marks[TOPN_LAST_DBL], (long long)(w * 64 + 64 - __clzll(m)));
}

__global__ void k_topn_grid_tiles(int64_t NB, int64_t tiles,
                                  int32_t* __restrict__ table) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b > NB) return;
  int32_t run = 0;
  for (int64_t t = 0; t < tiles; ++t) {
    const int32_t v = table[t * (NB + 1) + b];
    table[t * (NB + 1) + b] = run;
    run += v;
  }
}

__global__ __launch_bounds__(256) void k_topn_grid_rows(
    int64_t NB, int64_t tiles, int32_t* __restrict__ table) {
  const int lane = LANE;
  const int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= tiles) return;
  int32_t* row = table + t * (NB + 1);
  int32_t carry = 0;
  for (int64_t c0 = 0; c0 <= NB; c0 += 64) {
    const int64_t b = c0 + lane;
    int32_t v = b <= NB ? row[b] : 0;
    for (int d = 1; d < 64; d <<= 1) {
      const int32_t u = __shfl_up(v, d);
      if (lane >= d) v += u;
    }
    if (b <= NB) row[b] = v + carry;
    carry += __shfl(v, 63);
  }
}

__global__ __launch_bounds__(256) void k_topn_grid_max(
    TopnGrid Q, int64_t S, const int64_t* __restrict__ n_dev,
    const int64_t* __restrict__ members, const TopnSrc* __restrict__ src,
    const int32_t* __restrict__ sres, const int64_t* __restrict__ sp0,
    const int64_t* __restrict__ slen,
    const unsigned long long* __restrict__ bitmap,
    const int64_t* __restrict__ lo, const int32_t* __restrict__ fb,
    const int32_t* __restrict__ lb, const int32_t* __restrict__ table,
    unsigned long long* __restrict__ maxd, int* err_word) {
  // the tile's earlier series' [fb, lb], one copy per wavefront (no barrier:
  // a wavefront reads only what it wrote itself)
  __shared__ int32_t sfb[4][kTopnTile], slb[4][kTopnTile];
  const int lane = LANE, w = threadIdx.x >> 6;
  const int64_t k = (int64_t)blockIdx.x * 4 + w;
  if (k >= S || k >= *n_dev) return;
  const int32_t myf = fb[k], myl = lb[k];
  if (myf > myl) return;
  {
    const int64_t t0 = (k / kTopnTile) * kTopnTile;
    const bool in = t0 + lane < k;
    sfb[w][lane] = in ? fb[t0 + lane] : 1;
    slb[w][lane] = in ? lb[t0 + lane] : 0;
  }
  const int64_t s = members[k];
  const TopnSrc R = src[sres[s]];
  const int64_t p0 = sp0[s], n = slen[s];
  const int64_t k0 = (k / kTopnTile) * kTopnTile;
  const int kk = (int)(k - k0);
  const int32_t* row = table + (k / kTopnTile) * (Q.NB + 1);
  int err = 0;
  // the slot of this series at bucket b, and the fold into it
  auto put = [&](int64_t b, double v) {
    if (b < myf || b > myl) return;  // (only when the promise is broken)
    int64_t pos = row[b];
    for (int j = 0; j < kk; ++j) pos += (sfb[w][j] <= b && b <= slb[w][j]) ? 1 : 0;
    const unsigned long long key = topn_dkey(v);
    if (key > maxd[pos]) atomicMax(&maxd[pos], key);
  };
  for (int64_t j = lo[k] + lane; j < n; j += 64) {
    const int64_t x0 = R.ts[p0 + j];
    const int64_t b0 = grid_bucket(Q, x0);
    if (b0 < 0 || b0 >= Q.NB) continue;
    const double y0 = __longlong_as_double(R.val[p0 + j]);
    put(b0, y0);
    if (j + 1 >= n) continue;
    const int64_t x1 = R.ts[p0 + j + 1];
    int64_t b1 = grid_bucket(Q, x1);
    if (b1 > Q.NB) b1 = Q.NB;
    if (b1 <= b0 + 1) continue;
    const double y1 = __longlong_as_double(R.val[p0 + j + 1]);
    for (int64_t b = b0 + 1; b < b1; ++b) {
      if (!grid_emitted(bitmap, b)) continue;
      const int64_t x = Q.gbase + b * Q.iv;
      if (x1 & kMsMask) err |= ERR_X1_MASK;
      put(b, y0 + (double)jsub(x, x0) * (y1 - y0) / (double)jsub(x1, x0));
    }
  }
  if (err) atomicOr(err_word, err);
}

__global__ __launch_bounds__(kTopnRound) void k_topn_grid_current(
    TopnGrid Q, const int64_t* __restrict__ n_dev,
    const int64_t* __restrict__ members, const TopnSrc* __restrict__ src,
    const int32_t* __restrict__ sres, const int64_t* __restrict__ sp0,
    const int64_t* __restrict__ slen, const int64_t* __restrict__ lo,
    const int32_t* __restrict__ fb, const int32_t* __restrict__ lb,
    const long long* __restrict__ marks, int64_t* __restrict__ vecd,
    int* err_word) {
  __shared__ int wcount[kTopnRound / 64];
  const int64_t n = *n_dev;
  const int64_t bL = marks[TOPN_LAST_DBL] - 1;
  if (bL < 0) return;
  const int64_t x = Q.gbase + bL * Q.iv;
  const int tid = threadIdx.x, lane = LANE, w = tid >> 6;
  int err = 0;
  int64_t base = 0;
  for (int64_t k0 = 0; k0 < n; k0 += kTopnRound) {
    const int64_t k = k0 + tid;
    bool act = false;
    int64_t bits = 0;
    if (k < n && fb[k] <= bL && bL <= lb[k]) {
      const int64_t s = members[k];
      const TopnSrc R = src[sres[s]];
      const int64_t p0 = sp0[s], a = p0 + lo[k], e = p0 + slen[s];
      const int64_t c = last_le(R.ts, a, e, x);
      if (c >= a) {  // (always, when the promise holds)
        act = true;
        const int64_t x0 = R.ts[c];
        const double y0 = __longlong_as_double(R.val[c]);
        double v = y0;
        if (x0 != x && c + 1 < e) {
          const int64_t x1 = R.ts[c + 1];
          const double y1 = __longlong_as_double(R.val[c + 1]);
          if (x1 & kMsMask) err |= ERR_X1_MASK;
          v = x == x1 ? y1
                      : y0 + (double)jsub(x, x0) * (y1 - y0) / (double)jsub(x1, x0);
        }
        bits = __double_as_longlong(v);
      }
    }
    const uint64_t m = __ballot(act);
    if (lane == 0) wcount[w] = __popcll(m);
    __syncthreads();
    int before = 0, total = 0;
    for (int j = 0; j < kTopnRound / 64; ++j) {
      if (j < w) before += wcount[j];
      total += wcount[j];
    }
    if (act) vecd[base + before + __popcll(m & ((1ULL << lane) - 1))] = bits;
    base += total;
    __syncthreads();
  }
  for (int64_t k = base + tid; k < n; k += kTopnRound) vecd[k] = 0;
  if (err) atomicOr(err_word, err);
}

}  // namespace otsdb
