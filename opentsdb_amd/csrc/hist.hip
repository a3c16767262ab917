// hist.hip — histogram queries (otsdb_hist_*): the members'
// histogram points are downsampled and summed across each group on the GPU,
// the percentiles read off the sums.  gfx950, wave64, integer arithmetic only
// up to the percentile's `area`.  (Included by engine_hist.hip after kernels.hip
// and compact.hip: Params, bucket_of, bucket_ts, lower_bound_interp,
// compact_count, LANE.)
//
// Reference: HistogramSpanGroup.add (HistogramSpanGroup.java:160-204),
// HistogramDownsampler / ValuesInInterval (HistogramDownsampler.java:129-149,
// :195-377), HistogramAggregationIterator.next (:240-287),
// SimpleHistogram.aggregate / percentile (SimpleHistogram.java:124-164,
// :246-261).
//
//   k_hist_prep         per series: the SpanGroup filter, the points of
//                       [seek_ts, stop_ts)
//   k_hist_fold         per (tile of <= 64 members, window of W buckets): a
//                       wavefront streams a member's records (two bins a
//                       lane), sums a bucket in registers and adds it into the
//                       window's LDS rows when the bucket changes
//   k_hist_combine      groups of several tiles: the sum of their partials
//   k_hist_percentiles  per emitted (group, bucket): every percentile from
//                       one read of the row
//   k_hist_count / k_scan / k_hist_scatter   dense -> per-group arrays
#pragma once
#include "histplan.h"

namespace otsdb {

constexpr int HIST_THREADS = 256;
constexpr int HIST_INFLIGHT = 4;  // records a wavefront has in flight

typedef unsigned long long hu64;

struct HistPct {
  double p[kHistMaxPct];  // the float percentiles, widened
};

// ------------------------------------------------------------------------
// k_hist_prep: one thread per series.  keep as HistogramSpanGroup.add; the
// downsampler's seek (the first point >= seek_ts) and the first point of the
// first bucket past end_ms (stop_ts): a bucket is read to its end.
// ------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_hist_prep(
    Params P, int64_t S, const int64_t* __restrict__ offsets,
    const int64_t* __restrict__ ts, int64_t* __restrict__ lo,
    int64_t* __restrict__ hi) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  const int64_t p0 = offsets[s], p1 = offsets[s + 1];
  const bool keep = p1 > p0 && ts[p0] <= P.end_ms && ts[p1 - 1] >= P.start_ms;
  int64_t l = p1, h = p1;
  if (keep) {
    l = lower_bound_interp(ts, p0, p1, P.seek_ts);
    h = lower_bound_interp(ts, l, p1, P.stop_ts);
  }
  lo[s] = l;
  hi[s] = h;
}

// ------------------------------------------------------------------------
// k_hist_fold.  Dynamic LDS: header (the member queue) | state u64
// [nw][pitch] | emit u32 [nw].  Lane l of pass p owns bins 128 p + 2 l and
// + 1, so the lanes of one add never share an address: only wavefronts
// closing the same bucket meet on a row, and integer adds commute — the sums
// are the same bits in any order.
// NP: wave passes over a row (ceil((K + 2) / 128)); VEC: 16-byte loads (an
// even row length on a 16-byte aligned matrix), else two 8-byte loads a lane.
// first_only: the downsampling function is not `sum` — the bucket keeps its
// first histogram alone (aggregate(x, null) does nothing).
// ------------------------------------------------------------------------
template <int NP, bool VEC>
__global__ __launch_bounds__(HIST_THREADS) void k_hist_fold(
    Params P, const int64_t* __restrict__ ts,
    const int64_t* __restrict__ counts, int R, int W, int first_only,
    const int64_t* __restrict__ lo, const int64_t* __restrict__ hi,
    int64_t n_tiles, const int64_t* __restrict__ tile_g,
    const int64_t* __restrict__ tile_m0, const int64_t* __restrict__ tile_m1,
    const int64_t* __restrict__ tile_slot,
    const int64_t* __restrict__ members, int64_t* __restrict__ dense,
    uint8_t* __restrict__ emit, int64_t* __restrict__ partial,
    uint8_t* __restrict__ part_emit) {
  extern __shared__ __attribute__((aligned(16))) unsigned char hist_dyn[];
  const int tid = threadIdx.x, lane = LANE;
  const int pitch = (R + 1) & ~1;
  const int64_t nb = P.nb;
  const int64_t t = (int64_t)blockIdx.x % n_tiles;
  const int64_t win = (int64_t)blockIdx.x / n_tiles;
  const int64_t W0 = win * W;
  const int64_t W1 = W0 + W < nb ? W0 + W : nb;
  const int nw = (int)(W1 - W0);
  int* s_next = reinterpret_cast<int*>(hist_dyn);
  hu64* st = reinterpret_cast<hu64*>(hist_dyn + kHistLdsHeader);
  uint32_t* em = reinterpret_cast<uint32_t*>(st + (size_t)nw * pitch);
  for (int i = tid; i < nw * pitch; i += HIST_THREADS) st[i] = 0;
  for (int i = tid; i < nw; i += HIST_THREADS) em[i] = 0;
  if (tid == 0) *s_next = 0;
  __syncthreads();
  const int64_t m0 = tile_m0[t], m1 = tile_m1[t];
  for (;;) {
    // every lane takes part in the claim (lane 0 adds 1, the others 0) and
    // the wavefront takes lane 0's ticket: no branch on the lane id, so the
    // ticket and the loop's exit are wave-uniform
    int i = atomicAdd(s_next, lane == 0 ? 1 : 0);
    i = __builtin_amdgcn_readfirstlane(i);
    if (m0 + i >= m1) break;
    const int64_t s = members[m0 + i];
    int64_t pa = lo[s], pb = hi[s];
    // the member's points inside this window
    if (win > 0) pa = lower_bound_interp(ts, pa, pb, P.gbase + W0 * P.interval);
    if (W1 < nb) pb = lower_bound_interp(ts, pa, pb, P.gbase + W1 * P.interval);
    hu64 acc[NP][2];
#pragma unroll
    for (int p = 0; p < NP; ++p) acc[p][0] = acc[p][1] = 0;
    int cur = -1;
    bool taken = false;
    auto flush = [&]() {
      if (cur < 0) return;
      hu64* row = st + (size_t)cur * pitch;
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        const int bin = 128 * p + 2 * lane;
        if (bin < R && acc[p][0]) atomicAdd(&row[bin], acc[p][0]);
        if (bin + 1 < R && acc[p][1]) atomicAdd(&row[bin + 1], acc[p][1]);
        acc[p][0] = acc[p][1] = 0;
      }
      if (lane == 0) em[cur] = 1;
    };
    for (int64_t q = pa; q < pb; q += HIST_INFLIGHT) {
      hu64 v[HIST_INFLIGHT][NP][2];
      int64_t tq[HIST_INFLIGHT];
#pragma unroll
      for (int u = 0; u < HIST_INFLIGHT; ++u) {
        const bool in = q + u < pb;  // wave-uniform
        tq[u] = in ? ts[q + u] : 0;
        const int64_t* rec = counts + (q + u) * (int64_t)R;
#pragma unroll
        for (int p = 0; p < NP; ++p) {
          const int bin = 128 * p + 2 * lane;
          v[u][p][0] = v[u][p][1] = 0;
          if (VEC) {
            if (in && bin < R) {  // R even: bin + 1 < R too
              const ll2_t x = *reinterpret_cast<const ll2_t*>(rec + bin);
              v[u][p][0] = (hu64)x.x;
              v[u][p][1] = (hu64)x.y;
            }
          } else {
            if (in && bin < R) v[u][p][0] = (hu64)rec[bin];
            if (in && bin + 1 < R) v[u][p][1] = (hu64)rec[bin + 1];
          }
        }
      }
#pragma unroll
      for (int u = 0; u < HIST_INFLIGHT; ++u) {
        if (q + u >= pb) break;
        const int64_t bq = bucket_of(P, tq[u]) - W0;
        if (bq < 0 || bq >= nw) continue;  // (never: pa / pb bound the window)
        const int b = (int)bq;
        if (b != cur) {
          flush();
          cur = b;
          taken = false;
        }
        if (!first_only || !taken) {
#pragma unroll
          for (int p = 0; p < NP; ++p) {
            acc[p][0] += v[u][p][0];
            acc[p][1] += v[u][p][1];
          }
        }
        taken = true;
      }
    }
    flush();
  }
  __syncthreads();
  // a tile that is its whole group: straight into the dense arrays; the
  // tiles of a larger group leave partials for k_hist_combine
  const int64_t slot = tile_slot[t];
  int64_t* dst = slot < 0 ? dense + (tile_g[t] * nb + W0) * R
                          : partial + (slot * nb + W0) * R;
  uint8_t* de = slot < 0 ? emit + tile_g[t] * nb + W0 : part_emit + slot * nb + W0;
  if ((R & 1) == 0 && (((uintptr_t)dst) & 15) == 0) {
    // an even row length: pitch == R, the window's rows are one contiguous
    // run in LDS and in the destination — plain 16-byte copies
    const ll2_t* src2 = reinterpret_cast<const ll2_t*>(st);
    ll2_t* dst2 = reinterpret_cast<ll2_t*>(dst);
    for (int e = tid; e < nw * (R >> 1); e += HIST_THREADS) dst2[e] = src2[e];
  } else {
    for (int e = tid; e < nw * R; e += HIST_THREADS) {
      const int b = e / R, r = e - b * R;
      dst[e] = (int64_t)st[(size_t)b * pitch + r];
    }
  }
  for (int b = tid; b < nw; b += HIST_THREADS) de[b] = (uint8_t)em[b];
}

// ------------------------------------------------------------------------
// k_hist_combine: a group of several tiles is the sum of their partials
// (slots [s0, s1) of the partial array, the tiles in member order), one
// thread per (bucket, bin).  No atomics: each dense cell has one writer.
// ------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_hist_combine(
    int64_t nb, int R, const int64_t* __restrict__ mg_g,
    const int64_t* __restrict__ mg_s0, const int64_t* __restrict__ mg_s1,
    const int64_t* __restrict__ partial, const uint8_t* __restrict__ part_emit,
    int64_t* __restrict__ dense, uint8_t* __restrict__ emit) {
  const int64_t k = blockIdx.y;
  const int64_t g = mg_g[k], s0 = mg_s0[k], s1 = mg_s1[k];
  const int64_t row = nb * R;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= row) return;
  hu64 sum = 0;
  for (int64_t s = s0; s < s1; ++s) sum += (hu64)partial[s * row + e];
  dense[g * row + e] = (int64_t)sum;
  if (e < nb) {
    uint8_t any = 0;
    for (int64_t s = s0; s < s1; ++s) any |= part_emit[s * nb + e];
    emit[g * nb + e] = any;
  }
}

// ------------------------------------------------------------------------
// k_hist_percentiles: SimpleHistogram.percentile for every percentile of the
// call from one read of the K regular counts.  One wavefront per emitted
// (group, bucket); lane l holds the C = ceil(K / 64) consecutive bins from
// l C on, so key order is (lane, j) order.
//   int bucketSum   = the wrapping sum of the counts' intValue()
//   long running   += intValue(), area = running * 100.0 / bucketSum in
//                     separate double operations
//   the first key with area >= p gives (double)((lower + upper) / 2), float
// ------------------------------------------------------------------------
template <int C>
__global__ __launch_bounds__(256) void k_hist_percentiles(
    int64_t n_cells, int R, int K, const int64_t* __restrict__ dense,
    const uint8_t* __restrict__ emit, const float* __restrict__ lower,
    const float* __restrict__ upper, HistPct pct, int n_pct,
    double* __restrict__ dense_pct) {
  const int lane = LANE;
  const int64_t cell = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (cell >= n_cells || !emit[cell]) return;
  const int64_t* row = dense + cell * R;
  int64_t run[C];
  uint32_t isum = 0;
  int64_t r = 0;
#pragma unroll
  for (int j = 0; j < C; ++j) {
    const int bin = lane * C + j;
    const int32_t iv = bin < K ? (int32_t)(uint64_t)row[bin] : 0;  // intValue()
    isum += (uint32_t)iv;
    r += (int64_t)iv;
    run[j] = r;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) isum += (uint32_t)__shfl_xor((int)isum, d);
  int64_t incl = r;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int64_t y = __shfl_up(incl, d);
    if (lane >= d) incl += y;
  }
  const int64_t excl = incl - r;
  const double bs = (double)(int32_t)isum;
  double area[C];
#pragma unroll
  for (int j = 0; j < C; ++j) {
    const double x = (double)(run[j] + excl) * 100.0;
    area[j] = x / bs;
  }
  for (int q = 0; q < n_pct; ++q) {
    const double p = pct.p[q];
    double res;
    if (p < 1.0 || p > 100.0) {
      res = -1.0;
    } else {
      int fj = C;
#pragma unroll
      for (int j = C - 1; j >= 0; --j)
        if (lane * C + j < K && area[j] >= p) fj = j;
      const uint64_t m = __ballot(fj < C);
      res = 0.0;
      if (m) {
        const int src = __builtin_ctzll(m);
        double mid = 0.0;
        if (fj < C) {
          const int bin = lane * C + fj;
          const float h = (lower[bin] + upper[bin]) / 2.0f;
          mid = (double)h;
        }
        res = __shfl(mid, src);
      }
    }
    if (lane == 0) dense_pct[(int64_t)q * n_cells + cell] = res;
  }
}

// ------------------------------------------------------------------------
// Compaction: emit flags -> offsets (k_hist_count, then k_scan), then one
// scatter of the timestamps, every percentile and the merged rows.  One
// wavefront per group.
// ------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_hist_count(
    int64_t G, int64_t nb, const uint8_t* __restrict__ emit,
    int64_t* __restrict__ cnt) {
  const int64_t g = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (g >= G) return;
  const int64_t n = compact_count(emit + g * nb, nb, LANE);
  if (LANE == 0) cnt[g] = n;
}

__global__ __launch_bounds__(256) void k_hist_scatter(
    Params P, int64_t G, int R, int n_pct, const uint8_t* __restrict__ emit,
    const int64_t* __restrict__ offsets, int64_t cap,
    const int64_t* __restrict__ dense, const double* __restrict__ dense_pct,
    int64_t* __restrict__ r_ts, double* __restrict__ r_pct,
    int64_t* __restrict__ r_counts) {
  const int lane = LANE;
  const int64_t g = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (g >= G) return;
  const int64_t nb = P.nb, n_cells = G * nb;
  int64_t pos = offsets[g];
  for (int64_t c0 = 0; c0 < nb; c0 += 64) {
    const int64_t b = c0 + lane;
    const bool e = b < nb && emit[g * nb + b];
    const uint64_t m = __ballot(e);
    if (e) {
      const int64_t p = pos + __popcll(m & ((1ULL << lane) - 1));
      if (p < cap) {
        r_ts[p] = bucket_ts(P, b);
        for (int q = 0; q < n_pct; ++q)
          r_pct[(int64_t)q * cap + p] = dense_pct[(int64_t)q * n_cells + g * nb + b];
      }
    }
    if (r_counts) {  // the merged rows: the wavefront copies one at a time
      uint64_t mm = m;
      int64_t p = pos;
      while (mm) {
        const int l = __builtin_ctzll(mm);
        mm &= mm - 1;
        if (p < cap) {
          const int64_t* src = dense + (g * nb + c0 + l) * R;
          for (int r = lane; r < R; r += 64) r_counts[p * R + r] = src[r];
        }
        ++p;
      }
    }
    pos += __popcll(m);
  }
}

}  // namespace otsdb
