// hist_rows.hip — the scanner's storage rows -> histogram points (ts_ms and
// the dense [N][K + 2] count matrix of otsdb_hist_columns), DESIGN.md §4.4.1.
// gfx950, wave64.  (Included by engine_hist.hip after hist.hip: LANE, ll2_t,
// kHistMaxRow.)
//
// What the reference does with the rows, restated:
//   * a histogram cell is a column whose qualifier has odd length and starts
//     with 0x06, HistogramDataPoint.PREFIX (CompactionQueue.java:441-452,
//     SaltScanner.java:788-795); every other column is not looked at here;
//   * Internal.decodeHistogramDataPoint (Internal.java:1095-1104): value[0]
//     picks the codec, Internal.getTimeStampFromNonDP (:1059-1074) gives the
//     timestamp — a 3-byte qualifier (base_s + (signed q[1] << 8 | q[2])) *
//     1000, a 5-byte one base_s * 1000 + int32(q[1..4]), any other length
//     throws — and SimpleHistogram.fromHistogram (SimpleHistogram.java:97-122)
//     reads the id byte, a big-endian short bucketCount, bucketCount times
//     {float lower, float upper, var-long count} and the var-long underflow
//     and overflow; a value under 6 bytes throws, trailing bytes are ignored,
//     a repeated key keeps the later count (TreeMap.put), keys are equal when
//     Float.compare is 0 on both bounds;
//   * the var-long is Kryo 3.0.0's Output.writeLong(v, true): 7 value bits a
//     byte, least significant group first, bit 7 "another byte follows", the
//     ninth byte whole; reading past the value's end throws;
//   * a cell that throws is logged and skipped (the catch (Throwable) at
//     SaltScanner.java:793 / CompactionQueue.java:450); a row left without a
//     point is no row;
//   * HistogramSpan.addRow (HistogramSpan.java:280-328) and
//     HistogramRowSeq.addRow (HistogramRowSeq.java:66-105): a row whose key
//     is in the span already and whose first timestamp is <= the span's last
//     is merged with two pointers, an equal timestamp keeping the earlier
//     row's point.
// Refused here (E_UNSUPPORTED, engine_hist.hip): a cell of another codec, a
// bucketCount above 254, timestamps that do not strictly increase along a
// row's surviving cells, base times that decrease inside a series, more than
// 64 consecutive rows of one key, an assembled series out of order.
//
// Kernels:
//   k_hr_cells   a thread per column: histogram cell or not, its timestamp,
//                the checks that need no walk (length, id, bucketCount);
//   k_hr_walk    a wavefront per histogram cell: the value staged in LDS, the
//                entry chain resolved from one ballot per 64-byte window with
//                wave-uniform arithmetic, then a lane per entry.  MODE 0:
//                validity and the keys into a global set (schema discovery);
//                MODE 1: validity and every key looked up in the schema;
//                MODE 2: the record written at its assembled index;
//   k_hr_rows    a thread per row: order checks, survivors, run heads, the
//                ranks of a run of one row;
//   k_hr_merge   a thread per run of several rows: the merge, ranks, drops;
//   k_hr_series  a thread per series: the assembled timestamps increase.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace otsdb {

constexpr int kHrMaxEntries = kHistMaxRow - 2;             // 254 keys a blob
constexpr int kHrMaxValue = 3 + kHrMaxEntries * 17 + 18;   // 4,339 bytes read
// the staged image: the value from the 16-byte line it starts in
constexpr int kHrImage = (kHrMaxValue + 15 + 15) & ~15;
constexpr int kHrWaves = 4;      // wavefronts (cells) of one workgroup
constexpr int kHrRunRows = 64;   // consecutive rows of one key
constexpr int kHrSetSlots = 1024;  // schema discovery's key set
constexpr unsigned long long kHrEmpty = ~0ULL;  // (no key: 0x7FFFFFFF is a
                                                // NaN that is never canonical)

// a column's state
enum : int { HR_NONE = 0, HR_SKIP = 1, HR_ALIVE = 2, HR_ERR = 3 };
// status codes of a failing cell or row (otsdb_status values)
enum : int { HR_ILLEGAL_ARGUMENT = 3, HR_UNSUPPORTED = 5 };
// words of HistRowsDev::small
enum : int { HR_W_ERR = 0, HR_W_ERR2 = 1, HR_W_DECODED = 2, HR_W_SKIPPED = 3,
             HR_W_DROPPED = 4, HR_W_KEYS = 5, HR_W_FULL = 6, HR_W_TOTAL = 7 };

struct HistRowsDev {
  int64_t R, C, S;
  const int64_t* row_series;
  const int64_t* row_base_s;
  const int64_t* row_col_off;  // [R+1]
  const int64_t* col_qoff;     // [C+1]
  const uint8_t* qual;
  const int64_t* col_voff;     // [C+1]
  const uint8_t* val;
  int32_t codec;               // SimpleHistogramDecoder's id
  int32_t K;                   // keys of the schema (MODE 1, 2)
  const unsigned long long* schema;  // [K] ordered keys, ascending
  // per column
  int64_t* rec_ts;
  int32_t* rec_state;
  int32_t* rec_rank;  // rank among its run's points, -1: dropped by a merge
  int32_t* rec_row;
  // per row ([R+1]); first / last / cnt are a run's, at its head row
  int64_t* row_cnt;
  int64_t* row_out;
  int64_t* row_head;
  int64_t* row_first;
  int64_t* row_last;
  unsigned long long* small;  // [8], HR_W_*
  unsigned long long* set;    // [kHrSetSlots]
};

// The first failure in row order, then in column order: cell c sits at
// 2 c + 1, a failure of row r as a whole before its first cell.
DEV void hr_error(const HistRowsDev& T, int word, int64_t pos, int code) {
  atomicMin(&T.small[word], ((unsigned long long)pos << 8) | (unsigned)code);
}
DEV int64_t hr_cell_pos(int64_t c) { return 2 * c + 1; }
DEV int64_t hr_row_pos(const HistRowsDev& T, int64_t r) {
  return 2 * T.row_col_off[r];
}

// Float.compare's order as unsigned order, NaN canonical (floatToIntBits)
DEV uint32_t hr_ord(uint32_t bits) {
  if ((bits & 0x7FFFFFFFu) > 0x7F800000u) bits = 0x7FC00000u;
  return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
}

DEV uint32_t hr_be32(const uint8_t* p) {
  return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) |
         ((uint32_t)p[2] << 8) | (uint32_t)p[3];
}

// Input.readLong(true) of a var-long the walk found whole
DEV unsigned long long hr_varlong(const uint8_t* b) {
  unsigned long long x = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const unsigned y = b[i];
    x |= (unsigned long long)(y & 0x7F) << (7 * i);
    if (!(y & 0x80)) return x;
  }
  return x | ((unsigned long long)b[8] << 56);
}

// ------------------------------------------------------------------------
// k_hr_cells: one thread per column.
// ------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_hr_cells(HistRowsDev T) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= T.C) return;
  // the column's row: the last one that starts at or before it
  int64_t lo = 0, hi = T.R - 1;
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if (T.row_col_off[mid] <= c) lo = mid;
    else hi = mid - 1;
  }
  const int64_t q0 = T.col_qoff[c], qlen = T.col_qoff[c + 1] - q0;
  const int64_t v0 = T.col_voff[c], vlen = T.col_voff[c + 1] - v0;
  int state = HR_NONE;
  int64_t ts = 0;
  if (qlen >= 1 && (qlen & 1) && T.qual[q0] == 0x06) {
    const uint8_t* q = T.qual + q0;
    const uint8_t* v = T.val + v0;
    const int64_t base = T.row_base_s[lo];
    if (vlen < 1) {
      state = HR_SKIP;  // value[0]: ArrayIndexOutOfBounds
    } else if (qlen != 3 && qlen != 5) {
      state = HR_SKIP;  // getTimeStampFromNonDP throws
    } else if (v[0] != (uint8_t)T.codec) {
      state = HR_ERR;
      hr_error(T, HR_W_ERR, hr_cell_pos(c), HR_UNSUPPORTED);
    } else if (vlen < 6) {
      state = HR_SKIP;  // "Byte array shorter than 6 bytes"
    } else if ((int16_t)((v[1] << 8) | v[2]) > kHrMaxEntries) {
      state = HR_ERR;
      hr_error(T, HR_W_ERR, hr_cell_pos(c), HR_UNSUPPORTED);
    } else {
      state = HR_ALIVE;
    }
    if (qlen == 3)
      ts = (base + (int32_t)(((int32_t)(int8_t)q[1] << 8) | q[2])) * 1000;
    else if (qlen == 5)
      ts = base * 1000 + (int32_t)hr_be32(q + 1);
  }
  T.rec_ts[c] = ts;
  T.rec_state[c] = state;
  T.rec_rank[c] = -1;
  T.rec_row[c] = (int32_t)lo;
}

// schema discovery: the key into the open-addressed set (read first, a CAS
// only on an empty slot); a full set raises HR_W_FULL
DEV void hr_set_insert(const HistRowsDev& T, unsigned long long key) {
  if (__atomic_load_n(&T.small[HR_W_FULL], __ATOMIC_RELAXED)) return;
  const uint32_t h = (uint32_t)((key * 0x9E3779B97F4A7C15ULL) >> 54);
  for (int i = 0; i < kHrSetSlots; ++i) {
    unsigned long long* slot = &T.set[(h + i) & (kHrSetSlots - 1)];
    const unsigned long long cur = __atomic_load_n(slot, __ATOMIC_RELAXED);
    if (cur == key) return;
    if (cur != kHrEmpty) continue;
    const unsigned long long old = atomicCAS(slot, kHrEmpty, key);
    if (old == kHrEmpty) {
      atomicAdd(&T.small[HR_W_KEYS], 1ULL);
      return;
    }
    if (old == key) return;
  }
  atomicMax(&T.small[HR_W_FULL], 1ULL);
}

// ------------------------------------------------------------------------
// k_hr_walk.  Static LDS, per wavefront: the value's image (16-byte lines of
// the value pool, so the loads are aligned), the entry starts, and in MODE 2
// the record and each column's last entry.  The wavefronts of a workgroup
// share only the schema, loaded before any of them leaves.
// ------------------------------------------------------------------------
template <int MODE>
__global__ __launch_bounds__(64 * kHrWaves) void k_hr_walk(
    HistRowsDev T, int64_t* __restrict__ ts_out, int64_t* __restrict__ counts,
    int64_t cap) {
  constexpr int W2 = MODE == 2 ? kHrWaves : 1;
  __shared__ __attribute__((aligned(16))) uint8_t s_img[kHrWaves][kHrImage];
  __shared__ __attribute__((aligned(16))) unsigned long long
      s_row[W2][MODE == 2 ? kHistMaxRow : 2];
  __shared__ unsigned long long s_schema[MODE == 0 ? 2 : kHrMaxEntries];
  __shared__ int s_owner[W2][MODE == 2 ? kHrMaxEntries : 1];
  __shared__ uint16_t s_start[kHrWaves][kHrMaxEntries + 2];
  const int tid = threadIdx.x, lane = LANE;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int K = T.K;
  if (MODE != 0) {
    for (int i = tid; i < K; i += 64 * kHrWaves) s_schema[i] = T.schema[i];
    __syncthreads();
  }
  const int64_t c = (int64_t)blockIdx.x * kHrWaves + wv;
  if (c >= T.C) return;
  if (T.rec_state[c] != HR_ALIVE) return;
  int64_t rec = 0;
  if (MODE == 2) {
    const int rank = T.rec_rank[c];
    if (rank < 0) return;
    rec = T.row_out[T.row_head[T.rec_row[c]]] + rank;
    if (rec >= cap) return;
  }
  // ---- stage the value
  const int64_t v0 = T.col_voff[c];
  const int64_t vlen = T.col_voff[c + 1] - v0;
  const int len = __builtin_amdgcn_readfirstlane(
      (int)(vlen < kHrMaxValue ? vlen : kHrMaxValue));
  const uint8_t* src = T.val + v0;
  const int d = __builtin_amdgcn_readfirstlane((int)((uintptr_t)src & 15));
  uint8_t* img = s_img[wv];
  const int nch = (d + len + 15) >> 4;
  for (int k = lane; k < nch; k += 64) {
    const int a = k * 16 - d;  // the line's first byte, as a value offset
    if (a >= 0 && a + 16 <= len) {
      *reinterpret_cast<uint4*>(img + k * 16) =
          *reinterpret_cast<const uint4*>(src + a);
    } else {
      for (int j = 0; j < 16; ++j) {
        const int p = a + j;
        img[k * 16 + j] = (p >= 0 && p < len) ? src[p] : (uint8_t)0;
      }
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  const uint8_t* v = img + d;
  int n = __builtin_amdgcn_readfirstlane((int)(int16_t)((v[1] << 8) | v[2]));
  if (n < 0) n = 0;
  if (n > kHrMaxEntries) return;  // (never: k_hr_cells refused it)

  // ---- the chain: entry e starts at p, its count at p + 8; every quantity
  // below is wave-uniform (ballots, len, n)
  auto mask_of = [&](int win) -> unsigned long long {
    const int i = win * 64 + lane;
    const int b = i < len ? v[i] : 0;
    return __ballot((b & 0x80) != 0);
  };
  int w = -2;
  unsigned long long mc = 0, mn = 0;
  int p = 3;
  bool ok = true;
  for (int e = 0; e < n + 2; ++e) {
    const int q = e < n ? p + 8 : p;
    const int win = q >> 6;
    if (win != w) {
      mc = win == w + 1 ? mn : mask_of(win);
      mn = mask_of(win + 1);
      w = win;
    }
    const int l = q & 63;
    unsigned long long bits = mc >> l;
    if (l) bits |= mn << (64 - l);
    const unsigned long long nb = ~bits;
    const int run = nb ? __builtin_ctzll(nb) : 64;
    if (lane == 0) s_start[wv][e] = (uint16_t)p;
    p = q + (run + 1 < 9 ? run + 1 : 9);
    if (p > len) {  // Kryo: buffer underflow
      ok = false;
      break;
    }
  }
  if (!ok) {
    if (MODE != 2 && lane == 0) T.rec_state[c] = HR_SKIP;
    return;
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();

  // ---- a lane per entry
  if (MODE == 2) {
    for (int i = lane; i < K + 2; i += 64) s_row[wv][i] = 0;
    for (int i = lane; i < K; i += 64) s_owner[wv][i] = -1;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
  constexpr int NP = (kHrMaxEntries + 63) / 64;
  int col_[NP];
  unsigned long long cnt_[NP];
  bool bad = false;
#pragma unroll
  for (int k = 0; k < NP; ++k) {
    const int e = k * 64 + lane;
    col_[k] = -1;
    cnt_[k] = 0;
    if (e >= n) continue;
    const uint8_t* b = v + s_start[wv][e];
    const unsigned long long key =
        ((unsigned long long)hr_ord(hr_be32(b)) << 32) | hr_ord(hr_be32(b + 4));
    if (MODE == 0) {
      hr_set_insert(T, key);
      continue;
    }
    // blobs usually carry the whole schema in order: position e first
    int col = -1;
    if (e < K && s_schema[e] == key) {
      col = e;
    } else {
      int a = 0, z = K;
      while (a < z) {
        const int m = (a + z) >> 1;
        if (s_schema[m] < key) a = m + 1;
        else z = m;
      }
      if (a < K && s_schema[a] == key) col = a;
    }
    if (col < 0) bad = true;
    col_[k] = col;
    if (MODE == 2 && col >= 0) {
      cnt_[k] = hr_varlong(b + 8);
      atomicMax(&s_owner[wv][col], e);  // a repeated key: the later entry
    }
  }
  if (MODE == 1) {
    if (__ballot(bad) && lane == 0)
      hr_error(T, HR_W_ERR, hr_cell_pos(c), HR_ILLEGAL_ARGUMENT);
  }
  if (MODE == 2) {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int k = 0; k < NP; ++k) {
      const int e = k * 64 + lane;
      if (col_[k] >= 0 && s_owner[wv][col_[k]] == e)
        s_row[wv][col_[k]] = cnt_[k];
    }
    if (lane < 2) s_row[wv][K + lane] = hr_varlong(v + s_start[wv][n + lane]);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const int R = K + 2;
    int64_t* dst = counts + rec * (int64_t)R;
    if ((R & 1) == 0 && (((uintptr_t)dst) & 15) == 0) {
      const ll2_t* s2 = reinterpret_cast<const ll2_t*>(s_row[wv]);
      ll2_t* d2 = reinterpret_cast<ll2_t*>(dst);
      for (int i = lane; i < (R >> 1); i += 64) d2[i] = s2[i];
    } else {
      for (int i = lane; i < R; i += 64) dst[i] = (int64_t)s_row[wv][i];
    }
    if (lane == 0) ts_out[rec] = T.rec_ts[c];
  }
}

// a row's columns, kept inside the column arrays whatever the offsets say
DEV int64_t hr_col0(const HistRowsDev& T, int64_t r) {
  const int64_t a = T.row_col_off[r];
  return a < 0 ? 0 : (a > T.C ? T.C : a);
}
DEV int64_t hr_col1(const HistRowsDev& T, int64_t r) {
  const int64_t e = T.row_col_off[r + 1];
  return e < 0 ? 0 : (e > T.C ? T.C : e);
}

DEV bool hr_same_key(const HistRowsDev& T, int64_t a, int64_t b) {
  return T.row_series[a] == T.row_series[b] &&
         T.row_base_s[a] == T.row_base_s[b];
}

// ------------------------------------------------------------------------
// k_hr_rows: one thread per row, after the scan walk.
// ------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_hr_rows(HistRowsDev T) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= T.R) return;
  const int64_t s = T.row_series[r];
  if (s < 0 || s >= T.S || (r > 0 && T.row_series[r - 1] > s))
    hr_error(T, HR_W_ERR, hr_row_pos(T, r), HR_ILLEGAL_ARGUMENT);
  if (r > 0 && T.row_series[r - 1] == s && T.row_base_s[r] < T.row_base_s[r - 1])
    hr_error(T, HR_W_ERR, hr_row_pos(T, r), HR_UNSUPPORTED);
  int d = 0;
  while (d < kHrRunRows && r - d - 1 >= 0 && hr_same_key(T, r - d - 1, r)) ++d;
  if (d >= kHrRunRows)  // the 65th row of its key, and every one after it
    hr_error(T, HR_W_ERR, hr_row_pos(T, r), HR_UNSUPPORTED);
  T.row_head[r] = r - d;
  const bool multi = d > 0 || (r + 1 < T.R && hr_same_key(T, r + 1, r));
  int64_t prev = 0, first = 0;
  int n = 0, skipped = 0;
  for (int64_t c = hr_col0(T, r), c1 = hr_col1(T, r); c < c1; ++c) {
    const int st = T.rec_state[c];
    if (st == HR_SKIP) ++skipped;
    if (st != HR_ALIVE) continue;
    const int64_t t = T.rec_ts[c];
    if (n > 0 && t <= prev)
      hr_error(T, HR_W_ERR, hr_cell_pos(c), HR_UNSUPPORTED);
    if (n == 0) first = t;
    prev = t;
    if (!multi) T.rec_rank[c] = n;
    ++n;
  }
  T.row_cnt[r] = multi ? 0 : n;
  T.row_first[r] = first;
  T.row_last[r] = prev;
  if (n) atomicAdd(&T.small[HR_W_DECODED], (unsigned long long)n);
  if (skipped) atomicAdd(&T.small[HR_W_SKIPPED], (unsigned long long)skipped);
}

// ------------------------------------------------------------------------
// k_hr_merge: one thread per row, at work on the head of a run of several
// rows: the rows' surviving cells merged by timestamp, the earliest row
// winning an equal one (HistogramRowSeq.addRow applied row after row).
// ------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_hr_merge(HistRowsDev T) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= T.R || T.row_head[r] != r) return;
  if (r + 1 >= T.R || !hr_same_key(T, r + 1, r)) return;
  int nr = 1;
  while (nr < kHrRunRows && r + nr < T.R && hr_same_key(T, r + nr, r)) ++nr;
  int64_t cur[kHrRunRows], end[kHrRunRows];
  auto alive_from = [&](int64_t c, int64_t e) {
    while (c < e && T.rec_state[c] != HR_ALIVE) ++c;
    return c;
  };
  for (int j = 0; j < nr; ++j) {
    end[j] = hr_col1(T, r + j);
    cur[j] = alive_from(hr_col0(T, r + j), end[j]);
  }
  int64_t rank = 0, dropped = 0, first = 0, last = 0;
  for (;;) {
    int jm = -1;
    int64_t tm = 0;
    for (int j = 0; j < nr; ++j) {
      if (cur[j] >= end[j]) continue;
      const int64_t t = T.rec_ts[cur[j]];
      if (jm < 0 || t < tm) {
        jm = j;
        tm = t;
      }
    }
    if (jm < 0) break;
    if (rank == 0) first = tm;
    last = tm;
    for (int j = 0; j < nr; ++j) {
      if (cur[j] >= end[j] || T.rec_ts[cur[j]] != tm) continue;
      if (j == jm) {
        T.rec_rank[cur[j]] = (int32_t)rank;
      } else {
        T.rec_rank[cur[j]] = -1;
        ++dropped;
      }
      cur[j] = alive_from(cur[j] + 1, end[j]);
    }
    ++rank;
  }
  T.row_cnt[r] = rank;
  T.row_first[r] = first;
  T.row_last[r] = last;
  if (dropped) atomicAdd(&T.small[HR_W_DROPPED], (unsigned long long)dropped);
}

// ------------------------------------------------------------------------
// k_hr_series: one thread per row, at work on a series' first row: each
// run's first timestamp lies after the run before's last.
// ------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_hr_series(HistRowsDev T) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= T.R) return;
  const int64_t s = T.row_series[r];
  if (r > 0 && T.row_series[r - 1] == s) return;
  bool has = false;
  int64_t last = 0;
  for (int64_t q = r; q < T.R && T.row_series[q] == s; ++q) {
    if (T.row_head[q] != q || T.row_cnt[q] <= 0) continue;
    if (has && T.row_first[q] <= last)
      hr_error(T, HR_W_ERR2, hr_row_pos(T, q), HR_UNSUPPORTED);
    last = T.row_last[q];
    has = true;
  }
}

}  // namespace otsdb
