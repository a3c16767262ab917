// rollup.hip — the downsample kernels of rollup queries:
// k_prep's and the ring k_bucketize_k's bodies (prep_series,
// bucketize_series) over the two rollup states of rollup_monoids.h, with the
// points' value_count column beside the batch.  Nothing else is instantiated
// for them: rollup queries take the row path (k_transform, k_group /
// selection, compaction — none of which knows the downsampling state), and
// rate runs through k_transform's RateSpan over the rows.
#define OTSDB_DS_TU 1
// the ring's production shape (as ds_tu.hip; tuning builds override)
#ifndef OTSDB_RING_NT
#define OTSDB_RING_NT 0
#endif
#ifndef OTSDB_RING_WAVES
#define OTSDB_RING_WAVES 1
#endif
#ifndef OTSDB_RING_WIN
#define OTSDB_RING_WIN 256
#endif
#ifndef OTSDB_RING_FL
#define OTSDB_RING_FL 64
#endif
#ifndef OTSDB_PREP_TPB
#define OTSDB_PREP_TPB 64
#endif
#include "kernels.hip"
#include "launch.h"

namespace otsdb {

// k_prep with the counts: the bucket past the window and the rate buckets
// beyond it are rollup values too
template <class M>
__global__ void k_prep_rollup(Params P, BatchDev B, const int64_t* cnt,
                              SeriesMeta SM, int* err_word) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= B.S) return;
  bool keep;
  int64_t lo, hi;
  prep_series<M>(P, B, SM, err_word, s, true, &keep, &lo, &hi, cnt);
}

// k_bucketize_k's ring shape (LDS ring sink, sentinel rows, DPP scan) with
// the counts: 24 B a point, the counts in the same 16-byte loads as ts / val
template <class M>
__global__ __launch_bounds__(256, OTSDB_RING_WAVES) void k_bucketize_rollup(
    Params P, BatchDev B, const int64_t* cnt, SeriesMeta SM, Rows R) {
  __shared__ double ring_v[4][OTSDB_RING_WIN];
  const int w = threadIdx.x >> 6;
  const int64_t s = (int64_t)blockIdx.x * 4 + w;
  if (s >= B.S) return;
  RowSink S{R.val + s * P.nb, R.state + s * P.nb, ring_v[w],
            OTSDB_RING_WIN - 1, 0, 0, 0, OTSDB_RING_NT == 2};
  bucketize_series<M, 8, 0, OTSDB_RING_NT, 0, 1, OTSDB_RING_WIN,
                   OTSDB_RING_FL, 0>(P, B, SM, S, s, cnt);
}

namespace {
template <class M>
bool launch_rollup_m(DsKernel k, const DsLaunch& a, const int64_t* cnt) {
  const int64_t S = a.B.S;
  switch (k) {
    case DS_PREP:
      hipLaunchKernelGGL(k_prep_rollup<M>,
                         dim3((unsigned)((S + OTSDB_PREP_TPB - 1) / OTSDB_PREP_TPB)),
                         dim3(OTSDB_PREP_TPB), 0, a.st, a.P, a.B, cnt, a.SM,
                         a.err);
      OTSDB_DBG(a.st, "k_prep_rollup");
      return true;
    case DS_RING:
      hipLaunchKernelGGL(k_bucketize_rollup<M>, dim3((unsigned)((S + 3) / 4)),
                         dim3(256), 0, a.st, a.P, a.B, cnt, a.SM, a.R);
      OTSDB_DBG(a.st, "k_bucketize_rollup");
      return true;
    default:
      return false;
  }
}
}  // namespace

bool launch_rollup(RollupKind kind, DsKernel k, const DsLaunch& a,
                   const int64_t* value_count) {
  switch (kind) {
    case ROLLUP_AVG: return launch_rollup_m<MRollAvg>(k, a, value_count);
    case ROLLUP_COUNT: return launch_rollup_m<MRollCount>(k, a, nullptr);
    default: return false;
  }
}

}  // namespace otsdb
