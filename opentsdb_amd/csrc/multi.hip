// multi.hip — several cross-series aggregators over ONE per-series bucket
// matrix (otsdb_agg_run_multi*, DESIGN.md §4 "Multi-aggregator queries").
//
//   k_group_multi       k_group's work item — one thread per (tile, bucket),
//                       the same 8-deep gather of the members' states and
//                       values in SpanCmp order — pushing every gathered
//                       contribution into every requested unordered monoid
//                       state: the matrix is read once (9 B per series and
//                       bucket) instead of once per aggregator.
//                       PARTIAL (otsdb_agg_partials_multi_device): a tile
//                       that is a whole group packs every state into its
//                       output's per-(group, bucket) partial instead.
//   k_partial_empty_multi  the identity state of every output for the groups
//                       without a member on this rank (PARTIAL only).
//   k_finalize_ranks_multi  k_finalize_ranks for every output of a
//                       multi-aggregator call: the ranks' emit bytes read
//                       once, each output's partials merged in rank order.
//   k_transform_interp  k_transform's NONE-fill, non-rate branch out of
//                       place: reads the downsampler's pristine rows, writes
//                       one interpolation class's matrix.
// (included by engine.hip after kernels.hip)

namespace otsdb {

// the distinct unordered reduction states of monoids.h (dispatch.h
// with_monoid: which aggregators share one); dev (ordered) keeps k_group
#define OTSDB_MULTI_MONOIDS(X)                                              \
  X(0, MSum<0>) X(1, MSum<1>) X(2, MSum<2>) X(3, MSum<3>)                   \
  X(4, MMinMax<false>) X(5, MMinMax<true>) X(6, MFirstLast<false>)          \
  X(7, MFirstLast<true>) X(8, MMult) X(9, MDiff) X(10, MNone)
constexpr int kMultiSlots = 11;

// (-1: not an unordered state — dev)
template <class M> struct MultiSlot { static constexpr int value = -1; };
#define OTSDB_X(k, M) \
  template <> struct MultiSlot<M> { static constexpr int value = k; };
OTSDB_MULTI_MONOIDS(OTSDB_X)
#undef OTSDB_X

struct MultiOut {
  double* val;    // [G * nb]
  uint8_t* emit;  // [G * nb] (PARTIAL: the one emit mask of every output)
  int* err;       // this output's device error word
  Packed* part;   // [G * nb], PARTIAL only: this output's partials
};

struct MultiArgs {
  uint32_t mask;   // bit k: monoid slot k is requested (kernel-uniform)
  int32_t n_out;   // outputs of this launch
  int32_t slot[OTSDB_MULTI_MAX];  // monoid slot of output j
  MultiOut out[OTSDB_MULTI_MAX];
  Packed* partial[kMultiSlots];   // [n_tiles * nb] per requested slot
};

// A tile that is a whole group finishes every state straight into the
// outputs of its slot (Infinity / `none` checks against each output's own
// error word); otherwise one Packed partial per slot, merged by the
// unchanged k_combine<M> per output.  Every state is a named variable behind
// a kernel-uniform mask test — an indexed array of states would live in
// scratch.  push / finish are the code k_group<M> runs, so each monoid's
// result is bit-identical to k_group<M> over the same rows and tiles.
// PARTIAL: the whole-group tile packs each state into the partials of its
// outputs (what k_combine<M> writes for a group of several tiles) and one
// emit byte for all of them: emission does not depend on the aggregator.
template <bool PARTIAL>
__global__ __launch_bounds__(256) void k_group_multi(
    int64_t nb, int64_t n_tiles, const int64_t* __restrict__ tile_g,
    const int64_t* __restrict__ tile_m0, const int64_t* __restrict__ tile_m1,
    const uint8_t* __restrict__ tile_single,
    const int64_t* __restrict__ members, Rows R,
    uint8_t* __restrict__ tile_emit, MultiArgs A) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t t = idx / nb;
  if (t >= n_tiles) return;
  const int64_t b = idx - t * nb;
  const int64_t m0 = tile_m0[t], m1 = tile_m1[t];
  const uint32_t mask = A.mask;
#define OTSDB_X(k, M) M s##k = M::init();
  OTSDB_MULTI_MONOIDS(OTSDB_X)
#undef OTSDB_X
  int emit = 0;
  auto push_all = [&](double v) {
#define OTSDB_X(k, M) \
  if (mask & (1u << k)) s##k.push(v);
    OTSDB_MULTI_MONOIDS(OTSDB_X)
#undef OTSDB_X
  };
  int64_t m = m0;
  for (; m + 8 <= m1; m += 8) {
    int64_t off[8];
    uint8_t sv[8];
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) off[u] = members[m + u] * nb + b;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      sv[u] = R.state[off[u]];
      v[u] = R.val[off[u]];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      if (sv[u]) {
        push_all(v[u]);
        emit |= sv[u] == ST_REAL;
      }
    }
  }
  for (; m < m1; ++m) {
    const int64_t off = members[m] * nb + b;
    const uint8_t sv = R.state[off];
    if (sv) {
      push_all(R.val[off]);
      emit |= sv == ST_REAL;
    }
  }
  if (PARTIAL && tile_single[t]) {
    const int64_t o = tile_g[t] * nb + b;
#define OTSDB_X(k, M)                                     \
  if (mask & (1u << k)) {                                 \
    const Packed p = s##k.pack();                         \
    for (int j = 0; j < A.n_out; ++j)                     \
      if (A.slot[j] == k) A.out[j].part[o] = p;           \
  }
    OTSDB_MULTI_MONOIDS(OTSDB_X)
#undef OTSDB_X
    A.out[0].emit[o] = (uint8_t)emit;
  } else if (tile_single[t]) {
    const int64_t o = tile_g[t] * nb + b;
#define OTSDB_X(k, M)                                     \
  if (mask & (1u << k)) {                                 \
    double r = 0.0;                                       \
    int e = 0;                                            \
    if (emit) {                                           \
      r = s##k.finish(&e);                                \
      if (is_inf(r)) e |= ERR_INFINITY;                   \
    }                                                     \
    for (int j = 0; j < A.n_out; ++j)                     \
      if (A.slot[j] == k) {                               \
        if (e) atomicOr(A.out[j].err, e);                 \
        A.out[j].val[o] = r;                              \
        A.out[j].emit[o] = (uint8_t)emit;                 \
      }                                                   \
  }
    OTSDB_MULTI_MONOIDS(OTSDB_X)
#undef OTSDB_X
  } else {
#define OTSDB_X(k, M) \
  if (mask & (1u << k)) A.partial[k][t * nb + b] = s##k.pack();
    OTSDB_MULTI_MONOIDS(OTSDB_X)
#undef OTSDB_X
    tile_emit[t * nb + b] = (uint8_t)emit;
  }
}

// PARTIAL: a group with no member on this rank (no tile: grp_t0 == grp_t1,
// build_tiles' per-group tile ranges) contributes the identity of every
// output's monoid (not all-zero bits: min / max start at +-Infinity) and no
// emission.  One thread per (group, bucket).
__global__ __launch_bounds__(256) void k_partial_empty_multi(
    int64_t nb, int64_t n_groups, const int64_t* __restrict__ grp_t0,
    const int64_t* __restrict__ grp_t1, MultiArgs A) {
  const int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t g = o / nb;
  if (g >= n_groups || grp_t0[g] != grp_t1[g]) return;
  for (int j = 0; j < A.n_out; ++j) {
    const int sl = A.slot[j];
#define OTSDB_X(k, M) \
  if (sl == k) A.out[j].part[o] = M::init().pack();
    OTSDB_MULTI_MONOIDS(OTSDB_X)
#undef OTSDB_X
  }
  A.out[0].emit[o] = 0;
}

// the slot of dev in FinalizeArgs (its partials come from k_group<MDev>)
constexpr int kMultiSlotDev = kMultiSlots;

struct FinalizeArgs {
  int32_t n_out;
  int32_t slot[OTSDB_MULTI_MAX];  // monoid slot of output i (kMultiSlotDev)
  MultiOut out[OTSDB_MULTI_MAX];  // dense results and error word of output i
};

// k_finalize_ranks<M>'s merge of one (group, bucket) of output i:
// partials [n_ranks][n_out][GB], combined in rank (= series) order
template <class M>
DEV double finalize_ranks_one(const Packed* __restrict__ partials, int n_ranks,
                              int n_out, int i, int64_t GB, int64_t o, int emit,
                              int* e) {
  M st = M::init();
  for (int r = 0; r < n_ranks; ++r)
    st = M::combine(st, M::unpack(partials[((int64_t)r * n_out + i) * GB + o]));
  double v = 0.0;
  if (emit) {
    v = st.finish(e);
    if (is_inf(v)) *e |= ERR_INFINITY;
  }
  return v;
}

// multi-GPU, several outputs: one thread per (group, bucket) reads the
// ranks' emit bytes once, then merges and finishes each output into its own
// dense result (Infinity / `none` into the output's own error word).  The
// monoid of an output is a kernel-uniform slot test around one merge each
// (no indexed array of states, as in k_group_multi); the merge is
// k_finalize_ranks<M>'s, so output i has the bits of
// otsdb_agg_finalize_device over slice i.
__global__ __launch_bounds__(256) void k_finalize_ranks_multi(
    int64_t GB, int n_ranks, const Packed* __restrict__ partials,
    const uint8_t* __restrict__ emits, FinalizeArgs A) {
  const int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= GB) return;
  int emit = 0;
  for (int r = 0; r < n_ranks; ++r) emit |= emits[(int64_t)r * GB + o];
  for (int i = 0; i < A.n_out; ++i) {
    const int sl = A.slot[i];
    double v = 0.0;
    int e = 0;
#define OTSDB_X(k, M) \
  if (sl == k)        \
    v = finalize_ranks_one<M>(partials, n_ranks, A.n_out, i, GB, o, emit, &e);
    OTSDB_MULTI_MONOIDS(OTSDB_X)
    OTSDB_X(kMultiSlotDev, MDev)
#undef OTSDB_X
    if (e) atomicOr(A.out[i].err, e);
    A.out[i].val[o] = v;
    A.out[i].emit[o] = (uint8_t)emit;
  }
}

// k_transform's interpolation branch (fill NONE, no rate), out of place: the
// downsampler's rows `in` stay pristine for the next interpolation class,
// `out` takes this class's contributions (P.interp).  One wavefront per
// series.  Non-sentinel rows (cells / selection downsamplers): out.state is
// zeroed by the caller, as in.state was before the downsample.
__global__ __launch_bounds__(256) void k_transform_interp(Params P, BatchDev B,
                                                          SeriesMeta SM,
                                                          Rows in, Rows out) {
  const int lane = LANE;
  const int64_t s = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (s >= B.S) return;
  const int64_t nb = P.nb;
  const double* srcv = in.val + s * nb;
  const uint8_t* srcs = in.state + s * nb;
  double* rowv = out.val + s * nb;
  uint8_t* rows = out.state + s * nb;
  const bool sent = P.sentinel != 0;
  if (!SM.keep[s]) {
    if (sent)
      for (int64_t b = lane; b < nb; b += 64) rows[b] = ST_ABSENT;
    return;
  }
  const int64_t kf = sent ? SM.kf[s] : 0, kl = sent ? SM.kl[s] : -1;
  auto real_at = [&](int64_t b, double v) {
    return sent ? (b >= kf && b <= kl && __double_as_longlong(v) != kAbsentBits)
                : srcs[b] == ST_REAL;
  };
  const bool of = SM.of_has[s] != 0;
  int64_t carry_idx = -1;
  double carry_val = 0.0;
  double va = lane < nb ? srcv[lane] : 0.0;
  double vn = lane + 64 < nb ? srcv[lane + 64] : 0.0;
  for (int64_t c0 = 0; c0 < nb; c0 += 64) {
    const int64_t b = c0 + lane;
    const double vb = va;
    va = vn;
    vn = b + 128 < nb ? srcv[b + 128] : 0.0;
    const bool p = b < nb && real_at(b, vb);
    const double v = p ? vb : 0.0;
    if (p) rowv[b] = vb;
    if (sent && b < nb)  // every state of the row, written once
      rows[b] = p ? ST_REAL
                  : (((b > kf && b < kl) || (of && kf <= kl && b > kl))
                         ? ST_INTERP
                         : ST_ABSENT);
    else if (p)
      rows[b] = ST_REAL;
    const uint64_t rm = __ballot(p);
    const uint64_t below = rm & ((1ULL << lane) - 1);
    const int pl = below ? 63 - __builtin_clzll(below) : -1;
    const int64_t prev = pl >= 0 ? c0 + pl : carry_idx;
    uint64_t gaps = __ballot(p && prev >= 0 && prev < b - 1);
    if (gaps) {
      const double yp = __shfl(v, pl >= 0 ? pl : 0);
      const double yprev = pl >= 0 ? yp : carry_val;
      while (gaps) {
        const int g = __builtin_ctzll(gaps);
        gaps &= gaps - 1;
        const int64_t k0 = __shfl(prev, g), k1 = c0 + g;
        const double y0 = __shfl(yprev, g), y1 = __shfl(v, g);
        const int64_t x0 = bucket_ts(P, k0), x1 = bucket_ts(P, k1);
        for (int64_t j = k0 + 1 + lane; j < k1; j += 64) {
          rowv[j] = interp_value(P.interp, bucket_ts(P, j), x0, y0, x1, y1);
          rows[j] = ST_INTERP;
        }
      }
    }
    if (rm) {
      const int l = 63 - __builtin_clzll(rm);
      carry_val = readlane_d(v, l);
      carry_idx = c0 + l;
    }
  }
  if (of && carry_idx >= 0) {
    const int64_t x0 = bucket_ts(P, carry_idx), x1 = SM.of_ts[s];
    const double y1 = SM.of_val[s];
    for (int64_t j = carry_idx + 1 + lane; j < nb; j += 64) {
      rowv[j] = interp_value(P.interp, bucket_ts(P, j), x0, carry_val, x1, y1);
      rows[j] = ST_INTERP;
    }
  }
}

}  // namespace otsdb
