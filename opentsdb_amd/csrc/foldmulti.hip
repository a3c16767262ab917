// foldmulti.hip — the ordered group fold for several cross-series aggregators
// at once (otsdb_agg_run_multi* with OTSDB_SPEC_MULTI_FOLD).
//
// k_fold_multi is k_fold's workgroup (fold.hip: one workgroup per (tile,
// window), the LDS work queue, the per-member progress marks, fold_member /
// fold_flush / fold_fill_gap / fold_member_tail unchanged) over the envelope
// state MEnv = {sum, count, min, max} (menv.h) in place of one aggregator's
// state: every contribution is pushed once, in SpanCmp order, and sum /
// zimsum / pfsum, avg, count, min / mimmin and max / mimmax are all finished
// from the same 32-byte state.  Each component is MSum<0|1|3> / MMinMax<*>
// operation for operation, and the tiles are the single fold's, so output j
// has the contribution order of the single query with that aggregator.
// Only the finalisation differs from k_fold: a whole-group tile writes every
// output (Infinity into the error word of the output that holds it), a tile
// of a larger group leaves the per-monoid partials k_combine<M> merges.
// CELLS != 0 (otsdb_agg_run_cells_multi_device with
// OTSDB_SPEC_CELLS_MULTI_FOLD): the members are streamed from compacted
// columns — k_fold's CELLS variants (the CellsMember slot per wave, the
// ERR_CELLS_GENERIC early-out, fold_member_cells / fold_member_cells_u of
// cellfold.hip, the cells fold's launch bound) over the same state.
// (Included by both parts of ds_tu.hip: the columnar kernel is launched from
// part 0, the cells ones from part 1.)
#pragma once
#include "fold.hip"
#include "menv.h"

namespace otsdb {

// output kind -> value of the envelope: named branches over a kernel-uniform
// kind (no indexed array of states)
DEV double fold_multi_finish(const MEnv& m, int32_t kind) {
  switch (kind) {
    case FM_SUM: return m.sum();
    case FM_AVG: return m.avg();
    case FM_CNT: return m.count();
    case FM_MIN: return m.min();
    default: return m.max();
  }
}

#ifndef OTSDB_CELLS_MULTI_FOLD_WAVES  // (tuning builds: another bound)
#define OTSDB_CELLS_MULTI_FOLD_WAVES OTSDB_CELLS_FOLD_WAVES
#endif

template <class M, int K = 8, int CELLS = 0>
__global__ __launch_bounds__(FOLD_THREADS, CELLS ? OTSDB_CELLS_MULTI_FOLD_WAVES
                                        : OTSDB_FOLD_WAVES) void k_fold_multi(
    Params P, BatchDev B, SeriesMeta SM, int64_t n_tiles,
    const int64_t* __restrict__ tile_g, const int64_t* __restrict__ tile_m0,
    const int64_t* __restrict__ tile_m1,
    const uint8_t* __restrict__ tile_single,
    const int64_t* __restrict__ members, const WinCtx* __restrict__ wc,
    int64_t NW, uint8_t* __restrict__ tile_emit, int* err_word,
    FoldMultiArgs FM, CellsFold CF) {
  using A = MEnv;
  // the window's envelope states and emit flags (fold_lds_bytes<MEnv>: 1,024
  // buckets at most, 33,792 B)
  extern __shared__ __attribute__((aligned(16))) unsigned char fold_dyn[];
  A* st = reinterpret_cast<A*>(fold_dyn);
  uint8_t* emit = fold_dyn + fold_lds_states<A>(P);
  __shared__ double ring[FOLD_WG][FOLD_WIN];
  __shared__ int32_t prog[256];
  __shared__ int s_next;
  __shared__ FoldKernel kc;
  __shared__ FoldMember mc[FOLD_WG];
  __shared__ CellsMember cm[CELLS ? FOLD_WG : 1];
  const int tid = threadIdx.x, lane = LANE, w = tid >> 6;
  const int64_t nb = P.nb;
  int32_t W0, W1;
  {
    const int64_t t = (int64_t)blockIdx.x % n_tiles;
    const int64_t win = (int64_t)blockIdx.x / n_tiles;
    const int64_t wb = fold_window<A>(P);  // <= fold_wb<MEnv>()
    W0 = (int32_t)(win * wb);
    W1 = (int32_t)((W0 + wb < nb) ? W0 + wb : nb);
    if (tid == 0) {
      kc.SM = SM;
      kc.members = members;
      kc.wc = wc;
      kc.series_float = B.series_float;
      kc.nbd = NW - 1;
      kc.win = win;
      kc.m0 = tile_m0[t];
      kc.m1 = tile_m1[t];
      kc.g = tile_g[t];
      kc.t = t;
      kc.partial = nullptr;  // (the outputs' own: FM)
      kc.tile_emit = tile_emit;
      kc.out_val = nullptr;
      kc.out_emit = nullptr;
      kc.fin = tile_single[t];
      // a cells fold whose prep already sent the batch to the generic path
      // (as k_fold: the engine rewrites the columns and runs again)
      s_next = (CELLS && (__hip_atomic_load(err_word, __ATOMIC_RELAXED,
                                            __HIP_MEMORY_SCOPE_AGENT) &
                          ERR_CELLS_GENERIC)) ? -1 : 0;
    }
  }
  const int nw = W1 - W0;
  for (int b = tid; b < nw; b += FOLD_THREADS) {
    st[b] = A::init();
    emit[b] = 0;
  }
  for (int j = tid; j < 256; j += FOLD_THREADS) prog[j] = 0;
  for (int i = lane; i < FOLD_WIN; i += 64) ring[w][i] = absent_value();
  __syncthreads();
  if (CELLS && s_next < 0) return;  // (block-uniform)
  int dbg_n = 0;
  FoldSink<A> F{st, emit, ring[w], prog, err_word, 0, 0, W0, W1, W0, -1, 0, 0.0};
  // a member's window context (k_prep / k_fold_prep's results for series s)
  auto member_ctx = [&](int64_t s) {
    const SeriesMeta& sm = kc.SM;
    const int64_t nbd = kc.nbd, win = kc.win;
    FoldMember m;
    m.kept = sm.keep[s] != 0;
    m.pa = m.kept ? sm.lo[s] : 0;
    m.pb = m.kept ? sm.hi[s] : 0;
    m.has_prev = m.has_next = 0;
    m.px = m.nx = 0;
    m.py = m.ny = 0.0;
    if (win > 0) {
      const WinCtx& c = kc.wc[s * nbd + win - 1];
      m.pa = c.bnd;
      if (c.prev_ts != INT64_MIN) {
        m.has_prev = 1;
        m.px = c.prev_ts;
        m.py = c.prev_val;
      }
    }
    if (win < nbd) {
      const WinCtx& c = kc.wc[s * nbd + win];
      m.pb = c.bnd;
      if (c.next_ts != INT64_MIN) {
        m.has_next = 1;
        m.nx = c.next_ts;
        m.ny = c.next_val;
      }
    }
    if (!m.has_next && sm.of_has[s]) {  // toward the point past the grid
      m.has_next = 1;
      m.nx = sm.of_ts[s];
      m.ny = sm.of_val[s];
    }
    m.sf = kc.series_float ? (int)kc.series_float[s] : 1;
    return m;
  };
  // every member context loaded at once when the host sized the dynamic LDS
  // for them (P.fold_ctx > 0: windows short of full width)
  const int64_t n_mem = kc.m1 - kc.m0;
  const bool ctx_on = !CELLS && P.fold_ctx > 0 && n_mem <= P.fold_ctx;
  FoldMember* ctx = reinterpret_cast<FoldMember*>(fold_dyn + fold_lds_bytes<A>(P));
  if (ctx_on) {
    for (int64_t j = tid; j < n_mem; j += FOLD_THREADS) ctx[j] = member_ctx(kc.members[kc.m0 + j]);
    __syncthreads();
  }
  for (;;) {
    int i = 0;
    if (lane == 0) i = atomicAdd(&s_next, 1);
    i = __builtin_amdgcn_readlane(i, 0);
    const int64_t m0 = uni(kc.m0);
    if (m0 + i >= uni(kc.m1)) break;
    FOLD_GUARD(dbg_n, 1 << 20, err_word, "claim loop i=%d\n", i)
    F.mi = i;
    F.eff = 0;
    // the member's window context, lane 0 -> LDS (preloaded: a copy)
    if (lane == 0) {
      const int64_t s = ctx_on ? 0 : kc.members[m0 + i];
      mc[w] = ctx_on ? ctx[i] : member_ctx(s);
      if (CELLS) {  // the stream's cursor at the window's first point
        const int64_t nbd = kc.nbd, win = kc.win;
        CellsMember c;
        c.qb = CF.C.qual_off[CF.series_row[s]];
        c.vb0 = CF.C.val_off[CF.series_row[s]];
        c.r1 = CF.series_row[s + 1];
        if (win > 0) {
          const int64_t o = s * nbd + win - 1;
          c.rlo = CF.wrlo[o];
          c.vcur = CF.wvlo[o];
          c.vl0 = CF.wvl0[o];
        } else {
          c.rlo = CF.rlo[s];
          c.vcur = CF.vlo[s];
          c.vl0 = CF.vl0[s];
        }
        c.qw = CF.qw[s];
        c.uf = CF.uf ? CF.uf[s] : 0xFF;
        c.qend = CF.C.qual_off[CF.C.R];
        c.vend = CF.C.val_off[CF.C.R];
        cm[CELLS ? w : 0] = c;
      }
    }
    if constexpr (CELLS >= 8)  // every kept series uniform (k_cells_uniform)
      fold_member_cells_u<M, A, K, CELLS - 8>(P, CF.C, F, &mc[w], &cm[w]);
    else if constexpr (CELLS != 0)
      fold_member_cells<M, A, K, CELLS>(P, CF.C, F, &mc[w], &cm[w]);
    else
      fold_member<M, A, K>(P, B, F, &mc[w]);
    fold_publish(F, kProgDone);
  }
  __syncthreads();
  const bool fin = kc.fin;
  const int64_t g = kc.g, t = kc.t;
  if (fin) {
    // a whole group: every output from the one state; Infinity fails only
    // the output that holds it (bit j of einf)
    uint32_t einf = 0;
    for (int b = tid; b < nw; b += FOLD_THREADS) {
      const int64_t o = g * nb + W0 + b;
      const A m = st[b];
      const uint8_t em = emit[b];
      for (int j = 0; j < FM.n_out; ++j) {
        double r = 0.0;
        if (em) {
          r = fold_multi_finish(m, FM.kind[j]);
          if (is_inf(r)) einf |= 1u << j;
        }
        FM.out[j].val[o] = r;
        FM.out[j].emit[o] = em;
      }
    }
    for (int j = 0; j < FM.n_out; ++j)
      if (einf >> j & 1) atomicOr(FM.out[j].err, ERR_INFINITY);
  } else {
    for (int b = tid; b < nw; b += FOLD_THREADS) {
      const int64_t o = t * nb + W0 + b;
      const A m = st[b];
      if (FM.part_sn) FM.part_sn[o] = Packed{m.s, 0.0, 0.0, m.n};
      if (FM.part_mn) FM.part_mn[o] = Packed{m.mn, 0.0, 0.0, 0};
      if (FM.part_mx) FM.part_mx[o] = Packed{m.mx, 0.0, 0.0, 0};
      kc.tile_emit[o] = emit[b];
    }
  }
}

}  // namespace otsdb
