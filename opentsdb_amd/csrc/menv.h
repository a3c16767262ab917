// menv.h — the envelope state {sum, count, min, max}: MSum<0|1|3> (s, n) and
// MMinMax<false|true> (mn, mx) side by side, operation for operation and in
// the same order, so every component has the bits of the single monoid.
// Shared by the panel pass (panel.hip: one downsample pass, up to five rows)
// and the multi-aggregator fold (foldmulti.hip: one ordered fold, up to five
// kinds of output).
#pragma once
#include "monoids.h"

namespace otsdb {

struct MEnv {
  static constexpr bool kOrdered = false;
  static constexpr bool kCostlyFinish = true;  // avg: s / n
  double s;
  int32_t n;
  double mn, mx;
  DEV static MEnv init() {
    return {0.0, 0, __builtin_inf(), -__builtin_inf()};
  }
  DEV static MEnv from(double v) {
    if (is_nan(v)) return init();
    return {0.0 + v, 1, v, v};
  }
  DEV void push(double v) {
    if (!is_nan(v)) {
      s += v;
      ++n;
      if (v < mn) mn = v;
      if (v > mx) mx = v;
    }
  }
  DEV void push_if(bool mk, double v) {  // branch free; NaN compares false
    const bool ok = mk & !is_nan(v);
    s += ok ? v : 0.0;
    n += ok ? 1 : 0;
    mn = (mk & (v < mn)) ? v : mn;
    mx = (mk & (v > mx)) ? v : mx;
  }
  DEV static MEnv combine(const MEnv& a, const MEnv& b) {
    return {a.s + b.s, a.n + b.n, b.mn < a.mn ? b.mn : a.mn,  // the earliest
            b.mx > a.mx ? b.mx : a.mx};                       // extreme stays
  }
  DEV double sum() const { return n == 0 ? qnan() : s; }
  DEV double avg() const { return n == 0 ? qnan() : s / (double)(int32_t)n; }
  DEV double count() const { return (double)n; }
  DEV double min() const { return mn == __builtin_inf() ? qnan() : mn; }
  DEV double max() const { return mx == -__builtin_inf() ? qnan() : mx; }
  DEV Packed pack() const { return {s, mn, mx, n}; }
  DEV static MEnv unpack(const Packed& p) {
    return {p.x, (int32_t)p.w, p.y, p.z};
  }
  DEV void shfl_up(int d) {
    s = __shfl_up(s, d);
    n = __shfl_up(n, d);
    mn = __shfl_up(mn, d);
    mx = __shfl_up(mx, d);
  }
  template <int CTRL, int RM>
  DEV void dpp() {
    s = dppv<CTRL, RM>(s);
    n = dppv<CTRL, RM>(n);
    mn = dppv<CTRL, RM>(mn);
    mx = dppv<CTRL, RM>(mx);
  }
};

}  // namespace otsdb
