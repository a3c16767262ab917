// rollup_monoids.h — downsampling states of rollup queries.
//
// A rollup table stores pre-aggregated cells; Downsampler / FillingDownsampler
// given a RollupQuery compute two functions from them differently
// (Downsampler.java:162-228, FillingDownsampler.java:196-252):
//   avg    sum of the sum cells / sum of the count cells (RollupSeq.java:
//          659-679 valueCount); the count is a Java long and wraps, NaN is
//          NOT skipped, and a total count of zero gives a present 0.0
//   count  sum of the count cells as doubles, NaN not skipped
// Both follow monoids.h's interface (init / from / push / push_if / combine /
// finish / pack / unpack / shfl_up / dpp).  MRollAvg's operand is the
// (value, count) pair of a point, not a double: PointBits / RollBits say what
// a lane keeps per point and point_operand (kernels.hip) builds the operand.
#pragma once
#include "monoids.h"

namespace otsdb {

// a point of a rollup average as a lane holds it (value bits + valueCount)
// and as MRollAvg takes it
struct RollBits {
  int64_t bits, cnt;
};
struct RollPoint {
  double v;
  int64_t n;
};

// Java's wrapping long add
DEV int64_t wrap_add(int64_t a, int64_t b) {
  return (int64_t)((uint64_t)a + (uint64_t)b);
}

struct MRollAvg {
  static constexpr bool kOrdered = false;
  static constexpr bool kCostlyFinish = true;  // s / n
  double s;
  int64_t n;  // 64-bit: one bucket's rollup counts pass 2^31
  DEV static MRollAvg init() { return {0.0, 0}; }
  DEV static MRollAvg from(RollPoint x) { return {0.0 + x.v, x.n}; }
  DEV void push(RollPoint x) {
    s += x.v;
    n = wrap_add(n, x.n);
  }
  DEV void push_if(bool mk, RollPoint x) {  // branch free; s is never -0.0
    s += mk ? x.v : 0.0;
    n = wrap_add(n, mk ? x.n : 0);
  }
  DEV static MRollAvg combine(const MRollAvg& a, const MRollAvg& b) {
    return {a.s + b.s, wrap_add(a.n, b.n)};
  }
  DEV double finish(int* err) const { return n == 0 ? 0.0 : s / (double)n; }
  DEV Packed pack() const { return {s, 0.0, 0.0, n}; }
  DEV static MRollAvg unpack(const Packed& p) { return {p.x, p.w}; }
  DEV void shfl_up(int d) {
    s = __shfl_up(s, d);
    n = __shfl_up(n, d);
  }
  template <int CTRL, int RM>
  DEV void dpp() {
    s = dppv<CTRL, RM>(s);
    n = dppv<CTRL, RM>(n);
  }
};

struct MRollCount {
  static constexpr bool kOrdered = false;
  static constexpr bool kCostlyFinish = false;
  double s;
  DEV static MRollCount init() { return {0.0}; }
  DEV static MRollCount from(double v) { return {0.0 + v}; }
  DEV void push(double v) { s += v; }
  DEV void push_if(bool mk, double v) { s += mk ? v : 0.0; }  // s is never -0.0
  DEV static MRollCount combine(const MRollCount& a, const MRollCount& b) {
    return {a.s + b.s};
  }
  DEV double finish(int* err) const { return s; }
  DEV Packed pack() const { return {s, 0.0, 0.0, 0}; }
  DEV static MRollCount unpack(const Packed& p) { return {p.x}; }
  DEV void shfl_up(int d) { s = __shfl_up(s, d); }
  template <int CTRL, int RM>
  DEV void dpp() { s = dppv<CTRL, RM>(s); }
};

// What a lane keeps per point for downsampling state M: the value bits, for
// MRollAvg with the point's count beside them.
template <class M>
struct PointBits {
  using type = int64_t;
};
template <>
struct PointBits<MRollAvg> {
  using type = RollBits;
};
DEV int64_t& value_bits(int64_t& b) { return b; }
DEV int64_t& value_bits(RollBits& b) { return b.bits; }
// the count(s) of point(s) i (and i + 1) into them: nothing to read for plain
// value bits; two consecutive points in one 16-byte load (cnt + i 16-byte
// aligned)
DEV void load_count(int64_t&, const int64_t*, int64_t) {}
DEV void load_count(RollBits& b, const int64_t* cnt, int64_t i) {
  b.cnt = cnt[i];
}
DEV void load_count_if(bool, int64_t&, const int64_t*, int64_t) {}
DEV void load_count_if(bool ok, RollBits& b, const int64_t* cnt, int64_t i) {
  b.cnt = ok ? cnt[i] : 0;
}
DEV void load_count2(int64_t&, int64_t&, const int64_t*, int64_t) {}
DEV void load_count2(RollBits& a, RollBits& b, const int64_t* cnt, int64_t i) {
  typedef long long cnt2_t __attribute__((ext_vector_type(2)));
  const cnt2_t c = *reinterpret_cast<const cnt2_t*>(cnt + i);
  a.cnt = c.x;
  b.cnt = c.y;
}

}  // namespace otsdb
