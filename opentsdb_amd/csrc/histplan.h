// histplan.h — how a histogram query (hist.hip, otsdb_hist_*) is cut into
// workgroups: the members of a tile, the buckets of a window, the LDS a
// window's state takes.  One (tile, window) pair is one workgroup; the plan
// decides the fold's speed and nothing of its results (every sum is a
// wrapping 64-bit integer add).  Host code without a device header: the
// engine plans with it, the library exports hist_window as
// otsdb_hist_window so that tests reach the window edges without naming them.
#pragma once
#include <stdint.h>

namespace otsdb {

constexpr int kHistMaxRow = 256;  // K + 2: two bins a lane, two wave passes
constexpr int kHistMaxPct = 16;   // percentiles of one call
constexpr int64_t kHistTile = 64;  // members of one tile
// a workgroup's LDS: the figure at which the ordered folds keep 4 workgroups
// a CU
constexpr int kHistLdsBudget = 34816;
constexpr int kHistLdsHeader = 64;  // the work queue's counter, 16-B aligned
constexpr int kHistMinWindow = 16, kHistMaxWindow = 256;
// dense [G][B][K+2] int64 of one call (otsdb_hist_columns: E_CAPACITY past it)
constexpr int64_t kHistDenseBudget = int64_t(8) << 30;

// row pitch of a window's state in LDS: K + 2 rounded up to a whole pair
inline int hist_pitch(int row) { return (row + 1) & ~1; }

// buckets per window for rows of `row` = K + 2 counts: what fits the budget
// beside one 4-byte emit flag a bucket, within [16, 256]
inline int hist_window(int row) {
  const int per = hist_pitch(row) * 8 + 4;
  int w = (kHistLdsBudget - kHistLdsHeader) / per;
  if (w > kHistMaxWindow) w = kHistMaxWindow;
  if (w < kHistMinWindow) w = kHistMinWindow;
  return w;
}

// dynamic LDS of a workgroup over `w` buckets (a short grid takes less)
inline int hist_lds_bytes(int row, int w) {
  return (kHistLdsHeader + w * (hist_pitch(row) * 8 + 4) + 15) & ~15;
}

}  // namespace otsdb
