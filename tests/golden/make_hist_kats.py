"""Writes tests/golden/kat_histogram.json: the reference's histogram JUnit
tests as known-answer vectors (data only; every case cites its test, paths
under the reference's tree).

Kinds:
  percentile  `hist` = {buckets: [[lower, upper, count]], underflow, overflow},
              `percentiles` and the asserted `expect` values with the test's
              `tol`
  merge       `hists`: the first aggregates the others with SUM; `expect` =
              the asserted bucket counts, `underflow` / `overflow` where the
              test asserts them
  query       `ds` (the downsampling specifier), `series` (one list of
              [ts_ms, value] per span) and `expect` = [[ts_ms, value]].  The
              reference tests use a one-long test histogram
              (LongHistogramDataPointForTest): K = 1 here, the merged counts
              column as the value.  `seek`: the timestamp the test seeks the
              downsampler to (null: none).  `start_ms` / `end_ms`: the
              aggregation window — the test's own for the
              HistogramAggregationIterator cases; for the downsampler cases,
              which have no window, the seek timestamp (the first expected
              timestamp without a seek, a grid point) and the last expected
              timestamp, which leave the downsampler's output as it is.

Left out, with the reason:
  testDownsampler_all*, testHistogramSpanDownsampler_all*      0all
  testDownsampler_calendar*, _noDataCalendar, testSeek_useCalendar,
  testHistogramSpanDownsampler_calendar*                       calendar
  TestHistogramAggregationIterator *NoDownsampler* / *NoDownSampler*
                                                               no downsampler
  testRemove                                                   no data

Run:  python tests/golden/make_hist_kats.py
"""
import json
import os

BASE = 1356998400000  # BASE_TIME of both downsampler test classes
TS = "test/core/TestSimpleHistogram.java"
TD = "test/core/TestHistogramDownsampler.java"
TA = "test/core/TestHistogramAggregationIterator.java"

cases = []


def add(**kw):
    cases.append(kw)


# ---- TestSimpleHistogram ---------------------------------------------------
H3 = dict(buckets=[[1.0, 6.0, 5], [6.0, 10.0, 10], [10.0, 20.0, 1]],
          underflow=0, overflow=5)
H4 = dict(buckets=[[1.0, 6.0, 5], [6.0, 10.0, 10], [10.0, 20.0, 1],
                   [20.0, 40.0, 0]], underflow=0, overflow=5)
add(name="simple_single_percentile", kind="percentile", hist=H3,
    percentiles=[50.0, 1000.0], expect=[8.0, -1.0], tol=0.0001,
    cite=TS + ":280-303")
add(name="simple_percentile_list", kind="percentile", hist=H4,
    percentiles=[50.0, 99.0], expect=[8.0, 15.0], tol=0.001,
    cite=TS + ":306-337")
add(name="simple_single_merge", kind="merge",
    hists=[H4, dict(H4, underflow=2)],
    expect=[[1.0, 6.0, 10], [6.0, 10.0, 20], [10.0, 20.0, 2]],
    underflow=2, overflow=10, cite=TS + ":340-373")
add(name="simple_multiple_merge", kind="merge", hists=[H4, H4, H4],
    expect=[[1.0, 6.0, 15], [6.0, 10.0, 30], [10.0, 20.0, 3]],
    underflow=None, overflow=15, cite=TS + ":376-412")
add(name="simple_missing_buckets_merge", kind="merge",
    hists=[dict(buckets=[[5.0, 7.0, 3], [7.0, 10.0, 5], [15.0, 20.0, 2]],
                underflow=0, overflow=0),
           dict(buckets=[[5.0, 7.0, 3], [7.0, 10.0, 5], [10.0, 15.0, 2],
                         [15.0, 20.0, 1]], underflow=0, overflow=0)],
    expect=[[10.0, 15.0, 2]], underflow=None, overflow=None,
    cite=TS + ":527-541")

# ---- TestHistogramDownsampler ----------------------------------------------
SIX = [[BASE, 40], [BASE + 2000000, 50], [BASE + 3600000, 40],
       [BASE + 3605000, 50], [BASE + 7200000, 40], [BASE + 9200000, 50]]
POW2 = [[BASE + 5000 * i, 1 << i] for i in range(11)]
FIFTEEN = [[BASE + 5000 + 10000 * i, 1 << i] for i in range(6)]
E_SIX = [[BASE - 400000, 40], [BASE + 1600000, 50], [BASE + 3600000, 90],
         [BASE + 6600000, 40], [BASE + 8600000, 50]]
E_POW2 = [[BASE, 3], [BASE + 10000, 12], [BASE + 20000, 48],
          [BASE + 30000, 192], [BASE + 40000, 768], [BASE + 50000, 1024]]
E_FIFTEEN = [[BASE, 1], [BASE + 15000, 6], [BASE + 30000, 8],
             [BASE + 45000, 48]]


def query(name, ds, series, expect, cite, seek=None, start=None, end=None):
    if start is None:
        start = seek if seek is not None else (expect[0][0] if expect else 0)
    if end is None:
        end = expect[-1][0] if expect else start
    add(name=name, kind="query", ds=ds, series=series, expect=expect,
        seek=seek, start_ms=start, end_ms=end, cite=cite)


query("ds_1000s", "1000s-sum", [SIX], E_SIX, TD + ":113-136")
query("ds_10seconds", "10s-sum", [POW2], E_POW2, TD + ":139-190")
query("ds_15seconds", "15s-sum", [FIFTEEN], E_FIFTEEN, TD + ":193-228")
query("ds_no_data", "1d-sum", [[]], [], TD + ":818-824", start=BASE,
      end=BASE + 86400000)
query("seek", "1000s-sum", [SIX], E_SIX[2:], TD + ":842-862",
      seek=BASE + 3600000)
query("seek_skip_partial_interval", "1000s-sum", [SIX], E_SIX[3:],
      TD + ":865-889", seek=BASE + 3800000)
query("seek_double_iteration", "1000s-sum", [SIX], E_SIX[2:],
      TD + ":892-914", seek=BASE + 3600000)
FORTY = [[BASE + 100 + 1000 * i, 40] for i in range(11)]
# the first next() after seek(BASE): the test reads one point (the window
# ends inside that bucket: the span's first point must lie in the window)
query("seek_abandoning_aligned", "10s-sum", [FORTY], [[BASE, 400]],
      TD + ":917-949", seek=BASE, end=BASE + 9999)
for k in range(1, 11):  # seek_timestamp = BASE + 1000, ..., BASE + 10000
    query("seek_abandoning_%d" % k, "10s-sum", [FORTY], [[BASE + 10000, 40]],
          TD + ":952-964", seek=BASE + 1000 * k)
query("span_ds_1000s", "1000s-sum", [SIX], E_SIX, TD + ":1010-1052")
query("span_ds_10seconds", "10s-sum", [POW2], E_POW2, TD + ":1055-1107")
query("span_ds_15seconds", "15s-sum", [FIFTEEN], E_FIFTEEN,
      TD + ":1110-1148")

# ---- TestHistogramAggregationIterator --------------------------------------
TEN = [[BASE + 5000 * i, i] for i in range(10)]
query("agg_one_span_10secs", "10s-sum", [TEN],
      [[BASE + 10000 * i, 4 * i + 1] for i in range(5)], TA + ":84-132",
      start=BASE, end=BASE + 50000)
query("agg_one_span_later_data_points", "10s-sum", [TEN],
      [[BASE, 1], [BASE + 10000, 5], [BASE + 20000, 9]], TA + ":225-264",
      start=BASE, end=BASE + 25000)
query("agg_two_spans_same_timestamp", "10s-sum", [TEN, TEN],
      [[BASE + 10000 * i, 2 * (4 * i + 1)] for i in range(5)],
      TA + ":311-353", start=BASE, end=BASE + 50000)

if __name__ == "__main__":
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                       "kat_histogram.json")
    with open(out, "w") as f:
        json.dump({"cases": cases}, f, indent=1)
        f.write("\n")
    print("%d cases -> %s" % (len(cases), out))
