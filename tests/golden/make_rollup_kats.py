"""Writes tests/golden/kat_rollup.json: the reference's rollup JUnit tests as
known-answer vectors (data only; every case cites its test, paths under the
reference's tree).

A case: `rollup_agg` (RollupQuery.getRollupAgg), `spec` (tests/kat.py's
spec_from_case fields), `points` as [ts_ms, value, is_float, value_count]
and `expect` as [ts_ms, value, is_float]; `error` where the test expects an
exception.  MutableDataPoint.valueCount() is 1 (the Downsampler tests);
TestTsdbQueryRollup stores a sum cell and a count cell per timestamp, written
here as one (ts, sum, count) point.

Of TestTsdbQueryRollup's avg tests only run10mAvgLongSingleTS pairs every
stored sum cell with a count cell: MissingCount / MissingSum store one kind
only, and MissingACount, MissingASum and the three MissingToZero* tests each
leave at least one cell without its partner (pairing them is RollupSeq's
sync(), which stays with the caller), so they are not transcribed.

Run:  python tests/golden/make_rollup_kats.py
"""
import json
import os

NAN = "NaN"
BASE = 1356998400000  # TestDownsampler BASE_TIME
TD = "test/core/TestDownsampler.java"
TF = "test/core/TestFillingDownsampler.java"
TQ = "test/core/TestTsdbQueryRollup.java"

cases = []


def P(ts, v, c=1):
    return [int(ts), float(v), 1, int(c)]


def E(ts, v):
    return [int(ts), v if v == NAN else float(v), 1]


def add(**kw):
    cases.append(kw)


# ------------------------------------------------------------- Downsampler
# "10s-*" over points every 5 s from BASE_TIME, a lone Downsampler (no window)
def _view(ds_agg):
    return dict(ds_interval_ms=10000, ds_agg=ds_agg, query_start_ms=0,
                query_end_ms=2**63 - 1)


# :1188-1235 testDownsampler_rollupSum (R = sum, F = sum)
add(name="ds_rollup_sum", rollup_agg="sum", spec=_view("sum"),
    points=[P(BASE + 5000 * i, 2 ** i) for i in range(11)],
    expect=[E(BASE, 3), E(BASE + 10000, 12), E(BASE + 20000, 48),
            E(BASE + 30000, 192), E(BASE + 40000, 768),
            E(BASE + 50000, 1024)], tol=1e-7, cite=TD + ":1188-1235")
# :1238-1270 testDownsampler_rollupAvg (R = avg, F = avg)
add(name="ds_rollup_avg", rollup_agg="avg", spec=_view("avg"),
    points=[P(BASE + 5000 * i, 2 ** i) for i in range(4)],
    expect=[E(BASE, 1.5), E(BASE + 10000, 6)], tol=1e-7,
    cite=TD + ":1238-1270")
# :1273-1320 testDownsampler_rollupCount (R = count, F = count)
add(name="ds_rollup_count", rollup_agg="count", spec=_view("count"),
    points=[P(BASE + 5000 * i, 2 ** i) for i in range(4)],
    expect=[E(BASE, 3), E(BASE + 10000, 12)], tol=1e-7,
    cite=TD + ":1273-1320")
# :1322-1337 testDownsampler_rollupDev (R = dev: UnsupportedOperationException)
add(name="ds_rollup_dev", rollup_agg="dev", spec=_view("dev"),
    points=[P(BASE + 5000 * i, 2 ** i) for i in range(4)],
    error="UnsupportedOperationException", cite=TD + ":1322-1337")

# ------------------------------------------------------ FillingDownsampler
B1, B5 = 1000, 500
FULL = [P(B1 + 25 * k, 12 - k) for k in range(12)]
GAPS = [P(B5 + 25 * k, 1.0) for k in (4, 5, 7, 12, 15, 24, 25, 26, 27)]


def _fill(base, n, ds_agg):
    return dict(start_ms=base, end_ms=base + n * 25, ds_interval_ms=100,
                ds_agg=ds_agg, fill="nan", query_start_ms=0, query_end_ms=0)


def _grid(base, vals):
    return [E(base + 100 * i, v) for i, v in enumerate(vals)]


# :820-855 testDownsampler_rollup (R = sum, F = sum)
add(name="fill_rollup", rollup_agg="sum", spec=_fill(B1, 12, "sum"),
    points=FULL, expect=_grid(B1, [42, 26, 10]), tol=0, cite=TF + ":820-855")
# :858-896 testDownsampler_rollupMissing (R = sum, F = sum)
add(name="fill_rollup_missing", rollup_agg="sum", spec=_fill(B5, 36, "sum"),
    points=GAPS, expect=_grid(B5, [NAN, 3, NAN, 2, NAN, NAN, 4, NAN, NAN]),
    tol=0, cite=TF + ":858-896")
# :899-936 testDownsampler_rollupAvg (R = avg, F = avg)
add(name="fill_rollup_avg", rollup_agg="avg", spec=_fill(B1, 12, "avg"),
    points=FULL, expect=_grid(B1, [10.5, 6.5, 2.5]), tol=0,
    cite=TF + ":899-936")
# :939-977 testDownsampler_rollupAvgMissing (R = sum, F = avg: the ordinary
# avg, the counts ignored)
add(name="fill_rollup_avg_missing", rollup_agg="sum",
    spec=_fill(B5, 36, "avg"), points=GAPS,
    expect=_grid(B5, [NAN, 1, NAN, 1, NAN, NAN, 1, NAN, NAN]), tol=0,
    cite=TF + ":939-977")
# :980-1031 testDownsampler_rollupCount (R = count, F = count)
add(name="fill_rollup_count", rollup_agg="count", spec=_fill(B1, 12, "count"),
    points=FULL, expect=_grid(B1, [42, 26, 10]), tol=0, cite=TF + ":980-1031")
# :1034-1072 testDownsampler_rollupCountMissing (R = sum, F = count: sums)
add(name="fill_rollup_count_missing", rollup_agg="sum",
    spec=_fill(B5, 36, "count"), points=GAPS,
    expect=_grid(B5, [NAN, 3, NAN, 2, NAN, NAN, 4, NAN, NAN]), tol=0,
    cite=TF + ":1034-1072")
# :1074-1110 testDownsampler_rollupDev (R = dev)
add(name="fill_rollup_dev", rollup_agg="dev", spec=_fill(B1, 12, "dev"),
    points=FULL, error="UnsupportedOperationException",
    cite=TF + ":1074-1110")

# --------------------------------------------------------------- TsdbQuery
# :523-554 run10mAvgLongSingleTS: storeLongRollup's web01 sums 600, 1200, ...
# every 600 s over [1356998400, 1357041600] s, storeCount 2 beside each;
# "10m-avg", avg across the one series: 73 points 300, 600, ...
T0S, T1S = 1356998400, 1357041600
add(name="tsdb_10m_avg_long_single_ts", rollup_agg="avg",
    spec=dict(start_ms=T0S * 1000, end_ms=T1S * 1000,
              query_start_ms=T0S * 1000, query_end_ms=T1S * 1000, agg="avg",
              ds_interval_ms=600000, ds_agg="avg"),
    points=[[(T0S + 600 * i) * 1000, 600 * (i + 1), 0, 2] for i in range(73)],
    expect=[E((T0S + 600 * i) * 1000, 300 * (i + 1)) for i in range(73)],
    tol=0.0001, cite=TQ + ":523-554")

if __name__ == "__main__":
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                       "kat_rollup.json")
    with open(out, "w") as f:
        json.dump({"cases": cases}, f, indent=1)
        f.write("\n")
    print("%d cases -> %s" % (len(cases), out))
