"""Rollup queries on the GPU (otsdb_agg_run_rollup / _device)
against the model + oracle expectation of tests/rollup_model.py.

Bit-exact where the data is integer-valued with |sums| < 2^53 (every sum is
exact, so any order gives the reference's bits); the pure 1e-12 relative bound
otherwise — the float cases hold non-negative sums, so no contribution floor
applies and no point is excluded from any comparison.
"""
import ctypes as C

import numpy as np
import pytest

from opentsdb_amd import abi, core
from opentsdb_amd.batch import HostBatch, groups_from_ids
from opentsdb_amd.engine import (DataPoints, DeviceBatch, DeviceResult, Engine,
                                 run_rollup_device)
from oracle import pyoracle
from tests import datasets, kat, rollup_model as RM
from tests.test_gpu_parity import compare

pytestmark = pytest.mark.gpu

T0 = datasets.T0
MIN = 60000
A = core.Aggregators


@pytest.fixture(scope="module")
def engine():
    from opentsdb_amd import build
    build.build()
    e = Engine(0)
    yield e
    e.close()


# ------------------------------------------------------------------ helpers
def mkspec(agg, ds, start, end, rate=False, ro=None, interp=None, tz=None,
           cover=None):
    d = core.DownsamplingSpecification(ds)
    if tz:
        d.setTimezone(tz)
    return core.make_spec(start, end, A.get(agg), d, start, end, rate, ro,
                          interp, cal_cover_ms=cover)


def mkbatch(series, gid=None, n_groups=None, layout="is_float"):
    """series: [(ts, bits, is_float)] arrays per series.  layout: how the
    value types reach the engine — per-point is_float, series_float (each
    series of one type), "double" (no type arrays: all doubles)."""
    offs = np.zeros(len(series) + 1, np.int64)
    np.cumsum([len(s[0]) for s in series], out=offs[1:])
    cat = lambda k, dt: (np.concatenate([np.asarray(s[k], dt) for s in series])
                         if series else np.zeros(0, dt))  # noqa: E731
    ts, val, isf = cat(0, np.int64), cat(1, np.int64), cat(2, np.uint8)
    g_off = members = None
    if gid is not None:
        g_off, members = groups_from_ids(gid, n_groups)
    if layout == "is_float":
        return HostBatch(offs, ts, val, isf, None, g_off, members)
    if layout == "series_float":
        sf = np.array([int(s[2][0]) if len(s[2]) else 1 for s in series],
                      np.uint8)
        assert all((np.asarray(s[2]) == f).all() for s, f in zip(series, sf))
        return HostBatch(offs, ts, val, None, sf, g_off, members)
    assert layout == "double" and (isf == 1).all()
    return HostBatch(offs, ts, val, None, None, g_off, members)


def ints(rng, n, lo=0, hi=1000):
    """n long points: (bits, is_float)."""
    return rng.integers(lo, hi, n).astype(np.int64), np.zeros(n, np.uint8)


def dbl(v):
    v = np.asarray(v, np.float64)
    return v.view(np.int64), np.ones(len(v), np.uint8)


def regular(n, step, t0=T0, phase=0):
    return t0 + phase + step * np.arange(n, dtype=np.int64)


def run_device(engine, spec, hb, rollup, counts):
    import torch
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()  # noqa
    n = len(hb.ts)

    def col(x, dt):  # (never an empty allocation: the pointer must be real)
        buf = torch.zeros(max(n, 2), dtype=dt, device="cuda")
        if x is not None:
            buf[:n] = t(x)
        return buf[:n]
    db = DeviceBatch(t(hb.offsets), col(hb.ts, torch.int64),
                     col(hb.val, torch.int64), t(hb.group_offsets),
                     t(hb.group_members),
                     None if hb.is_float is None else col(hb.is_float,
                                                          torch.uint8),
                     None if hb.series_float is None else t(hb.series_float))
    dc = None if counts is None else col(counts, torch.int64)
    cap = max(1, int(engine.plan(spec, hb).max_out_points))
    res = DeviceResult(torch, hb.n_groups, cap, "cuda")
    run_rollup_device(engine, spec, db, rollup, dc, res)
    torch.cuda.synchronize()
    offs = res.offsets.cpu().numpy()
    ts, val, ii = (res.ts.cpu().numpy(), res.val.cpu().numpy(),
                   res.is_int.cpu().numpy())
    return [DataPoints(ts[offs[g]:offs[g + 1]], val[offs[g]:offs[g + 1]],
                       ii[offs[g]:offs[g + 1]]) for g in range(hb.n_groups)]


def same_bits(a, b, where=""):
    assert len(a) == len(b), where
    for g, (x, y) in enumerate(zip(a, b)):
        w = "%s/g%d" % (where, g)
        assert np.array_equal(x.ts, y.ts), w
        assert np.array_equal(x.bits, y.bits), w
        assert np.array_equal(x.is_int, y.is_int), w


def check(engine, spec, hb, kind, counts, exact, where="", device=True):
    """Both entries against the model + oracle expectation."""
    ref = RM.expect_query(spec, kind, hb, counts)
    got = engine.run_rollup(spec, hb, kind, counts)
    compare(got, ref, exact, where + "/host")
    for g in got:
        assert not g.is_int.any(), where + ": output points are doubles"
    if device:
        same_bits(run_device(engine, spec, hb, kind, counts), got,
                  where + "/device")
    return got


def count_of(rng, n, kind):
    return rng.integers(1, 50, n).astype(np.int64) if kind == RM.AVG else None


# 1 ------------------------------------------------------------------- KATs
@pytest.mark.parametrize("c", RM.load_kats(), ids=lambda c: c["name"])
def test_reference_rollup_kat(engine, c):
    """Every transcribed rollup test through both entries: the KAT's points
    where the one-span query yields the lone view's own points (the model +
    oracle expectation reproduces them), and that expectation elsewhere (a
    filling grid ends with the iterator's window, kat.view_as_query)."""
    spec, batch, counts = RM.kat_query(c)
    rollup = c["rollup_agg"]
    if "error" in c:
        with pytest.raises(core.UnsupportedOperationException):
            engine.run_rollup(spec, batch, rollup, counts)
        cnt = np.ascontiguousarray(counts)
        b, r = batch.as_abi(), abi.Result()
        assert engine.lib.otsdb_agg_run_rollup(
            engine.ctx, C.byref(spec), C.byref(b), A.get(rollup).id,
            cnt.ctypes.data, C.byref(r)) == abi.E_UNSUPPORTED
        return
    got = engine.run_rollup(spec, batch, rollup, counts)
    dev = run_device(engine, spec, batch, rollup, counts)
    same_bits(dev, got, c["name"])
    kind = RM.kat_kind(c)
    if kind is None:  # the ordinary function: the single query, bit for bit
        same_bits(got, engine.run(spec, batch), c["name"])
        ref = pyoracle.group_by(spec, batch)
    else:
        ref = RM.expect_query(spec, kind, batch, counts)
    compare(got, ref, True, c["name"])
    pts = np.zeros(len(got[0].ts), pyoracle.POINT)
    pts["ts"], pts["bits"], pts["is_int"] = got[0].ts, got[0].bits, \
        got[0].is_int
    exp = c["expect"]
    try:
        kat.check_points(ref[0], exp, c["tol"], c["name"])
    except AssertionError:
        return  # the query differs from the lone view: held to `ref` above
    kat.check_points(pts, exp, c["tol"], c["name"])


# 2 ----------------------------------------------------------------- shapes
SHAPES = [
    # (name, points per series, point step ms, downsampler interval)
    ("n1", [1], 10000, "1m"), ("n7", [7], 10000, "1m"),
    ("n8", [8], 10000, "1m"), ("n9", [9], 10000, "1m"),
    ("n511", [511], 10000, "1m"), ("n512", [512], 10000, "1m"),
    ("n513", [513], 10000, "1m"), ("n1025", [1025], 10000, "1m"),
    ("one_a_bucket", [100, 513], 60000, "1m"),   # fold_lane: 8 buckets a lane
    ("two_a_bucket", [100, 513], 30000, "1m"),   # ... 4 buckets a lane
    ("b17", [600, 1025], 10000, "170s"),         # buckets spanning lanes
    ("b600", [1300, 2000], 1000, "10m"),         # ... and a step
    ("all", [513, 9, 1025], 10000, "0all"),
    ("ring_700_buckets", [1400, 701], 30000, "1m"),  # 256-bucket ring flushes
]
FILLS = [("none", None), ("none", core.Interpolation.ZIM), ("zero", None),
         ("nan", None)]


def aligned_up(t, iv_ms):
    return (t + iv_ms - 1) // iv_ms * iv_ms


def _shape_series(rng, kind, n, step, t0, phase):
    ts = regular(n, step, t0=t0, phase=phase)
    keep = rng.random(n) > 0.03 if n > 9 else np.ones(n, bool)
    ts = ts[keep]
    bits, isf = ints(rng, len(ts))
    return (ts, bits, isf), count_of(rng, len(ts), kind)


@pytest.mark.parametrize("kind", [RM.AVG, RM.COUNT])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: s[0])
def test_shapes(engine, shape, kind):
    name, ns, step, iv = shape
    rng = np.random.default_rng(100 + [s[0] for s in SHAPES].index(name))
    series, cnts = [], []
    # (the oracle route needs the window's start on a bucket boundary)
    start = T0 if iv == "0all" else aligned_up(
        T0, core.DateTime.parseDuration(iv))
    for i, n in enumerate(ns):
        s, c = _shape_series(rng, kind, n, step, start,
                             phase=(i * 3000) % step)
        series.append(s)
        cnts.append(c)
    hb = mkbatch(series)
    counts = np.concatenate(cnts) if kind == RM.AVG else None
    end = start + max(ns) * step + 5 * MIN
    for fill, interp in FILLS:
        if iv == "0all" and fill != "none":
            continue
        spec = mkspec("sum", "%s-%s-%s" % (iv, kind, fill), start, end,
                      interp=interp)
        check(engine, spec, hb, kind, counts, True,
              "%s/%s/%s/%s" % (name, kind, fill, interp),
              device=(fill == "none" and interp is None))


@pytest.mark.parametrize("kind", [RM.AVG, RM.COUNT])
def test_outage_and_points_outside_the_window(engine, kind):
    """An outage of 1,000 empty buckets (wider than the ring), a series
    whose only points lie past the window, one with none inside it (before
    and after), and an empty one."""
    rng = np.random.default_rng(5)
    end = T0 + 1200 * MIN
    a = np.concatenate([regular(300, 10000), regular(300, 10000,
                                                     t0=T0 + 1050 * MIN)])
    past = regular(40, 10000, t0=end + 3 * MIN)
    around = np.concatenate([regular(20, 10000, t0=T0 - 10 * MIN),
                             regular(20, 10000, t0=end + 2 * MIN)])
    series, cnts = [], []
    for ts in (a, past, around, np.zeros(0, np.int64), regular(50, 10000)):
        bits, isf = ints(rng, len(ts))
        series.append((ts, bits, isf))
        cnts.append(rng.integers(1, 9, len(ts)).astype(np.int64))
    counts = np.concatenate(cnts) if kind == RM.AVG else None
    for gid in ([0, 0, 0, 0, 0], [0, 1, 2, 3, 4]):
        hb = mkbatch(series, gid, max(gid) + 1)
        for fill, interp in FILLS:
            spec = mkspec("sum", "1m-%s-%s" % (kind, fill), T0, end,
                          interp=interp)
            check(engine, spec, hb, kind, counts, True,
                  "outage/%s/%s/%s" % (fill, interp, gid), device=False)


@pytest.mark.parametrize("kind", [RM.AVG, RM.COUNT])
@pytest.mark.parametrize("off", [1, 29999, 59999])
def test_unaligned_start_single_series(engine, kind, off):
    """A start inside a bucket: the seek rounds up, the cut bucket's points
    are dropped.  Against the model alone (one series, sum across it)."""
    rng = np.random.default_rng(off)
    ts = regular(700, 7000, t0=T0 - 5 * MIN)
    bits, isf = ints(rng, len(ts))
    counts = count_of(rng, len(ts), kind)
    hb = mkbatch([(ts, bits, isf)])
    spec = mkspec("sum", "1m-%s" % kind, T0 + off, T0 + 60 * MIN + off)
    exp = RM.expect_single(spec, kind, hb, counts)
    assert len(exp) == 60
    got = engine.run_rollup(spec, hb, kind, counts)[0]
    assert list(got.ts) == [t for t, _ in exp]
    assert np.array_equal(got.bits.view(np.float64),
                          np.array([v for _, v in exp]))
    same_bits(run_device(engine, spec, hb, kind, counts), [got])


# 3 ----------------------------------------------------------------- counts
def _count_case(cnt_rows, val_rows, fill="none", step=20000):
    """One series, three points a 1m bucket: row r holds bucket r's counts
    (None: the bucket has no points)."""
    ts, cnt, val = [], [], []
    for r, row in enumerate(cnt_rows):
        if row is None:
            continue
        for j, c in enumerate(row):
            ts.append(T0 + r * MIN + j * step)
            cnt.append(c)
            val.append(val_rows[r][j])
    bits, isf = np.array(val, np.int64), np.zeros(len(val), np.uint8)
    hb = mkbatch([(np.array(ts, np.int64), bits, isf)])
    spec = mkspec("sum", "1m-avg-%s" % fill, T0, T0 + len(cnt_rows) * MIN)
    return spec, hb, np.array(cnt, np.int64)


@pytest.mark.parametrize("fill", ["none", "zero", "nan"])
def test_zero_total_count_is_a_present_zero(engine, fill):
    """Counts totalling 0 (zeros, and +/- pairs): a real 0.0 point, alone and
    next to absent buckets."""
    spec, hb, cnt = _count_case(
        [[0, 0, 0], None, [5, -5, 0], None, None, [1, 2, 3], [0, 0, 0]],
        [[7, 8, 9], None, [1, 2, 3], None, None, [6, 6, 6], [4, 4, 4]], fill)
    got = check(engine, spec, hb, RM.AVG, cnt, True, "zero_count/" + fill)
    v = dict(zip(got[0].ts.tolist(), got[0].bits.view(np.float64).tolist()))
    assert v[T0] == 0.0 and v[T0 + 2 * MIN] == 0.0
    assert v[T0 + 5 * MIN] == 3.0
    if fill == "none":
        assert T0 + MIN not in v and T0 + 3 * MIN not in v
    elif fill == "zero":
        assert v[T0 + MIN] == 0.0
    else:
        assert np.isnan(v[T0 + MIN])


def test_negative_and_wide_counts(engine):
    """Negative counts; two counts of 2^31 in one bucket (a 32-bit state
    fails here); totals past 2^53; totals that wrap 2^63 (and on to 0)."""
    rows = [[-3, -4, -5], [2 ** 31, 2 ** 31, 0], [2 ** 31, 2 ** 31, 2 ** 31],
            [2 ** 53, 2 ** 53, 3], [2 ** 62, 2 ** 62, 0],
            [2 ** 62, 2 ** 62, 2 ** 63 - 1], [-2 ** 63, -2 ** 63, 0],
            [2 ** 63 - 1, 1, 5]]
    vals = [[10, 20, 30]] * len(rows)
    for fill in ("none", "zero"):
        spec, hb, cnt = _count_case(rows, vals, fill)
        got = check(engine, spec, hb, RM.AVG, cnt, True, "wide/" + fill)
        v = got[0].bits.view(np.float64)
        assert v[0] == 60.0 / -12.0
        assert v[1] == 60.0 / 2.0 ** 32
        assert v[4] == 60.0 / -2.0 ** 63      # 2^62 + 2^62 wraps
        assert v[6] == 0.0                    # -2^63 - 2^63 wraps to 0
        assert v[7] == 60.0 / float(-2 ** 63 + 5)


def test_wide_counts_across_lanes_and_steps(engine):
    """Counts of 2^31 and 2^61 in buckets that span lanes and steps: the
    wave scan and the step carry keep 64 bits and wrap like the long."""
    rng = np.random.default_rng(3)
    n = 1300
    start = aligned_up(T0, 17000 * 600)  # on both grids
    ts = regular(n, 1000, t0=start)
    bits, isf = ints(rng, n)
    hb = mkbatch([(ts, bits, isf)])
    for big in (2 ** 31, 2 ** 61):
        cnt = np.full(n, big, np.int64)
        for iv in ("17s", "10m"):
            spec = mkspec("sum", iv + "-avg", start, start + 30 * MIN)
            check(engine, spec, hb, RM.AVG, cnt, True, "lanes/%s/%d" % (iv, big))


# 4 ----------------------------------------------------------------- values
def _typed_series(rng, layout, n_series=6, n=300):
    series = []
    for s in range(n_series):
        ts = regular(n, 10000, phase=int(rng.integers(0, 10000)))
        if layout == "long":
            bits, isf = ints(rng, n, -500, 500)
        elif layout == "double":
            bits, isf = dbl(rng.integers(-500, 500, n).astype(np.float64))
        elif layout == "series_float":
            bits, isf = (ints(rng, n, -500, 500) if s % 2 else
                         dbl(rng.integers(-500, 500, n).astype(np.float64)))
        else:  # per-point
            f = rng.random(n) < 0.5
            iv = rng.integers(-500, 500, n)
            bits = np.where(f, iv.astype(np.float64).view(np.int64), iv)
            isf = f.astype(np.uint8)
        series.append((ts, bits, isf))
    return series


@pytest.mark.parametrize("kind", [RM.AVG, RM.COUNT])
@pytest.mark.parametrize("layout", ["long", "is_float", "series_float",
                                    "double"])
def test_value_layouts(engine, layout, kind):
    rng = np.random.default_rng(17)
    series = _typed_series(rng, layout)
    hb = mkbatch(series, [0, 0, 0, 1, 1, 2], 3,
                 {"long": "series_float"}.get(layout, layout))
    counts = count_of(rng, len(hb.ts), kind)
    for fill in ("none", "nan"):
        spec = mkspec("sum", "1m-%s-%s" % (kind, fill), T0, T0 + 55 * MIN)
        check(engine, spec, hb, kind, counts, True,
              "%s/%s/%s" % (layout, kind, fill))


@pytest.mark.parametrize("kind", [RM.AVG, RM.COUNT])
def test_nan_and_signed_zero_cells(engine, kind):
    """A NaN sum cell: the bucket is NaN and PRESENT (not the absent
    sentinel: fill zero must not replace it, LERP reads it).  -0.0 cells sum
    to +0.0 (the sums start at +0.0)."""
    v = np.array([1.0, np.nan, 2.0,   # bucket 0: NaN
                  -0.0, -0.0, -0.0,   # bucket 1: 0.0
                  4.0, 5.0, 6.0,      # bucket 2
                  np.nan, np.nan, np.nan,
                  0.0, -0.0, 3.0], np.float64)
    ts = np.array([T0 + (i // 3) * MIN + (i % 3) * 20000 for i in range(15)],
                  np.int64)
    ts[12:] += 2 * MIN  # buckets 4, 5 absent, bucket 6 real
    other = (regular(42, 10000), *dbl(np.arange(42, dtype=np.float64)))
    counts = (np.arange(1, 16 + 42, dtype=np.int64) if kind == RM.AVG
              else None)
    for layout in ("is_float", "double"):
        hb = mkbatch([(ts, *dbl(v)), other], [0, 0], 1, layout)
        for fill in ("none", "zero", "nan"):
            for agg in ("sum", "max"):
                spec = mkspec(agg, "1m-%s-%s" % (kind, fill), T0, T0 + 7 * MIN)
                check(engine, spec, hb, kind, counts, True,
                      "nan/%s/%s/%s" % (layout, fill, agg))
    # alone: the NaN buckets are emitted as points
    hb = mkbatch([(ts, *dbl(v))])
    c1 = None if counts is None else counts[:15]
    spec = mkspec("sum", "1m-%s-zero" % kind, T0, T0 + 7 * MIN)
    got = check(engine, spec, hb, kind, c1, True, "nan/alone")[0]
    out = got.bits.view(np.float64)
    assert np.isnan(out[0]) and np.isnan(out[3])
    assert out[1] == 0.0 and not np.signbit(out[1])
    assert out[4] == 0.0 and out[5] == 0.0  # filled


@pytest.mark.parametrize("ek", ["signed", "wide", "f4edge"])
@pytest.mark.parametrize("kind", [RM.AVG, RM.COUNT])
def test_edge_values_non_negative(engine, ek, kind):
    """datasets.edge_values restricted to non-negative finite doubles (up to
    1e300: a bucket's sum stays finite): the 1e-12 relative bound with no
    floor (a sum of non-negative terms has no cancellation), every point
    compared."""
    rng = np.random.default_rng(23)
    series = []
    for s in range(5):
        n = 400
        bits, _ = datasets.edge_values(ek, rng, 8 * n)
        v = bits.view(np.float64)
        v = v[np.isfinite(v) & (v >= 0.0) & (v <= 1e300)][:n]
        assert len(v) == n
        series.append((regular(n, 10000, phase=1000 * s), *dbl(v)))
    hb = mkbatch(series, [0, 0, 1, 1, 1], 2)
    counts = count_of(rng, len(hb.ts), kind)
    spec = mkspec("max", "2m-%s" % kind, T0, T0 + 70 * MIN)
    check(engine, spec, hb, kind, counts, False, "edge/%s/%s" % (ek, kind))


# 5 ------------------------------------------------------------- downstream
def _grouped(rng, kind, n=360, step=10000, value="int", t0=T0,
             sizes=(1, 5, 40)):
    """3 groups of 1, 5 and 40 members, some series late, short or gappy."""
    series = []
    for s in range(sum(sizes)):
        ts = regular(n, step, t0=t0, phase=int(rng.integers(0, step)))
        keep = rng.random(n) > 0.1
        if s % 7 == 3:
            keep[:n // 3] = False
        if s % 11 == 5:
            keep[n // 2:n // 2 + 60] = False
        ts = ts[keep]
        if value == "int":
            bits, isf = ints(rng, len(ts))
        else:
            bits, isf = dbl(rng.random(len(ts)) * 100.0)
        series.append((ts, bits, isf))
    gid = [g for g, k in enumerate(sizes) for _ in range(k)]
    hb = mkbatch(series, gid, len(sizes))
    return hb, count_of(rng, len(hb.ts), kind)


@pytest.mark.parametrize("kind", [RM.AVG, RM.COUNT])
@pytest.mark.parametrize("agg", ["sum", "avg", "min", "max", "dev", "count",
                                 "p99", "median"])
def test_cross_series_aggregators(engine, agg, kind):
    hb, counts = _grouped(np.random.default_rng(31), kind)
    # integer data: every bucket sum is exact, so the rows are the model's
    # bits; sum / min / max / count / selections of them are order-free or
    # exact, avg / dev run in the reference's member order (groups <= 256)
    spec = mkspec(agg, "1m-%s" % kind, T0, T0 + 50 * MIN)
    check(engine, spec, hb, kind, counts, True, "agg/%s/%s" % (agg, kind))


@pytest.mark.parametrize("kind", [RM.AVG, RM.COUNT])
def test_float_sums_within_1e12(engine, kind):
    hb, counts = _grouped(np.random.default_rng(37), kind, value="float")
    for agg, fill in (("sum", "none"), ("avg", "nan"), ("max", "zero")):
        spec = mkspec(agg, "1m-%s-%s" % (kind, fill), T0, T0 + 50 * MIN)
        check(engine, spec, hb, kind, counts, False,
              "float/%s/%s" % (agg, fill), device=False)


@pytest.mark.parametrize("kind", [RM.AVG, RM.COUNT])
def test_mimmin_with_a_member_missing(engine, kind):
    rng = np.random.default_rng(41)
    series = []
    for s in range(4):
        ts = regular(300, 10000, phase=1000 * s)
        if s == 2:
            ts = np.concatenate([ts[:60], ts[200:]])  # missing 10 m .. 33 m
        if s == 3:
            ts = ts[150:]
        series.append((ts, *ints(rng, len(ts))))
    hb = mkbatch(series, [0, 0, 0, 0], 1)
    counts = count_of(rng, len(hb.ts), kind)
    for agg in ("mimmin", "mimmax", "zimsum"):
        spec = mkspec(agg, "1m-%s" % kind, T0, T0 + 50 * MIN)
        check(engine, spec, hb, kind, counts, True, "mim/%s" % agg)


@pytest.mark.parametrize("kind", [RM.AVG, RM.COUNT])
@pytest.mark.parametrize("fill", ["none", "zero"])
def test_rate_and_counter_rate(engine, kind, fill):
    """RateSpan over the rollup buckets (k_transform's, never the fused
    ring): plain rate, and a counter whose bucket values reset once."""
    rng = np.random.default_rng(43)
    series = []
    for s in range(7):
        n = 330
        ts = regular(n, 10000, phase=int(rng.integers(0, 10000)))
        v = np.cumsum(rng.integers(0, 50, n)) + 1000
        v[n // 2:] -= v[n // 2] - 3  # a reset
        keep = np.ones(n, bool)
        if s == 4:
            keep[60:200] = False
        series.append((ts[keep], v[keep].astype(np.int64),
                       np.zeros(int(keep.sum()), np.uint8)))
    # a series whose points all lie past the window (rates beyond it)
    ts = regular(40, 10000, t0=T0 + 52 * MIN)
    series.append((ts, np.arange(40, dtype=np.int64) * 7,
                   np.zeros(40, np.uint8)))
    hb = mkbatch(series, [0, 0, 0, 1, 1, 1, 2, 2], 3)
    # equal counts in a bucket keep the avg buckets a rising counter
    counts = (np.full(len(hb.ts), 2, np.int64) if kind == RM.AVG else None)
    for ro in (None, core.RateOptions(True, 2 ** 20, 0, False),
               core.RateOptions(True, 2 ** 20, 0, True)):
        spec = mkspec("sum", "1m-%s-%s" % (kind, fill), T0, T0 + 50 * MIN,
                      rate=True, ro=ro)
        check(engine, spec, hb, kind, counts, True,
              "rate/%s/%s/%s" % (kind, fill, ro is not None), device=False)


@pytest.mark.parametrize("kind", [RM.AVG, RM.COUNT])
def test_calendar_grid(engine, kind):
    """One 1dc grid (America/Denver across the spring change)."""
    t0 = 1362870000000  # 2013-03-09 23:00 UTC
    rng = np.random.default_rng(47)
    series = []
    for s in range(5):
        ts = regular(700, 600000, t0=t0, phase=int(rng.integers(0, 600000)))
        series.append((ts, *ints(rng, len(ts))))
    hb = mkbatch(series, [0, 0, 1, 1, 1], 2)
    counts = count_of(rng, len(hb.ts), kind)
    for fill in ("none", "nan"):
        spec = mkspec("sum", "1dc-%s-%s" % (kind, fill), t0 + 3600000,
                      t0 + 4 * 86400000, tz="America/Denver",
                      cover=int(hb.ts.max()))
        assert spec.use_calendar and spec.n_cal_anchors == 0
        check(engine, spec, hb, kind, counts, True, "cal/%s/%s" % (kind, fill))


@pytest.mark.parametrize("kind", [RM.AVG, RM.COUNT])
def test_window_end_inside_a_bucket(engine, kind):
    """The window ends inside a bucket with points after it: the bucket past
    the window (k_prep's, a rollup value too) is what LERP reads at the last
    emitted timestamps."""
    rng = np.random.default_rng(53)
    a = regular(400, 10000)                       # on through the end
    b = np.concatenate([regular(100, 10000, phase=5000),
                        regular(60, 10000, t0=T0 + 43 * MIN)])  # gap over end
    series = [(a, *ints(rng, len(a))), (b, *ints(rng, len(b)))]
    hb = mkbatch(series, [0, 0], 1)
    counts = count_of(rng, len(hb.ts), kind)
    end = T0 + 40 * MIN + 25000
    for agg in ("sum", "max"):
        spec = mkspec(agg, "1m-%s" % kind, T0, end)
        got = check(engine, spec, hb, kind, counts, True,
                    "end/%s/%s" % (kind, agg))
        assert got[0].ts[-1] == T0 + 40 * MIN


# 6 ------------------------------------------------------------ equivalences
# Engine.run takes the ordered fold where a rollup call takes the row path:
# the two feed a group's members to the aggregator in the same order only
# while the group is one fold tile (32 members), so that is where "bit for
# bit" can hold between them (a sum over interpolated, non-integer
# contributions depends on its order; larger groups are held to the
# reference above, as Engine.run's are in test_gpu_parity).
EQ_SIZES = (1, 5, 30)


def test_counts_of_one_equal_ds_avg(engine):
    hb, _ = _grouped(np.random.default_rng(59), RM.COUNT, sizes=EQ_SIZES)
    ones = np.ones(len(hb.ts), np.int64)
    for agg, fill in (("sum", "none"), ("max", "nan"), ("avg", "zero")):
        spec = mkspec(agg, "1m-avg-%s" % fill, T0, T0 + 50 * MIN)
        same_bits(engine.run_rollup(spec, hb, "avg", ones),
                  engine.run(spec, hb), "ones/%s" % agg)


def test_rollup_count_equals_ds_sum(engine):
    hb, _ = _grouped(np.random.default_rng(61), RM.COUNT, sizes=EQ_SIZES)
    for agg, fill in (("sum", "none"), ("max", "nan")):
        got = engine.run_rollup(
            mkspec(agg, "1m-count-%s" % fill, T0, T0 + 50 * MIN), hb, "count")
        ref = engine.run(mkspec(agg, "1m-sum-%s" % fill, T0, T0 + 50 * MIN),
                         hb)
        same_bits(got, ref, "count/%s" % agg)


@pytest.mark.parametrize("f", ["sum", "min", "max"])
def test_ordinary_functions_are_the_single_query(engine, f):
    hb, _ = _grouped(np.random.default_rng(67), RM.COUNT)
    junk = np.full(len(hb.ts), -7, np.int64)
    spec = mkspec("sum", "1m-%s" % f, T0, T0 + 50 * MIN)
    ref = engine.run(spec, hb)
    same_bits(engine.run_rollup(spec, hb, f, junk), ref, f)
    same_bits(engine.run_rollup(spec, hb, f, None), ref, f)
    same_bits(run_device(engine, spec, hb, f, None), ref, f)
    # ... and R = sum with F = avg (the reference's own tests pair them)
    spec = mkspec("sum", "1m-avg", T0, T0 + 50 * MIN)
    same_bits(engine.run_rollup(spec, hb, "sum", junk), engine.run(spec, hb))


# 7 ----------------------------------------------------------------- status
def _raw_call(engine, spec, hb, rollup_id, counts, cap=None):
    G = hb.n_groups
    cap = int(engine.plan(spec, hb).max_out_points) if cap is None else cap
    offs = np.full(G + 1, -1, np.int64)
    ts, bits = np.zeros(max(cap, 1), np.int64), np.zeros(max(cap, 1), np.int64)
    ii = np.zeros(max(cap, 1), np.uint8)
    r = abi.Result(cap, offs.ctypes.data, ts.ctypes.data, bits.ctypes.data,
                   ii.ctypes.data)
    b = hb.as_abi()
    st = engine.lib.otsdb_agg_run_rollup(
        engine.ctx, C.byref(spec), C.byref(b), rollup_id,
        None if counts is None else counts.ctypes.data, C.byref(r))
    return st, offs


def test_status_codes(engine):
    hb, _ = _grouped(np.random.default_rng(71), RM.COUNT, n=60)
    cnt = np.ones(len(hb.ts), np.int64)
    avg, mx, dev = A.AVG.id, A.MAX.id, A.DEV.id
    ok = mkspec("sum", "1m-avg", T0, T0 + 9 * MIN)
    assert _raw_call(engine, ok, hb, avg, cnt)[0] == abi.OK
    assert _raw_call(engine, ok, hb, dev, cnt)[0] == abi.E_UNSUPPORTED
    assert _raw_call(engine, mkspec("sum", "1m-dev", T0, T0 + 9 * MIN), hb,
                     dev, cnt)[0] == abi.E_UNSUPPORTED
    assert _raw_call(engine, mkspec("sum", "1m-max", T0, T0 + 9 * MIN), hb,
                     avg, cnt)[0] == abi.E_UNSUPPORTED
    assert _raw_call(engine, ok, hb, avg, None)[0] == abi.E_ILLEGAL_ARGUMENT
    assert _raw_call(engine, ok, hb, 99, cnt)[0] == abi.E_NO_SUCH_ELEMENT
    raw = core.make_spec(T0, T0 + 9 * MIN, A.SUM)
    assert engine.lib.otsdb_agg_run_rollup(
        engine.ctx, C.byref(raw), C.byref(hb.as_abi()), avg, cnt.ctypes.data,
        C.byref(abi.Result())) == abi.E_UNSUPPORTED
    ts = 1362614400000 + 3600000  # (a 7-minute calendar grid: per series)
    anch = core.make_spec(ts, ts + 23 * 3600000, A.SUM,
                          core.DownsamplingSpecification("7mc-avg"), ts,
                          ts + 23 * 3600000)
    assert anch.n_cal_anchors > 0
    assert engine.lib.otsdb_agg_run_rollup(
        engine.ctx, C.byref(anch), C.byref(hb.as_abi()), avg,
        cnt.ctypes.data, C.byref(abi.Result())) == abi.E_UNSUPPORTED


@pytest.mark.parametrize("kind", [RM.AVG, RM.COUNT])
def test_capacity_miss_fills_the_offsets(engine, kind):
    hb, counts = _grouped(np.random.default_rng(73), kind, n=120)
    spec = mkspec("sum", "1m-%s" % kind, T0, T0 + 15 * MIN)
    full = engine.run_rollup(spec, hb, kind, counts)
    total = sum(len(g.ts) for g in full)
    assert total > 8
    st, offs = _raw_call(engine, spec, hb, A.get(kind).id, counts, cap=8)
    assert st == abi.E_CAPACITY
    assert list(offs) == list(np.cumsum([0] + [len(g.ts) for g in full]))


def test_a_single_query_after_a_rollup_call_is_unaffected(engine):
    """The context's rollup state ends with the call, errors included, and
    the "error word known zero" mark holds across the entries."""
    hb, counts = _grouped(np.random.default_rng(79), RM.AVG, n=120)
    spec = mkspec("sum", "1m-avg", T0, T0 + 15 * MIN)
    ref = engine.run(spec, hb)
    for call in (lambda: engine.run_rollup(spec, hb, "avg", counts),
                 lambda: _raw_call(engine, spec, hb, A.AVG.id, counts, cap=8),
                 lambda: _raw_call(engine, spec, hb, A.DEV.id, counts)):
        call()
        same_bits(engine.run(spec, hb), ref)
        same_bits(engine.run(spec, hb), ref)
    # Infinity in a rollup call reports, and the next call starts clean
    big = mkbatch([(regular(6, 10000), *dbl(np.full(6, 1.7e308)))])
    with pytest.raises(core.IllegalStateException):
        engine.run_rollup(mkspec("sum", "1m-count", T0, T0 + 2 * MIN), big,
                          "count")
    same_bits(engine.run(spec, hb), ref)
    got = engine.run_rollup(spec, hb, "avg", counts)
    compare(got, RM.expect_query(spec, RM.AVG, hb, counts), False)
