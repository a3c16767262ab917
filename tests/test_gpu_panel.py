"""Panel queries (otsdb_agg_run_panel*): sub-queries that differ in the
downsampling function as well as in the aggregator; the envelope functions
(sum, avg, count, min, max and their aliases) are reduced from ONE pass over
the point stream.  Needs an MI355X.

Every output i of a panel call is checked
 (a) against the CPU oracle run with its own downsampler and aggregator:
     bit-exact where both are order-free, 1e-12 relative otherwise (diff:
     cancel_floor) — the rule of the single-query tests;
 (b) bit for bit against engine.run_multi(spec with ds_i, [agg_i, agg_i])[0],
     the existing row path with that function: the envelope kernel's row
     contract;
 (c) where the function is min / max / count, bit for bit against engine.run.
Engine.panel_counters() shows what was shared.
"""
import ctypes as C

import numpy as np
import pytest

from opentsdb_amd import abi, core
from opentsdb_amd.batch import HostBatch, groups_from_ids
from opentsdb_amd.engine import Engine, run_panel_device
from oracle import pyoracle
from tests import datasets
from tests.test_gpu_multi import (_device_batch, _device_results, _points,
                                  same_bits, with_agg)
from tests.test_gpu_parity import ORDER_FREE, _spec, cancel_floor, compare

pytestmark = pytest.mark.gpu

T0 = datasets.T0
HOUR = 3600 * 1000
EXACT_DS = {"min", "max", "mimmin", "mimmax", "count"}
SELECTIONS = {"median", "p50", "p75", "p90", "p95", "p99", "p999"}
ENVELOPE = [("min", "min"), ("avg", "avg"), ("max", "max")]
ALL_FIVE = ENVELOPE + [("sum", "sum"), ("count", "count")]


@pytest.fixture(scope="module")
def engine():
    from opentsdb_amd import build
    build.build()
    e = Engine(0)
    yield e
    e.close()


def with_query(spec, q):
    s = with_agg(spec, q[0], q[2] if len(q) > 2 else None)
    s.ds_agg_id = core.Aggregators.get(q[1]).id
    return s


def check_outputs(engine, spec, queries, batch, got, where, floor=0.0,
                  rows=True, rate=False):
    """(a), (b) and (c) for every output of a panel call.  rows=False: the
    query's multi call shares no rows (per-series calendar anchors); rate:
    the values are quotients, held to 1e-12."""
    assert len(got) == len(queries)
    for i, q in enumerate(queries):
        agg, ds = q[0], q[1]
        si = with_query(spec, q)
        w = "%s/%d:%s-%s" % (where, i, agg, ds)
        exact = not rate and ds in EXACT_DS and (agg in ORDER_FREE or
                                                 agg in SELECTIONS)
        fl = floor + (cancel_floor(batch, 2) if agg == "diff" else 0.0)
        compare(got[i], pyoracle.group_by(si, batch), exact, w, fl)
        if rows:
            it = None if len(q) < 3 else [q[2], q[2]]
            same_bits(got[i], engine.run_multi(si, [agg, agg], batch, it)[0],
                      w + "/rows")
        if ds in ("min", "max", "count"):
            same_bits(got[i], engine.run(si, batch), w + "/single")


def check_panel(engine, spec, queries, batch, where, floor=0.0, rows=True,
                rate=False):
    got = engine.run_panel(spec, queries, batch)
    c = engine.panel_counters()
    check_outputs(engine, spec, queries, batch, got, where, floor, rows, rate)
    return got, c


# 1 ------------------------------------------------ all five, with aliases
@pytest.mark.parametrize("kind", ["float", "int", "mixed"])
def test_all_functions_and_aliases(engine, kind):
    """float: 10 s buckets of 10 s points with 5 % NaNs — buckets holding
    only a NaN (sum NaN, count 0, min / max NaN)."""
    b = datasets.random_batch(23, n_series=30, n_groups=3, value_kind=kind,
                              nan_frac=0.05 if kind == "float" else 0)
    queries = ALL_FIVE + [("zimsum", "zimsum"), ("sum", "pfsum"),
                          ("mimmin", "mimmin"), ("mimmax", "mimmax"),
                          ("count", "avg"), ("p90", "max")]
    spec = _spec("sum", "avg", interval="10s" if kind == "float" else "1m")
    # integer data of both signs: mixed-sign sums (test_downsample_functions)
    fl = cancel_floor(b, 300) if kind != "float" else 0.0
    got, c = check_panel(engine, spec, queries, b, "all/" + kind, fl)
    assert c == dict(point_stream_passes=1, row_matrices=5), c
    if kind == "float":
        # one series alone in its group: its NaN-only buckets reach the output
        b1 = datasets.random_batch(29, n_series=1, n_groups=1, nan_frac=0.2,
                                   empty_frac=0, outside=False)
        q1 = [("sum", "sum"), ("sum", "count"), ("sum", "avg"),
              ("min", "min"), ("max", "max")]
        got, c = check_panel(engine, spec, q1, b1, "all/one-series")
        assert c == dict(point_stream_passes=1, row_matrices=5), c
        s, n = got[0][0].values(), got[1][0].values()
        assert np.isnan(s).any() and (n[np.isnan(s)] == 0).all()
        for i in (2, 3, 4):
            assert np.array_equal(np.isnan(got[i][0].values()), np.isnan(s))


# 2 ----------------------- bucket length against the lane and step shape
@pytest.mark.parametrize("interval", ["10s", "30s", "1m", "5m", "2h"])
def test_bucket_lengths(engine, interval):
    """10 s cadence: one point a bucket (fold_lane), three buckets a lane,
    a boundary in every lane (scan skipped), runs over three lanes, and
    720-point buckets whose carry crosses the 512-point steps."""
    span = 6 * HOUR if interval == "2h" else 3 * HOUR
    b = datasets.random_batch(31, n_series=20, n_groups=3, span_ms=span)
    spec = _spec("sum", "avg", interval=interval, end=T0 + span)
    _, c = check_panel(engine, spec, ALL_FIVE, b, "len/" + interval)
    assert c == dict(point_stream_passes=1, row_matrices=5), c


def test_run_all(engine):
    b = datasets.random_batch(61, n_series=20, n_groups=4)
    qs, qe = T0 + 600000, T0 + 7200000
    d = core.DownsamplingSpecification("0all-max")
    spec = core.make_spec(T0, T0 + 4 * HOUR, core.Aggregators.get("sum"), d,
                          qs, qe)
    _, c = check_panel(engine, spec, ALL_FIVE, b, "0all")
    assert c == dict(point_stream_passes=1, row_matrices=5), c


# 3 ---------------------------------------------------------------- ring edges
def _edge_batch():
    rng = np.random.default_rng(7)

    def series(t):
        return [(int(x), float(rng.random() * 100.0), 1) for x in t]
    step = 10000
    # a 1 h hole (360 buckets of 10 s: more than the ring's 256) between
    # points 100 and 101, inside the first 512-point step
    hole = series(np.concatenate([T0 + 3000 + step * np.arange(100),
                                  T0 + 3000 + step * (460 + np.arange(500))]))
    short = series(T0 + 1000 + step * np.arange(37))  # less than one step
    # three points before the window: the first kept point has index 3
    odd = series(T0 - 3 * step + 500 + step * np.arange(700))
    before = series(T0 - 2 * HOUR + step * np.arange(50))  # none in the window
    plain = series(T0 + 9000 + step * np.arange(1000))
    return HostBatch.from_groups([[hole, short, odd], [[], before, plain]])


@pytest.mark.parametrize("interval", ["10s", "1m"])
def test_ring_edges(engine, interval):
    """A gap wider than the ring inside one step (the direct path), short,
    empty and out-of-window series, an odd first index, a window that starts
    and ends off the grid."""
    b = _edge_batch()
    spec = _spec("sum", "avg", interval=interval, start=T0 + 7000,
                 end=T0 + 3 * HOUR - 3000)
    _, c = check_panel(engine, spec, ALL_FIVE, b, "edges/" + interval)
    assert c["point_stream_passes"] == 1, c


# 4 ------------------------------------------- fill, window, interpolation
@pytest.mark.parametrize("fill", ["nan", "zero", "null"])
@pytest.mark.parametrize("aligned", [True, False])
def test_fill_and_window(engine, fill, aligned):
    b = datasets.random_batch(31, n_series=25, n_groups=4, nan_frac=0.02)
    start = T0 + (0 if aligned else 61000)
    queries = ENVELOPE + [("sum", "count"), ("p99", "max"), ("count", "min")]
    _, c = check_panel(engine, _spec("sum", "max", fill, start=start),
                       queries, b, "fill/%s/%s" % (fill, aligned))
    assert c == dict(point_stream_passes=1, row_matrices=4), c


def test_interpolation_overrides(engine):
    """Several interpolation classes over one function's matrix, beside a
    second function (NONE fill: the series interpolate over their outages,
    toward the bucket past an unaligned window's end too)."""
    b = datasets.random_batch(41, n_series=30, n_groups=3)
    I = core.Interpolation
    queries = [("sum", "min", I.LERP), ("sum", "min", I.ZIM),
               ("sum", "min", I.PREV), ("max", "max", I.MAX),
               ("sum", "avg", I.MIN), ("zimsum", "avg"), ("first", "max")]
    for end in (T0 + 3 * HOUR, T0 + 2 * HOUR + 61000):
        got, c = check_panel(engine, _spec("sum", "min", end=end), queries, b,
                             "interp/%d" % end)
        assert c == dict(point_stream_passes=1, row_matrices=3), c
        assert engine.multi_counters()["downsample_passes"] == 1
        bits = [np.concatenate([np.asarray(g.bits) for g in got[i]])
                for i in range(3)]
        assert not np.array_equal(bits[0], bits[1])
        assert not np.array_equal(bits[0], bits[2])


# 5 ------------------------------------------------------------- calendar grid
DAY = 86400000
T_SPRING = 1362614400000  # 2013-03-07 00:00 UTC: spans the US spring-forward


def _cal_spec(ds, tz, start, end, batch):
    d = core.DownsamplingSpecification(ds)
    if tz:
        d.setTimezone(tz)
    return core.make_spec(start, end, core.Aggregators.get("sum"), d, start,
                          end, False, None, cal_cover_ms=int(batch.ts.max()))


def test_single_table_calendar(engine):
    b = datasets.random_batch(97, n_series=24, n_groups=3, span_ms=7 * DAY,
                              cadence_ms=600000, t0=T_SPRING)
    spec = _cal_spec("1dc-sum", "America/Denver", T_SPRING + HOUR,
                     T_SPRING + 6 * DAY, b)
    _, c = check_panel(engine, spec, ALL_FIVE, b, "1dc")
    assert c == dict(point_stream_passes=1, row_matrices=5), c


# 6 ----------------------------------------------------------------- group sizes
def test_group_sizes(engine):
    """One group of 300 members (tiles merged in order, selections through
    the key transpose) next to small ones; selections and dev as aggregators
    over envelope rows."""
    b = datasets.random_batch(71, n_series=330, span_ms=HOUR,
                              cadence_ms=30000, big_group=True)
    gid = np.zeros(330, np.int64)
    gid[300:] = 1 + np.arange(30) % 3
    g_off, members = groups_from_ids(gid, 4)
    b = HostBatch(b.offsets, b.ts, b.val, b.is_float, None, g_off, members)
    queries = [("p99", "max"), ("dev", "avg"), ("median", "min"),
               ("sum", "sum"), ("min", "min"), ("avg", "avg"), ("dev", "max")]
    _, c = check_panel(engine, _spec("sum", "avg", end=T0 + HOUR), queries, b,
                       "groups")
    assert c == dict(point_stream_passes=1, row_matrices=4), c


# 7 --------------------------------------------------------------------- routing
def test_mixed_request(engine):
    """p95 and dev downsampling beside envelope functions: one pass for the
    envelope functions, one per other function."""
    b = datasets.random_batch(27, n_series=24, n_groups=3, nan_frac=0.1)
    queries = ENVELOPE + [("p99", "p95"), ("sum", "dev"), ("max", "p95")]
    _, c = check_panel(engine, _spec("sum", "avg", interval="5m"), queries, b,
                       "mixed")
    assert c["point_stream_passes"] == 3, c
    assert c["row_matrices"] == 5, c


def test_rate_runs_function_by_function(engine):
    from tests.test_gpu_parity import RATES
    b = datasets.random_batch(52, n_series=30, n_groups=3, counter=True)
    spec = _spec("sum", "sum", rate=True, ro=RATES[1])
    queries = [("sum", "sum"), ("max", "max"), ("avg", "max")]
    got, c = check_panel(engine, spec, queries, b, "rate", rate=True)
    assert c["point_stream_passes"] == 2, c


def test_raw_group_by_ignores_the_functions(engine):
    b = datasets.random_batch(101, n_series=24, n_groups=4, cadence_ms=37000)
    raw = core.make_spec(T0, T0 + 3 * HOUR, core.Aggregators.get("sum"), None,
                         T0, T0 + 3 * HOUR)
    queries = [("sum", "min"), ("max", "avg"), ("p90", "max")]
    got = engine.run_panel(raw, queries, b)
    for i, q in enumerate(queries):
        si = with_agg(raw, q[0])
        compare(got[i], pyoracle.group_by(si, b),
                q[0] in ORDER_FREE or q[0] in SELECTIONS, "raw/" + q[0])
        same_bits(got[i], engine.run(si, b), "raw/single/" + q[0])


def test_anchored_calendar_runs_function_by_function(engine):
    b = datasets.random_batch(97, n_series=24, n_groups=3, span_ms=3 * DAY,
                              cadence_ms=60000, t0=T_SPRING)
    spec = _cal_spec("7mc-sum", None, T_SPRING + HOUR, T_SPRING + 2 * DAY, b)
    got = engine.run_panel(spec, ENVELOPE, b)
    c = engine.panel_counters()
    assert c["point_stream_passes"] == 3, c
    check_outputs(engine, spec, ENVELOPE, b, got, "7mc", rows=False)


def test_single_function_is_the_multi_call(engine):
    b = datasets.random_batch(11, n_series=60, n_groups=6)
    aggs = ["sum", "max", "p99", "dev"]
    got = engine.run_panel(_spec("min", "max"), [(a, "avg") for a in aggs], b)
    c = engine.panel_counters()
    assert c == dict(point_stream_passes=1, row_matrices=1), c
    want = engine.run_multi(_spec("sum", "avg"), aggs, b)
    for i, a in enumerate(aggs):
        same_bits(got[i], want[i], "onefn/" + a)


def test_duplicates(engine):
    b = datasets.random_batch(11, n_series=60, n_groups=6)
    queries = [("sum", "avg"), ("max", "max"), ("sum", "avg"), ("max", "max"),
               ("p99", "min"), ("p99", "mimmin")]
    got = engine.run_panel(_spec("sum", "avg"), queries, b)
    assert engine.panel_counters() == dict(point_stream_passes=1,
                                           row_matrices=3)
    same_bits(got[0], got[2], "dup/sum-avg")
    same_bits(got[1], got[3], "dup/max-max")
    same_bits(got[4], got[5], "dup/alias")


def test_empty_and_degenerate(engine):
    b = HostBatch.from_groups([[[], []], []])
    check_panel(engine, _spec("sum", "avg"), ALL_FIVE, b, "empty")
    b = datasets.random_batch(91, n_series=10, n_groups=2)
    spec = _spec("sum", "avg", start=T0 - 10 * HOUR, end=T0 - 9 * HOUR)
    check_panel(engine, spec, ALL_FIVE, b, "before")
    # a group without members beside groups with data (the shared pass)
    g_off = np.concatenate([b.group_offsets, [b.group_offsets[-1]]])
    b3 = HostBatch(b.offsets, b.ts, b.val, b.is_float, None, g_off,
                   b.group_members)
    _, c = check_panel(engine, _spec("sum", "max"), ALL_FIVE, b3, "emptygroup")
    assert c == dict(point_stream_passes=1, row_matrices=5), c


# 8 ---------------------------------------------------------------------- status
def _infinity_batch():
    big = 1.5e308
    return HostBatch.from_groups(
        [[[(T0 + 1000 * i, big, 1) for i in range(5)]] * 3])


def _device_call(engine, spec, queries, batch, cap, stream=None):
    import torch
    db = _device_batch(batch)
    res = _device_results(len(queries), batch.n_groups, cap)
    try:
        run_panel_device(engine, spec, queries, db, res, stream)
        err = None
    except core.OpenTSDBException as e:
        err = e
    torch.cuda.synchronize()
    return err, [_points(r, batch.n_groups) for r in res]


def test_none_fails_alone(engine):
    """none fed by two spans: E_ILLEGAL_DATA, the lowest-index failing
    output, while the other outputs' arrays are whole."""
    b = datasets.random_batch(81, n_series=6, n_groups=2, outside=False,
                              empty_frac=0)
    spec = _spec("sum", "avg")
    queries = [("max", "max"), ("none", "sum"), ("min", "min"),
               ("avg", "avg")]
    with pytest.raises(core.IllegalDataException):
        engine.run_panel(spec, queries, b)
    others = [queries[0]] + queries[2:]
    want = engine.run_panel(spec, others, b)
    cap = max(sum(len(g.ts) for g in out) for out in want) + 8
    err, got = _device_call(engine, spec, queries, b, cap)
    assert isinstance(err, core.IllegalDataException)
    for j, i in enumerate((0, 2, 3)):
        same_bits(got[i], want[j], "none/others/%d" % i)


def test_got_infinity_fails_only_who_reaches_it(engine):
    b = _infinity_batch()
    spec = _spec("sum", "max", end=T0 + 60000)
    with pytest.raises(core.IllegalStateException):  # sum: "Got Infinity"
        engine.run_panel(spec, [("max", "max"), ("sum", "max"),
                                ("min", "min")], b)
    ok = [("max", "max"), ("min", "min"), ("count", "count")]
    got = engine.run_panel(spec, ok, b)
    check_outputs(engine, spec, ok, b, got, "inf/ok")
    # two outputs fail differently: the lower index decides
    with pytest.raises(core.IllegalDataException):
        engine.run_panel(spec, [("max", "max"), ("none", "min"),
                                ("sum", "max")], b)
    with pytest.raises(core.IllegalStateException):
        engine.run_panel(spec, [("max", "max"), ("sum", "max"),
                                ("none", "min")], b)
    # ... and across the shared pass and a function beside it
    with pytest.raises(core.IllegalDataException):
        engine.run_panel(spec, [("max", "max"), ("none", "p95"),
                                ("sum", "min")], b)
    with pytest.raises(core.IllegalStateException):
        engine.run_panel(spec, [("max", "max"), ("sum", "min"),
                                ("none", "p95")], b)


def _host_call(engine, spec, queries, batch, caps):
    from opentsdb_amd.engine import panel_args
    n, ds, ids, it = panel_args(queries)
    G = batch.n_groups
    offs = np.full((n, G + 1), -7, np.int64)
    keep = []
    rs = (abi.Result * n)()
    for i in range(n):
        arr = [np.zeros(max(caps[i], 1), np.int64),
               np.zeros(max(caps[i], 1), np.int64),
               np.zeros(max(caps[i], 1), np.uint8)]
        keep.append(arr)
        rs[i] = abi.Result(caps[i], offs[i].ctypes.data, arr[0].ctypes.data,
                           arr[1].ctypes.data, arr[2].ctypes.data)
    ab = batch.as_abi()
    st = engine.lib.otsdb_agg_run_panel(
        engine.ctx, C.byref(spec), n, ds.ctypes.data, ids.ctypes.data,
        it.ctypes.data, C.byref(ab), rs)
    return st, offs


def test_host_capacity(engine):
    """A result too small: E_CAPACITY, its offsets whole (offsets[G] the
    point count it needs), as otsdb_agg_run leaves them."""
    b = datasets.random_batch(11, n_series=60, n_groups=6)
    spec = _spec("sum", "max")
    full = engine.run_panel(spec, ENVELOPE, b)
    need = [sum(len(g.ts) for g in out) for out in full]
    st, offs = _host_call(engine, spec, ENVELOPE, b, [need[0], 5, need[2]])
    assert st == abi.E_CAPACITY
    s1 = with_query(spec, ENVELOPE[1])
    o1 = np.full(b.n_groups + 1, -7, np.int64)
    a = [np.zeros(5, np.int64), np.zeros(5, np.int64), np.zeros(5, np.uint8)]
    r1 = abi.Result(5, o1.ctypes.data, a[0].ctypes.data, a[1].ctypes.data,
                    a[2].ctypes.data)
    ab = b.as_abi()
    assert engine.lib.otsdb_agg_run(engine.ctx, C.byref(s1), C.byref(ab),
                                    C.byref(r1)) == abi.E_CAPACITY
    assert np.array_equal(offs[1], o1) and offs[1][-1] == need[1]
    assert offs[0][-1] == need[0]  # (the result before it: whole too)
    st, offs = _host_call(engine, spec, ENVELOPE, b, need)
    assert st == abi.OK and [int(o[-1]) for o in offs] == need


@pytest.mark.parametrize("n_out", [0, 33])
def test_n_out_out_of_range(engine, n_out):
    b = datasets.random_batch(11, n_series=6, n_groups=2)
    spec = _spec("sum", "max")
    ids = np.zeros(max(n_out, 1), np.int32)
    rs = (abi.Result * max(n_out, 1))()
    ab = b.as_abi()
    p = ids.ctypes.data
    assert engine.lib.otsdb_agg_run_panel(
        engine.ctx, C.byref(spec), n_out, p, p, None, C.byref(ab),
        rs) == abi.E_ILLEGAL_ARGUMENT
    assert engine.lib.otsdb_agg_run_panel_device(
        engine.ctx, C.byref(spec), n_out, p, p, None, C.byref(ab), rs,
        None) == abi.E_ILLEGAL_ARGUMENT


# 9 ---------------------------------------------------------- entry points agree
def test_device_entry_equals_host_entry(engine):
    import torch
    b = datasets.random_batch(11, n_series=60, n_groups=6)
    spec = _spec("sum", "avg")
    queries = ALL_FIVE + [("p99", "max"), ("dev", "avg"), ("sum", "p95")]
    host = engine.run_panel(spec, queries, b)
    cap = max(sum(len(g.ts) for g in out) for out in host) + 8
    stream = torch.cuda.Stream()
    for name, st in (("ctx", None), ("caller", stream.cuda_stream)):
        err, got = _device_call(engine, spec, queries, b, cap, st)
        assert err is None
        for i, q in enumerate(queries):
            same_bits(got[i], host[i], "device/%s/%s-%s" % (name, q[0], q[1]))


# 10 ---------------------------------------------------------- context hygiene
def test_single_query_after_a_panel_call():
    """panel -> single -> failing panel -> single on one context: the
    singles equal a fresh context's (error words, tile cache, workspace)."""
    b = datasets.random_batch(11, n_series=60, n_groups=6)
    bi = _infinity_batch()
    s_sum, s_p99 = _spec("sum", "max"), _spec("p99", "avg", "nan")
    s_inf = _spec("sum", "max", end=T0 + 60000)

    def fresh(f):
        e = Engine(0)
        try:
            return f(e)
        finally:
            e.close()
    want = [fresh(lambda e: e.run(s_sum, b)), fresh(lambda e: e.run(s_p99, b)),
            fresh(lambda e: e.run_panel(s_sum, ALL_FIVE, b))]
    e = Engine(0)
    try:
        got = e.run_panel(s_sum, ALL_FIVE, b)
        same_bits(e.run(s_sum, b), want[0], "h0")
        with pytest.raises(core.IllegalStateException):
            e.run_panel(s_inf, [("max", "max"), ("sum", "min")], bi)
        same_bits(e.run(s_p99, b), want[1], "h1")
        e.run_panel(s_p99, ENVELOPE + [("sum", "p95")], b)
        same_bits(e.run(s_sum, b), want[0], "h2")
        again = e.run_panel(s_sum, ALL_FIVE, b)
        for i in range(len(ALL_FIVE)):
            same_bits(got[i], want[2][i], "h3/%d" % i)
            same_bits(again[i], want[2][i], "h4/%d" % i)
    finally:
        e.close()
