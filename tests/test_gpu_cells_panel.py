"""Panel queries from compacted cells (otsdb_agg_run_cells_panel_device): the
envelope functions are reduced from ONE decode of each series' columns
(k_bucketize_panel_cells).  Needs an MI355X.

Every output i of a call is checked
 (a) against the CPU oracle run with its own downsampler and aggregator:
     bit-exact where the function is min / max / count and the aggregator is
     order-free or a selection, 1e-12 relative otherwise (diff: cancel_floor)
     — the rule of the single-query tests;
 (b) bit for bit against workload.run_cells_multi_device(spec with ds_i,
     [agg_i, agg_i])[0], the existing cells row path with that function (the
     walk is the same, so are the lanes' summation trees: avg and sum too);
 (c) where the function is min / max / count, bit for bit against the
     columnar engine.run.
Engine.panel_counters() shows what was shared.
"""
import numpy as np
import pytest

from opentsdb_amd import core, workload
from opentsdb_amd.batch import HostBatch
from opentsdb_amd.engine import Engine
from oracle import pyoracle
from tests import cells, datasets
from tests.test_gpu_multi import (_device_batch, _device_results, _points,
                                  same_bits)
from tests.test_gpu_panel import (ALL_FIVE, ENVELOPE, EXACT_DS, SELECTIONS,
                                  _cal_spec, with_query)
from tests.test_gpu_parity import ORDER_FREE, _spec, cancel_floor, compare

pytestmark = pytest.mark.gpu

T0 = datasets.T0
HOUR = 3600 * 1000
MIN = 60 * 1000
SHARED5 = dict(point_stream_passes=1, row_matrices=5)


@pytest.fixture(scope="module")
def engine():
    from opentsdb_amd import build
    build.build()
    e = Engine(0)
    yield e
    e.close()


def whole_seconds(b):
    """The batch with its timestamps cut to whole seconds (2-byte
    qualifiers unless the encoder is told otherwise)."""
    b = datasets.with_values(b, b.val, b.is_float)
    b.ts = np.ascontiguousarray(b.ts - b.ts % 1000)
    return b


def device_cells(b, float4_frac=0.0, ms_frac=0.0, enc=None):
    import torch
    if enc is None:
        enc = cells.encode_batch(b, np.random.default_rng(5), float4_frac,
                                 ms_frac)
    d = {k: torch.from_numpy(np.array(v)).cuda() for k, v in enc.items()}
    return workload.DeviceCells(d, b.n_series)


class Case:
    """A batch as columnar device arrays (the groups) and as cells."""

    def __init__(self, b, float4_frac=0.0, ms_frac=0.0, enc=None):
        self.b = b
        self.db = _device_batch(b)
        self.dc = device_cells(b, float4_frac, ms_frac, enc)

    def cap(self, spec):
        # every group emits at most one point a bucket; raw: a point a point
        sz = 4 + (spec.end_ms - spec.start_ms) // max(spec.ds_interval_ms, 1) \
            if spec.ds_interval_ms > 0 else len(self.b.ts)
        return int(sz) * self.b.n_groups + 8


def panel(engine, case, spec, queries):
    import torch
    G = case.b.n_groups
    res = _device_results(len(queries), G, case.cap(spec))
    workload.run_cells_panel_device(engine, spec, queries, case.dc, case.db,
                                    res)
    torch.cuda.synchronize()
    return [_points(r, G) for r in res]


def cells_multi(engine, case, spec, aggs, interps=None):
    import torch
    G = case.b.n_groups
    res = _device_results(len(aggs), G, case.cap(spec))
    workload.run_cells_multi_device(engine, spec, aggs, case.dc, case.db, res,
                                    interps)
    torch.cuda.synchronize()
    return [_points(r, G) for r in res]


def cells_single(engine, case, spec):
    import torch
    G = case.b.n_groups
    res = _device_results(1, G, case.cap(spec))[0]
    workload.run_cells_device(engine, spec, case.dc, case.db, res)
    torch.cuda.synchronize()
    return _points(res, G)


def check_outputs(engine, case, spec, queries, got, where, floor=0.0,
                  rows=True, rate=False):
    """(a), (b) and (c) for every output.  rows=False: a fallback whose rows
    are not the cells row path's."""
    b = case.b
    assert len(got) == len(queries)
    for i, q in enumerate(queries):
        agg, ds = q[0], q[1]
        si = with_query(spec, q)
        w = "%s/%d:%s-%s" % (where, i, agg, ds)
        exact = not rate and ds in EXACT_DS and (agg in ORDER_FREE or
                                                 agg in SELECTIONS)
        fl = floor + (cancel_floor(b, 2) if agg == "diff" else 0.0)
        compare(got[i], pyoracle.group_by(si, b), exact, w, fl)
        if rows:
            it = None if len(q) < 3 else [q[2], q[2]]
            same_bits(got[i], cells_multi(engine, case, si, [agg, agg], it)[0],
                      w + "/rows")
        if ds in ("min", "max", "count") and not rate:
            same_bits(got[i], engine.run(si, b), w + "/columnar")


def check_panel(engine, case, spec, queries, where, floor=0.0, rows=True,
                rate=False):
    got = panel(engine, case, spec, queries)
    c = engine.panel_counters()
    check_outputs(engine, case, spec, queries, got, where, floor, rows, rate)
    return got, c


# 1 ------------------------------------------------ all five, with aliases
def _wide_ints(b):
    """Integer values spread over 1 / 2 / 4 / 8 stored bytes, point by
    point (the float values stay)."""
    rng = np.random.default_rng(3)
    scale = 10 ** rng.integers(0, 11, len(b.val))
    val = np.where(np.asarray(b.is_float) == 1, b.val, b.val * scale)
    return datasets.with_values(b, val, b.is_float)


def _float32_values(b):
    """Float values that a 4-byte float holds exactly (either encoding of a
    point then decodes to the batch's value)."""
    f = np.asarray(b.val, np.int64).view(np.float64)
    r = f.astype(np.float32).astype(np.float64).view(np.int64)
    val = np.where(np.asarray(b.is_float) == 1, r, b.val)
    return datasets.with_values(b, val, b.is_float)


@pytest.mark.parametrize("kind", ["float", "int", "mixed"])
def test_all_functions_and_aliases(engine, kind):
    """Every row of the envelope, the aliases sharing theirs, selections and
    dev as aggregators over them.  float: half the values stored in 4 bytes,
    5 % NaNs; int: 1 / 2 / 4 / 8-byte longs in one column (the length scan
    and the per-point decode); mixed: floats and longs in one column."""
    b = whole_seconds(datasets.random_batch(
        23, n_series=30, n_groups=3, value_kind=kind,
        nan_frac=0.05 if kind == "float" else 0))
    b = _float32_values(_wide_ints(b))
    case = Case(b, float4_frac=0.5)
    queries = ALL_FIVE + [("zimsum", "zimsum"), ("sum", "pfsum"),
                          ("mimmin", "mimmin"), ("mimmax", "mimmax"),
                          ("p90", "max"), ("dev", "avg")]
    spec = _spec("sum", "avg", interval="10s" if kind == "float" else "1m")
    fl = cancel_floor(b, 300) if kind != "float" else 0.0
    _, c = check_panel(engine, case, spec, queries, "all/" + kind, fl)
    assert c == SHARED5, c


# 2 ----------------------- bucket length against the row and step shape
@pytest.mark.parametrize("interval", ["10s", "1m", "5m", "2h"])
def test_bucket_lengths(engine, interval):
    """10 s cadence over 6 storage rows: one point a bucket, a boundary in
    every lane, runs over several lanes, and 2 h buckets that span a row
    boundary (the carry crosses rows)."""
    span = 6 * HOUR
    b = whole_seconds(datasets.random_batch(31, n_series=20, n_groups=3,
                                            span_ms=span))
    spec = _spec("sum", "avg", interval=interval, end=T0 + span)
    _, c = check_panel(engine, Case(b), spec, ALL_FIVE, "len/" + interval)
    assert c == SHARED5, c


# 3 --------------------------------------------------- window edges in rows
def _series(rng, t):
    return [(int(x), float(rng.random() * 100.0), 1) for x in t]


def test_window_edges_inside_rows(engine):
    """The window starts and ends inside storage rows (the seek / stop
    counting; the stop row is reached mid-row); a series wholly before the
    window, one wholly after it, an empty one, one shorter than a step."""
    rng = np.random.default_rng(7)
    step = 10000
    plain = _series(rng, T0 + 9000 + step * np.arange(1080))
    odd = _series(rng, T0 - 3 * step + step * np.arange(700))
    short = _series(rng, T0 + 50 * MIN + step * np.arange(37))
    before = _series(rng, T0 - 2 * HOUR + step * np.arange(50))
    after = _series(rng, T0 + 3 * HOUR + step * np.arange(50))
    b = HostBatch.from_groups([[plain, short, odd], [[], before, plain],
                               [after, odd]])
    case = Case(b)
    for interval in ("10s", "1m"):
        spec = _spec("sum", "avg", interval=interval, start=T0 + 40 * MIN + 7000,
                     end=T0 + 2 * HOUR + 20 * MIN - 3000)
        _, c = check_panel(engine, case, spec, ALL_FIVE, "edges/" + interval)
        assert c == SHARED5, c


# 4 ------------------------------------- NONE fill: the bucket past the window
def test_bucket_past_the_window_is_each_functions_own(engine):
    """Series `gap` has no point in the window's last five minutes and three
    different values in the bucket past it; beside `full` in one group, its
    LERP contribution to the last emitted buckets runs toward that bucket's
    min, avg or max — each function's own SeriesMeta.of_val."""
    rng = np.random.default_rng(11)
    step = 10000
    end = T0 + 2 * HOUR
    t = T0 + step * np.arange(1080)
    full = _series(rng, t)
    tg = t[(t < end - 5 * MIN) | (t >= end)]
    gap = [(int(x), float(10.0 + 80.0 * rng.random()), 1) for x in tg]
    b = HostBatch.from_groups([[full, gap], [gap]])
    past = np.array([v for x, v, _ in gap if end <= x < end + MIN])
    assert len(past) == 6
    assert past.min() < past.mean() < past.max()
    I = core.Interpolation
    queries = [("sum", "min", I.LERP), ("sum", "max", I.LERP),
               ("sum", "avg", I.LERP), ("sum", "sum", I.LERP),
               ("sum", "count", I.LERP)]
    spec = _spec("sum", "avg", interval="1m", end=end - 1000)
    got, c = check_panel(engine, Case(b), spec, queries, "past")
    assert c == SHARED5, c
    # group 0 emits the window's last bucket (full's point); gap's share of
    # it is interpolated toward the bucket past the window
    last = [g[0] for g in got]
    assert all(int(x.ts[-1]) == end - MIN for x in last)
    vals = [float(np.asarray(x.bits[-1:], np.int64).view(np.float64)[0])
            for x in last[:3]]
    assert len(set(vals)) == 3, vals
    # the same through random data and a window ending off the grid
    b = whole_seconds(datasets.random_batch(41, n_series=30, n_groups=3))
    case = Case(b)
    for e in (T0 + 3 * HOUR, T0 + 2 * HOUR + 61000):
        _, c = check_panel(engine, case, _spec("sum", "min", end=e),
                           queries + [("sum", "min", I.ZIM), ("max", "max")],
                           "past/%d" % e)
        assert c == SHARED5, c


# 5 ------------------------------------------------ fill policies, calendar
@pytest.mark.parametrize("fill", ["nan", "zero", "null"])
def test_fill_policies(engine, fill):
    b = whole_seconds(datasets.random_batch(31, n_series=25, n_groups=4,
                                            nan_frac=0.02))
    queries = ENVELOPE + [("sum", "count"), ("p99", "max"), ("count", "min")]
    _, c = check_panel(engine, Case(b),
                       _spec("sum", "max", fill, start=T0 + 61000), queries,
                       "fill/" + fill)
    assert c == dict(point_stream_passes=1, row_matrices=4), c


def test_single_table_calendar(engine):
    b = whole_seconds(datasets.random_batch(97, n_series=24, n_groups=3))
    spec = _cal_spec("1hc-sum", "America/Denver", T0 + 40 * MIN,
                     T0 + 2 * HOUR + 50 * MIN, b)
    assert spec.use_calendar and spec.n_cal_anchors == 0
    _, c = check_panel(engine, Case(b), spec, ALL_FIVE, "1hc")
    assert c == SHARED5, c


# 6 ----------------------------------------------------- 4-byte ms qualifiers
def test_ms_qualifiers_uniform(engine):
    b = datasets.random_batch(43, n_series=24, n_groups=3)  # ms timestamps
    _, c = check_panel(engine, Case(b, ms_frac=1.0), _spec("sum", "avg"),
                       ALL_FIVE, "ms")
    assert c == SHARED5, c


def test_ms_qualifiers_mixed_widths(engine):
    """30 % of the points forced to 4-byte qualifiers inside 2-byte columns:
    the pass raises ERR_CELLS_GENERIC, the qualifiers are rewritten with one
    width, the pass runs again — two attempts, each a pass over the cells."""
    b = whole_seconds(datasets.random_batch(43, n_series=24, n_groups=3))
    _, c = check_panel(engine, Case(b, ms_frac=0.3), _spec("sum", "avg"),
                       ALL_FIVE, "mixedw")
    assert c == dict(point_stream_passes=2, row_matrices=5), c


def test_ms_row_longer_than_a_step(engine):
    """720 ms-qualified points a row: more than the prefetch buffers hold
    (64 lanes x OTSDB_PANEL_CELLS_K points, and past 512): the rows are
    staged step by step."""
    b = datasets.random_batch(47, n_series=20, n_groups=3, cadence_ms=5000)
    enc = cells.encode_batch(b, np.random.default_rng(5), 0.0, 1.0)
    assert (np.diff(enc["qual_off"]) // 4).max() > 512
    _, c = check_panel(engine, Case(b, enc=enc),
                       _spec("sum", "avg", interval="5m"), ALL_FIVE, "long")
    assert c == SHARED5, c


# 7 ------------------------------------------------------------ corrupt column
def test_corrupt_column_fails_every_output(engine):
    """One value byte short in a column of a kept series: the call is
    E_ILLEGAL_DATA whichever outputs are asked for, and the next good call
    on the context is whole."""
    b = whole_seconds(datasets.random_batch(31, n_series=25, n_groups=4,
                                            empty_frac=0, outside=False))
    good = Case(b)
    enc = cells.encode_batch(b, np.random.default_rng(5))
    nq = np.diff(enc["qual_off"])
    r = int(np.nonzero((enc["row_series"] == 3) & (nq > 2))[0][1])
    cut = int(enc["val_off"][r + 1]) - 1  # the column's meta byte
    bad = dict(enc)
    bad["val"] = np.delete(enc["val"], cut)
    bad["val_off"] = enc["val_off"].copy()
    bad["val_off"][r + 1:] -= 1
    spec = _spec("sum", "avg")
    case = Case(b, enc=bad)
    for queries in (ALL_FIVE, ENVELOPE[::-1], [("max", "max"), ("min", "min")]):
        with pytest.raises(core.IllegalDataException):
            panel(engine, case, spec, queries)
    with pytest.raises(core.IllegalDataException):  # the row path's own status
        cells_multi(engine, case, with_query(spec, ("sum", "avg")),
                    ["sum", "sum"])
    _, c = check_panel(engine, good, spec, ALL_FIVE, "after-corrupt")
    assert c == SHARED5, c


# 8 ------------------------------------------------------------------ fallbacks
def _check_fallback(engine, case, spec, queries, where, rate=False):
    """(a), (c), and min / max / count bit for bit against the single cells
    query."""
    got, c = check_panel(engine, case, spec, queries, where, rows=False,
                         rate=rate)
    for i, q in enumerate(queries):
        if q[1] in ("min", "max", "count") and not rate:
            same_bits(got[i], cells_single(engine, case, with_query(spec, q)),
                      "%s/%d/single" % (where, i))
    return got, c


def test_fallback_run_all(engine):
    """`0all-*`: one decode into the columnar buffer, then the columnar
    shared pass."""
    b = whole_seconds(datasets.random_batch(61, n_series=20, n_groups=4))
    d = core.DownsamplingSpecification("0all-max")
    spec = core.make_spec(T0, T0 + 4 * HOUR, core.Aggregators.get("sum"), d,
                          T0 + 600000, T0 + 7200000)
    _, c = _check_fallback(engine, Case(b), spec, ALL_FIVE, "0all")
    assert c == SHARED5, c


def test_fallback_percentile_downsampler(engine):
    """p95 beside the envelope: the shared cells pass, then one cells call
    for p95's outputs."""
    b = whole_seconds(datasets.random_batch(27, n_series=24, n_groups=3,
                                            nan_frac=0.1))
    case = Case(b)
    queries = ENVELOPE + [("p99", "p95"), ("max", "p95")]
    spec = _spec("sum", "avg", interval="5m")
    got, c = panel(engine, case, spec, queries), engine.panel_counters()
    assert c == dict(point_stream_passes=2, row_matrices=4), c
    check_outputs(engine, case, spec, queries[:3], got[:3], "p95/env")
    for i in (3, 4):
        si = with_query(spec, queries[i])
        compare(got[i], pyoracle.group_by(si, b), False, "p95/%d" % i)


def test_fallback_rate(engine):
    from tests.test_gpu_parity import RATES
    b = whole_seconds(datasets.random_batch(52, n_series=30, n_groups=3,
                                            counter=True))
    spec = _spec("sum", "sum", rate=True, ro=RATES[1])
    queries = [("sum", "sum"), ("max", "max"), ("avg", "max")]
    _, c = _check_fallback(engine, Case(b), spec, queries, "rate", rate=True)
    assert c["point_stream_passes"] == 2, c


def test_fallback_one_function(engine):
    """One distinct function, and two outputs of one function through an
    alias: the cells multi call."""
    b = whole_seconds(datasets.random_batch(11, n_series=60, n_groups=6))
    case = Case(b)
    aggs = ["sum", "max", "p99", "dev"]
    spec = _spec("min", "max")
    got = panel(engine, case, spec, [(a, "avg") for a in aggs])
    assert engine.panel_counters() == dict(point_stream_passes=1,
                                           row_matrices=1)
    want = cells_multi(engine, case, _spec("sum", "avg"), aggs)
    for i, a in enumerate(aggs):
        same_bits(got[i], want[i], "onefn/" + a)
    got, c = check_panel(engine, case, spec, [("sum", "max"),
                                              ("p99", "mimmax")], "two")
    assert c == dict(point_stream_passes=1, row_matrices=1), c
    got, c = check_panel(engine, case, spec, [("sum", "max")], "one")
    assert c == dict(point_stream_passes=1, row_matrices=1), c


# 9 ---------------------------------------------------------- context hygiene
def test_calls_after_a_cells_panel_call():
    """cells panel -> single cells query -> columnar panel -> cells multi on
    one context: each equals a fresh context's."""
    b = whole_seconds(datasets.random_batch(11, n_series=60, n_groups=6))
    s_sum, s_p99 = _spec("sum", "max"), _spec("p99", "avg", "nan")
    aggs = ["dev", "sum", "median"]

    def calls(e, case, with_panel):
        out = []
        if with_panel:
            out.append(panel(e, case, s_sum, ALL_FIVE))
        out.append(cells_single(e, case, s_sum))
        if with_panel:
            panel(e, case, s_p99, ENVELOPE + [("sum", "p95")])
        out.append(e.run_panel(s_p99, ENVELOPE, b))
        if with_panel:
            out.append(panel(e, case, s_sum, ALL_FIVE))
        out.append(cells_multi(e, case, s_sum, aggs))
        return out

    def on_fresh(with_panel):
        e = Engine(0)
        try:
            return calls(e, Case(b), with_panel)
        finally:
            e.close()
    want = on_fresh(False)
    got = on_fresh(True)
    same_bits(got[1], want[0], "single")
    for i in range(len(ENVELOPE)):
        same_bits(got[2][i], want[1][i], "columnar panel/%d" % i)
    for i in range(len(ALL_FIVE)):
        same_bits(got[3][i], got[0][i], "panel again/%d" % i)
    for i in range(len(aggs)):
        same_bits(got[4][i], want[2][i], "cells multi/%d" % i)
