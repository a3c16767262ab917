"""Cells multi-aggregator queries through the cells fold
(OTSDB_SPEC_CELLS_MULTI_FOLD, workload.run_cells_multi_device(..., fold=True)):
sum / avg / count / min / max sets of one interpolation class from ONE decode
and ONE fold of the compacted columns over the envelope state, no row matrix.
Needs an MI355X.

Every eligible case is checked (`check`)
 (a) per output against the CPU oracle run with that aggregator, under the
     single-aggregator rule of tests/test_gpu_multi_fold.py: exact where the
     downsampling function is order-free and the group is reduced in one
     chain (or the aggregator is order-free), 1e-12 otherwise;
 (b) per output against workload.run_cells_device with that aggregator: bit
     for bit where the downsampling function is order-free (any grid) or the
     grid has at most 128 buckets (both calls fold one window), within 1e-12
     otherwise (windows of 1,024 against 2,048 buckets, a window's stream
     starts at its own cursor);
 (c) fold_launches >= 1 (== 1 where no retry is expected) and
     multi_counters() == (1, 0, 0, 0).
An ineligible request with the bit gives the bits and the counters of the same
call without it.  Cells are built with tests/cells.encode_batch; timestamps
sit on whole seconds unless a case says otherwise.
"""
import numpy as np
import pytest

from opentsdb_amd import abi, core, workload
from opentsdb_amd.batch import HostBatch, groups_from_ids
from opentsdb_amd.engine import Engine, _fold_spec
from oracle import pyoracle
from tests import cells, datasets
from tests.test_gpu_cells_panel import (Case, _wide_ints, cells_multi,
                                        cells_single, panel, whole_seconds)
from tests.test_gpu_multi import (_device_results, _infinity_batch, _points,
                                  same_bits, with_agg)
from tests.test_gpu_multi_fold import FIVE, FOLDED, SETS
from tests.test_gpu_parity import (ORDER_FREE, ORDER_FREE_DS, RATES,
                                   _empty_member_batch, _member_scales, _spec,
                                   compare, contribution_floor)

pytestmark = pytest.mark.gpu

T0 = datasets.T0
HOUR = 3600 * 1000
I = core.Interpolation
LERP5 = [I.LERP] * 5


@pytest.fixture(scope="module")
def engine():
    from opentsdb_amd import build
    build.build()
    e = Engine(0)
    yield e
    e.close()


def flagged(spec):
    return _fold_spec(spec, True, abi.SPEC_CELLS_MULTI_FOLD)


def cells_multi_fold(engine, case, spec, aggs, interps=None):
    """The flagged call through the Python entry (fold=True)."""
    import torch
    G = case.b.n_groups
    res = _device_results(len(aggs), G, case.cap(spec))
    workload.run_cells_multi_device(engine, spec, aggs, case.dc, case.db, res,
                                    interps, fold=True)
    torch.cuda.synchronize()
    return [_points(r, G) for r in res]


def folded(engine, case, spec, aggs, interps=None, launches=1):
    """The flagged call, with (c).  launches: the fold launches expected,
    None where an attempt is run again (at least one)."""
    got = cells_multi_fold(engine, case, spec, aggs, interps)
    n = engine.multi_fold_counters()["fold_launches"]
    assert n >= 1 and (launches is None or n == launches), n
    assert engine.multi_counters() == FOLDED
    assert len(got) == len(aggs)
    return got


def _as_ref(points):
    """A result as `compare` takes its reference: one record array a group."""
    out = []
    for p in points:
        r = np.zeros(len(p.ts), [("ts", np.int64), ("bits", np.int64),
                                 ("is_int", np.uint8)])
        r["ts"], r["bits"], r["is_int"] = p.ts, p.bits, p.is_int
        out.append(r)
    return out


def check(engine, case, spec, ds, aggs, where, interps=None, whole=True,
          floor=False, launches=1):
    """(a), (b), (c).  ds: the spec's downsampling function; whole: every
    group is one fold tile (at most 32 members); floor: the inexact outputs
    are held to contribution_floor (values of both signs)."""
    b = case.b
    got = folded(engine, case, spec, aggs, interps, launches)
    nb = int(engine.plan(spec, b).n_buckets)
    bits = ds in ORDER_FREE_DS or nb <= 128
    seen = {}
    for i, agg in enumerate(aggs):
        it = None if interps is None else interps[i]
        w = "%s/%d:%s" % (where, i, agg)
        if (agg, it) not in seen:
            si = with_agg(spec, agg, it)
            ref = pyoracle.group_by(si, b)
            exact = ds in ORDER_FREE_DS and (whole or agg in ORDER_FREE)
            fl = 0.0
            if floor and not exact:
                fl = contribution_floor(si, b, ref, _member_scales(si, b))
            seen[(agg, it)] = (ref, exact, fl, cells_single(engine, case, si))
        ref, exact, fl, single = seen[(agg, it)]
        compare(got[i], ref, exact, w, fl)
        if bits:
            same_bits(got[i], single, w + "/single")
        else:
            compare(got[i], _as_ref(single), False, w + "/single", fl)
    return got


def check_ignored(engine, case, spec, aggs, where, interps=None):
    """An ineligible request: bit 4 changes nothing."""
    plain = cells_multi(engine, case, spec, aggs, interps)
    c0 = engine.multi_counters()
    assert engine.multi_fold_counters() == dict(fold_launches=0)
    got = cells_multi_fold(engine, case, spec, aggs, interps)
    assert engine.multi_fold_counters() == dict(fold_launches=0), where
    assert engine.multi_counters() == c0, where
    for i in range(len(aggs)):
        same_bits(got[i], plain[i], "%s/%d" % (where, i))


# 1 ------------------------------------------------------------ sets and classes
@pytest.fixture(scope="module")
def sets_case():
    return Case(whole_seconds(datasets.random_batch(41, n_series=30,
                                                    n_groups=3)))


@pytest.mark.parametrize("ds", ["max", "avg"])
@pytest.mark.parametrize("name", ["five-lerp", "zim", "prev", "dups", "32"])
def test_aggregator_sets(engine, sets_case, name, ds):
    """100 buckets of 10 s: one window, every function bit-identical to the
    single cells queries."""
    aggs, interps = SETS[name]
    spec = _spec("sum", ds, interval="10s", end=T0 + 99 * 10000)
    assert engine.plan(spec, sets_case.b).n_buckets == 100
    got = check(engine, sets_case, spec, ds, aggs, "sets/%s/%s" % (name, ds),
                interps)
    if name == "dups":
        same_bits(got[0], got[1], "dups")


# 2 ------------------------------------------------------------------------ fill
def test_fill_is_one_class(engine):
    """A fill policy: zimsum + min + mimmax (three classes under NONE) and
    the plain five are one class.  181 buckets: two narrowed windows."""
    case = Case(whole_seconds(datasets.random_batch(31, n_series=25,
                                                    n_groups=4,
                                                    nan_frac=0.02)))
    for ds in ("max", "avg"):
        check(engine, case, _spec("sum", ds, "nan"), ds,
              ["zimsum", "min", "mimmax"] + FIVE, "fill/" + ds)


# 3 --------------------------------------------------------------------- walkers
def _walker_batch(kind, wide=True):
    """wide: the integers spread over 1 / 2 / 4 / 8 stored bytes point by
    point.  (random_batch's own integers, -50 .. 99, are all stored in one
    byte: such a column is uniform, and the uniform kernel takes it — for the
    single cells query as for this call.)"""
    b = whole_seconds(datasets.random_batch(23, n_series=30, n_groups=3,
                                            value_kind=kind))
    return _wide_ints(b) if wide and kind != "float" else b


def test_walker_uniform_2_byte(engine):
    case = Case(_walker_batch("float"))
    assert int(case.dc.t["qual_off"][-1]) == 2 * len(case.b.ts)
    c0 = engine.counters()
    for ds in ("max", "avg"):
        check(engine, case, _spec("sum", ds), ds, FIVE, "u2/" + ds, LERP5)
    c1 = engine.counters()
    assert c1["cells_uniform"] > c0["cells_uniform"]
    assert c1["cells_uniform_miss"] == c0["cells_uniform_miss"]


def test_walker_uniform_4_byte(engine):
    case = Case(_walker_batch("float"), ms_frac=1.0)
    assert int(case.dc.t["qual_off"][-1]) == 4 * len(case.b.ts)
    c0 = engine.counters()
    for ds in ("max", "avg"):
        check(engine, case, _spec("sum", ds), ds, FIVE, "u4/" + ds, LERP5)
    assert engine.counters()["cells_uniform"] > c0["cells_uniform"]


def test_walker_uniform_one_byte_integers(engine):
    case = Case(_walker_batch("int", wide=False))
    c0 = engine.counters()
    for ds in ("max", "avg"):
        check(engine, case, _spec("sum", ds), ds, FIVE, "u-int/" + ds, LERP5,
              floor=True)
    c1 = engine.counters()
    assert c1["cells_uniform"] > c0["cells_uniform"]
    assert c1["cells_general"] == c0["cells_general"]


@pytest.mark.parametrize("kind", ["int", "mixed"])
@pytest.mark.parametrize("ms_frac", [0.0, 1.0])
def test_walker_general(engine, kind, ms_frac):
    """Integer and mixed columns whose value lengths change point by point:
    the general kernel, 2- and 4-byte qualifiers."""
    case = Case(_walker_batch(kind), ms_frac=ms_frac)
    for ds in ("max", "avg"):
        c0 = engine.counters()
        cells_multi_fold(engine, case, _spec("sum", ds), FIVE, LERP5)
        assert engine.multi_fold_counters() == dict(fold_launches=1)
        c1 = engine.counters()
        assert c1["cells_general"] == c0["cells_general"] + 1
        assert c1["cells_uniform"] == c0["cells_uniform"]
        check(engine, case, _spec("sum", ds), ds, FIVE,
              "general/%s/%s/%s" % (kind, ms_frac, ds), LERP5, floor=True)


def test_walker_mixed_widths_are_rewritten(engine):
    """30 % of the points forced to 4-byte qualifiers inside 2-byte columns:
    ERR_CELLS_GENERIC, the qualifiers are rewritten with one width and the
    pass runs again — the result is the 4-byte encoding's."""
    b = _walker_batch("float")
    mixed, wide = Case(b, ms_frac=0.3), Case(b, ms_frac=1.0)
    for ds in ("max", "avg"):
        spec = _spec("sum", ds)
        got = check(engine, mixed, spec, ds, FIVE, "requal/" + ds, LERP5,
                    launches=None)
        want = folded(engine, wide, spec, FIVE, LERP5)
        for i in range(5):
            same_bits(got[i], want[i], "requal/%s/%d" % (ds, i))


# 4 --------------------------------------------------------------------- windows
@pytest.mark.parametrize("nb", [1024, 1025, 2049])
@pytest.mark.parametrize("fill", ["none", "nan"])
def test_narrowed_windows(engine, nb, fill):
    """20 series in 3 tiles: windows narrowed to 128 buckets, the cursors of
    every window after the first from k_cells_fold_prep."""
    b = whole_seconds(datasets.random_batch(53, n_series=20, n_groups=3,
                                            span_ms=nb * 10000 + 600000,
                                            cadence_ms=5000))
    case = Case(b)
    end = T0 + (nb - 1) * 10000 + (10000 if fill != "none" else 0)
    for ds in ("max", "avg"):
        spec = _spec("sum", ds, fill, end=end, interval="10s")
        assert engine.plan(spec, b).n_buckets == nb
        check(engine, case, spec, ds, FIVE,
              "narrow/%d/%s/%s" % (nb, fill, ds), LERP5)


@pytest.mark.parametrize("fill,ds,aggs,interps", [
    ("none", "avg", FIVE, LERP5),
    ("nan", "max", ["zimsum", "mimmax", "count"], None)])
def test_two_envelope_windows_where_the_single_query_has_one(engine, fill, ds,
                                                             aggs, interps):
    """1,100 single-series groups x 1,100 buckets: two full-width windows of
    the envelope state (1,024 + 76 buckets) where the single query folds one
    of 2,048 — the cursor arrays are sized for this state's windows."""
    n = 1100
    b = datasets.random_batch(57, n_series=n, n_groups=n, span_ms=n * 10000,
                              cadence_ms=5000, empty_frac=0.02)
    g_off, members = groups_from_ids(np.arange(n, dtype=np.int64), n)
    b = whole_seconds(HostBatch(b.offsets, b.ts, b.val, b.is_float, None,
                                g_off, members))
    end = T0 + (n - 1) * 10000 + (10000 if fill != "none" else 0)
    spec = _spec("sum", ds, fill, end=end, interval="10s")
    assert engine.plan(spec, b).n_buckets == n
    check(engine, Case(b), spec, ds, aggs, "full/%s" % fill, interps)


# 5 ----------------------------------------------------------------- group sizes
def test_group_sizes_1_32_33_and_empty(engine):
    """Groups of 1, 32 (one tile) and 33 members (tiles of 8, merged by
    k_combine per output), a group without members, series without rows."""
    b = datasets.random_batch(61, n_series=66, n_groups=3, span_ms=HOUR,
                              cadence_ms=15000, empty_frac=0.1, nan_frac=0.03)
    gid = np.array([0] + [1] * 32 + [2] * 33, np.int64)
    g_off, members = groups_from_ids(gid, 4)
    assert list(np.diff(g_off)) == [1, 32, 33, 0]
    b = whole_seconds(HostBatch(b.offsets, b.ts, b.val, b.is_float, None,
                                g_off, members))
    assert (np.diff(b.offsets) == 0).any()
    case = Case(b)
    for ds, fill in (("max", "none"), ("avg", "none"), ("max", "zero")):
        spec = _spec("sum", ds, fill, end=T0 + HOUR)
        got = check(engine, case, spec, ds, FIVE, "sizes/%s/%s" % (ds, fill),
                    LERP5, whole=False)
        assert all(len(out[3].ts) == 0 for out in got)


def test_700_members(engine):
    b = whole_seconds(datasets.random_batch(71, n_series=700, big_group=True,
                                            span_ms=HOUR, cadence_ms=30000))
    case = Case(b)
    for ds in ("max", "avg"):
        check(engine, case, _spec("sum", ds, end=T0 + HOUR), ds, FIVE,
              "big/" + ds, LERP5, whole=False)
    check(engine, case, _spec("sum", "max", "nan", end=T0 + HOUR), "max",
          ["zimsum", "mimmin", "count"], "big/nan", whole=False)


@pytest.mark.parametrize("after", [False, True])
@pytest.mark.parametrize("fill", ["none", "zero"])
def test_member_without_window_points(engine, after, fill):
    """A member SpanGroup.add keeps with no point inside the window."""
    b = _empty_member_batch(after)
    assert (np.asarray(b.ts) % 1000 == 0).all()
    case = Case(b)
    t0, t1 = T0 + HOUR + 125000, T0 + 3 * HOUR
    for ds, iv in (("sum", "1m"), ("min", "30s"), ("count", "2m")):
        spec = _spec("sum", ds, fill, t0, t1, interval=iv)
        check(engine, case, spec, ds, FIVE,
              "nopoint/%s/%s/%s" % (ds, fill, after), LERP5)


# 6 ----------------------------------------- window edges inside hour rows
@pytest.mark.parametrize("fill", ["none", "nan"])
def test_window_edges_inside_hour_rows(engine, fill):
    """The window starts 61 s into an hour row and ends inside another."""
    case = Case(whole_seconds(datasets.random_batch(31, n_series=25,
                                                    n_groups=4,
                                                    nan_frac=0.02)))
    start, end = T0 + 61000, T0 + 2 * HOUR + 1234000
    assert start % HOUR != 0 and end % HOUR != 0
    for ds in ("max", "avg"):
        check(engine, case, _spec("sum", ds, fill, start=start, end=end), ds,
              FIVE, "edges/%s/%s" % (fill, ds), LERP5)


# 7 ----------------------------------------------------------- value-domain edges
@pytest.mark.parametrize("kind", ["signed", "nanpayload"])
def test_value_domain_edges(engine, kind):
    from tests.value_domain import WINDOWS, edge_batch
    case = Case(whole_seconds(edge_batch(kind, "a")))
    s, e = WINDOWS[0]
    for ds, fill in (("max", "none"), ("min", "nan"), ("sum", "none"),
                     ("avg", "zero")):
        check(engine, case, _spec("sum", ds, fill, s, e), ds, FIVE,
              "edge/%s/%s/%s" % (kind, ds, fill), LERP5, floor=True)


# 8 ---------------------------------------------------------------------- errors
def test_overflow_fails_the_output_that_holds_it(engine):
    case = Case(_infinity_batch())
    spec = _spec("sum", "max", end=T0 + 60000)
    with pytest.raises(core.IllegalStateException):  # sum: "Got Infinity"
        cells_multi_fold(engine, case, spec, ["max", "sum", "min"])
    assert engine.multi_fold_counters() == dict(fold_launches=1)
    got = folded(engine, case, spec, ["max", "min"])
    same_bits(got[0], cells_single(engine, case, with_agg(spec, "max")),
              "inf/max")
    same_bits(got[1], cells_single(engine, case, with_agg(spec, "min")),
              "inf/min")


def _series3_rows(enc):
    nq = np.diff(enc["qual_off"])
    return np.nonzero((enc["row_series"] == 3) & (nq > 2))[0]


def test_corrupt_cell_is_illegal_data(engine):
    """A row that loses a value byte (test_decode_corrupt_column's corruption):
    E_ILLEGAL_DATA for the call, and the next good call is whole."""
    b = whole_seconds(datasets.random_batch(31, n_series=25, n_groups=4,
                                            empty_frac=0, outside=False))
    enc = cells.encode_batch(b, np.random.default_rng(5))
    bad = dict(enc)
    bad["val_off"] = enc["val_off"].copy()
    # one row a value byte short, the next one a byte long
    bad["val_off"][int(_series3_rows(enc)[1]) + 1] -= 1
    spec = _spec("sum", "avg")
    with pytest.raises(core.IllegalDataException):
        cells_single(engine, Case(b, enc=bad), spec)
    with pytest.raises(core.IllegalDataException):
        cells_multi_fold(engine, Case(b, enc=bad), spec, FIVE, LERP5)
    check(engine, Case(b, enc=enc), spec, "avg", FIVE, "after-corrupt", LERP5)


def test_column_without_its_meta_byte_has_the_single_querys_status(engine):
    b = whole_seconds(datasets.random_batch(31, n_series=25, n_groups=4,
                                            empty_frac=0, outside=False))
    enc = cells.encode_batch(b, np.random.default_rng(5))
    r = int(_series3_rows(enc)[1])
    cut = int(enc["val_off"][r + 1]) - 1  # the column's meta byte
    bad = dict(enc)
    bad["val"] = np.delete(enc["val"], cut)
    bad["val_off"] = enc["val_off"].copy()
    bad["val_off"][r + 1:] -= 1
    case = Case(b, enc=bad)
    spec = _spec("sum", "avg")

    def status(f):
        try:
            return None, f()
        except core.OpenTSDBException as e:
            return e.status, None
    want, single = status(lambda: cells_single(engine, case,
                                               with_agg(spec, "max", I.LERP)))
    got, outs = status(lambda: cells_multi_fold(engine, case, spec, FIVE,
                                                LERP5))
    assert got == want
    if want is None:
        assert engine.multi_fold_counters()["fold_launches"] >= 1
        same = _as_ref(single)
        compare(outs[3], same, False, "nometa/max")


# 9 ------------------------------------------------------------------ ineligible
def test_ineligible_requests_ignore_the_bit(engine):
    b = whole_seconds(datasets.random_batch(11, n_series=60, n_groups=6))
    case = Case(b)
    spec = _spec("sum", "avg")
    check_ignored(engine, case, spec, ["sum", "dev"], "dev")
    check_ignored(engine, case, spec, ["sum", "p99"], "p99")
    check_ignored(engine, case, spec, ["zimsum", "min"], "two classes")
    check_ignored(engine, case, spec, FIVE, "count is ZIM")
    check_ignored(engine, case, _spec("sum", "p90"), ["sum", "max"], "ds p90")
    bc = whole_seconds(datasets.random_batch(52, n_series=30, n_groups=3,
                                             counter=True))
    check_ignored(engine, Case(bc),
                  _spec("sum", "sum", rate=True, ro=RATES[1]), ["sum", "max"],
                  "rate")
    d = core.DownsamplingSpecification("0all-max")
    all_spec = core.make_spec(T0, T0 + 4 * HOUR, core.Aggregators.get("sum"),
                              d, T0 + 600000, T0 + 7200000)
    check_ignored(engine, case, all_spec, ["sum", "max"], "0all")
    raw = core.make_spec(T0, T0 + 3 * HOUR, core.Aggregators.get("sum"), None,
                         T0, T0 + 3 * HOUR)
    check_ignored(engine, case, raw, ["sum", "max"], "raw")
    check_ignored(engine, case, spec, ["max"], "n_out 1")


def test_calendar_grid_keeps_the_row_path(engine):
    from tests.test_gpu_panel import DAY, T_SPRING, _cal_spec
    b = whole_seconds(datasets.random_batch(97, n_series=24, n_groups=3,
                                            span_ms=4 * DAY,
                                            cadence_ms=600000, t0=T_SPRING))
    spec = _cal_spec("1dc-sum", "America/Denver", T_SPRING + HOUR,
                     T_SPRING + 3 * DAY, b)
    assert spec.use_calendar
    check_ignored(engine, Case(b), spec, FIVE, "1dc", LERP5)


def test_columnar_entry_ignores_bit_4(engine):
    b = datasets.random_batch(11, n_series=60, n_groups=6)
    spec = _spec("sum", "avg", "nan")
    plain = engine.run_multi(spec, FIVE, b)
    c0 = engine.multi_counters()
    got = engine.run_multi(flagged(spec), FIVE, b)
    assert engine.multi_fold_counters() == dict(fold_launches=0)
    assert engine.multi_counters() == c0
    for i in range(5):
        same_bits(got[i], plain[i], "columnar/%d" % i)


# 10 ------------------------------------------------------ panel of one function
def test_panel_of_one_function_inherits_the_bit(engine):
    case = Case(whole_seconds(datasets.random_batch(11, n_series=60,
                                                    n_groups=6)))
    spec = _spec("sum", "avg", "nan")
    got = panel(engine, case, flagged(spec), [(a, "avg") for a in FIVE])
    assert engine.multi_fold_counters() == dict(fold_launches=1)
    want = folded(engine, case, spec, FIVE)
    for i in range(5):
        same_bits(got[i], want[i], "panel/%d" % i)
    # several distinct functions: the panel's own pass
    q = [("min", "min"), ("avg", "avg"), ("max", "max")]
    plain = panel(engine, case, spec, q)
    got = panel(engine, case, flagged(spec), q)
    assert engine.multi_fold_counters() == dict(fold_launches=0)
    for i in range(3):
        same_bits(got[i], plain[i], "panel3/%d" % i)


# 11 ------------------------------------------------------------- context hygiene
def test_call_sequence_on_one_context():
    """flagged cells multi -> single cells query -> unflagged cells multi ->
    (a failing flagged call) -> flagged cells multi on one context: every
    result equals a fresh context's."""
    case = Case(whole_seconds(datasets.random_batch(11, n_series=60,
                                                    n_groups=6)))
    inf = Case(_infinity_batch())
    s_avg, s_max = _spec("sum", "avg", "nan"), _spec("sum", "max")
    s_inf = _spec("sum", "max", end=T0 + 60000)

    def fresh(f):
        e = Engine(0)
        try:
            return f(e)
        finally:
            e.close()
    steps = [lambda e: cells_multi_fold(e, case, s_avg, FIVE),
             lambda e: [cells_single(e, case, s_max)],
             lambda e: cells_multi(e, case, s_max, FIVE),
             lambda e: cells_multi_fold(e, case, s_max, FIVE, LERP5)]
    want = [fresh(f) for f in steps]
    e = Engine(0)
    try:
        for k, f in enumerate(steps):
            if k == 3:
                with pytest.raises(core.IllegalStateException):
                    cells_multi_fold(e, inf, s_inf, ["max", "sum"])
            got = f(e)
            if k != 1:  # (the counters are the last multi call's)
                assert e.multi_fold_counters()["fold_launches"] == \
                    (1 if k in (0, 3) else 0)
            for i in range(len(got)):
                same_bits(got[i], want[k][i], "seq%d/%d" % (k, i))
    finally:
        e.close()
