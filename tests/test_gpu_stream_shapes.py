"""Stream-shape edges of reduce_step (kernels.hip) through each of its
consumers: the case list of tests/stream_shapes.py puts bucket boundaries on
purpose against lanes, DPP rows, steps and the rings (points per lane,
fold_fast / fold_lane, the scan's row steps, the carry, ring pressure), one
single-series group per case, every case of a test in one query.  Needs an
MI355X.

Every comparison is bit for bit: the values are distinct integers whose
bucket sums are exact in a double in any order.  A result is held to
expected_single (numpy, straight from the run profile) wherever the query of
a single-series group is the downsampled series itself, and to the CPU oracle
always.  tests/test_stream_shapes_cpu.py shows that the cases reach every
structure class and that the oracle equals expected_single on them.
"""
import pytest

from opentsdb_amd import core
from opentsdb_amd.engine import Engine
from oracle import pyoracle
from tests import stream_shapes as SS
from tests.test_gpu_multi import same_bits, with_agg
from tests.test_gpu_panel import with_query
from tests.test_gpu_parity import compare

pytestmark = pytest.mark.gpu

I = core.Interpolation
FIVE = ["min", "avg", "max", "sum", "count"]
PANEL = [("min", "min"), ("avg", "avg"), ("max", "max"), ("sum", "sum"),
         ("count", "count")]
# an aggregator that hands a single member's value on unchanged
IDENTITY = ("sum", "min", "max", "avg", "p90")
COUNTER = core.RateOptions(True, core.LONG_MAX, 0)
TEN_MIN = 600_000
# buckets of 1,500 ms: the K = 6 grid (2,300 buckets) lies inside one storage
# row, and a bucket still holds the longest run at 1 ms a point
ONE_ROW = 1_500


@pytest.fixture(scope="module")
def engine():
    from opentsdb_amd import build
    build.build()
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def built8():
    cases = list(SS.case_list(SS.K_COLUMNS))
    return {f: SS.build(cases, f) for f in SS.FORMS}


def spec_of(b, agg, ds, fill, rate=False, ro=None, interp=None):
    s, e = SS.window(b, fill)
    name = {SS.INTERVAL: "10s", SS.HOUR: "1h", TEN_MIN: "10m",
            ONE_ROW: "1500ms"}[b.interval]
    d = core.DownsamplingSpecification("%s-%s-%s" % (name, ds, fill))
    return core.make_spec(s, e, core.Aggregators.get(agg), d, s, e, rate, ro,
                          interp)


class Oracle:
    """The oracle's result per spec of one batch, computed once."""

    def __init__(self, batch):
        self.batch, self.kept = batch, {}

    def __call__(self, spec):
        key = bytes(spec)
        if key not in self.kept:
            self.kept[key] = pyoracle.group_by(spec, self.batch)
        return self.kept[key]


def same_as_oracle(got, ref, b, where):
    """compare(), group by group, so that a failure names the case."""
    assert len(got) == len(ref), where
    names = [] if b.mixed else [c.name for c in b.cases]
    for g in range(len(ref)):
        w = "%s/%s" % (where, names[g] if g < len(names) else "g%d" % g)
        compare(got[g:g + 1], ref[g:g + 1], True, w)


def held(got, b, ora, spec, agg, ds, fill, where):
    """expected_single's bits where the aggregator hands a single member's
    value on, and the oracle's always."""
    if agg in IDENTITY and ds in SS.FUNCS and not b.mixed:
        SS.check_expected(got, b, ds, fill, where)
    same_as_oracle(got, ora(spec), b, where)


# ---------------------------------------------- the row path, k_bucketize_k
@pytest.mark.parametrize("fill", ["none", "zero"])
@pytest.mark.parametrize("form", SS.FORMS)
def test_row_path_ring(engine, built8, form, fill):
    """A percentile across series takes the row path: p90 of a single member
    is its value.  Every downsampling function of the ring kernel, dev's
    ordered replay included."""
    b = built8[form]
    ora = Oracle(b.batch)
    for ds in SS.FUNCS + ("dev",):
        spec = spec_of(b, "p90", ds, fill)
        w = "row/%s/%s-%s" % (form, ds, fill)
        held(engine.run(spec, b.batch), b, ora, spec, "p90", ds, fill, w)


# ------------------------------------------------------------ the rate ring
@pytest.fixture(scope="module")
def counters8():
    return SS.build(list(SS.case_list(SS.K_COLUMNS)), "long", counter=True)


@pytest.mark.parametrize("ds", ["sum", "max", "last", "avg"])
def test_rate_ring(engine, counters8, ds):
    """The same profiles as rising counters under rate: RateSpan fused into
    the ring's flush; a step that spans more than the ring's 1,024 buckets
    (the gap cases) hands its series to the fallback kernels, same bits."""
    b = counters8
    ora = Oracle(b.batch)
    gaps = [c for c in b.cases if c.name.startswith("gap") and
            int(c.name[3:].split("-")[0]) > SS.RING_RATE[0]]
    assert len(gaps) >= 4
    for agg, ro in (("p90", None), ("sum", COUNTER)):
        spec = spec_of(b, agg, ds, "none", rate=True, ro=ro)
        same_as_oracle(engine.run(spec, b.batch), ora(spec), b,
                       "rate/%s/%s" % (agg, ds))


# ------------------------------------------------------------------- k_fold
FOLD_QUERIES = [("sum", "sum"), ("sum", "avg"), ("min", "min"), ("max", "max"),
                ("sum", "count"), ("min", "first"), ("max", "last"),
                ("count", "sum"), ("dev", "max"), ("sum", "dev")]


@pytest.fixture(scope="module")
def padded8():
    """The cases and 1,100 one-point groups behind them: enough tiles that
    the fold's plan keeps full windows, so the steps are full."""
    return SS.build(list(SS.case_list(SS.K_COLUMNS)), "mixed", pad=1100)


@pytest.mark.parametrize("fill", ["none", "zero"])
@pytest.mark.parametrize("plan", ["few", "padded"])
def test_fold(engine, built8, padded8, plan, fill):
    """The ordered fold under both plans: as the few groups the cases are
    (windows of 128 buckets, steps cut by the window bounds) and padded to
    1,200 tiles (full windows, full steps)."""
    b = built8["mixed"] if plan == "few" else padded8
    ora = Oracle(b.batch)
    for agg, ds in FOLD_QUERIES:
        spec = spec_of(b, agg, ds, fill)
        w = "fold/%s/%s:%s-%s" % (plan, agg, ds, fill)
        held(engine.run(spec, b.batch), b, ora, spec, agg, ds, fill, w)


@pytest.mark.parametrize("form", ["long", "double"])
def test_fold_plans_agree_per_form(engine, built8, form):
    """The few-groups plan once more with longs and with doubles only (the
    fold's `fonly` forms)."""
    b = built8[form]
    ora = Oracle(b.batch)
    for agg, ds in FOLD_QUERIES[:4]:
        spec = spec_of(b, agg, ds, "none")
        held(engine.run(spec, b.batch), b, ora, spec, agg, ds, "none",
             "fold/%s/%s:%s" % (form, agg, ds))


@pytest.fixture(scope="module")
def mixed8():
    """Three groups that each hold one member of every case: the singles,
    the 3-step bucket and the gap series side by side."""
    return SS.build(list(SS.case_list(SS.K_COLUMNS)), "long", mixed=3)


@pytest.mark.parametrize("agg,ds,fill", [
    ("sum", "sum", "zero"), ("min", "min", "zero"), ("max", "avg", "zero"),
    ("count", "max", "zero"), ("min", "max", "none"), ("max", "min", "none"),
    ("count", "sum", "none"), ("sum", "count", "zero")])
def test_fold_mixed_profile_groups(engine, mixed8, agg, ds, fill):
    """Members of every profile in one group: the progress marks wait across
    members that close a bucket a step and members that close none in three.
    Under `zero` every member gives integers at every bucket (sums exact in
    any order); under `none` the order-free aggregators."""
    b = mixed8
    assert b.batch.n_groups == 3 or b.batch.n_groups == 4
    spec = spec_of(b, agg, ds, fill)
    compare(engine.run(spec, b.batch), pyoracle.group_by(spec, b.batch), True,
            "fold-mixed/%s:%s-%s" % (agg, ds, fill))


# ------------------------------------------------------------- k_fold_multi
@pytest.mark.parametrize("ds,fill", [("sum", "none"), ("max", "zero"),
                                     ("avg", "none"), ("min", "zero")])
def test_fold_multi(engine, built8, ds, fill):
    b = built8["mixed"]
    ora = Oracle(b.batch)
    it = [I.LERP] * 5 if fill == "none" else None
    spec = spec_of(b, "sum", ds, fill)
    got = engine.run_multi(spec, FIVE, b.batch, it, fold=True)
    assert engine.multi_fold_counters()["fold_launches"] == 1
    for i, agg in enumerate(FIVE):
        si = with_agg(spec, agg, None if it is None else it[i])
        w = "fold-multi/%s:%s-%s" % (agg, ds, fill)
        same_bits(got[i], engine.run(si, b.batch), w + "/single")
        held(got[i], b, ora, si, agg, ds, fill, w)


# ---------------------------------------------------------- the panel ring
@pytest.mark.parametrize("fill", ["none", "zero"])
@pytest.mark.parametrize("form", SS.FORMS)
def test_panel_ring(engine, built8, form, fill):
    b = built8[form]
    ora = Oracle(b.batch)
    spec = spec_of(b, "sum", "sum", fill)
    got = engine.run_panel(spec, PANEL, b.batch)
    assert engine.panel_counters()["point_stream_passes"] == 1
    for i, q in enumerate(PANEL):
        held(got[i], b, ora, with_query(spec, q), q[0], q[1], fill,
             "panel/%s/%s-%s" % (form, q[1], fill))


# -------------------------------------------------------------- cells, K = 6
@pytest.fixture(scope="module")
def cells_ms():
    """The K = 6 cases as compacted cells with millisecond qualifiers, on
    buckets of 1,500 ms: k_bucketize_cells starts a step at every storage
    row, so the whole grid is put inside one row, where its lane mapping is
    the columns' (what classify restates)."""
    from tests.test_gpu_cells_panel import Case
    out = {}
    cases = list(SS.case_list(SS.K_CELLS))
    for form in ("mixed", "double"):
        b = SS.build(cases, form, interval=ONE_ROW)
        assert b.nb * ONE_ROW <= SS.HOUR and SS.START % SS.HOUR == 0
        case = Case(b.batch, ms_frac=1.0)
        assert int(case.dc.t["qual_off"][-1]) == 4 * len(b.batch.ts)
        out[form] = (b, case)
    return out


@pytest.fixture(scope="module")
def cells_seconds():
    """1 h buckets of second points with the same run lengths (2-byte
    qualifiers, all doubles: the uniform walker), for the cases whose grid
    stays narrow at 1 h.  Every bucket is a storage row of its own."""
    from tests.test_gpu_cells_panel import Case
    lim = 2**32 // SS.HOUR
    cases = [c for c in SS.case_list(SS.K_CELLS)
             if c.profile[-1][0] < lim - 2 and
             max(n for _, n in c.profile) <= 3600]
    assert len(cases) > 60
    b = SS.build(cases, "double", interval=SS.HOUR, spacing=1000)
    return b, Case(b.batch)


@pytest.fixture(scope="module")
def cells_seconds10m():
    """The same with 10 m buckets, six to a storage row: runs of up to 600
    second points."""
    from tests.test_gpu_cells_panel import Case
    cases = [c for c in SS.case_list(SS.K_CELLS)
             if max(n for _, n in c.profile) <= 600]
    assert len(cases) > 60
    b = SS.build(cases, "double", interval=TEN_MIN, spacing=1000)
    return b, Case(b.batch)


@pytest.fixture(scope="module")
def cells_ms8(built8):
    """The K = 8 cases as cells: the cells fold streams 8 points a lane."""
    from tests.test_gpu_cells_panel import Case
    b = built8["mixed"]
    return b, Case(b.batch, ms_frac=1.0)


def _cells(request, which, form="mixed"):
    if which == "ms":
        return request.getfixturevalue("cells_ms")[form]
    if which == "ms8":
        return request.getfixturevalue("cells_ms8")
    return request.getfixturevalue("cells_" + which)


@pytest.mark.parametrize("fill", ["none", "zero"])
@pytest.mark.parametrize("which", ["ms", "seconds", "seconds10m"])
def test_cells_fused_query(engine, request, which, fill):
    """k_bucketize_cells (K = 6): a percentile across series from cells."""
    from tests.test_gpu_cells_panel import cells_single
    b, case = _cells(request, which)
    ora = Oracle(b.batch)
    for ds in SS.FUNCS + ("dev",):
        spec = spec_of(b, "p90", ds, fill)
        held(cells_single(engine, case, spec), b, ora, spec, "p90", ds, fill,
             "cells/%s/%s-%s" % (which, ds, fill))


@pytest.mark.parametrize("fill", ["none", "zero"])
@pytest.mark.parametrize("which,form", [("ms", "mixed"), ("ms", "double"),
                                        ("seconds", "double"),
                                        ("seconds10m", "double"),
                                        ("ms8", "mixed")])
def test_cells_fold(engine, request, which, form, fill):
    from tests.test_gpu_cells_panel import cells_single
    b, case = _cells(request, which, form)
    ora = Oracle(b.batch)
    c0 = engine.counters()
    for agg, ds in FOLD_QUERIES:
        spec = spec_of(b, agg, ds, fill)
        held(cells_single(engine, case, spec), b, ora, spec, agg, ds, fill,
             "cells-fold/%s/%s/%s:%s-%s" % (which, form, agg, ds, fill))
    c1 = engine.counters()
    assert sum(c1[k] - c0[k] for k in ("cells_uniform", "cells_general")) > 0


@pytest.mark.parametrize("ds,fill", [("sum", "none"), ("max", "zero"),
                                     ("avg", "none")])
@pytest.mark.parametrize("which", ["ms", "seconds", "seconds10m", "ms8"])
def test_cells_multi_fold(engine, request, which, ds, fill):
    from tests.test_gpu_cells_multi_fold import cells_multi_fold
    b, case = _cells(request, which)
    ora = Oracle(b.batch)
    it = [I.LERP] * 5 if fill == "none" else None
    spec = spec_of(b, "sum", ds, fill)
    got = cells_multi_fold(engine, case, spec, FIVE, it)
    assert engine.multi_fold_counters()["fold_launches"] >= 1
    for i, agg in enumerate(FIVE):
        si = with_agg(spec, agg, None if it is None else it[i])
        held(got[i], b, ora, si, agg, ds, fill,
             "cells-multi-fold/%s/%s:%s-%s" % (which, agg, ds, fill))


@pytest.mark.parametrize("fill", ["none", "zero"])
@pytest.mark.parametrize("which", ["ms", "seconds", "seconds10m"])
def test_cells_panel(engine, request, which, fill):
    from tests.test_gpu_cells_panel import panel
    b, case = _cells(request, which)
    ora = Oracle(b.batch)
    spec = spec_of(b, "sum", "sum", fill)
    got = panel(engine, case, spec, PANEL)
    for i, q in enumerate(PANEL):
        held(got[i], b, ora, with_query(spec, q), q[0], q[1], fill,
             "cells-panel/%s/%s-%s" % (which, q[1], fill))


# --------------------------------------------------------------- wide grids
@pytest.fixture(scope="module")
def wide8():
    """Every K = 8 case on 1 h buckets over 2,354 buckets: past 2^32 ms, the
    grid is not `narrow`; fold_fast and the tail form are off, everything
    goes through fold_lane on 64-bit times."""
    cases = list(SS.case_list(SS.K_COLUMNS))
    lim = 2**32 // SS.HOUR
    return {f: SS.build(cases, f, interval=SS.HOUR, nb_min=lim + 6)
            for f in ("mixed", "double")}


@pytest.mark.parametrize("fill", ["none", "zero"])
@pytest.mark.parametrize("form", ["mixed", "double"])
def test_wide_grid(engine, wide8, form, fill):
    b = wide8[form]
    assert b.nb >= 1194
    assert int(engine.plan(spec_of(b, "sum", "sum", fill), b.batch).n_buckets) \
        == b.nb
    ora = Oracle(b.batch)
    for agg, ds in [("p90", d) for d in SS.FUNCS + ("dev",)] + FOLD_QUERIES:
        spec = spec_of(b, agg, ds, fill)
        held(engine.run(spec, b.batch), b, ora, spec, agg, ds, fill,
             "wide/%s/%s:%s-%s" % (form, agg, ds, fill))
