"""Multi-aggregator queries through the ordered fold
(OTSDB_SPEC_MULTI_FOLD, Engine.run_multi(..., fold=True)): sum / avg / count /
min / max sets of one interpolation class from ONE fold over the envelope
state, no row matrix.  Needs an MI355X.

Every eligible case is checked
 (a) per output against the CPU oracle run with that aggregator, under the
     single-aggregator rule: exact where the downsampling function is
     order-free and the group is reduced in one chain (or the aggregator is
     order-free), 1e-12 otherwise;
 (b) per output bit for bit against Engine.run with that aggregator where the
     downsampling function is order-free (any grid) or the grid has at most
     128 buckets (any function: both calls fold one window from the same
     stream start);
 (c) fold_launches == 1 and multi_counters() == (1, 0, 0, 0).
An ineligible request with the flag gives the bits and the counters of the
same call without it.

`count` contributes through ZIM by default (Aggregators.java: Count is built
with Interpolation.ZIM), sum / avg / min / max through LERP: under NONE fill
the five-aggregator set is one class only with an interpolation override;
under any fill policy it is one class as it stands.
"""
import numpy as np
import pytest

from opentsdb_amd import core
from opentsdb_amd.batch import HostBatch, groups_from_ids
from opentsdb_amd.engine import Engine, _fold_spec, run_multi_device
from oracle import pyoracle
from tests import cells, datasets
from tests.test_gpu_multi import (_device_batch, _device_results,
                                  _infinity_batch, _points, same_bits,
                                  with_agg)
from tests.test_gpu_parity import (ORDER_FREE, ORDER_FREE_DS, RATES,
                                   _empty_member_batch, _member_scales, _spec,
                                   compare, contribution_floor)

pytestmark = pytest.mark.gpu

T0 = datasets.T0
HOUR = 3600 * 1000
I = core.Interpolation
FIVE = ["sum", "avg", "min", "max", "count"]
FOLDED = dict(downsample_passes=1, group_passes=0, key_transposes=0,
              transform_passes=0)


@pytest.fixture(scope="module")
def engine():
    from opentsdb_amd import build
    build.build()
    e = Engine(0)
    yield e
    e.close()


def folded(engine, spec, aggs, batch, interps=None):
    """The flagged call, with (c)."""
    got = engine.run_multi(spec, aggs, batch, interps, fold=True)
    assert engine.multi_fold_counters() == dict(fold_launches=1)
    assert engine.multi_counters() == FOLDED
    assert len(got) == len(aggs)
    return got


def check_fold(engine, spec, ds, aggs, batch, where, interps=None, whole=True,
               floor=False):
    """(a), (b), (c).  ds: the spec's downsampling function; whole: every
    group is one fold tile (at most 32 members: one chain in SpanCmp order);
    floor: the inexact outputs are held to contribution_floor (values of
    both signs)."""
    got = folded(engine, spec, aggs, batch, interps)
    nb = int(engine.plan(spec, batch).n_buckets)
    bits = ds in ORDER_FREE_DS or nb <= 128
    seen = {}
    for i, agg in enumerate(aggs):
        it = None if interps is None else interps[i]
        w = "%s/%d:%s" % (where, i, agg)
        if (agg, it) not in seen:
            si = with_agg(spec, agg, it)
            seen[(agg, it)] = (si, pyoracle.group_by(si, batch),
                               engine.run(si, batch) if bits else None)
        si, ref, single = seen[(agg, it)]
        exact = ds in ORDER_FREE_DS and (whole or agg in ORDER_FREE)
        fl = 0.0
        if floor and not exact:
            fl = contribution_floor(si, batch, ref, _member_scales(si, batch))
        compare(got[i], ref, exact, w, fl)
        if bits:
            same_bits(got[i], single, w + "/single")
    return got


def check_ignored(engine, spec, aggs, batch, where, interps=None):
    """An ineligible request: the flag changes nothing."""
    plain = engine.run_multi(spec, aggs, batch, interps)
    c0 = engine.multi_counters()
    assert engine.multi_fold_counters() == dict(fold_launches=0)
    got = engine.run_multi(spec, aggs, batch, interps, fold=True)
    assert engine.multi_fold_counters() == dict(fold_launches=0), where
    assert engine.multi_counters() == c0, where
    for i in range(len(aggs)):
        same_bits(got[i], plain[i], "%s/%d" % (where, i))


# 1 ------------------------------------------------------------ aggregator sets
SETS = {
    "five-lerp": (FIVE, [I.LERP] * 5),
    "zim": (["zimsum", "count"], None),
    "prev": (["sum", "max"], [I.PREV] * 2),
    "max": (["sum", "max"], [I.MAX] * 2),
    "min": (["sum", "max"], [I.MIN] * 2),
    "dups": (["sum", "sum", "pfsum"], [None, None, I.LERP]),
    "32": ([FIVE[i % 5] for i in range(32)], [I.ZIM] * 32),
}


@pytest.mark.parametrize("ds", ["max", "avg"])
@pytest.mark.parametrize("name", sorted(SETS))
def test_aggregator_sets(engine, name, ds):
    """100 buckets of 10 s: one window, every function bit-identical to the
    single queries; gaps (outages, 10 s buckets of a 10 s cadence with 5 %
    of the points missing) make the interpolation class matter."""
    aggs, interps = SETS[name]
    b = datasets.random_batch(41, n_series=30, n_groups=3)
    spec = _spec("sum", ds, interval="10s", end=T0 + 99 * 10000)
    assert engine.plan(spec, b).n_buckets == 100
    if name in ("max", "min"):
        # a gap contributes +-Double.MAX_VALUE: two members in a gap at one
        # timestamp overflow the sum, in the reference ("Got Infinity") as in
        # the single query — the folded call fails as its sum output, and
        # the outputs that hold no Infinity pass alone
        with pytest.raises(pyoracle.OracleError):
            pyoracle.group_by(with_agg(spec, "sum", interps[0]), b)
        with pytest.raises(core.IllegalStateException):
            engine.run(with_agg(spec, "sum", interps[0]), b)
        with pytest.raises(core.IllegalStateException):
            engine.run_multi(spec, aggs, b, interps, fold=True)
        assert engine.multi_fold_counters() == dict(fold_launches=1)
        check_fold(engine, spec, ds, ["max", "min", "count"], b,
                   "sets/%s/%s/finite" % (name, ds), [interps[0]] * 3)
        # one member with gaps per group: the sum stays finite
        b = _one_gappy_member_batch()
    got = check_fold(engine, spec, ds, aggs, b, "sets/%s/%s" % (name, ds),
                     interps)
    if name == "dups":
        same_bits(got[0], got[1], "dups")


def _one_gappy_member_batch():
    """3 groups of 3 series on a 5 s cadence over 100 buckets of 10 s; the
    first member of each group has outages (gaps of 1 .. 12 buckets), the
    others none."""
    rng = np.random.default_rng(43)
    groups = []
    for g in range(3):
        series = []
        for m in range(3):
            keep = np.ones(200, bool)
            if m == 0:
                for a in rng.integers(4, 190, 6):
                    keep[a:a + 2 * int(rng.integers(1, 13))] = False
            series.append([(int(T0 + 5000 * i + 1000 * m),
                            float(rng.random() * 100.0), 1)
                           for i in np.nonzero(keep)[0]])
        groups.append(series)
    return HostBatch.from_groups(groups)


def test_classes_differ(engine):
    """The class is baked into the contributions: the PREV, ZIM and LERP
    sums over test_aggregator_sets' batch are not one result."""
    b = datasets.random_batch(41, n_series=30, n_groups=3)
    spec = _spec("sum", "max", interval="10s", end=T0 + 99 * 10000)
    r = [folded(engine, spec, ["sum", "max"], b, [k] * 2)[0]
         for k in (I.PREV, I.ZIM, I.LERP)]
    bits = [np.concatenate([np.asarray(g.bits) for g in x]) for x in r]
    assert not np.array_equal(bits[0], bits[1])
    assert not np.array_equal(bits[0], bits[2])


# 2 ---------------------------------------------------------- fill and window
@pytest.mark.parametrize("fill", ["nan", "zero", "null"])
@pytest.mark.parametrize("aligned", [True, False])
def test_fill_and_window(engine, fill, aligned):
    """A fill policy: the contribution does not depend on the interpolation,
    so zimsum + min + mimmax (three classes under NONE) and the plain five
    are one class.  181 buckets: two narrowed windows."""
    b = datasets.random_batch(31, n_series=25, n_groups=4, nan_frac=0.02)
    start = T0 + (0 if aligned else 61000)
    for ds in ("max", "avg"):
        check_fold(engine, _spec("sum", ds, fill, start=start), ds,
                   ["zimsum", "min", "mimmax"] + FIVE, b,
                   "fill/%s/%s/%s" % (fill, aligned, ds))


@pytest.mark.parametrize("aligned", [True, False])
def test_none_fill_window(engine, aligned):
    b = datasets.random_batch(31, n_series=25, n_groups=4, nan_frac=0.02)
    start = T0 + (0 if aligned else 61000)
    for ds in ("max", "avg"):
        check_fold(engine, _spec("sum", ds, start=start), ds, FIVE, b,
                   "none/%s/%s" % (aligned, ds), [I.LERP] * 5)


# 3 ---------------------------------------------------------------- grid widths
@pytest.mark.parametrize("nb", [1024, 1025, 2049])
@pytest.mark.parametrize("fill", ["none", "nan"])
def test_narrowed_windows(engine, nb, fill):
    """20 series in 3 tiles: windows narrowed to 128 buckets; outages and
    late starts cross the window boundaries (LERP from k_fold_prep's
    context, fills)."""
    b = datasets.random_batch(53, n_series=20, n_groups=3,
                              span_ms=nb * 10000 + 600000, cadence_ms=5000)
    end = T0 + (nb - 1) * 10000 + (10000 if fill != "none" else 0)
    for ds in ("max", "avg"):
        spec = _spec("sum", ds, fill, end=end, interval="10s")
        assert engine.plan(spec, b).n_buckets == nb
        check_fold(engine, spec, ds, FIVE, b, "narrow/%d/%s/%s" % (nb, fill, ds),
                   [I.LERP] * 5)


@pytest.mark.parametrize("fill,ds,aggs,interps", [
    ("none", "avg", FIVE, [I.LERP] * 5),
    ("nan", "max", ["zimsum", "mimmax", "count"], None)])
def test_full_width_windows(engine, fill, ds, aggs, interps):
    """1,100 single-series groups x 1,100 buckets: 2,200 workgroups, two
    full-width windows (1,024 + 76 buckets, no member-context preload)."""
    n = 1100
    b = datasets.random_batch(57, n_series=n, n_groups=n,
                              span_ms=n * 10000, cadence_ms=5000,
                              empty_frac=0.02)
    g_off, members = groups_from_ids(np.arange(n, dtype=np.int64), n)
    b = HostBatch(b.offsets, b.ts, b.val, b.is_float, None, g_off, members)
    end = T0 + (n - 1) * 10000 + (10000 if fill != "none" else 0)
    spec = _spec("sum", ds, fill, end=end, interval="10s")
    assert engine.plan(spec, b).n_buckets == n
    check_fold(engine, spec, ds, aggs, b, "full/%s" % fill, interps)


# 4 ---------------------------------------------------------------- group sizes
def test_group_sizes_1_32_33_and_empty(engine):
    """Groups of 1, 32 (one tile) and 33 members (tiles of 8, merged by
    k_combine per output) and a group without members."""
    b = datasets.random_batch(61, n_series=66, n_groups=3, span_ms=HOUR,
                              cadence_ms=15000, empty_frac=0.1, nan_frac=0.03)
    gid = np.array([0] + [1] * 32 + [2] * 33, np.int64)
    g_off, members = groups_from_ids(gid, 4)
    assert list(np.diff(g_off)) == [1, 32, 33, 0]
    b = HostBatch(b.offsets, b.ts, b.val, b.is_float, None, g_off, members)
    for ds, fill in (("max", "none"), ("avg", "none"), ("max", "zero")):
        spec = _spec("sum", ds, fill, end=T0 + HOUR)
        got = check_fold(engine, spec, ds, FIVE, b,
                         "sizes/%s/%s" % (ds, fill), [I.LERP] * 5, whole=False)
        assert all(len(out[3].ts) == 0 for out in got)


def test_700_members(engine):
    b = datasets.random_batch(71, n_series=700, big_group=True,
                              span_ms=HOUR, cadence_ms=30000)
    for ds in ("max", "avg"):
        check_fold(engine, _spec("sum", ds, end=T0 + HOUR), ds, FIVE, b,
                   "big/" + ds, [I.LERP] * 5, whole=False)
    check_fold(engine, _spec("sum", "max", "nan", end=T0 + HOUR), "max",
               ["zimsum", "mimmin", "count"], b, "big/nan", whole=False)


def test_1100_members_two_level_combine(engine):
    """138 tiles of 8 in one group (more than 128): each output's partials go
    through k_combine_l1 + k_combine."""
    from tests.value_domain import SPAN, base_batch
    b = base_batch("c")
    assert b.n_groups == 1 and b.n_series == 1100
    for ds, fill in (("max", "none"), ("avg", "nan")):
        check_fold(engine, _spec("sum", ds, fill, T0, T0 + SPAN), ds, FIVE, b,
                   "1100/%s/%s" % (ds, fill), [I.LERP] * 5, whole=False)


@pytest.mark.parametrize("after", [False, True])
@pytest.mark.parametrize("fill", ["none", "zero"])
def test_member_without_window_points(engine, after, fill):
    """A member SpanGroup.add keeps with no point inside the window
    (test_fold_member_without_window_points' batch): 30 s buckets, two
    narrowed windows."""
    b = _empty_member_batch(after)
    t0, t1 = T0 + HOUR + 125000, T0 + 3 * HOUR
    for ds, iv in (("sum", "1m"), ("min", "30s"), ("count", "2m")):
        spec = _spec("sum", ds, fill, t0, t1, interval=iv)
        check_fold(engine, spec, ds, FIVE, b,
                   "nopoint/%s/%s/%s" % (ds, fill, after), [I.LERP] * 5)


@pytest.mark.parametrize("kind", ["float", "int", "mixed"])
def test_value_kinds_empty_and_nan(engine, kind):
    b = datasets.random_batch(23, n_series=30, n_groups=3, value_kind=kind,
                              nan_frac=0.1 if kind == "float" else 0,
                              empty_frac=0.3)
    for ds in ("max", "avg"):
        check_fold(engine, _spec("sum", ds), ds, FIVE, b,
                   "kinds/%s/%s" % (kind, ds), [I.LERP] * 5, floor=True)


# 5 ----------------------------------------------------------- value-domain edges
@pytest.mark.parametrize("kind", ["signed", "nanpayload"])
def test_value_domain_edges(engine, kind):
    """+-0.0 ties (min / max keep the earliest, sum normalises -0.0),
    subnormals and NaNs of several payloads (the absent-bucket sentinel
    among them) as points: ten 1 m buckets, every function bit-identical to
    the single queries."""
    from tests.value_domain import WINDOWS, edge_batch
    b = edge_batch(kind, "a")
    s, e = WINDOWS[0]
    for ds, fill in (("max", "none"), ("min", "nan"), ("sum", "none"),
                     ("avg", "zero")):
        check_fold(engine, _spec("sum", ds, fill, s, e), ds, FIVE, b,
                   "edge/%s/%s/%s" % (kind, ds, fill), [I.LERP] * 5,
                   floor=True)


def test_overflow_fails_the_output_that_holds_it(engine):
    b = _infinity_batch()
    spec = _spec("sum", "max", end=T0 + 60000)
    with pytest.raises(core.IllegalStateException):  # sum: "Got Infinity"
        engine.run_multi(spec, ["max", "sum", "min"], b, fold=True)
    assert engine.multi_fold_counters() == dict(fold_launches=1)
    got = folded(engine, spec, ["max", "min"], b)
    same_bits(got[0], engine.run(with_agg(spec, "max"), b), "inf/max")
    same_bits(got[1], engine.run(with_agg(spec, "min"), b), "inf/min")


# 6 ----------------------------------------------------------------- entries
def test_device_entry(engine):
    import torch
    b = datasets.random_batch(11, n_series=60, n_groups=6)
    for ds in ("avg", "max"):
        spec = _spec("sum", ds, "nan")
        host = folded(engine, spec, FIVE, b)
        cap = max(sum(len(g.ts) for g in out) for out in host) + 8
        db = _device_batch(b)
        res = _device_results(len(FIVE), b.n_groups, cap)
        run_multi_device(engine, spec, FIVE, db, res, fold=True)
        torch.cuda.synchronize()
        assert engine.multi_fold_counters() == dict(fold_launches=1)
        assert engine.multi_counters() == FOLDED
        for i, a in enumerate(FIVE):
            same_bits(_points(res[i], b.n_groups), host[i], "device/" + a)


def test_single_table_calendar(engine):
    from tests.test_gpu_panel import DAY, T_SPRING, _cal_spec
    b = datasets.random_batch(97, n_series=24, n_groups=3, span_ms=4 * DAY,
                              cadence_ms=600000, t0=T_SPRING)
    spec = _cal_spec("1dc-sum", "America/Denver", T_SPRING + HOUR,
                     T_SPRING + 3 * DAY, b)
    assert spec.use_calendar and spec.n_cal_anchors == 0
    check_fold(engine, spec, "sum", FIVE, b, "1dc", [I.LERP] * 5)


def test_panel_of_one_function_inherits_the_flag(engine):
    b = datasets.random_batch(11, n_series=60, n_groups=6)
    spec = _spec("sum", "avg", "nan")
    flagged = _fold_spec(spec, True)
    got = engine.run_panel(flagged, [(a, "avg") for a in FIVE], b)
    assert engine.multi_fold_counters() == dict(fold_launches=1)
    want = folded(engine, spec, FIVE, b)
    for i in range(5):
        same_bits(got[i], want[i], "panel/%d" % i)
    # several distinct functions: the panel's own row path
    q = [("min", "min"), ("avg", "avg"), ("max", "max")]
    plain = engine.run_panel(spec, q, b)
    got = engine.run_panel(flagged, q, b)
    assert engine.multi_fold_counters() == dict(fold_launches=0)
    for i in range(3):
        same_bits(got[i], plain[i], "panel3/%d" % i)


# 7 -------------------------------------------------------------- ineligible
def test_ineligible_requests_ignore_the_flag(engine):
    b = datasets.random_batch(11, n_series=60, n_groups=6)
    spec = _spec("sum", "avg")
    check_ignored(engine, spec, ["sum", "dev"], b, "dev")
    check_ignored(engine, spec, ["sum", "p99"], b, "p99")
    check_ignored(engine, spec, ["zimsum", "min"], b, "two classes")
    check_ignored(engine, spec, FIVE, b, "count is ZIM")
    check_ignored(engine, spec, ["sum", "squareSum"], b, "squareSum",
                  [I.LERP] * 2)
    check_ignored(engine, _spec("sum", "p90"), ["sum", "max"], b, "ds p90")
    bc = datasets.random_batch(52, n_series=30, n_groups=3, counter=True)
    check_ignored(engine, _spec("sum", "sum", rate=True, ro=RATES[1]),
                  ["sum", "max"], bc, "rate")
    d = core.DownsamplingSpecification("0all-max")
    all_spec = core.make_spec(T0, T0 + 4 * HOUR, core.Aggregators.get("sum"),
                              d, T0 + 600000, T0 + 7200000)
    check_ignored(engine, all_spec, ["sum", "max"], b, "0all")
    raw = core.make_spec(T0, T0 + 3 * HOUR, core.Aggregators.get("sum"), None,
                         T0, T0 + 3 * HOUR)
    check_ignored(engine, raw, ["sum", "max"], b, "raw")


def test_cells_entry_ignores_the_flag(engine):
    import torch
    from opentsdb_amd import workload
    b = datasets.random_batch(11, n_series=60, n_groups=6)
    b = datasets.with_values(b, b.val, b.is_float)
    b.ts = np.ascontiguousarray(b.ts - b.ts % 1000)
    aggs = ["sum", "max"]
    db = _device_batch(b)
    for ms_frac in (0.0, 0.3):  # (mixed widths: decoded, then the multi call)
        enc = cells.encode_batch(b, np.random.default_rng(5), 0.0, ms_frac)
        d = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda()
             for k, v in enc.items()}
        dc = workload.DeviceCells(d, b.n_series)
        out = []
        for spec in (_spec("sum", "max", "nan"),
                     _fold_spec(_spec("sum", "max", "nan"), True)):
            res = _device_results(2, b.n_groups, 4 * len(b.ts) + 64)
            workload.run_cells_multi_device(engine, spec, aggs, dc, db, res)
            torch.cuda.synchronize()
            out.append(([_points(r, b.n_groups) for r in res],
                        engine.multi_counters(),
                        engine.multi_fold_counters()))
        assert out[1][2] == dict(fold_launches=0)
        assert out[0][1] == out[1][1]
        for i in range(2):
            same_bits(out[1][0][i], out[0][0][i], "cells/%d" % i)


# 8 ---------------------------------------------------------- context hygiene
def test_call_sequence_on_one_context():
    """folded multi -> single -> unflagged multi -> folded multi on one
    context, a failing folded call in between: every result equals a fresh
    context's (error words, clean-entry mark, tile cache, workspace)."""
    b = datasets.random_batch(11, n_series=60, n_groups=6)
    bi = _infinity_batch()
    s_avg, s_max = _spec("sum", "avg", "nan"), _spec("sum", "max")
    s_inf = _spec("sum", "max", end=T0 + 60000)
    lerp = [I.LERP] * 5

    def fresh(f):
        e = Engine(0)
        try:
            return f(e)
        finally:
            e.close()
    steps = [lambda e: e.run_multi(s_avg, FIVE, b, fold=True),
             lambda e: [e.run(s_max, b)],
             lambda e: e.run_multi(s_max, FIVE, b),
             lambda e: e.run_multi(s_max, FIVE, b, lerp, fold=True)]
    want = [fresh(f) for f in steps]
    e = Engine(0)
    try:
        for k, f in enumerate(steps):
            got = f(e)
            if k != 1:  # (the counters are the last multi call's)
                assert e.multi_fold_counters()["fold_launches"] == \
                    (1 if k in (0, 3) else 0)
            for i in range(len(got)):
                same_bits(got[i], want[k][i], "seq%d/%d" % (k, i))
            if k == 1:
                with pytest.raises(core.IllegalStateException):
                    e.run_multi(s_inf, ["max", "sum"], bi, fold=True)
    finally:
        e.close()
