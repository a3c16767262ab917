"""Value-domain edges against the CPU oracle: negative and huge doubles,
+-0.0, subnormals, longs over the whole 64-bit range, NaNs with payloads,
float32 cells, counters that wrap next to 2^63, and overflow to "Got
Infinity" — the values tests/datasets.py::random_batch never draws (floats
in [0, 100), longs in [-50, 100), counters near 2^32).  They reach the
order-preserving keys of every selection kernel (negative branch, -0.0
before 0.0), the raw path's Java `long` arithmetic, long -> double
conversion above 2^53, the order-free monoids at +-0.0 ties and the
absent-bucket sentinel.  tests/test_value_domain_cpu.py pins the oracle on
the same domain against references that share no code with it.

The comparison rules are the suite's: bit-exact where the downsampling
function and the aggregator are both computed in the reference's order
(ORDER_FREE_DS / EXACT_DS, EXACT_AGG; the whole raw path), 1e-12 relative
plus contribution_floor elsewhere.  One leniency is added, zero_sign_blind
below.
"""
import functools

import numpy as np
import pytest

from opentsdb_amd import core
from opentsdb_amd.engine import Engine
from oracle import pyoracle
from tests import datasets
from tests.test_gpu_parity import (ORDER_FREE_DS, RAW_AGGS, _member_scales,
                                   _raw, _spec, compare, contribution_floor,
                                   run_both)
from tests.test_gpu_sweep import EXACT_AGG, EXACT_DS
from tests.value_domain import (AGGS, COUNTER_TOPS, DS, FILLS, PERCENTILES,
                                RATE_AGGS, RATE_DS, SEL, SPAN, T0, WINDOWS,
                                base_batch, counter_batch, edge_batch,
                                matrix, rate_options)

pytestmark = pytest.mark.gpu


def is_exact(agg, ds):
    """The suite's rule: a downsampling function computed bit-identically
    (order-free ones, selections, dev's one Welford pass, diff) feeding an
    aggregator that is (order-free ones, selections, dev, diff)."""
    sel = set(SEL) | PERCENTILES
    return ((ds in EXACT_DS or ds in ORDER_FREE_DS or ds in sel) and
            (agg in EXACT_AGG or agg in sel))


@pytest.fixture(scope="module")
def engine():
    from opentsdb_amd import build
    build.build()
    e = Engine(0)
    yield e
    e.close()


def zero_sign_blind(got, ref):
    """The one leniency of this file.  The reference's percentile sorts its
    doubles with `<` (commons-math Percentile over a double[]), under which
    -0.0 and 0.0 are equal: which of the two a percentile lands on is
    unspecified, in the reference as in the oracle's qsort.  A percentile
    result that is +-0.0 on both sides therefore compares by value: its
    bits are taken from the oracle.  It is applied only where the
    aggregator or the downsampling function is one of PERCENTILES.  Median
    does not get this: Median sorts a List<Double> (Double.compareTo, -0.0
    first), which the oracle and the kernels' keys both follow; nor does
    any other aggregator."""
    for a, r in zip(got, ref):
        if len(a.ts) != len(r):
            continue
        bits = np.array(a.bits, np.int64)
        z = ((bits << 1) == 0) & ((r["bits"] << 1) == 0) & \
            ~np.asarray(a.is_int).astype(bool) & ~r["is_int"].astype(bool)
        bits[z] = r["bits"][z]
        a.bits = bits
    return got


class Checker:
    """check() of test_gpu_parity with the per-member view streams of
    contribution_floor shared between the aggregators of one downsampling
    specification (they do not depend on the aggregator)."""

    def __init__(self, engine, batch):
        self.engine, self.batch, self.views = engine, batch, {}
        self.got = None  # the engine's result of the last accepted query

    def __call__(self, spec, exact, where, key=None, blind=False,
                 may_reject=False):
        got, ref = run_both(self.engine, spec, self.batch)
        self.got = got
        if ref is None:  # both sides reject the query: status parity
            assert may_reject, where + ": rejected by the reference"
            return None
        floor = 0.0
        if not exact:
            views = self.views.get(key) if key is not None else None
            if views is None:
                views = _member_scales(spec, self.batch)
                if key is not None:
                    self.views[key] = views
            floor = contribution_floor(spec, self.batch, ref, views)
        if blind:
            self.got = got = zero_sign_blind(got, ref)
        compare(got, ref, exact, where, floor)
        return ref


# ------------------------------------------- 1. downsampled fold x kinds
@pytest.mark.parametrize("grouping", ["a", "b"])
@pytest.mark.parametrize("kind", ["signed", "bigint", "bigmixed",
                                  "nanpayload"])
def test_downsampled_fold(engine, kind, grouping):
    """Every cross-series aggregator over every 1m downsampling function
    and fill policy: the monoids at +-0.0 ties (MMinMax keeps the earliest,
    MSum normalises -0.0), long -> double above 2^53, sums whose terms span
    300 decades and cancel."""
    b = edge_batch(kind, grouping)
    ck = Checker(engine, b)
    n = 0
    for agg, ds, fill in matrix():
        s, e = WINDOWS[0]
        n += ck(_spec(agg, ds, fill, s, e), is_exact(agg, ds),
                "%s/%s/%s:1m-%s-%s" % (kind, grouping, agg, ds, fill),
                key=(ds, fill, 0)) is not None
    assert n == len(matrix())  # tests/test_value_domain_cpu.py: all accepted
    s, e = WINDOWS[1]
    for i, agg in enumerate(AGGS):
        ds, fill = DS[i % len(DS)], FILLS[i % 3]
        ck(_spec(agg, ds, fill, s, e), is_exact(agg, ds),
           "%s/%s/cut/%s:1m-%s-%s" % (kind, grouping, agg, ds, fill),
           key=(ds, fill, 1))
    # interpolation between values of opposite sign and of 2^63 magnitude:
    # 10s buckets over a 20s cadence leave every other bucket to LERP / PREV
    for interp in (core.Interpolation.LERP, core.Interpolation.PREV):
        for agg in ("sum", "max", "min"):
            s, e = WINDOWS[0]
            ck(_spec(agg, "max", "none", s, e, interp=interp, interval="10s"),
               agg != "sum",
               "%s/%s/%s/%s" % (kind, grouping, interp.name, agg),
               key=("max", "none", "10s"))


@pytest.mark.parametrize("grouping", ["a", "b"])
def test_nan_payload_buckets(engine, grouping):
    """NaNs of several bit patterns, the absent-bucket sentinel
    0x7FF4DEAD0BADF00D among them, as bucket values: first / last / mult do
    not skip NaN, so a 10s bucket holding one such point is that NaN (1m
    buckets hold three points).  The emitted timestamps and the NaN pattern
    must be the oracle's: a bucket whose value is a NaN is present."""
    b = edge_batch("nanpayload", grouping)
    sentinel = np.uint64(datasets.NAN_PATTERNS[-1]).view(np.int64)
    assert (b.val == sentinel).sum() >= 5
    ck = Checker(engine, b)
    for interval in ("10s", "1m"):
        for ds in ("first", "last", "mult"):
            for agg in ("sum", "count", "first", "last", "max", "min"):
                for fill in FILLS:
                    s, e = WINDOWS[0]
                    ck(_spec(agg, ds, fill, s, e, interval=interval),
                       is_exact(agg, ds) and ds != "mult",
                       "nanp/%s/%s:%s-%s-%s" % (grouping, agg, interval, ds,
                                                fill),
                       key=(ds, fill, interval),
                       may_reject=ds == "mult")  # a product overflows


# ------------------------------------------------ 2. selection everywhere
@pytest.mark.parametrize("grouping", ["a", "b", "c"])
@pytest.mark.parametrize("kind", ["signed", "bigint"])
def test_selection_across_series(engine, kind, grouping):
    """median / percentiles across series: the LDS sort (a), k_seg_select's
    direct gather (b) and its digit passes (c) on keys of both signs."""
    b = edge_batch(kind, grouping)
    ck = Checker(engine, b)
    for s, e in WINDOWS:
        for agg in SEL:
            for fill in ("none", "nan"):
                ck(_spec(agg, "max", fill, s, e), True,
                   "sel/%s/%s/%s/%s" % (kind, grouping, agg, fill),
                   blind=agg in PERCENTILES)


@pytest.mark.parametrize("kind", ["signed", "bigint"])
def test_selection_fill_large_groups(engine, kind):
    """Fill-mode percentiles with every group large: the keys transpose
    applies the fill (FILL) — a 0.0 fill between keys of both signs."""
    b = edge_batch(kind, "f")
    ck = Checker(engine, b)
    for s, e in WINDOWS:
        for agg in SEL:
            for fill in ("zero", "null"):
                ck(_spec(agg, "max", fill, s, e), True,
                   "selfill/%s/%s/%s" % (kind, agg, fill),
                   blind=agg in PERCENTILES)


@pytest.mark.parametrize("kind", ["signed", "bigint"])
def test_selection_downsampling(engine, kind):
    """median / percentiles as the downsampling function (k_ds_select): 1m
    buckets of 3 points (the LDS insertion sort, at most DS_SMALL) and one
    10m bucket of 30 (the wave radix select)."""
    b = edge_batch(kind, "a")
    ck = Checker(engine, b)
    for interval in ("1m", "10m"):
        for ds in SEL:
            for agg, fill in (("max", "none"), ("min", "nan"),
                              ("last", "zero")):
                s, e = WINDOWS[0]
                ck(_spec(agg, ds, fill, s, e, interval=interval), True,
                   "selds/%s/%s:%s-%s-%s" % (kind, agg, interval, ds, fill),
                   blind=ds in PERCENTILES)


@pytest.mark.parametrize("grouping", ["a", "b"])
@pytest.mark.parametrize("kind", ["signed", "bigint"])
def test_selection_raw(engine, kind, grouping):
    """k_raw_select / wave_select: raw_dkey on doubles of both signs,
    raw_lkey on longs (median) and (double)long keys (percentiles)."""
    b = edge_batch(kind, grouping)
    ck = Checker(engine, b)
    for s, e in WINDOWS:
        for agg in SEL:
            ck(_raw(agg, s, e), True,
               "selraw/%s/%s/%s" % (kind, grouping, agg),
               blind=agg in PERCENTILES)


# ----------------------------------------------------- 3. raw long path
@pytest.mark.parametrize("grouping", ["a", "b"])
@pytest.mark.parametrize("kind", ["bigint", "bigmixed"])
def test_raw_long_arithmetic(engine, kind, grouping):
    """runLong in Java long arithmetic over the whole 64-bit range: sums,
    squares and products that wrap, truncating division, the long LERP
    y0 + (x - x0) * (y1 - y0) / (x1 - x0) with wrapping operands, (long)
    casts that saturate, isInteger over current and next slots."""
    b = edge_batch(kind, grouping)
    ck = Checker(engine, b)
    for agg in RAW_AGGS:
        for s, e in WINDOWS:
            ck(_raw(agg, s, e), True, "rawlong/%s/%s/%s" % (kind, grouping,
                                                           agg),
               blind=agg in PERCENTILES,
               may_reject=agg in ("none", "mult"))  # > 1 value; overflow
    for interp in core.Interpolation:
        for agg in ("sum", "avg", "max"):
            s, e = WINDOWS[0]
            ck(_raw(agg, s, e, interp=interp), True,
               "rawlong/%s/%s/%s/%s" % (kind, grouping, interp.name, agg),
               # several +-Double.MAX_VALUE fill-ins in one double sum
               may_reject=kind == "bigmixed" and interp.name in ("MAX",
                                                                "MIN"))


def dup_edge_batch(kind, seed=113):
    """_dup_batch's construction (runs of 2-4 copies of a point with new
    values, inside spans and at their ends) over grouping a, every value
    drawn from edge_values(kind)."""
    from opentsdb_amd.batch import HostBatch
    b = base_batch("a")
    rng = np.random.default_rng(seed)
    offs, ts = [0], []
    for s in range(b.n_series):
        t = b.ts[b.offsets[s]:b.offsets[s + 1]]
        reps = np.ones(len(t), np.int64)
        if len(t):
            pick = rng.random(len(t)) < 0.08
            if rng.random() < 0.5:
                pick[-1] = True  # copies of the span's last point
            reps[pick] = rng.integers(2, 5, int(pick.sum()))
        ts.append(np.repeat(t, reps))
        offs.append(offs[-1] + len(ts[-1]))
    ts = np.concatenate(ts)
    bits, isf = datasets.edge_values(kind, rng, len(ts))
    return HostBatch(np.array(offs, np.int64), ts, bits, isf, None,
                     b.group_offsets, b.group_members)


@pytest.mark.parametrize("kind", ["bigint", "bigmixed"])
def test_raw_long_repeated_timestamps(engine, kind):
    b = dup_edge_batch(kind)
    assert (np.diff(b.ts) == 0).sum() > 10
    ck = Checker(engine, b)
    for agg in ("sum", "avg", "max", "dev", "count", "first", "last", "diff",
                "mimmin", "squareSum", "mult", "p90", "median"):
        for interp in (None, core.Interpolation.PREV):
            ck(_raw(agg, T0 + 40_000, T0 + SPAN, interp=interp), True,
               "rawdup/%s/%s/%s" % (kind, agg, interp),
               blind=agg in PERCENTILES, may_reject=agg == "mult")


# ------------------------------------------- 4. rates of large counters
@pytest.mark.parametrize("ri", range(5))
@pytest.mark.parametrize("top_name", list(COUNTER_TOPS))
def test_rates_of_large_counters(engine, top_name, ri):
    """Counters that run up to and wrap at 2^63 - 1 and 2^62 (longs) and
    2^53 (doubles).  The raw path differences two longs in long arithmetic
    (RateSpan.java:121-180: exact above 2^53, where differencing their
    doubles is not), the downsampled path differences bucket doubles."""
    b = counter_batch(top_name)
    ro = rate_options(COUNTER_TOPS[top_name][0])[ri]
    ck = Checker(engine, b)
    for s, e in WINDOWS:
        for agg in RATE_AGGS:
            blind = agg in PERCENTILES
            ck(_raw(agg, s, e, rate=True, ro=ro), True,
               "rawrate/%s/r%d/%s" % (top_name, ri, agg), blind=blind)
            for ds in RATE_DS:
                ck(_spec(agg, ds, "none", s, e, rate=True, ro=ro),
                   is_exact(agg, ds),
                   "rate/%s/r%d/%s:1m-%s" % (top_name, ri, agg, ds),
                   key=(ds, s), blind=blind or ds in PERCENTILES)


# --------------------------------------------------- 5. overflow parity
@pytest.mark.parametrize("rate", [False, True])
@pytest.mark.parametrize("grouping", ["a", "b"])
def test_overflow_parity(engine, grouping, rate):
    """+-Double.MAX_VALUE and 10^+-300: sums, squares, LERPs, percentile
    interpolation and rates overflow.  The engine must reject exactly the
    queries the reference rejects ("Got Infinity",
    AggregationIterator.java:640-643; run_both asserts the statuses equal)
    and be bit-exact on the accepted bit-exact combinations."""
    b = edge_batch("wide", grouping)
    ck = Checker(engine, b)
    ro = core.RateOptions() if rate else None
    s, e = WINDOWS[0]
    n_ok = n_rej = 0
    for agg, ds, fill in matrix():
        spec = _spec(agg, ds, fill, s, e, rate=rate, ro=ro)
        if is_exact(agg, ds):
            ok = ck(spec, True, "wide/%s/%s:1m-%s-%s" % (grouping, agg, ds,
                                                         fill),
                    may_reject=True) is not None
        else:
            ok = run_both(engine, spec, b)[1] is not None
        n_ok += ok
        n_rej += not ok
    for agg in RAW_AGGS:
        spec = _raw(agg, s, e, rate=rate, ro=ro)
        ok = ck(spec, True, "wide/%s/raw/%s" % (grouping, agg),
                blind=agg in PERCENTILES, may_reject=True) is not None
        n_ok += ok
        n_rej += not ok
    assert n_ok > 0 and n_rej > 0, (n_ok, n_rej)


# ------------------------------------------------------- 6. byte paths
def _whole_seconds(hb):
    hb = datasets.with_values(hb, hb.val, hb.is_float)
    hb.ts[:] = hb.ts - hb.ts % 1000
    for s in range(hb.n_series):
        assert (np.diff(hb.ts[hb.offsets[s]:hb.offsets[s + 1]]) > 0).all()
    return hb


BYTE_QUERIES = [("sum", "max"), ("min", "min"), ("p99", "max")]


def _byte_spec(agg, ds):
    return core.make_spec(T0, T0 + SPAN, core.Aggregators.get(agg),
                          core.DownsamplingSpecification("1m-" + ds), T0,
                          T0 + SPAN)


def test_float4_cells(engine):
    """4-byte float cells holding float32 subnormals, +-0.0, +-FLT_MAX and
    NaNs: the decode alone against RowSeq's, then the fused cells query."""
    import torch
    from opentsdb_amd import workload
    from opentsdb_amd.batch import HostBatch
    from opentsdb_amd.engine import DeviceResult
    from tests import cells
    from tests.test_gpu_decode import (_device_batch, _result_points,
                                       decode_gpu)
    b = _whole_seconds(edge_batch("f4edge", "a"))
    enc = cells.encode_batch(b, np.random.default_rng(5), float4_frac=1.0)
    # every value is a 4-byte float: 4 bytes per 2-byte qualifier, and the
    # trailing meta byte on columns of more than one value
    n_pts = np.diff(enc["qual_off"]) // 2
    assert np.array_equal(np.diff(enc["qual_off"]), 2 * n_pts)
    assert np.array_equal(np.diff(enc["val_off"]), 4 * n_pts + (n_pts > 1))
    pts = [pyoracle.decode_row(
        enc["qual"][enc["qual_off"][r]:enc["qual_off"][r + 1]].tobytes(),
        enc["val"][enc["val_off"][r]:enc["val_off"][r + 1]].tobytes(),
        enc["row_base_s"][r]) for r in range(len(enc["row_series"]))]
    pts = np.concatenate(pts)
    offs, ts, val, isf = decode_gpu(engine, enc, b.n_series)
    assert np.array_equal(offs, b.offsets)
    assert np.array_equal(ts, pts["ts"]) and np.array_equal(ts, b.ts)
    assert (isf == 1).all() and not pts["is_int"].any()
    nan = np.isnan(pts["bits"].view(np.float64))
    assert nan.sum() > 5 and np.array_equal(np.isnan(val.view(np.float64)),
                                            nan)
    assert np.array_equal(val[~nan], pts["bits"][~nan])
    # every non-NaN float32 value comes back as the double it is
    assert np.array_equal(val[~nan], b.val[~nan])
    hb = HostBatch(b.offsets, pts["ts"], pts["bits"],
                   np.ones(len(pts), np.uint8), None, b.group_offsets,
                   b.group_members)
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda()
         for k, v in enc.items()}
    dc = workload.DeviceCells(d, b.n_series)
    db = _device_batch(hb, "float")
    for agg, ds in (("sum", "max"), ("max", "first")):
        spec = _byte_spec(agg, ds)
        ref = pyoracle.group_by(spec, hb)
        res = DeviceResult(torch, db.n_groups, 4 * len(hb.ts) + 64, "cuda")
        workload.run_cells_device(engine, spec, dc, db, res)
        compare(_result_points(res, db.n_groups), ref, is_exact(agg, ds),
                "f4cells/%s:1m-%s" % (agg, ds),
                floor=contribution_floor(spec, hb, ref))


@pytest.mark.parametrize("kind", ["bigint", "signed"])
def test_device_encoded_cells_and_rows(engine, kind):
    """8-byte longs next to 1 / 2 / 4-byte ones (-1, 0, small values) and
    8-byte floats through the device encoder, the cells fold and the
    storage-row path (compaction, span assembly)."""
    import torch
    from opentsdb_amd import storage, workload
    from opentsdb_amd.engine import DeviceResult
    from tests import cells
    from tests.test_gpu_decode import _device_batch, _result_points
    from tests.test_gpu_rows import _raw_from_hb
    b = _whole_seconds(edge_batch(kind, "a"))
    if kind == "bigint":  # every value width in every row
        small = np.array([1, -1, 0, 127, -128, 300, -32768, 70000, -2**31,
                          2**31 - 1, 2**31, -2**31 - 1], np.int64)
        b.val[::3] = small[np.arange(len(b.val[::3])) % len(small)]
    db = _device_batch(b, "float" if kind == "signed" else "int")
    dc = workload.encode_cells_device(engine, db)
    ref_enc = cells.encode_batch(b)
    got = {k: v.cpu().numpy() for k, v in dc.t.items()}
    V = ref_enc["val_off"][-1]
    assert np.array_equal(got["val_off"], ref_enc["val_off"])
    assert np.array_equal(got["val"][:V], ref_enc["val"][:V])
    rng = np.random.default_rng(7)
    raw = storage.HostRawRows(_raw_from_hb(rng, b), with_ts=True).to_device()
    raw.n_series = b.n_series
    for agg, ds in BYTE_QUERIES:
        spec = _byte_spec(agg, ds)
        ref = pyoracle.group_by(spec, b)
        fl = contribution_floor(spec, b, ref)
        res = DeviceResult(torch, b.n_groups, 4 * len(b.ts) + 4096, "cuda")
        workload.run_cells_device(engine, spec, dc, db, res)
        got_c = _result_points(res, b.n_groups)
        res = DeviceResult(torch, b.n_groups, 4 * len(b.ts) + 4096, "cuda")
        storage.run_raw_device(engine, spec, raw, db, res)
        got_r = _result_points(res, b.n_groups)
        for name, g in (("cells", got_c), ("rows", got_r)):
            if agg in PERCENTILES:
                g = zero_sign_blind(g, ref)
            compare(g, ref, is_exact(agg, ds),
                    "%s/%s/%s:1m-%s" % (name, kind, agg, ds), floor=fl)


# ----------------------------------------------- 7. transpose tile edges
KT_NB = [1, 63, 64, 65, 256, 257]


@functools.lru_cache(maxsize=None)
def tile_batch(m, split):
    """m series over 2,600 s (260 10s buckets) of friendly values, 5 % NaN,
    a few empty series; one group, or two whose boundary lies inside a
    k_keys_transpose tile (5/12 of m: never a multiple of KT_M)."""
    from opentsdb_amd.batch import groups_from_ids
    b = datasets.random_batch(400 + m, n_series=m, big_group=True,
                              span_ms=2_600_000, cadence_ms=20_000,
                              nan_frac=0.05, empty_frac=0.03, outside=False)
    if split:
        gid = (np.arange(m) >= (m * 5) // 12).astype(np.int64)
        b.group_offsets, b.group_members = groups_from_ids(gid, 2)
    return b


@pytest.mark.parametrize("split", [False, True], ids=["1group", "2groups"])
@pytest.mark.parametrize("m", [33, 127, 128, 129, 256, 257])
def test_keys_transpose_tile_edges(engine, m, split):
    """k_keys_transpose works in tiles of KT_M = 128 members and
    OTSDB_KT_SLICES = 4 bucket slices: member counts at and next to a
    multiple of KT_M, group boundaries inside a tile, and 1 .. 257 buckets
    (one slice, 63 / 64 / 65 around a 64-bucket sweep, every slice
    occupied), non-fill and fill."""
    b = tile_batch(m, split)
    ck = Checker(engine, b)
    for nb in KT_NB:
        for agg in ("p99", "median"):
            for fill in ("none", "zero"):
                # nb buckets: the iterator's window ends inside the last
                # one, the filling grid stops short of the window's end
                end = T0 + nb * 10_000 - (1 if fill == "none" else 0)
                ref = ck(_spec(agg, "max", fill, T0, end, interval="10s"),
                         True, "kt/%d/%s/nb%d/%s/%s" % (m, split, nb, agg,
                                                       fill))
                assert all(len(r) == nb for r in ref), (nb, fill)
