"""The CPU oracle on the edges of the time domain (CPU only), against a
plain-Python model that shares no code with it, and the proof that the
batches of tests/time_domain.py tell a kernel whose relative times wrap at 32
bits from a correct one.  tests/test_gpu_time_domain.py compares the HIP
engine with the oracle on these batches.

The model: every bucket index is a Python int, (ts - grid0) // interval,
unbounded.  Downsampling sum / avg / min / max / count under fill none / nan /
zero (Downsampler.java:162-228, FillingDownsampler.java:172-298: a filling
grid is [align(start), align(end)), the seek rounds the start up to a bucket),
then the aggregation iterator's rules (AggregationIterator.java:395-797) for
sum / count / min / max under LERP and ZIM: a kept member contributes from its
first to its last bucket, its own value where it has one, interpolated toward
its next bucket otherwise, the bucket past the window included.

wrap32 is the same model with `ts - grid0` cut to 32 bits before the division:
  "bucket"  for the points the window holds, [grid0, grid0 + nb * interval)
            (the bounds are right, the bucket function is the narrow one: a
            wide grid sent down the narrow path);
  "bounds"  for every point of a kept series, one that then lands inside the
            grid being taken in (the bounds themselves are 32-bit compares).
"bucket" must agree with the oracle wherever nb * interval <= 2^32 and differ
where the window runs past 2^32 ms.  A window of lim = 2^32 // interval buckets
is wide by the predicate and still spans less than 2^32 ms (2^32 is a multiple
of none of the intervals), so it agrees there; the window of lim + 20 buckets
over the same batch is the one that differs.  "bounds" cannot agree on a
narrow grid whose batch holds points 2^32 ms past the base, as every batch
here does on purpose: it is asserted to differ, on the far-outside batches.
"""
import math

import numpy as np
import pytest

from opentsdb_amd import core
from oracle import pyoracle
from tests import time_domain as TD
from tests.test_gpu_parity import _raw, _spec, _vals

I = core.Interpolation
M32 = (1 << 32) - 1
DS_FNS = ["sum", "avg", "min", "max", "count"]
FILLS = ["none", "nan", "zero"]
AGGS = [("sum", I.LERP), ("sum", I.ZIM), ("count", I.ZIM), ("min", I.LERP),
        ("max", I.LERP), ("max", I.ZIM)]
ORDER_FREE_FN = {"min", "max", "count"}


# ------------------------------------------------------------------ model
def _double(bits, is_float):
    b = np.asarray(bits, np.int64)
    return np.where(np.asarray(is_float) == 1, b.view(np.float64),
                    b.astype(np.float64))


def grid(start, end, iv, fill):
    g0 = (start + iv - 1) // iv * iv
    if fill == "none":
        nb = (end - g0) // iv + 1 if end >= g0 else 0
    else:
        nb = max(0, (end // iv * iv - g0) // iv)
    return g0, nb


def bucket_lists(ts, vals, g0, nb, iv, wrap32):
    """{bucket index: the bucket's values in time order}."""
    out = {}
    stop = g0 + nb * iv
    for t, v in zip(ts.tolist(), vals.tolist()):
        inside = g0 <= t < stop
        if wrap32 == "bounds" and not inside:
            k = ((t - g0) & M32) // iv
            if k >= nb:
                k = (t - g0) // iv if t >= stop else None
        elif t < g0:
            continue
        elif wrap32 and inside:
            k = ((t - g0) & M32) // iv
        else:
            k = (t - g0) // iv
        if k is not None:
            out.setdefault(k, []).append(v)
    return out


def reduce_bucket(fn, v):
    if fn == "count":
        return float(len(v))
    if fn == "min":
        return min(v)
    if fn == "max":
        return max(v)
    s = 0.0
    for x in v:
        s += x
    return s / len(v) if fn == "avg" else s


def member_stream(buckets, fn, g0, nb, iv, fill):
    """The member's view stream, (ts[], value[]) in time order."""
    if fill == "none":
        ks = sorted(buckets)
        return (np.array([g0 + k * iv for k in ks], np.int64),
                np.array([reduce_bucket(fn, buckets[k]) for k in ks]))
    fv = math.nan if fill == "nan" else 0.0
    return (g0 + iv * np.arange(nb, dtype=np.int64),
            np.array([reduce_bucket(fn, buckets[k]) if k in buckets else fv
                      for k in range(nb)]))


def aggregate(streams, agg, interp, start, end):
    """One group: (ts[], value[]).  Sequential over the members in their
    order, as the iterator feeds the aggregator."""
    streams = [s for s in streams if len(s[0])]
    if not streams:
        return np.zeros(0, np.int64), np.zeros(0)
    x = np.unique(np.concatenate([t for t, _ in streams]))
    x = x[(x >= start) & (x <= end)]
    acc = np.zeros(len(x))
    n = np.zeros(len(x), np.int64)
    started = np.zeros(len(x), bool)
    for t, v in streams:
        live = (x >= t[0]) & (x <= t[-1])
        i = np.searchsorted(t, x)
        i1 = np.minimum(i, len(t) - 1)
        i0 = np.maximum(i - 1, 0)
        own = live & (t[i1] == x)
        if interp == I.ZIM:
            c = np.zeros(len(x))
        else:
            with np.errstate(invalid="ignore", divide="ignore"):
                c = v[i0] + (x - t[i0]).astype(np.float64) * (v[i1] - v[i0]) \
                    / (t[i1] - t[i0]).astype(np.float64)
        c = np.where(own, v[i1], c)
        ok = live & ~np.isnan(c)
        if agg in ("sum", "count"):
            acc = np.where(ok, acc + (c if agg == "sum" else 1.0), acc)
            n += ok
        else:
            first = live & ~started
            worst = math.inf if agg == "min" else -math.inf
            acc = np.where(first, np.where(np.isnan(c), worst, c), acc)
            better = (c < acc) if agg == "min" else (c > acc)
            acc = np.where(live & ~first & ok & better, c, acc)
            started |= live
    if agg == "sum":
        acc = np.where(n == 0, math.nan, acc)
    elif agg != "count":
        acc = np.where(np.isinf(acc), math.nan, acc)
    return x, acc


class Model:
    """The model over one (batch, window, interval, fill): the bucket lists
    are shared by every function and aggregator."""

    def __init__(self, hb, start, end, iv, fill, wrap32=None):
        self.hb, self.start, self.end, self.iv, self.fill = (hb, start, end,
                                                             iv, fill)
        self.g0, self.nb = grid(start, end, iv, fill)
        vals = _double(hb.val, hb.is_float)
        self.buckets = {}
        for s in range(hb.n_series):
            a, e = int(hb.offsets[s]), int(hb.offsets[s + 1])
            if e > a and hb.ts[a] <= end and hb.ts[e - 1] >= start:
                self.buckets[s] = bucket_lists(hb.ts[a:e], vals[a:e], self.g0,
                                               self.nb, iv, wrap32)

    def run(self, agg, interp, fn):
        hb, out = self.hb, []
        streams = {s: member_stream(b, fn, self.g0, self.nb, self.iv,
                                    self.fill)
                   for s, b in self.buckets.items()}
        for g in range(hb.n_groups):
            m = hb.group_members[hb.group_offsets[g]:hb.group_offsets[g + 1]]
            out.append(aggregate([streams[s] for s in m if s in streams], agg,
                                 interp, self.start, self.end))
        return out


def same(model, ref, exact):
    """None, or where the model and the oracle differ."""
    for g, ((ts, v), r) in enumerate(zip(model, ref)):
        if len(ts) != len(r) or not np.array_equal(ts, r["ts"]):
            return "g%d: timestamps" % g
        if r["is_int"].any():
            return "g%d: is_int" % g
        rv = r["bits"].view(np.float64)
        nan = np.isnan(rv)
        if not np.array_equal(np.isnan(v), nan):
            return "g%d: NaN pattern" % g
        if exact:
            bad = (v.view(np.int64) != r["bits"]) & ~nan
        else:
            bad = (np.abs(v - rv) > 1e-12 * np.maximum(np.abs(v),
                                                      np.abs(rv))) & ~nan
        if bad.any():
            k = int(np.nonzero(bad)[0][0])
            return "g%d: point %d, %r vs %r" % (g, k, v[k], rv[k])
    return None


def oracle(agg, interp, fn, fill, start, end, interval, hb):
    return pyoracle.group_by(_spec(agg, fn, fill, start, end, interp=interp,
                                   interval=interval), hb)


def sweep(hb, start, end, interval, fills=FILLS, fns=DS_FNS, aggs=AGGS,
          wrap32=None):
    """Every (fill, function, aggregator): [(where, None or difference)].
    Counts (the `count` function and aggregator) and timestamps compare bit
    for bit, as do the order-free functions; sums and averages to 1e-12."""
    iv = TD.interval_ms(interval)
    out = []
    for fill in fills:
        m = Model(hb, start, end, iv, fill, wrap32)
        for fn in fns:
            for agg, interp in aggs:
                ref = oracle(agg, interp, fn, fill, start, end, interval, hb)
                assert sum(len(r) for r in ref) > 0
                out.append(("%s:%s-%s-%s/%s" % (agg, interval, fn, fill,
                                                interp.name),
                            same(m.run(agg, interp, fn), ref,
                                 fn in ORDER_FREE_FN)))
    return out


def assert_agrees(res):
    bad = [(w, d) for w, d in res if d is not None]
    assert not bad, bad[:5]


def assert_differs(res, what):
    """The aliasing model is off for every function under some aggregator
    and for every fill."""
    diff = {w for w, d in res if d is not None}
    assert diff, what
    return diff


# ---------------------------------------------------- 1. the oracle, pinned
NAMES = {3_600_000: "1h", 1_800_000: "30m", 60_000: "1m"}


def boundary_sizes(iv):
    lim = TD.boundary_grid(iv)[0]
    return lim - 1, lim, lim + 20


@pytest.mark.parametrize("iv", TD.BOUNDARY_IVS)
def test_model_boundary_grids(iv):
    _, hb = TD.boundary_grid(iv)
    # (the 1 m grid holds 71,582 buckets a member: a reduced sweep)
    fns = {3_600_000: DS_FNS, 1_800_000: ["avg", "max", "count"],
           60_000: ["avg", "max"]}[iv]
    aggs = AGGS if iv != 60_000 else AGGS[:3]
    for nb in boundary_sizes(iv):
        for fill in FILLS if iv != 60_000 else FILLS[:2]:
            s, e = TD.boundary_window(iv, nb, fill)
            assert grid(s, e, iv, fill) == (TD.T0, nb)
            assert_agrees(sweep(hb, s, e, NAMES[iv], [fill], fns, aggs))


@pytest.mark.parametrize("interval", TD.WIDE_INTERVALS)
def test_model_wide_intervals(interval):
    iv = TD.interval_ms(interval)
    for hb in (TD.wide_interval_batch(), TD.wide_interval_batch(iv)):
        for s, e in TD.wide_windows(iv):
            assert_agrees(sweep(hb, s, e, interval))


def test_model_edge_points_sit_on_the_edges():
    for interval in TD.WIDE_INTERVALS:
        iv = TD.interval_ms(interval)
        hb = TD.wide_interval_batch(iv)
        t = hb.ts[hb.offsets[0]:hb.offsets[1]]
        assert (t % iv == 0).sum() >= 2 and (t % iv == iv - 1).sum() >= 2


def test_model_big_groups():
    nb, hb = TD.big_group_batch()
    assert list(np.diff(hb.group_offsets)) == list(TD.BIG_SIZES)
    assert not TD.is_narrow(TD.HOUR, nb)
    s, e = TD.boundary_window(TD.HOUR, nb, "none")
    assert_agrees(sweep(hb, s, e, "1h", ["none", "nan"], ["avg", "max"]))


@pytest.mark.parametrize("ms", [False, True])
@pytest.mark.parametrize("kind", TD.FAR_KINDS)
def test_model_far_outside(kind, ms):
    hb = TD.far_outside_batch(kind, ms)
    s, e = TD.far_window()
    for interval in ("1m", "10s"):
        assert_agrees(sweep(hb, s, e, interval))
        assert_agrees(sweep(hb, s, e + 1, interval, ["nan"]))


def test_model_trimmed_window():
    s, e, hb = TD.trimmed_window()
    assert_agrees(sweep(hb, s, e, "1h", ["none"]))
    ref = oracle("sum", I.LERP, "avg", "none", s, e, "1h", hb)
    first = min(int(r["ts"][0]) for r in ref if len(r))
    assert first > s + 2 * TD.HOUR  # the trimmed grid's base is not the start
    assert hb.n_series * ((e - s) // TD.HOUR) > 4e9


# ------------------------------------------- 2. the inputs tell them apart
@pytest.mark.parametrize("iv", TD.BOUNDARY_IVS)
def test_wrap32_at_the_boundary(iv):
    _, hb = TD.boundary_grid(iv)
    narrow, lim, wider = boundary_sizes(iv)
    fns = ["avg", "max", "count"] if iv == 3_600_000 else ["avg", "count"]
    aggs = AGGS if iv != 60_000 else AGGS[:3]
    for fill in FILLS if iv != 60_000 else FILLS[:2]:
        for nb in (narrow, lim):  # both span less than 2^32 ms
            assert nb * iv < TD.TWO32
            s, e = TD.boundary_window(iv, nb, fill)
            assert_agrees(sweep(hb, s, e, NAMES[iv], [fill], fns, aggs,
                                wrap32="bucket"))
        assert wider * iv > TD.TWO32
        s, e = TD.boundary_window(iv, wider, fill)
        res = sweep(hb, s, e, NAMES[iv], [fill], fns, aggs, wrap32="bucket")
        diff = assert_differs(res, (iv, fill))
        # every function is moved: count by whole points
        for fn in fns:
            assert any("-%s-" % fn in w for w in diff), (iv, fill, fn)


@pytest.mark.parametrize("interval", TD.WIDE_INTERVALS)
def test_wrap32_wide_intervals(interval):
    iv = TD.interval_ms(interval)
    hb = TD.wide_interval_batch()
    for s, e in TD.wide_windows(iv):
        for fill in FILLS:
            res = sweep(hb, s, e, interval, [fill], wrap32="bucket")
            g0, nb = grid(s, e, iv, fill)
            if nb < 2:
                # "1y" under a fill policy: one bucket of 2^34.9 ms, and a
                # truncated time below the interval is still bucket 0
                assert interval == "1y" and fill != "none"
                assert_agrees(res)
                continue
            assert nb * iv > TD.TWO32
            diff = assert_differs(res, (interval, fill))
            for fn in DS_FNS:
                assert any("-%s-" % fn in w for w in diff), (interval, fn)
    # the narrow neighbour: "24d" with one bucket
    if interval == "24d":
        a = TD.wide_windows(iv)[0][0]
        assert TD.is_narrow(iv, 1)
        assert_agrees(sweep(hb, a, a + iv - 1, interval, ["none"],
                            wrap32="bucket"))
        assert_agrees(sweep(hb, a, a + iv, interval, ["nan", "zero"],
                            wrap32="bucket"))


@pytest.mark.parametrize("ms", [False, True])
@pytest.mark.parametrize("kind", TD.FAR_KINDS)
def test_wrap32_far_outside(kind, ms):
    """32-bit bounds take the ghosts in: every function and fill is off, by
    1e6 x the in-window scale (sum, avg, max) or by whole points (count).
    With the bounds right, the window (1 h) has nothing to alias."""
    hb = TD.far_outside_batch(kind, ms)
    s, e = TD.far_window()
    for interval in ("1m", "10s"):
        for fill in FILLS:
            res = sweep(hb, s, e, interval, [fill], wrap32="bounds")
            diff = assert_differs(res, (kind, interval, fill))
            for fn in ("sum", "avg", "max", "count"):
                assert any("-%s-" % fn in w for w in diff), (interval, fn)
            assert_agrees(sweep(hb, s, e, interval, [fill], wrap32="bucket"))


@pytest.mark.parametrize("ms", [False, True])
@pytest.mark.parametrize("kind", TD.FAR_KINDS)
def test_far_outside_batch_holds_its_ghosts(kind, ms):
    hb = TD.far_outside_batch(kind, ms)
    census = TD.ghost_census(hb)
    assert len(census) == 2 * len(TD.G)
    assert all(n >= 100 for n in census.values()), census
    assert ((hb.ts % 1000 == 0).all()) == (not ms)
    # ghost-only members: before only, after only, both sides
    sides = set()
    for s in range(hb.n_series):
        t = hb.ts[hb.offsets[s]:hb.offsets[s + 1]]
        if len(t) and not ((t >= TD.W0) & (t < TD.W0 + TD.HOUR)).any():
            sides.add((bool((t < TD.W0).any()), bool((t > TD.W0).any())))
    assert sides == {(True, False), (False, True), (True, True)}
    # a ghost congruent to an occupied 10 s bucket, one to an empty one
    s0 = next(s for s in range(0, 24, 3)
              if hb.offsets[s + 1] > hb.offsets[s])  # a series with copies
    t = hb.ts[hb.offsets[s0]:hb.offsets[s0 + 1]]
    inw = t[(t >= TD.W0) & (t < TD.W0 + TD.HOUR)]
    out = t[(t < TD.W0) | (t >= TD.W0 + TD.HOUR)]
    g0 = grid(TD.W0, TD.W0 + TD.HOUR, 10_000, "none")[0]
    inw = inw[inw >= g0]
    occ = set(((inw - g0) // 10_000).tolist())
    alias = set((((out - g0) % TD.TWO32) // 10_000).tolist())
    alias = {k for k in alias if k < 360}
    assert alias & occ and alias - occ
    v = np.abs(_vals(hb.val, 1 - hb.is_float))
    far = (hb.ts < TD.W0 - TD.HOUR) | (hb.ts > TD.W0 + 2 * TD.HOUR)
    assert np.median(v[far]) > 1e4 * np.median(v[~far])


# -------------------------------------------------------- 3. the predicate
def test_narrow_predicate():
    def narrow(iv, nb):  # make_params: 32-bit offsets inside [gbase, stop_ts)
        return iv < 2**31 and nb < 2**32 // iv
    for iv, lim in ((3_600_000, 1193), (1_800_000, 2386), (60_000, 71582)):
        assert TD.boundary_grid(iv)[0] == lim
        assert narrow(iv, lim - 1) and not narrow(iv, lim)
        assert TD.is_narrow(iv, lim - 1) and not TD.is_narrow(iv, lim)
    d24, d25 = TD.interval_ms("24d"), TD.interval_ms("25d")
    assert d24 == 2_073_600_000
    assert narrow(d24, 1) and not narrow(d24, 2) and not narrow(d25, 1)
    assert not narrow(TD.interval_ms("1n"), 1)
    assert not narrow(TD.interval_ms("1y"), 1)
    assert all(TD.T0 % iv == 0 for iv in TD.BOUNDARY_IVS)


# ------------------------------------------- 4. every GPU query is accepted
def test_every_gpu_query_is_accepted():
    """The GPU file asserts n_accepted == n_queries: no query of it has a
    status other than OK, but the 2^44 case."""
    n = 0
    for where, spec, hb in TD.gpu_queries():
        try:
            ref = pyoracle.group_by(spec, hb)
        except pyoracle.OracleError as e:
            raise AssertionError("%s: status %d" % (where, e.status))
        assert sum(len(r) for r in ref) > 0, where
        n += 1
    assert n > 1000


def test_x1_mask_case():
    s, e = TD.T0, TD.T0 + 100_000
    spec = _raw("sum", s, e, interp=I.LERP)
    with pytest.raises(pyoracle.OracleError) as ei:
        pyoracle.group_by(spec, TD.x1_mask_batch(2**44))
    assert ei.value.status == core.IllegalStateException.status
    ref = pyoracle.group_by(spec, TD.x1_mask_batch(2**44 - 1))
    assert len(ref[0]) == 8 and ref[0]["is_int"].all()
    # B, between its two points, is 3 + 5000 k * 697 / 1.6e13 = 3 (long LERP)
    assert ref[0]["bits"].tolist() == [3] + [13 + i for i in range(1, 8)]
