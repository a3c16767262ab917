"""Multi-aggregator queries (otsdb_agg_run_multi*): several cross-series
aggregators over ONE downsample pass of the same query.  Needs an MI355X.

Output i of a multi call obeys the contract of the single query with that
aggregator: (a) it is compared with the CPU oracle run with that aggregator
under the exact / tolerance rule the single-aggregator test of the same shape
uses (tests/test_gpu_parity.py), and (b) where the downsampling function is
order-free it is bit-identical to Engine.run with that aggregator.  The
counters of Engine.multi_counters() show what was shared.
"""
import ctypes as C

import numpy as np
import pytest

from opentsdb_amd import abi, core
from opentsdb_amd.batch import HostBatch
from opentsdb_amd.engine import DataPoints, Engine
from oracle import pyoracle
from tests import cells, datasets
from tests.test_gpu_parity import (AGGS, ORDER_FREE, RATES, _spec,
                                   cancel_floor, compare)

pytestmark = pytest.mark.gpu

T0 = datasets.T0
SEL_K = 32  # groups of more members take the key transpose + radix select


@pytest.fixture(scope="module")
def engine():
    from opentsdb_amd import build
    build.build()
    e = Engine(0)
    yield e
    e.close()


def same_bits(a, b, where=""):
    assert len(a) == len(b), where
    for g, (x, y) in enumerate(zip(a, b)):
        w = "%s/g%d" % (where, g)
        assert np.array_equal(np.asarray(x.ts), np.asarray(y.ts)), w + ": ts"
        assert np.array_equal(np.asarray(x.bits), np.asarray(y.bits)), w + ": bits"
        assert np.array_equal(np.asarray(x.is_int), np.asarray(y.is_int)), w


def with_agg(spec, agg, interp=None):
    s = type(spec).from_buffer_copy(spec)
    s.agg_id = core.Aggregators.get(agg).id
    s.interp = -1 if interp is None else int(interp)
    return s


def check_multi(engine, spec, aggs, batch, exact, where, interps=None,
                floor=None, singles=False):
    """run_multi, then per output: the oracle with that aggregator
    (exact(agg) / floor(agg): the single-aggregator test's rule) and, with
    singles, bit-identity with Engine.run."""
    got = engine.run_multi(spec, aggs, batch, interps)
    assert len(got) == len(aggs)
    for i, agg in enumerate(aggs):
        si = with_agg(spec, agg, None if interps is None else interps[i])
        w = "%s/%d:%s" % (where, i, agg)
        ref = pyoracle.group_by(si, batch)
        compare(got[i], ref, exact(agg) if callable(exact) else exact, w,
                floor(agg) if floor else 0.0)
        if singles:
            same_bits(got[i], engine.run(si, batch), w + "/single")
    return got


def big_groups(batch):
    k = np.diff(np.asarray(batch.group_offsets))
    return bool((k > SEL_K).any())


# 1 ------------------------------------------------ all aggregators, 5 classes
@pytest.mark.parametrize("ds", ["avg", "max"])
def test_all_aggregators_small_groups(engine, ds):
    """The 22 aggregators of the parity matrix in one call: every
    interpolation class (LERP, ZIM, MAX, MIN, PREV via pfsum), scalars, dev
    and selections.  max buckets are exact and every group is one chain in
    SpanCmp order: bit-exact, and bit-identical to the single queries; avg
    buckets are tree-reduced (1e-12; diff: cancellation)."""
    b = datasets.random_batch(11, n_series=60, n_groups=6)
    fl = cancel_floor(b, 2)
    check_multi(engine, _spec("sum", ds), AGGS, b, ds == "max", "all/" + ds,
                floor=lambda a: fl if a == "diff" else 0.0, singles=ds == "max")
    c = engine.multi_counters()
    assert c["downsample_passes"] == 1, c
    # one transpose serves every selection; it runs only when a group is past
    # the LDS-sort limit (none of this shape's six groups of ~10 is)
    assert c["key_transposes"] == (1 if big_groups(b) else 0), c
    assert c["transform_passes"] == 5, c


# 2 ------------------------------------------------- explicit interpolation
def test_explicit_interpolation(engine):
    b = datasets.random_batch(41, n_series=30, n_groups=3)
    I = core.Interpolation
    aggs = ["sum", "sum", "sum", "max", "first"]
    interps = [I.LERP, I.ZIM, I.PREV, I.MAX, I.MIN]
    spec = _spec("sum", "min", interval="10s")
    got = check_multi(engine, spec, aggs, b, True, "interp", interps=interps,
                      singles=True)
    assert engine.multi_counters()["transform_passes"] == 5
    # the class matrices differ: LERP / ZIM / PREV sums are not one result
    bits = [np.concatenate([np.asarray(g.bits) for g in got[i]])
            for i in range(3)]
    assert not np.array_equal(bits[0], bits[1])
    assert not np.array_equal(bits[0], bits[2])


# 3 ---------------------------------------------------------- fill and window
@pytest.mark.parametrize("fill", ["nan", "zero", "null"])
@pytest.mark.parametrize("aligned", [True, False])
def test_fill_and_window(engine, fill, aligned):
    b = datasets.random_batch(31, n_series=25, n_groups=4, nan_frac=0.02)
    start = T0 + (0 if aligned else 61000)
    aggs = ["sum", "avg", "min", "count", "p99", "median"]
    check_multi(engine, _spec("sum", "max", fill, start=start), aggs, b, True,
                "fill/%s/%s" % (fill, aligned), singles=True)
    c = engine.multi_counters()
    # a fill policy: the contribution does not depend on the interpolation
    assert c["transform_passes"] == 1 and c["downsample_passes"] == 1, c


# 4 ---------------------------------------------------------------------- rate
@pytest.mark.parametrize("ri", [1, 3])
@pytest.mark.parametrize("fill", ["none", "nan"])
def test_rate(engine, ri, fill):
    b = datasets.random_batch(52, n_series=30, n_groups=3, counter=True)
    aggs = ["sum", "dev", "avg", "count", "max", "p99"]
    for aligned in (True, False):
        start = T0 + (0 if aligned else 61000)
        spec = _spec("sum", "sum", fill, start=start, rate=True, ro=RATES[ri])
        check_multi(engine, spec, aggs, b, True,
                    "rate%d/%s/%s" % (ri, fill, aligned), singles=True)
        c = engine.multi_counters()
        assert c["transform_passes"] == 1 and c["downsample_passes"] == 1, c


# 5 ------------------------------------------------- groups past one chunk
def test_groups_past_one_chunk(engine):
    """700 members: per-slot tile partials + the ordered merge for the
    scalars, dev as one chain, and a large-group selection in the same
    call."""
    b = datasets.random_batch(71, n_series=700, big_group=True,
                              span_ms=3600 * 1000, cadence_ms=30000)
    aggs = ["sum", "avg", "dev", "min", "count", "first", "last", "diff",
            "median", "p99"]
    fl = cancel_floor(b, 2)
    exact = lambda a: a in ORDER_FREE or a in ("dev", "median", "p99")  # noqa
    check_multi(engine, _spec("sum", "max", end=T0 + 3600 * 1000), aggs, b,
                exact, "big", floor=lambda a: fl if a == "diff" else 0.0,
                singles=True)
    c = engine.multi_counters()
    assert c["downsample_passes"] == 1 and c["key_transposes"] == 1, c


# 6 ----------------------------------------------------------- percentile sets
SEL_AGGS = ["median", "p50", "p75", "p99", "p999", "ep95r3", "ep50r7"]


@pytest.mark.parametrize("n_series,kind", [(45, "float"), (300, "float"),
                                           (5000, "float"), (5000, "int")])
@pytest.mark.parametrize("fill", ["none", "nan"])
def test_percentile_sets(engine, n_series, kind, fill):
    b = datasets.random_batch(77, n_series=n_series, big_group=True,
                              span_ms=3600 * 1000, cadence_ms=30000,
                              nan_frac=0.05 if kind == "float" else 0.0,
                              value_kind=kind)
    check_multi(engine, _spec("p99", "max", fill, end=T0 + 3600 * 1000),
                SEL_AGGS, b, True, "sel%d/%s/%s" % (n_series, kind, fill))
    c = engine.multi_counters()
    assert c["key_transposes"] == 1 and c["downsample_passes"] == 1, c


def test_percentiles_fill_several_large_groups(engine):
    b = datasets.random_batch(79, n_series=300, n_groups=3,
                              span_ms=3600 * 1000, cadence_ms=30000,
                              nan_frac=0.05, empty_frac=0.1)
    n_empty = 40
    offs = np.concatenate([b.offsets, np.full(n_empty, b.offsets[-1])])
    g_off = np.concatenate([b.group_offsets, [b.group_offsets[-1] + n_empty]])
    members = np.concatenate([b.group_members,
                              300 + np.arange(n_empty, dtype=np.int64)])
    b2 = HostBatch(offs.astype(np.int64), b.ts, b.val, b.is_float, None,
                   g_off.astype(np.int64), members.astype(np.int64))
    check_multi(engine, _spec("p99", "avg", "zero", end=T0 + 3600 * 1000),
                ["median", "p50", "p99", "p999", "ep95r3"], b2, True,
                "selfill")
    assert engine.multi_counters()["key_transposes"] == 1


# 7 ---------------------------------------- selection downsampling and 0all
@pytest.mark.parametrize("ds", ["p90", "median"])
def test_selection_downsampling(engine, ds):
    b = datasets.random_batch(27, n_series=24, n_groups=3, nan_frac=0.1)
    check_multi(engine, _spec("sum", ds), ["sum", "max", "p50"], b, True,
                "dssel/" + ds, singles=True)
    assert engine.multi_counters()["downsample_passes"] == 1


def test_run_all(engine):
    b = datasets.random_batch(61, n_series=20, n_groups=4)
    qs, qe = T0 + 600000, T0 + 7200000
    d = core.DownsamplingSpecification("0all-max")
    spec = core.make_spec(T0, T0 + 4 * 3600 * 1000,
                          core.Aggregators.get("sum"), d, qs, qe)
    check_multi(engine, spec, ["sum", "max", "count"], b, True, "all",
                singles=True)
    assert engine.multi_counters()["downsample_passes"] == 1


# 8 -------------------------------------------------------------------- errors
def _infinity_batch():
    big = 1.5e308
    return HostBatch.from_groups(
        [[[(T0 + 1000 * i, big, 1) for i in range(5)]] * 3])


def test_errors(engine):
    b = _infinity_batch()
    spec = _spec("sum", "max", end=T0 + 60000)
    with pytest.raises(core.IllegalStateException):  # sum: "Got Infinity"
        engine.run_multi(spec, ["max", "sum", "min"], b)
    # the other outputs of such a set alone are fine
    same_bits(engine.run_multi(spec, ["max", "min"], b)[0],
              engine.run(with_agg(spec, "max"), b))
    b2 = datasets.random_batch(81, n_series=6, n_groups=2, outside=False,
                               empty_frac=0)
    with pytest.raises(core.IllegalDataException):  # none fed > 1 value
        engine.run_multi(_spec("count", "avg"), ["count", "none"], b2)
    # outputs 1 and 2 fail differently: the lower index decides
    with pytest.raises(core.IllegalDataException):
        engine.run_multi(spec, ["max", "none", "sum"], b)
    with pytest.raises(core.IllegalStateException):
        engine.run_multi(spec, ["max", "sum", "none"], b)
    # ... and in the unshared fallback (raw group-by)
    raw = core.make_spec(T0, T0 + 60000, core.Aggregators.get("sum"), None,
                         T0, T0 + 60000)
    with pytest.raises(core.IllegalDataException):
        engine.run_multi(raw, ["max", "none", "sum"], b)
    with pytest.raises(core.NoSuchElementException):
        engine.run_multi(spec, [0, 99], b)


@pytest.mark.parametrize("n_out", [0, 33])
def test_n_out_out_of_range(engine, n_out):
    b = datasets.random_batch(11, n_series=6, n_groups=2)
    spec = _spec("sum", "max")
    ids = np.zeros(max(n_out, 1), np.int32)
    it = np.full(max(n_out, 1), -1, np.int32)
    rs = (abi.Result * max(n_out, 1))()
    ab = b.as_abi()
    lib = engine.lib
    sz = abi.Sizes()
    assert lib.otsdb_agg_plan_multi(engine.ctx, C.byref(spec), n_out,
                                    ids.ctypes.data, it.ctypes.data,
                                    C.byref(ab), C.byref(sz)) == \
        abi.E_ILLEGAL_ARGUMENT
    assert lib.otsdb_agg_run_multi(engine.ctx, C.byref(spec), n_out,
                                   ids.ctypes.data, it.ctypes.data,
                                   C.byref(ab), rs) == abi.E_ILLEGAL_ARGUMENT
    assert lib.otsdb_agg_run_multi_device(
        engine.ctx, C.byref(spec), n_out, ids.ctypes.data, it.ctypes.data,
        C.byref(ab), rs, None) == abi.E_ILLEGAL_ARGUMENT


# 9 ---------------------------------------------------------------- degenerate
@pytest.mark.parametrize("ds", ["avg", "max"])
def test_single_output_is_the_single_query(engine, ds):
    b = datasets.random_batch(11, n_series=60, n_groups=6)
    for agg in ("sum", "dev", "p99"):
        spec = _spec(agg, ds)
        same_bits(engine.run_multi(spec, [agg], b)[0], engine.run(spec, b),
                  "one/%s/%s" % (agg, ds))


def test_duplicates(engine):
    b = datasets.random_batch(11, n_series=60, n_groups=6)
    got = engine.run_multi(_spec("sum", "avg"), ["sum", "sum", "p99", "p99"],
                           b)
    same_bits(got[0], got[1], "dup/sum")
    same_bits(got[2], got[3], "dup/p99")


def test_empty_and_degenerate(engine):
    aggs = ["sum", "max", "p99", "dev"]
    b = HostBatch.from_groups([[[], []], []])
    check_multi(engine, _spec("sum", "avg"), aggs, b, True, "empty")
    b = datasets.random_batch(91, n_series=10, n_groups=2)
    spec = _spec("sum", "avg", start=T0 - 10 * 3600 * 1000,
                 end=T0 - 9 * 3600 * 1000)
    check_multi(engine, spec, aggs, b, True, "before")
    # a group without members beside groups with data (shared rows)
    b = datasets.random_batch(91, n_series=10, n_groups=2)
    g_off = np.concatenate([b.group_offsets, [b.group_offsets[-1]]])
    b3 = HostBatch(b.offsets, b.ts, b.val, b.is_float, None, g_off,
                   b.group_members)
    check_multi(engine, _spec("sum", "max"), aggs, b3, True, "emptygroup",
                singles=True)
    assert engine.multi_counters()["downsample_passes"] == 1


def _host_call(engine, spec, aggs, batch, caps):
    """otsdb_agg_run_multi with caller-chosen capacities ->
    (status, offsets [n, G+1])."""
    n = len(aggs)
    ids = np.array([core.Aggregators.get(a).id for a in aggs], np.int32)
    it = np.full(n, -1, np.int32)
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
    st = engine.lib.otsdb_agg_run_multi(engine.ctx, C.byref(spec), n,
                                        ids.ctypes.data, it.ctypes.data,
                                        C.byref(ab), rs)
    return st, offs


def test_host_capacity(engine):
    """A result too small: E_CAPACITY, its offsets whole (offsets[G] the
    point count it needs), as otsdb_agg_run leaves them."""
    b = datasets.random_batch(11, n_series=60, n_groups=6)
    spec = _spec("sum", "max")
    aggs = ["sum", "max", "p99"]
    full = engine.run_multi(spec, aggs, b)
    need = [sum(len(g.ts) for g in out) for out in full]
    st, offs = _host_call(engine, spec, aggs, b, [need[0], 5, need[2]])
    assert st == abi.E_CAPACITY
    # what the single entry leaves for the same capacity
    s1 = with_agg(spec, "max")
    o1 = np.full(b.n_groups + 1, -7, np.int64)
    a = [np.zeros(5, np.int64), np.zeros(5, np.int64), np.zeros(5, np.uint8)]
    r1 = abi.Result(5, o1.ctypes.data, a[0].ctypes.data, a[1].ctypes.data,
                    a[2].ctypes.data)
    ab = b.as_abi()
    assert engine.lib.otsdb_agg_run(engine.ctx, C.byref(s1), C.byref(ab),
                                    C.byref(r1)) == abi.E_CAPACITY
    assert np.array_equal(offs[1], o1) and offs[1][-1] == need[1]
    # enough room everywhere: the same call passes
    st, offs = _host_call(engine, spec, aggs, b, need)
    assert st == abi.OK and [int(o[-1]) for o in offs] == need


# 10 --------------------------------------------------------- unshared fallback
def test_raw_query_runs_the_singles(engine):
    b = datasets.random_batch(101, n_series=24, n_groups=4, cadence_ms=37000)
    raw = core.make_spec(T0, T0 + 3 * 3600 * 1000,
                         core.Aggregators.get("sum"), None, T0,
                         T0 + 3 * 3600 * 1000)
    aggs = ["sum", "max", "p90"]
    got = engine.run_multi(raw, aggs, b)
    assert engine.multi_counters()["downsample_passes"] == len(aggs)
    for i, a in enumerate(aggs):
        same_bits(got[i], engine.run(with_agg(raw, a), b), "raw/" + a)


# 11 -------------------------------------------------------- entry points agree
def _device_batch(hb):
    import torch
    from opentsdb_amd.engine import DeviceBatch
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()  # noqa
    n = len(hb.ts)
    ts = torch.zeros(max(n, 2), dtype=torch.int64, device="cuda")
    val = torch.zeros_like(ts)
    isf = torch.zeros(max(n, 2), dtype=torch.uint8, device="cuda")
    ts[:n], val[:n], isf[:n] = t(hb.ts), t(hb.val), t(hb.is_float)
    return DeviceBatch(t(hb.offsets), ts[:n], val[:n], t(hb.group_offsets),
                       t(hb.group_members), isf[:n], None)


def _device_results(n, G, cap):
    import torch
    from opentsdb_amd.engine import DeviceResult
    return [DeviceResult(torch, G, cap, "cuda") for _ in range(n)]


def _points(res, G):
    offs = res.offsets.cpu().numpy()
    ts, val, ii = (res.ts.cpu().numpy(), res.val.cpu().numpy(),
                   res.is_int.cpu().numpy())
    return [DataPoints(ts[offs[g]:offs[g + 1]], val[offs[g]:offs[g + 1]],
                       ii[offs[g]:offs[g + 1]]) for g in range(G)]


@pytest.mark.parametrize("ms_frac", [0.0, 0.3])
def test_entry_points_agree(engine, ms_frac):
    """Host, device and cells entries: the same bits.  The cells are the
    batch as compacted columns, whole-second qualifiers or 30 % forced to
    4-byte ms ones (mixed widths: the engine rewrites the qualifiers).

    1m-max: all three bit-identical.  1m-avg: host and device bit-identical
    (the same kernels); the cells entry downsamples with k_bucketize_cells,
    whose lanes sum a bucket's points in another tree than k_bucketize_k's
    (as for any single row-path query from cells; measured here: last-bit
    differences on some buckets), so its avg outputs are held to the oracle
    under the rule of test_all_aggregators_small_groups instead."""
    import torch
    from opentsdb_amd import workload
    from opentsdb_amd.engine import run_multi_device
    b = datasets.random_batch(11, n_series=60, n_groups=6)
    b = datasets.with_values(b, b.val, b.is_float)
    b.ts = np.ascontiguousarray(b.ts - b.ts % 1000)
    aggs = AGGS
    for ds in ("avg", "max"):
        spec = _spec("sum", ds)
        host = engine.run_multi(spec, aggs, b)
        cap = max(sum(len(g.ts) for g in out) for out in host) + 8
        db = _device_batch(b)
        res = _device_results(len(aggs), b.n_groups, cap)
        run_multi_device(engine, spec, aggs, db, res)
        torch.cuda.synchronize()
        for i, a in enumerate(aggs):
            same_bits(_points(res[i], b.n_groups), host[i], "device/" + a)
        enc = cells.encode_batch(b, np.random.default_rng(5), 0.0, ms_frac)
        d = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda()
             for k, v in enc.items()}
        dc = workload.DeviceCells(d, b.n_series)
        res = _device_results(len(aggs), b.n_groups, cap)
        workload.run_cells_multi_device(engine, spec, aggs, dc, db, res)
        torch.cuda.synchronize()
        assert engine.multi_counters()["downsample_passes"] == 1
        fl = cancel_floor(b, 2)
        for i, a in enumerate(aggs):
            got = _points(res[i], b.n_groups)
            if ds == "max":
                same_bits(got, host[i], "cells/" + a)
            else:
                compare(got, pyoracle.group_by(with_agg(spec, a), b), False,
                        "cells/avg/" + a, fl if a == "diff" else 0.0)


# 12 ---------------------------------------------------------- context hygiene
def test_context_hygiene():
    """single -> multi -> single -> multi on one context: every result
    equals a fresh context's (error words, tile cache, workspace)."""
    b = datasets.random_batch(11, n_series=60, n_groups=6)
    bi = _infinity_batch()
    s_sum, s_p99 = _spec("sum", "max"), _spec("p99", "avg", "nan")
    s_inf = _spec("sum", "max", end=T0 + 60000)
    set1, set2 = ["min", "avg", "max", "p99"], ["dev", "sum", "median"]

    def fresh(f):
        e = Engine(0)
        try:
            return f(e)
        finally:
            e.close()
    want = [fresh(lambda e: e.run(s_sum, b)),
            fresh(lambda e: e.run_multi(s_sum, set1, b)),
            fresh(lambda e: e.run(s_p99, b)),
            fresh(lambda e: e.run_multi(s_p99, set2, b))]
    e = Engine(0)
    try:
        same_bits(e.run(s_sum, b), want[0], "h0")
        got = e.run_multi(s_sum, set1, b)
        for i in range(len(set1)):
            same_bits(got[i], want[1][i], "h1/%d" % i)
        # a failing multi call in between leaves nothing behind
        with pytest.raises(core.IllegalStateException):
            e.run_multi(s_inf, ["max", "sum"], bi)
        same_bits(e.run(s_p99, b), want[2], "h2")
        with pytest.raises(core.IllegalStateException):
            e.run(s_inf, bi)
        got = e.run_multi(s_p99, set2, b)
        for i in range(len(set2)):
            same_bits(got[i], want[3][i], "h3/%d" % i)
        same_bits(e.run(s_sum, b), want[0], "h4")
    finally:
        e.close()
