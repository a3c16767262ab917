"""The engine's three host units (engine.hip, engine_rows.hip,
engine_hist.hip) behind one C-ABI: a failure raised in any of them is the
calling thread's otsdb_last_error(), and one context serves queries of all
three in any order with the results of a fresh context, bit for bit (they
share the context's buffers and the call scopes of engine_int.h)."""
import ctypes as C

import numpy as np
import pytest

from opentsdb_amd import abi, core, storage
from opentsdb_amd.batch import HostBatch
from tests import datasets

pytestmark = pytest.mark.gpu

T0 = datasets.T0


def test_last_error_text_from_every_unit():
    """One argument check that fails before any device work in each unit:
    the status, and that unit's message right after its call."""
    from opentsdb_amd.engine import Engine
    eng = Engine(0)
    lib = eng.lib
    try:
        def last():
            return lib.otsdb_last_error().decode()

        # engine_rows.hip
        raw = abi.RawRows()
        raw.n_rows = -1
        n = C.c_int64()
        st = lib.otsdb_compact_rows_device(eng.ctx, C.byref(raw), 1, None, 0,
                                           0, C.byref(n), None)
        assert st == abi.E_ILLEGAL_ARGUMENT
        assert last() == "negative n_rows"

        # engine_hist.hip: no percentile and no counts output
        spec = core.make_spec(T0, T0 + 9999, core.Aggregators.get("sum"),
                              core.DownsamplingSpecification("1s-sum"))
        lower = np.array([0.0, 1.0], np.float32)
        upper = np.array([1.0, 2.0], np.float32)
        h = abi.HistColumns(2, lower.ctypes.data, upper.ctypes.data, None)
        offs = np.zeros(2, np.int64)
        ts = np.zeros(16, np.int64)
        hr = abi.HistResult(16, offs.ctypes.data, ts.ctypes.data, None, None)
        b = abi.Batch()
        st = lib.otsdb_hist_run_device(eng.ctx, C.byref(spec), C.byref(b),
                                       C.byref(h), None, 0, C.byref(hr), None)
        assert st == abi.E_ILLEGAL_ARGUMENT
        assert last() == "no percentile and no counts output asked for"

        # engine.hip: a null spec
        res = abi.Result()
        st = lib.otsdb_agg_run_device(eng.ctx, None, C.byref(b), C.byref(res),
                                      None)
        assert st == abi.E_ILLEGAL_ARGUMENT
        assert last() == "null"

        # and back: the text is the last failure's, whichever unit raised it
        st = lib.otsdb_compact_rows_device(eng.ctx, C.byref(raw), 1, None, 0,
                                           0, C.byref(n), None)
        assert st == abi.E_ILLEGAL_ARGUMENT
        assert last() == "negative n_rows"
    finally:
        eng.close()


# ------------------------------------------- one context, all three units
MIB = 1 << 20  # a context buffer's first allocation (DevBuf::ensure)


def _single(n_points, cadence):
    """3 groups x 5 series x n_points points, one every `cadence` ms,
    sum:1m-avg over the whole span."""
    rng = np.random.default_rng(11)
    S, G = 15, 3
    ts = np.concatenate([T0 + int(rng.integers(0, cadence)) +
                         cadence * np.arange(n_points, dtype=np.int64)
                         for _ in range(S)])
    val = (rng.random(S * n_points) * 100.0).view(np.int64)
    hb = HostBatch(np.arange(S + 1, dtype=np.int64) * n_points, ts, val,
                   np.ones(S * n_points, np.uint8), None,
                   np.array([0, 5, 10, 15], np.int64),
                   rng.permutation(S).astype(np.int64))
    end = T0 + cadence * n_points
    spec = core.make_spec(T0, end, core.Aggregators.get("sum"),
                          core.DownsamplingSpecification("1m-avg"), T0, end)

    def run(eng):
        return [(d.ts.copy(), d.bits.copy(), d.is_int.copy())
                for d in eng.run(spec, hb)]
    run.staged_bytes = 17 * len(ts)  # ts, value and type of every point
    # What run_pipeline carves from the workspace `ws`, on every path: per
    # (tile, bucket) a 32-byte partial and an emit byte, per (group, bucket)
    # an 8-byte value and an emit byte.  A group with members is one tile or
    # more and no tile holds less than a member, so G <= tiles <= S.  Off the
    # fold path the S x NB bucket rows (9 bytes a bucket) come on top; the
    # per-series arrays and the 256-byte alignment of ~30 blocks stay under
    # 64 KiB here.
    nb = (end - T0) // 60000 + 1
    partial = C.sizeof(abi.Partial) + 1
    run.ws_at_least = (G * partial + G * 9) * nb
    run.ws_at_most = (S * partial + G * 9 + S * 9) * nb + (64 << 10)
    return run


def _rows():
    """About 20 storage rows (4 series x 5 hours, some hours split over two
    rows, the points scattered over columns) through otsdb_agg_run_raw."""
    from tests.test_gpu_rows import _raw_from_hb
    hb = datasets.random_batch(7, n_series=4, n_groups=2,
                               span_ms=5 * 3600000, cadence_ms=60000,
                               empty_frac=0.0, outside=False)
    hb.ts[:] = hb.ts - hb.ts % 1000
    hb.is_float = np.ones(len(hb.ts), np.uint8)
    rows = _raw_from_hb(np.random.default_rng(5), hb)
    assert 20 <= len(rows) <= 40
    hraw = storage.HostRawRows(rows, with_ts=True)
    hraw.n_series = hb.n_series
    end = T0 + 5 * 3600000
    spec = core.make_spec(T0, end, core.Aggregators.get("sum"),
                          core.DownsamplingSpecification("1m-avg"), T0, end)

    def run(eng):
        return [a.copy() for a in storage.run_raw(
            eng, spec, hraw, hb.group_offsets, hb.group_members,
            4 * len(hb.ts) + 64)]
    return run


def _hist():
    """8 bins, 2 percentiles, 6 series in 2 groups over 20 buckets."""
    from tests import test_gpu_hist as TH
    rng = np.random.default_rng(3)
    K = 8
    series = [TH.rand_series(rng, K, sorted(rng.choice(20, 12, replace=False)))
              for _ in range(6)]
    case = TH.Case(series, [[0, 1, 2, 3], [4, 5, 1]], *TH.schema(K))
    spec = TH.spec_of("1s-sum", TH.T0, TH.T0 + 20 * TH.IV - 1)
    hb, hc = case.host()

    def run(eng):
        out = []
        for p in eng.run_hist(spec, hb, hc, [50.0, 99.0], want_counts=True):
            out += [p.ts.copy(), np.asarray(p.pct).view(np.int64).copy(),
                    p.counts.copy()]
        return out
    return run


def _flat(r):
    return [a for x in r for a in (x if isinstance(x, tuple) else (x,))]


def _same(got, want):
    got, want = _flat(got), _flat(want)
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and np.array_equal(a, b)


def test_one_context_serves_all_three_units():
    """single, rows, histogram, then histogram, rows and the single query
    with 50 x the points (10,000 a series, two minutes apart: 20,000 buckets)
    on one context: each result is the one a fresh context gives that ran
    only that query.  The first five leave the workspace `ws`, which all
    three units carve from, and the staging buffer at their first 1 MiB; the
    last query needs more of both, so both are freed and allocated anew."""
    from opentsdb_amd.engine import Engine
    small, large = _single(200, 10000), _single(10000, 120000)
    rows, hist = _rows(), _hist()
    want = {}
    for name, q in (("small", small), ("large", large), ("rows", rows),
                    ("hist", hist)):
        fresh = Engine(0)
        try:
            want[name] = q(fresh)
        finally:
            fresh.close()
    assert sum(len(t) for t, _, _ in want["small"]) > 0
    assert len(want["rows"][1]) > 0 and len(want["hist"][0]) > 0
    eng = Engine(0)
    try:
        # only the large query outgrows the buffers' first 1 MiB (the rows
        # and histogram queries are smaller than the small one: 4 and 6
        # series, 2 groups, 300 and 20 buckets, 10 counts a histogram cell)
        assert small.staged_bytes < MIB < large.staged_bytes
        assert small.ws_at_most < MIB < large.ws_at_least
        for name, q in (("small", small), ("rows", rows), ("hist", hist),
                        ("hist", hist), ("rows", rows), ("large", large)):
            _same(q(eng), want[name])
    finally:
        eng.close()
