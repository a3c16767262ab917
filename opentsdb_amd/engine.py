"""The aggregation engine as the reference's callers see it.

`Engine.run(spec, batch)` is the batched replacement of
`for each SpanGroup: SpanGroup.iterator()` (SpanGroup.java:525-530) — one
native call evaluates every group of a query on the GPU.  Results come back as
`DataPoints` (array-backed SeekableView, DataPoints.java:29-240 /
SeekableView.java:37-71), so code written against the reference's iterator
contract keeps working.

The native library is mandatory: there is no CPU fallback.
"""
import ctypes as C

import numpy as np

from . import abi
from .core import (Aggregator, Aggregators, IllegalArgumentException,
                   IllegalStateException, NoSuchElementException,
                   UnsupportedOperationException, raise_for_status)


class DataPoint:
    """One aggregated point (DataPoint.java:20)."""
    __slots__ = ("_ts", "_bits", "_is_int")

    def __init__(self, ts, bits, is_int):
        self._ts, self._bits, self._is_int = int(ts), int(bits), bool(is_int)

    def timestamp(self):
        return self._ts

    def isInteger(self):
        return self._is_int

    def longValue(self):
        if not self._is_int:
            raise TypeError("value is a double")
        return self._bits

    def doubleValue(self):
        if self._is_int:
            raise TypeError("value is a long")
        return float(np.int64(self._bits).view(np.float64))

    def toDouble(self):
        return float(self._bits) if self._is_int else self.doubleValue()


class DataPoints:
    """The output series of one group, array-backed."""

    def __init__(self, ts, bits, is_int):
        self.ts = ts
        self.bits = bits
        self.is_int = is_int

    def size(self):
        return len(self.ts)

    __len__ = size

    def timestamp(self, i):
        return int(self.ts[i])

    def values(self):
        """Values as float64 (longs converted)."""
        out = self.bits.view(np.float64).copy()
        ints = self.is_int.astype(bool)
        out[ints] = self.bits[ints].astype(np.float64)
        return out

    def iterator(self):
        return SeekableView(self)

    def __iter__(self):
        it = self.iterator()
        while it.hasNext():
            yield it.next()


class SeekableView:
    """hasNext/next/seek over a DataPoints (SeekableView.java:37-71)."""

    def __init__(self, dps):
        self.dps = dps
        self.i = 0

    def hasNext(self):
        return self.i < len(self.dps.ts)

    def next(self):
        if not self.hasNext():
            raise NoSuchElementException("no more elements")
        i = self.i
        self.i += 1
        return DataPoint(self.dps.ts[i], self.dps.bits[i], self.dps.is_int[i])

    def seek(self, timestamp):
        self.i = int(np.searchsorted(self.dps.ts, timestamp, side="left"))


def multi_args(aggs, interps=None):
    """The aggregator set of a multi-aggregator call as the C-ABI takes it:
    (n_out, int32 ids, int32 interpolations).  `aggs`: core.Aggregators
    entries, names (Aggregators.get: NoSuchElementException) or ids;
    `interps`: one interpolation per output, None = the aggregator's own.
    Checked before anything touches the device."""
    aggs = list(aggs)
    if not 1 <= len(aggs) <= abi.MULTI_MAX:
        raise IllegalArgumentException(
            "%d aggregators: a multi-aggregator call takes 1 to %d"
            % (len(aggs), abi.MULTI_MAX))
    ids = np.empty(len(aggs), np.int32)
    for i, a in enumerate(aggs):
        if isinstance(a, str):
            a = Aggregators.get(a)
        ids[i] = a.id if isinstance(a, Aggregator) else int(a)
    if interps is None:
        it = np.full(len(aggs), -1, np.int32)
    else:
        interps = list(interps)
        if len(interps) != len(aggs):
            raise IllegalArgumentException(
                "%d interpolations for %d aggregators"
                % (len(interps), len(aggs)))
        it = np.array([-1 if v is None else int(v) for v in interps], np.int32)
        if ((it < -1) | (it > 4)).any():
            raise IllegalArgumentException("bad interpolation in %r" % (interps,))
    return len(aggs), ids, it


def panel_args(queries):
    """The queries of a panel call as the C-ABI takes them: (n_out, int32
    downsampling function ids, int32 aggregator ids, int32 interpolations).
    `queries`: (aggregator, downsampling function[, interpolation]) each, the
    functions given as multi_args takes aggregators, the interpolation None
    for the aggregator's own.  Checked before anything touches the device."""
    queries = [tuple(q) for q in queries]
    if not 1 <= len(queries) <= abi.MULTI_MAX:
        raise IllegalArgumentException(
            "%d queries: a panel call takes 1 to %d"
            % (len(queries), abi.MULTI_MAX))
    for q in queries:
        if len(q) not in (2, 3):
            raise IllegalArgumentException(
                "a panel query is (aggregator, downsampling function"
                "[, interpolation]): %r" % (q,))
    n, ids, it = multi_args([q[0] for q in queries],
                            [q[2] if len(q) == 3 else None for q in queries])
    _, ds, _ = multi_args([q[1] for q in queries])
    if (ds == Aggregators.NONE.id).any():
        raise IllegalArgumentException(
            "cannot use the NONE aggregator for downsampling")
    return n, ds, ids, it


def rollup_args(spec, rollup_agg, value_count):
    """The rollup arguments of a rollup call as the C-ABI takes them:
    (rollup aggregator id, int64 counts or None).  `rollup_agg`: the rollup
    table's aggregator (RollupQuery.getRollupAgg) as multi_args takes
    aggregators; `value_count`: every point's valueCount(), required when the
    rollup aggregator is avg.  Checked before anything touches the device."""
    _, ids, _ = multi_args([rollup_agg])
    r = int(ids[0])
    if r not in Aggregators._by_id:
        raise NoSuchElementException("No such aggregator: %d" % r)
    if r == Aggregators.DEV.id:
        raise UnsupportedOperationException(
            "standard deviation over rolled up data is not supported")
    if not (spec.ds_interval_ms > 0 or spec.run_all):
        raise UnsupportedOperationException(
            "a rollup query downsamples: raw group-by is not supported")
    if spec.n_cal_anchors > 0:
        raise UnsupportedOperationException(
            "rollup queries over per-series calendar anchors are not supported")
    if r != Aggregators.AVG.id:
        return r, None  # the counts are ignored
    if spec.ds_agg_id != Aggregators.AVG.id:
        raise UnsupportedOperationException(
            "rollup avg downsampled with another function is not supported")
    if value_count is None:
        raise IllegalArgumentException(
            "a rollup avg query needs every point's value_count")
    return r, value_count


def rollup_rows_args(spec, rollup_agg, table):
    """The rollup arguments of a call over a rollup table's storage rows:
    (rollup aggregator id, abi.RollupTable).  rollup_args' checks with the
    counts still to come (the decode pairs them), then the table's.  `table`:
    an abi.RollupTable or (interval_s, value_id, count_id, fix_duplicates)."""
    r, _ = rollup_args(spec, rollup_agg, True)
    if not isinstance(table, abi.RollupTable):
        table = abi.RollupTable(*[int(v) for v in table])
    if table.interval_s <= 0:
        raise IllegalArgumentException(
            "rollup interval %d s" % table.interval_s)
    return r, table


def _groups_abi(batch):
    """The otsdb_batch of a call whose points come from storage rows:
    n_series and the groups of `batch` (host arrays), no point arrays."""
    b = abi.Batch()
    b.n_series = batch.n_series
    b.n_points = 0
    b.n_groups = batch.n_groups
    b.group_offsets = batch.group_offsets.ctypes.data
    b.group_members = (batch.group_members.ctypes.data
                       if len(batch.group_members) else None)
    return b


def _host_results(n, G, cap):
    """n host results of capacity `cap` for G groups: the abi.Result array
    and a function that slices them into one list of DataPoints (one per
    group) per result, after the call filled them."""
    offs = np.zeros((n, G + 1), np.int64)
    ts = np.zeros((n, cap), np.int64)
    bits = np.zeros((n, cap), np.int64)
    isint = np.zeros((n, cap), np.uint8)
    rs = (abi.Result * n)()
    for i in range(n):
        rs[i] = abi.Result(cap, offs[i].ctypes.data, ts[i].ctypes.data,
                           bits[i].ctypes.data, isint[i].ctypes.data)

    def points():
        return [[DataPoints(ts[i, offs[i, g]:offs[i, g + 1]],
                            bits[i, offs[i, g]:offs[i, g + 1]],
                            isint[i, offs[i, g]:offs[i, g + 1]])
                 for g in range(G)] for i in range(n)]
    return rs, points


class Engine:
    """One context per GPU (one process per GPU)."""

    def __init__(self, device=0):
        self.lib = abi.load()
        self.ctx = C.c_void_p()
        self._check(self.lib.otsdb_ctx_create(int(device), C.byref(self.ctx)))
        self.device = device

    def _counters(self, n):
        out = (C.c_int64 * n)()
        self._check(self.lib.otsdb_ctx_counters(self.ctx, out, n))
        return out

    def counters(self):
        """otsdb_ctx_counters: {cells folds run uniform / general, uniform
        folds re-run with the general kernel; the last otsdb_sel_* session's
        passes over the local keys and histogram passes}."""
        out = self._counters(5)
        return dict(cells_uniform=out[0], cells_general=out[1],
                    cells_uniform_miss=out[2], sel_key_reads=out[3],
                    sel_passes=out[4])

    def multi_counters(self):
        """Of the last multi-aggregator call (otsdb_ctx_counters [5..8]):
        downsample passes over the point stream, group-stage passes over a
        row matrix, key transposes, transform passes (one per interpolation
        class).  A call that cannot share the rows runs its outputs as single
        queries: downsample and group passes then count those."""
        out = self._counters(9)
        return dict(downsample_passes=out[5], group_passes=out[6],
                    key_transposes=out[7], transform_passes=out[8])

    def multi_fold_counters(self):
        """Of the last multi-aggregator call (otsdb_ctx_counters [12]):
        multi-aggregator folds launched — 1 when the call asked for the fold
        (fold=True) and was eligible, else 0."""
        return dict(fold_launches=int(self._counters(13)[12]))

    def panel_counters(self):
        """Of the last panel call (otsdb_ctx_counters [10..11]): passes over
        the point stream (one for all envelope functions that share a pass,
        one per multi call otherwise) and row matrices built."""
        out = self._counters(12)
        return dict(point_stream_passes=out[10], row_matrices=out[11])

    def sel_sessions(self):
        """otsdb_ctx_counters [9]: otsdb_sel_* sessions prepared since the
        context was created (a retargeted session counts once)."""
        return int(self._counters(10)[9])

    def close(self):
        if self.ctx:
            self.lib.otsdb_ctx_destroy(self.ctx)
            self.ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, st):
        if st != 0:
            raise_for_status(st, self.lib.otsdb_last_error().decode())

    def plan(self, spec, batch):
        sz = abi.Sizes()
        self._check(self.lib.otsdb_agg_plan(self.ctx, C.byref(spec),
                                            C.byref(batch.as_abi()),
                                            C.byref(sz)))
        return sz

    def run(self, spec, batch):
        """Host-array path (what a JNI shim calls).  Returns one DataPoints
        per group, in group order."""
        sz = self.plan(spec, batch)
        cap = max(1, int(sz.max_out_points))
        G = batch.n_groups
        offs = np.zeros(G + 1, np.int64)
        ts = np.zeros(cap, np.int64)
        bits = np.zeros(cap, np.int64)
        isint = np.zeros(cap, np.uint8)
        r = abi.Result(cap, offs.ctypes.data, ts.ctypes.data,
                       bits.ctypes.data, isint.ctypes.data)
        b = batch.as_abi()
        self._check(self.lib.otsdb_agg_run(self.ctx, C.byref(spec), C.byref(b),
                                           C.byref(r)))
        return [DataPoints(ts[offs[g]:offs[g + 1]], bits[offs[g]:offs[g + 1]],
                           isint[offs[g]:offs[g + 1]]) for g in range(G)]

    def run_rollup(self, spec, batch, rollup_agg, value_count=None):
        """A query over rollup-table points (host arrays): `batch` holds the
        rollup cells' values, `rollup_agg` is the table's aggregator and
        `value_count[i]` point i's valueCount().  Rollup avg downsampled with
        avg is sum of sums / sum of counts; any other rollup aggregator (dev
        aside) downsampled with count sums the cells; every other pair is
        what run() gives.  Results as run()'s."""
        r, vc = rollup_args(spec, rollup_agg, value_count)
        n = int(batch.offsets[-1]) if len(batch.offsets) else 0
        if vc is not None:
            vc = np.ascontiguousarray(vc, dtype=np.int64)
            if vc.shape != (n,):
                raise IllegalArgumentException(
                    "value_count has %s entries for %d points"
                    % (vc.shape, n))
        sz = self.plan(spec, batch)
        rs, points = _host_results(1, batch.n_groups,
                                   max(1, int(sz.max_out_points)))
        b = batch.as_abi()
        self._check(self.lib.otsdb_agg_run_rollup(
            self.ctx, C.byref(spec), C.byref(b), r,
            None if vc is None else vc.ctypes.data, rs))
        return points()[0]

    def run_rollup_rows(self, spec, rows, table, rollup_agg, batch):
        """run_rollup() from a rollup table's storage rows (host arrays):
        `rows` is a storage.HostRawRows of the scanner's rows (one column per
        cell), `table` an abi.RollupTable (or its four fields), `rollup_agg`
        the table's aggregator; `batch` supplies n_series and the groups (its
        point arrays are not read).  The sum and count cells are paired and
        decoded on the device.  Results as run()'s."""
        r, table = rollup_rows_args(spec, rollup_agg, table)
        b = _groups_abi(batch)
        sz = abi.Sizes()
        self._check(self.lib.otsdb_agg_plan(self.ctx, C.byref(spec),
                                            C.byref(b), C.byref(sz)))
        rs, points = _host_results(1, batch.n_groups,
                                   max(1, int(sz.max_out_points)))
        raw = rows.as_abi()
        self._check(self.lib.otsdb_agg_run_rollup_rows(
            self.ctx, C.byref(spec), C.byref(raw), C.byref(table), r,
            C.byref(b), rs))
        return points()[0]

    def hist_counters(self):
        """Of the last histogram call (otsdb_ctx_counters [13..14]):
        k_hist_fold launches (one aggregation for every percentile) and
        percentile passes over the dense sums."""
        out = self._counters(15)
        return dict(fold_launches=int(out[13]), percentile_passes=int(out[14]))

    def plan_hist(self, spec, batch, hist):
        sz = abi.Sizes()
        h = hist.as_abi()
        self._check(self.lib.otsdb_hist_plan(self.ctx, C.byref(spec),
                                             C.byref(batch.as_abi()),
                                             C.byref(h), C.byref(sz)))
        return sz

    def run_hist(self, spec, batch, hist, percentiles, want_counts=False):
        """A histogram query (host arrays): `batch` supplies the series'
        timestamps and the groups (its values are not read), `hist` is a
        histogram.HistColumns (schema and the [N][K + 2] counts) and
        `percentiles` the percentiles, held as float32.  The members are
        downsampled and summed once; returns one HistPoints per group with
        every percentile (and the merged counts when want_counts)."""
        from .histogram import percentile_spec
        p = percentile_spec(percentiles)
        sz = self.plan_hist(spec, batch, hist)
        cap = max(1, int(sz.max_out_points))
        G, R, n = batch.n_groups, hist.n_bins + 2, len(p)
        offs = np.zeros(G + 1, np.int64)
        ts = np.zeros(cap, np.int64)
        pct = np.zeros((max(n, 1), cap), np.float64)
        cnt = np.zeros((cap, R), np.int64) if want_counts else None
        r = abi.HistResult(cap, offs.ctypes.data, ts.ctypes.data,
                           pct.ctypes.data if n else None,
                           None if cnt is None else cnt.ctypes.data)
        b, h = batch.as_abi(), hist.as_abi()
        self._check(self.lib.otsdb_hist_run(
            self.ctx, C.byref(spec), C.byref(b), C.byref(h),
            p.ctypes.data if n else None, n, C.byref(r)))
        return [HistPoints(ts[offs[g]:offs[g + 1]],
                           pct[:n, offs[g]:offs[g + 1]],
                           None if cnt is None else cnt[offs[g]:offs[g + 1]])
                for g in range(G)]

    def hist_rows_counters(self):
        """Of the last histogram call from storage rows (otsdb_ctx_counters
        [15..17]): cells decoded into points, cells skipped as undecodable
        (what the reference logs), points dropped by a same-key merge."""
        out = self._counters(18)
        return dict(decoded=int(out[15]), skipped=int(out[16]),
                    merged_away=int(out[17]))

    def hist_rows_schema(self, rows, codec_id, stream=None):
        """otsdb_hist_rows_schema_device: the bucket schema of the rows (a
        storage.HostRawRows, copied to the device, or a DeviceRawRows) — the
        sorted union of the keys of every cell that decodes with the
        SimpleHistogramDecoder of id `codec_id`.  Returns (lower, upper)
        float32 arrays of K entries (K may be 0)."""
        draw = rows.to_device() if hasattr(rows, "to_device") else rows
        lower = np.zeros(abi.HIST_MAX_ROW - 2, np.float32)
        upper = np.zeros(abi.HIST_MAX_ROW - 2, np.float32)
        n = C.c_int32(0)
        raw = draw.as_abi()
        self._check(self.lib.otsdb_hist_rows_schema_device(
            self.ctx, C.byref(raw), int(codec_id), lower.ctypes.data,
            upper.ctypes.data, C.byref(n), _stream(stream)))
        return lower[:n.value].copy(), upper[:n.value].copy()

    def run_hist_rows(self, spec, rows, codec_id, batch, percentiles,
                      schema=None, want_counts=False):
        """run_hist() from the scanner's storage rows (host arrays): `rows`
        is a storage.HostRawRows, `codec_id` the id
        tsd.core.histograms.config gives SimpleHistogramDecoder, `batch`
        supplies n_series and the groups (its point arrays are not read) and
        `schema` = (lower, upper) the bucket schema, found with
        hist_rows_schema() when None.  The blobs are decoded on the device.
        Results as run_hist()'s; rows without a decodable bucket give no
        points."""
        from .histogram import percentile_spec
        p = percentile_spec(percentiles)
        if schema is None:
            schema = self.hist_rows_schema(rows, codec_id)
        lower = np.ascontiguousarray(schema[0], dtype=np.float32)
        upper = np.ascontiguousarray(schema[1], dtype=np.float32)
        G, K, n = batch.n_groups, len(lower), len(p)
        if K == 0:
            return [HistPoints(np.zeros(0, np.int64), np.zeros((n, 0)),
                               np.zeros((0, 2), np.int64) if want_counts
                               else None) for _ in range(G)]
        h = abi.HistColumns(K, lower.ctypes.data, upper.ctypes.data, None)
        b = _groups_abi(batch)
        sz = abi.Sizes()
        self._check(self.lib.otsdb_hist_plan(self.ctx, C.byref(spec),
                                             C.byref(b), C.byref(h),
                                             C.byref(sz)))
        cap = max(1, int(sz.max_out_points))
        offs = np.zeros(G + 1, np.int64)
        ts = np.zeros(cap, np.int64)
        pct = np.zeros((max(n, 1), cap), np.float64)
        cnt = np.zeros((cap, K + 2), np.int64) if want_counts else None
        r = abi.HistResult(cap, offs.ctypes.data, ts.ctypes.data,
                           pct.ctypes.data if n else None,
                           None if cnt is None else cnt.ctypes.data)
        raw = rows.as_abi()
        self._check(self.lib.otsdb_hist_run_rows(
            self.ctx, C.byref(spec), C.byref(raw), int(codec_id), C.byref(b),
            C.byref(h), p.ctypes.data if n else None, n, C.byref(r)))
        return [HistPoints(ts[offs[g]:offs[g + 1]],
                           pct[:n, offs[g]:offs[g + 1]],
                           None if cnt is None else cnt[offs[g]:offs[g + 1]])
                for g in range(G)]

    def topn_counters(self):
        """Of the last top-N call (otsdb_ctx_counters [18..20]): runs of the
        grid path, runs of the general path, grid promises missed (the
        general path then ran again)."""
        out = self._counters(21)
        return dict(grid=int(out[18]), general=int(out[19]),
                    grid_miss=int(out[20]))

    def run_topn(self, function, topn, start_ms, end_ms, results,
                 grid_interval_ms=0):
        """highestMax / highestCurrent (host arrays): `results` is a list of
        what run() returns, one list of DataPoints per sub-query; `function`
        a gexp name ("highestMax", "highestCurrent"), `topn` an int or the
        function's parameter string; start_ms / end_ms the TSQuery's bounds;
        grid_interval_ms core.topn_grid_interval_ms of the queries'
        downsampler (0: no promise).  Returns (picked, keys, series): the
        picked series' numbers in the inputs' flat order (empty series
        counted), their keys (float64, NaN canonical) and their whole point
        lists as DataPoints, in rank order."""
        ts = topn_spec(function, topn, start_ms, end_ms, grid_interval_ms)
        rs, ng, keep, S, N = _topn_host_inputs(results)
        n_out = min(ts.topn, S)
        cap = max(N, 1)
        offs = np.zeros(n_out + 1, np.int64)
        ots = np.zeros(cap, np.int64)
        bits = np.zeros(cap, np.int64)
        isint = np.zeros(cap, np.uint8)
        picked = np.zeros(max(n_out, 1), np.int64)
        key = np.zeros(max(n_out, 1), np.int64)
        out = abi.TopNResult(
            abi.Result(cap, offs.ctypes.data, ots.ctypes.data,
                       bits.ctypes.data, isint.ctypes.data),
            picked.ctypes.data, key.ctypes.data, 0)
        self._check(self.lib.otsdb_topn_run(
            self.ctx, C.byref(ts), len(results), rs, ng.ctypes.data,
            C.byref(out)))
        k = int(out.n_picked)
        return (picked[:k].copy(), key[:k].view(np.float64).copy(),
                [DataPoints(ots[offs[i]:offs[i + 1]], bits[offs[i]:offs[i + 1]],
                            isint[offs[i]:offs[i + 1]]) for i in range(k)])

    def plan_multi(self, spec, aggs, batch, interps=None):
        n, ids, it = multi_args(aggs, interps)
        sz = abi.Sizes()
        self._check(self.lib.otsdb_agg_plan_multi(
            self.ctx, C.byref(spec), n, ids.ctypes.data, it.ctypes.data,
            C.byref(batch.as_abi()), C.byref(sz)))
        return sz

    def run_multi(self, spec, aggs, batch, interps=None, fold=False):
        """Several cross-series aggregators over one downsample pass of the
        same query (host arrays): `spec` with its aggregator replaced by each
        of `aggs` in turn.  Returns one list of DataPoints (one per group)
        per aggregator, each what run() gives for that aggregator.
        fold: ask for the multi-aggregator fold (abi.SPEC_MULTI_FOLD on a
        copy of the spec): sum / avg / count / min / max sets of one
        interpolation take one ordered fold and no row matrix; a request that
        is not eligible runs as without it."""
        spec = _fold_spec(spec, fold)
        n, ids, it = multi_args(aggs, interps)
        sz = self.plan_multi(spec, ids, batch, it)
        rs, points = _host_results(n, batch.n_groups,
                                   max(1, int(sz.max_out_points)))
        b = batch.as_abi()
        self._check(self.lib.otsdb_agg_run_multi(
            self.ctx, C.byref(spec), n, ids.ctypes.data, it.ctypes.data,
            C.byref(b), rs))
        return points()

    def plan_panel(self, spec, queries, batch):
        n, ds, ids, it = panel_args(queries)
        sz = abi.Sizes()
        self._check(self.lib.otsdb_agg_plan_panel(
            self.ctx, C.byref(spec), n, ds.ctypes.data, ids.ctypes.data,
            it.ctypes.data, C.byref(batch.as_abi()), C.byref(sz)))
        return sz

    def run_panel(self, spec, queries, batch):
        """The sub-queries of one panel over one pass of the point stream
        (host arrays): `queries` is a list of (aggregator, downsampling
        function[, interpolation]); `spec`'s own aggregator, downsampling
        function and interpolation are ignored.  Returns one list of
        DataPoints (one per group) per query, each what run() gives for that
        query."""
        queries = [tuple(q) for q in queries]
        n, ds, ids, it = panel_args(queries)
        sz = self.plan_panel(spec, queries, batch)
        rs, points = _host_results(n, batch.n_groups,
                                   max(1, int(sz.max_out_points)))
        b = batch.as_abi()
        self._check(self.lib.otsdb_agg_run_panel(
            self.ctx, C.byref(spec), n, ds.ctypes.data, ids.ctypes.data,
            it.ctypes.data, C.byref(b), rs))
        return points()


def topn_spec(function, topn, start_ms, end_ms, grid_interval_ms=0):
    """The otsdb_topn_spec of a highestMax / highestCurrent call, checked as
    the reference checks it before anything touches the device: `function` a
    gexp name or id (core.topn_function), `topn` an int or the function's
    parameter string (core.parse_topn)."""
    from .core import parse_topn, topn_function
    fn = topn_function(function)
    if isinstance(topn, str):
        topn = parse_topn([topn])
    topn = int(topn)
    if topn < 1:
        raise IllegalArgumentException(
            "Top n value must be greater than zero: %d" % topn)
    if topn > 2 ** 31 - 1:
        raise IllegalArgumentException("Invalid parameter, must be an integer")
    if int(start_ms) < 0:
        raise IllegalArgumentException("negative start")
    if int(grid_interval_ms) < 0:
        raise IllegalArgumentException("negative grid interval")
    return abi.TopNSpec(fn, topn, int(start_ms), int(end_ms),
                        int(grid_interval_ms))


def _topn_host_inputs(results):
    """The sub-query results of Engine.run_topn (each a list of DataPoints)
    as host otsdb_result structs: (abi.Result array, int64 group counts, the
    arrays kept alive, total series, total points)."""
    R = len(results)
    rs = (abi.Result * max(R, 1))()
    ng = np.zeros(max(R, 1), np.int64)
    keep = []
    S = N = 0
    for r, groups in enumerate(results):
        groups = list(groups)
        offs = np.zeros(len(groups) + 1, np.int64)
        for g, d in enumerate(groups):
            offs[g + 1] = offs[g] + len(d.ts)
        cat = lambda xs, dt: (np.ascontiguousarray(np.concatenate(xs), dt)  # noqa: E731
                              if xs else np.zeros(0, dt))
        ts = cat([np.asarray(d.ts, np.int64) for d in groups], np.int64)
        bits = cat([np.asarray(d.bits, np.int64) for d in groups], np.int64)
        isint = cat([np.asarray(d.is_int, np.uint8) for d in groups], np.uint8)
        # (never a null array: an empty result still passes real pointers)
        pad = lambda a: a if len(a) else np.zeros(1, a.dtype)  # noqa: E731
        ts, bits, isint = pad(ts), pad(bits), pad(isint)
        keep.append((offs, ts, bits, isint))
        rs[r] = abi.Result(int(offs[-1]), offs.ctypes.data, ts.ctypes.data,
                           bits.ctypes.data, isint.ctypes.data)
        ng[r] = len(groups)
        S += len(groups)
        N += int(offs[-1])
    return rs, ng, keep, S, N


class DeviceTopN:
    """otsdb_topn_result for the device entry: the picked series in HBM
    (offsets [n_out + 1], ts / val / is_int [cap]) and the host arrays picked
    / key [n_out]; n_picked after the call."""

    def __init__(self, torch, n_out, cap, device):
        n_out, cap = max(int(n_out), 0), max(int(cap), 0)
        self.cap = cap
        self.offsets = torch.zeros(n_out + 1, dtype=torch.int64, device=device)
        self.ts = torch.zeros(max(cap, 1), dtype=torch.int64, device=device)
        self.val = torch.zeros(max(cap, 1), dtype=torch.int64, device=device)
        self.is_int = torch.zeros(max(cap, 1), dtype=torch.uint8, device=device)
        self.picked = np.zeros(max(n_out, 1), np.int64)
        self.key = np.zeros(max(n_out, 1), np.int64)
        self.n_picked = 0

    def as_abi(self):
        return abi.TopNResult(
            abi.Result(self.cap, self.offsets.data_ptr(), self.ts.data_ptr(),
                       self.val.data_ptr(), self.is_int.data_ptr()),
            self.picked.ctypes.data, self.key.ctypes.data, 0)

    def points(self):
        """The picked series as host DataPoints, in rank order."""
        k = self.n_picked
        offs = self.offsets[:k + 1].cpu().numpy()
        n = int(offs[-1]) if k else 0
        ts, bits = self.ts[:n].cpu().numpy(), self.val[:n].cpu().numpy()
        isint = self.is_int[:n].cpu().numpy()
        return [DataPoints(ts[offs[i]:offs[i + 1]], bits[offs[i]:offs[i + 1]],
                           isint[offs[i]:offs[i + 1]]) for i in range(k)]


def run_topn_device(engine, function, topn, start_ms, end_ms, dresults, dtop,
                    stream=None, grid_interval_ms=0):
    """Device-resident highestMax / highestCurrent: `dresults` is a list of
    DeviceResults as run_device and its kin filled them (one per sub-query),
    `dtop` a DeviceTopN.  The picked series stay in HBM; dtop.picked /
    dtop.key / dtop.n_picked are on the host when the call returns.  A
    DeviceTopN too small raises CapacityException with dtop.n_picked and
    dtop.offsets whole (offsets[n_picked] is the capacity a retry needs)."""
    ts = topn_spec(function, topn, start_ms, end_ms, grid_interval_ms)
    R = len(dresults)
    rs = (abi.Result * max(R, 1))()
    ng = np.zeros(max(R, 1), np.int64)
    for r, d in enumerate(dresults):
        rs[r] = d.as_abi()
        ng[r] = d.offsets.numel() - 1
    out = dtop.as_abi()
    st = engine.lib.otsdb_topn_run_device(
        engine.ctx, C.byref(ts), R, rs, ng.ctypes.data, C.byref(out),
        _stream(stream))
    dtop.n_picked = int(out.n_picked)
    engine._check(st)


class HistPoints:
    """One group's histogram result: ts [n], pct [P][n] (percentile q of
    point i at pct[q, i]) and the merged counts [n][K + 2] or None."""

    def __init__(self, ts, pct, counts):
        self.ts, self.pct, self.counts = ts, pct, counts

    def __len__(self):
        return len(self.ts)


class DeviceBatch:
    """A batch whose arrays are torch tensors resident in HBM (the bench and
    multi-GPU path).  Tensors are kept alive by this object.

    The engine plans its tiles from a host copy of group_offsets
    (otsdb_batch.group_offsets_host), refreshed when the tensor is replaced
    or torch bumps its version (an in-place torch op).  A write that torch
    does not see — through data_ptr by native code, DLPack, or a kernel on
    another stream — must be followed by invalidate_groups(), or the plan
    and the device offsets disagree."""

    def __init__(self, offsets, ts, val, group_offsets, group_members,
                 is_float=None, series_float=None):
        self.offsets, self.ts, self.val = offsets, ts, val
        self.group_offsets, self.group_members = group_offsets, group_members
        self.is_float, self.series_float = is_float, series_float

    @property
    def n_series(self):
        return self.offsets.numel() - 1

    @property
    def n_groups(self):
        return self.group_offsets.numel() - 1

    def as_abi(self):
        def p(t):
            return None if t is None else t.data_ptr()
        b = abi.Batch()
        b.n_series = self.n_series
        b.n_points = self.ts.numel()
        b.offsets = p(self.offsets)
        b.ts_ms = p(self.ts)
        b.val = p(self.val)
        b.is_float = p(self.is_float)
        b.series_float = p(self.series_float)
        b.n_groups = self.n_groups
        b.group_offsets = p(self.group_offsets)
        b.group_members = p(self.group_members)
        b.group_offsets_host = self._goff_host().ctypes.data
        return b

    def invalidate_groups(self):
        """Drop the host copy of group_offsets (and the cached ABI struct):
        the next call reads the device array again."""
        self.__dict__.pop("_goff_cache", None)
        self.__dict__.pop("_abi_cache", None)

    def _goff_host(self):
        """A host copy of group_offsets for otsdb_batch.group_offsets_host
        (re-read when the tensor is replaced or written in place)."""
        t = self.group_offsets
        key = (id(t), t.data_ptr(), t.numel(), t._version)
        c = getattr(self, "_goff_cache", None)
        if c is None or c[0] != key:
            c = (key, np.ascontiguousarray(t.cpu().numpy(), np.int64))
            self._goff_cache = c
        return c[1]


class DeviceResult:
    def __init__(self, torch, G, cap, device):
        self.offsets = torch.zeros(G + 1, dtype=torch.int64, device=device)
        self.ts = torch.empty(max(cap, 1), dtype=torch.int64, device=device)
        self.val = torch.empty(max(cap, 1), dtype=torch.int64, device=device)
        self.is_int = torch.empty(max(cap, 1), dtype=torch.uint8, device=device)
        self.cap = cap

    def as_abi(self):
        return abi.Result(self.cap, self.offsets.data_ptr(), self.ts.data_ptr(),
                          self.val.data_ptr(), self.is_int.data_ptr())


def _abi_cached(obj, names, build, version=None):
    """obj.as_abi()'s struct, rebuilt only when one of the named tensors is
    replaced (or `version` changes: the host group offsets' tensor version,
    the result capacity): C1's 0.12 ms queries spent ~8 us per call filling
    the ctypes fields.  The cache holds the tensors themselves, so the
    identity compares cannot be fooled by a reused id; tensors are never
    resized in place here (a resize_ would need a new DeviceBatch).  The
    struct is private to run_device (as_abi() still hands out a fresh one)."""
    c = obj.__dict__.get("_abi_cache")
    if c is not None and c[2] == version:
        same = True
        for n, t in zip(names, c[0]):
            if getattr(obj, n) is not t:
                same = False
                break
        if same:
            return c[1]
    st = build()
    obj._abi_cache = ([getattr(obj, n) for n in names], st, version)
    return st


_BATCH_TENSORS = ("offsets", "ts", "val", "is_float", "series_float",
                  "group_offsets", "group_members")
_RESULT_TENSORS = ("offsets", "ts", "val", "is_int")


def _stream(stream):
    return None if stream is None else C.c_void_p(stream)


def _result_array(dresults, n, what, cached=True):
    """The abi.Result array of n DeviceResults, one per output (`what`: what
    the outputs are, for the message); cached: their structs through
    _abi_cached."""
    if len(dresults) != n:
        raise IllegalArgumentException(
            "%d results for %d %s" % (len(dresults), n, what))
    rs = (abi.Result * n)()
    for i, r in enumerate(dresults):
        rs[i] = (_abi_cached(r, _RESULT_TENSORS, r.as_abi, r.cap) if cached
                 else r.as_abi())
    return rs


def run_device(engine, spec, dbatch, dresult, stream=None):
    """Device-resident path: no host copies of points in or out."""
    b = _abi_cached(dbatch, _BATCH_TENSORS, dbatch.as_abi,
                    dbatch.group_offsets._version)
    r = _abi_cached(dresult, _RESULT_TENSORS, dresult.as_abi, dresult.cap)
    engine._check(engine.lib.otsdb_agg_run_device(
        engine.ctx, C.byref(spec), C.byref(b), C.byref(r),
        None if stream is None else C.c_void_p(stream)))


def run_rollup_device(engine, spec, dbatch, rollup_agg, dcount, dresult,
                      stream=None):
    """Device-resident rollup call (Engine.run_rollup's semantics): `dcount`
    is an int64 tensor of every point's valueCount() beside dbatch's columns
    (16-byte aligned like them), or None when the rollup aggregator is not
    avg."""
    r, vc = rollup_args(spec, rollup_agg, dcount)
    if vc is not None and vc.numel() != dbatch.ts.numel():
        raise IllegalArgumentException(
            "value_count has %d entries for %d points"
            % (vc.numel(), dbatch.ts.numel()))
    b = _abi_cached(dbatch, _BATCH_TENSORS, dbatch.as_abi,
                    dbatch.group_offsets._version)
    res = _abi_cached(dresult, _RESULT_TENSORS, dresult.as_abi, dresult.cap)
    engine._check(engine.lib.otsdb_agg_run_rollup_device(
        engine.ctx, C.byref(spec), C.byref(b), r,
        None if vc is None else vc.data_ptr(), C.byref(res), _stream(stream)))


def run_rollup_rows_device(engine, spec, draw, table, rollup_agg, dbatch,
                           dresult, stream=None):
    """Device-resident Engine.run_rollup_rows: `draw` is a
    storage.DeviceRawRows, `dbatch` supplies n_series and the groups."""
    r, table = rollup_rows_args(spec, rollup_agg, table)
    b = abi.Batch()
    b.n_series = dbatch.n_series
    b.n_points = 0
    b.n_groups = dbatch.n_groups
    b.group_offsets = dbatch.group_offsets.data_ptr()
    b.group_members = dbatch.group_members.data_ptr()
    raw = draw.as_abi()
    res = dresult.as_abi()
    engine._check(engine.lib.otsdb_agg_run_rollup_rows_device(
        engine.ctx, C.byref(spec), C.byref(raw), C.byref(table), r,
        C.byref(b), C.byref(res), _stream(stream)))


def rollup_decode_rows_device(engine, draw, table, rollup_agg, n_series,
                              seek_ms=None, stream=None):
    """otsdb_rollup_decode_rows_device: the rows of a rollup table (a
    storage.DeviceRawRows) paired and decoded into torch tensors (offsets
    [n_series + 1], ts_ms, val, is_float, value_count) on the rows' device;
    value_count is None unless the rollup aggregator is avg.  seek_ms: the
    timestamp the query's downsampler hands its source, None for no seek."""
    import torch
    _, ids, _ = multi_args([rollup_agg])
    r = int(ids[0])
    if not isinstance(table, abi.RollupTable):
        table = abi.RollupTable(*[int(v) for v in table])
    seek = -2 ** 63 if seek_ms is None else int(seek_ms)
    dev = draw.t["qual"].device
    offsets = torch.zeros(n_series + 1, dtype=torch.int64, device=dev)
    raw = draw.as_abi()

    def call(ts, val, isf, cnt, cap):
        p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        engine._check(engine.lib.otsdb_rollup_decode_rows_device(
            engine.ctx, C.byref(raw), C.byref(table), r, n_series, seek,
            offsets.data_ptr(), p(ts), p(val), p(isf), p(cnt), cap,
            _stream(stream)))
    call(None, None, None, None, 0)
    n = int(offsets[-1].item())
    cap = max(n, 2)  # (never an empty allocation: the pointers must be real)
    ts = torch.zeros(cap, dtype=torch.int64, device=dev)
    val = torch.zeros(cap, dtype=torch.int64, device=dev)
    isf = torch.zeros(cap, dtype=torch.uint8, device=dev)
    cnt = (torch.zeros(cap, dtype=torch.int64, device=dev)
           if r == Aggregators.AVG.id else None)
    call(ts, val, isf, cnt, n)
    return (offsets, ts[:n], val[:n], isf[:n],
            None if cnt is None else cnt[:n])


def _fold_spec(spec, fold, bit=None):
    """spec, or a copy with abi.SPEC_MULTI_FOLD set (the caller's spec is
    never written).  bit: another flag bit in its place
    (abi.SPEC_CELLS_MULTI_FOLD for the cells entry)."""
    if not fold:
        return spec
    s = type(spec).from_buffer_copy(spec)
    s.flags |= abi.SPEC_MULTI_FOLD if bit is None else bit
    return s


def run_multi_device(engine, spec, aggs, dbatch, dresults, stream=None,
                     interps=None, fold=False):
    """Device-resident multi-aggregator call: dresults[i] (a DeviceResult)
    takes what run_device gives for aggs[i]; the point stream is downsampled
    once for all of them.  fold: as Engine.run_multi's."""
    spec = _fold_spec(spec, fold)
    n, ids, it = multi_args(aggs, interps)
    rs = _result_array(dresults, n, "aggregators")
    b = _abi_cached(dbatch, _BATCH_TENSORS, dbatch.as_abi,
                    dbatch.group_offsets._version)
    engine._check(engine.lib.otsdb_agg_run_multi_device(
        engine.ctx, C.byref(spec), n, ids.ctypes.data, it.ctypes.data,
        C.byref(b), rs, _stream(stream)))


def run_panel_device(engine, spec, queries, dbatch, dresults, stream=None):
    """Device-resident panel call: dresults[i] (a DeviceResult) takes what
    run_device gives for queries[i] = (aggregator, downsampling function
    [, interpolation]); the envelope functions share one pass over the point
    stream."""
    n, ds, ids, it = panel_args(queries)
    rs = _result_array(dresults, n, "queries")
    b = _abi_cached(dbatch, _BATCH_TENSORS, dbatch.as_abi,
                    dbatch.group_offsets._version)
    engine._check(engine.lib.otsdb_agg_run_panel_device(
        engine.ctx, C.byref(spec), n, ds.ctypes.data, ids.ctypes.data,
        it.ctypes.data, C.byref(b), rs, _stream(stream)))


def partials_multi_device(engine, spec, aggs, dbatch, partials, emit,
                          stream=None, interps=None):
    """otsdb_agg_partials_multi_device: one downsample pass of this rank's
    shard, output i's per-(group, bucket) states into partials[i] (an int64
    tensor [n_out, G * n_buckets, 4] of raw otsdb_partial words), one emit
    mask [G * n_buckets] (uint8) for all outputs."""
    n, ids, it = multi_args(aggs, interps)
    b = _abi_cached(dbatch, _BATCH_TENSORS, dbatch.as_abi,
                    dbatch.group_offsets._version)
    engine._check(engine.lib.otsdb_agg_partials_multi_device(
        engine.ctx, C.byref(spec), n, ids.ctypes.data, it.ctypes.data,
        C.byref(b), partials.data_ptr(), emit.data_ptr(), _stream(stream)))


def finalize_multi_device(engine, spec, aggs, n_groups, n_buckets, n_ranks,
                          partials, emit, dresults, stream=None, interps=None):
    """otsdb_agg_finalize_multi_device: partials [n_ranks, n_out, G *
    n_buckets, 4] and emit [n_ranks, G * n_buckets] merged in rank order,
    output i into dresults[i]."""
    n, ids, it = multi_args(aggs, interps)
    rs = _result_array(dresults, n, "aggregators", cached=False)
    engine._check(engine.lib.otsdb_agg_finalize_multi_device(
        engine.ctx, C.byref(spec), n, ids.ctypes.data, it.ctypes.data,
        int(n_groups), int(n_buckets), int(n_ranks), partials.data_ptr(),
        emit.data_ptr(), rs, _stream(stream)))


class DeviceHist:
    """otsdb_hist_columns for the device entries: the schema as host float32
    arrays, the [N][K + 2] count matrix as an int64 torch tensor in HBM
    (None for otsdb_hist_finalize_device, which reads the schema alone)."""

    def __init__(self, lower, upper, counts=None):
        self.lower = np.ascontiguousarray(lower, dtype=np.float32)
        self.upper = np.ascontiguousarray(upper, dtype=np.float32)
        self.counts = counts

    @property
    def n_bins(self):
        return len(self.lower)

    def as_abi(self):
        return abi.HistColumns(self.n_bins, self.lower.ctypes.data,
                               self.upper.ctypes.data,
                               None if self.counts is None
                               else self.counts.data_ptr())


class DeviceHistResult:
    """otsdb_hist_result in HBM: offsets [G + 1], ts [cap], pct [P][cap],
    counts [cap][K + 2] (want_counts)."""

    def __init__(self, torch, G, cap, n_bins, n_pct, want_counts, device):
        cap = max(int(cap), 1)
        self.cap = cap
        self.offsets = torch.zeros(G + 1, dtype=torch.int64, device=device)
        self.ts = torch.zeros(cap, dtype=torch.int64, device=device)
        self.pct = torch.zeros((max(n_pct, 1), cap), dtype=torch.float64,
                               device=device)
        self.counts = (torch.zeros((cap, n_bins + 2), dtype=torch.int64,
                                   device=device) if want_counts else None)
        self.n_pct = n_pct

    def as_abi(self):
        return abi.HistResult(self.cap, self.offsets.data_ptr(),
                              self.ts.data_ptr(),
                              self.pct.data_ptr() if self.n_pct else None,
                              None if self.counts is None
                              else self.counts.data_ptr())


def _pct_arg(percentiles):
    from .histogram import percentile_spec
    p = percentile_spec(percentiles)
    return p, (p.ctypes.data if len(p) else None), len(p)


def run_hist_device(engine, spec, dbatch, dhist, percentiles, dresult,
                    stream=None):
    """Device-resident histogram query (Engine.run_hist's semantics): the
    result lands in `dresult`, a DeviceHistResult."""
    p, pp, n = _pct_arg(percentiles)
    b, h, r = dbatch.as_abi(), dhist.as_abi(), dresult.as_abi()
    engine._check(engine.lib.otsdb_hist_run_device(
        engine.ctx, C.byref(spec), C.byref(b), C.byref(h), pp, n, C.byref(r),
        _stream(stream)))


def hist_partials_device(engine, spec, dbatch, dhist, dense, emit,
                         stream=None):
    """otsdb_hist_partials_device: this rank's dense sums into `dense` (int64
    [G, n_buckets, K + 2]) and `emit` (uint8 [G, n_buckets]); the ranks'
    arrays add up (SUM / MAX) to the single run's."""
    b, h = dbatch.as_abi(), dhist.as_abi()
    engine._check(engine.lib.otsdb_hist_partials_device(
        engine.ctx, C.byref(spec), C.byref(b), C.byref(h), dense.data_ptr(),
        emit.data_ptr(), _stream(stream)))


def hist_finalize_device(engine, spec, dhist, n_groups, n_buckets, dense,
                         emit, percentiles, dresult, stream=None):
    """otsdb_hist_finalize_device: percentiles and the compacted result from
    the (summed) dense arrays."""
    p, pp, n = _pct_arg(percentiles)
    h, r = dhist.as_abi(), dresult.as_abi()
    engine._check(engine.lib.otsdb_hist_finalize_device(
        engine.ctx, C.byref(spec), C.byref(h), int(n_groups), int(n_buckets),
        dense.data_ptr(), emit.data_ptr(), pp, n, C.byref(r),
        _stream(stream)))


def run_hist_rows_device(engine, spec, draw, codec_id, dbatch, dhist,
                         percentiles, dresult, stream=None):
    """Device-resident Engine.run_hist_rows: `draw` is a
    storage.DeviceRawRows, `dbatch` supplies n_series and the groups,
    `dhist` (a DeviceHist, counts None) the schema; the result lands in
    `dresult`, a DeviceHistResult."""
    p, pp, n = _pct_arg(percentiles)
    b = abi.Batch()
    b.n_series = dbatch.n_series
    b.n_points = 0
    b.n_groups = dbatch.n_groups
    b.group_offsets = dbatch.group_offsets.data_ptr()
    b.group_members = dbatch.group_members.data_ptr()
    raw, h, r = draw.as_abi(), dhist.as_abi(), dresult.as_abi()
    engine._check(engine.lib.otsdb_hist_run_rows_device(
        engine.ctx, C.byref(spec), C.byref(raw), int(codec_id), C.byref(b),
        C.byref(h), pp, n, C.byref(r), _stream(stream)))


def hist_decode_rows_device(engine, draw, codec_id, n_series, schema,
                            stream=None, counts_offset=0):
    """otsdb_hist_decode_rows_device: the histogram cells of the rows (a
    storage.DeviceRawRows) decoded into torch tensors (offsets
    [n_series + 1], ts_ms [N], counts [N][K + 2]) on the rows' device over
    `schema` = (lower, upper).  counts_offset: int64 words the count matrix
    is displaced by inside its allocation (tests: an 8-byte aligned
    destination)."""
    import torch
    lower = np.ascontiguousarray(schema[0], dtype=np.float32)
    upper = np.ascontiguousarray(schema[1], dtype=np.float32)
    K = len(lower)
    h = abi.HistColumns(K, lower.ctypes.data, upper.ctypes.data, None)
    dev = draw.t["qual"].device
    offsets = torch.zeros(n_series + 1, dtype=torch.int64, device=dev)
    raw = draw.as_abi()

    def call(ts, cnt, cap):
        engine._check(engine.lib.otsdb_hist_decode_rows_device(
            engine.ctx, C.byref(raw), int(codec_id), n_series, C.byref(h),
            offsets.data_ptr(), None if ts is None else ts.data_ptr(),
            None if cnt is None else cnt.data_ptr(), cap, _stream(stream)))
    call(None, None, 0)
    n = int(offsets[-1].item())
    cap = max(n, 2)  # (never an empty allocation: the pointers must be real)
    ts = torch.zeros(cap, dtype=torch.int64, device=dev)
    flat = torch.zeros(cap * (K + 2) + counts_offset + 2, dtype=torch.int64,
                       device=dev)
    cnt = flat[counts_offset:counts_offset + cap * (K + 2)].view(cap, K + 2)
    call(ts, cnt, n)
    return offsets, ts[:n], cnt[:n]
