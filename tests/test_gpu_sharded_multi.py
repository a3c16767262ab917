"""Multi-aggregator queries on the series-sharded path, on the one GPU of
the test box: otsdb_agg_partials_multi_device / _finalize_multi_device (one
downsample pass per rank, one exchange for every scalar output) and
otsdb_sel_retarget (several percentiles from one selection session).

Ranks are emulated in-process as in test_gpu_sharded.py (one context per
rank, tensors stacked in place of the collectives); then two real processes
run dist.run_sharded_multi over gloo.  Reference: the oracle over the
unsharded batch, and the single-aggregator entries.

Shapes: 40 series in 3 groups (every per-rank group one whole-group tile)
and 90 series in 2 groups (groups past 32 members on a rank are tiled by 8
and merged by k_combine).
"""
import ctypes as C
import os

import numpy as np
import pytest

from opentsdb_amd import abi, core, dist as odist
from opentsdb_amd.batch import HostBatch, groups_from_ids
from opentsdb_amd.engine import (DataPoints, DeviceResult, Engine,
                                 finalize_multi_device, partials_multi_device,
                                 run_device)
from oracle import pyoracle
from tests import datasets
from tests.test_gpu_parity import ORDER_FREE, compare, _spec
from tests.test_gpu_sharded import (_free_port, _host, _partials_emulated,
                                    _select_emulated)

pytestmark = pytest.mark.gpu

SETS = [["min", "avg", "max"],
        ["sum", "zimsum", "count", "first", "last"],  # two interpolations
        ["sum", "dev", "mult", "diff", "squareSum", "mimmin", "mimmax"]]
DOWNSAMPLERS = [("avg", "none"), ("max", "nan"), ("sum", "zero")]
H1 = datasets.T0 + 3600 * 1000


@pytest.fixture(scope="module")
def engines():
    from opentsdb_amd import build
    build.build()
    es = [Engine(0) for _ in range(3)]
    yield es
    for e in es:
        e.close()


@pytest.fixture(scope="module")
def batches():
    return {40: datasets.random_batch(201, n_series=40, n_groups=3,
                                      nan_frac=0.02),
            90: datasets.random_batch(203, n_series=90, n_groups=2,
                                      nan_frac=0.05)}


_REFS = {}


def _ref(key, spec, hb):
    """The oracle's result, computed once per (batch, query)."""
    if key not in _REFS:
        _REFS[key] = pyoracle.group_by(spec, hb)
    return _REFS[key]


def _slice(hb, a, b):
    """Series [a, b) of a HostBatch as one rank's shard: group offsets over
    every global group, members renumbered locally."""
    offs = hb.offsets[a:b + 1] - hb.offsets[a]
    p0, p1 = hb.offsets[a], hb.offsets[b]
    g_off, members = [0], []
    for g in range(hb.n_groups):
        m = hb.group_members[hb.group_offsets[g]:hb.group_offsets[g + 1]]
        members.extend((m[(m >= a) & (m < b)] - a).tolist())
        g_off.append(len(members))
    return HostBatch(offs, hb.ts[p0:p1], hb.val[p0:p1],
                     None if hb.is_float is None else hb.is_float[p0:p1],
                     None, np.array(g_off, np.int64),
                     np.array(members, np.int64))


def _shards(hb, world):
    return [odist.shard_host_batch(hb, world, r) for r in range(world)]


def _multi_partials(engines, spec, aggs, shards, G, passes=None):
    """Every rank's otsdb_agg_partials_multi_device, the all-gathers done by
    stacking: (partials [world, n_out, GB, 4], emit [world, GB], nb)."""
    import torch
    n = len(aggs)
    parts, emits, nb = [], [], None
    for r, sh in enumerate(shards):
        e = engines[r]
        db = odist.to_device(sh)
        nb = int(e.plan(spec, db).n_buckets)
        GB = G * nb
        p = torch.zeros((n, max(GB, 1), 4), dtype=torch.int64, device="cuda")
        m = torch.zeros(max(GB, 1), dtype=torch.uint8, device="cuda")
        partials_multi_device(e, spec, aggs, db, p, m)
        if passes is not None:
            passes.append(e.multi_counters()["downsample_passes"])
        parts.append(p[:, :GB])
        emits.append(m[:GB])
    return torch.stack(parts).contiguous(), torch.stack(emits).contiguous(), nb


def _multi_finalize(engine, spec, aggs, G, nb, gp, ge):
    import torch
    res = [DeviceResult(torch, G, max(G * nb, 1), "cuda") for _ in aggs]
    finalize_multi_device(engine, spec, aggs, G, nb, gp.shape[0], gp, ge, res)
    torch.cuda.synchronize()
    return [_host(r, G) for r in res]


def _single_finalize(engine, spec, G, nb, gp_i, ge):
    import torch
    res = DeviceResult(torch, G, max(G * nb, 1), "cuda")
    r = res.as_abi()
    gp_i = gp_i.contiguous()
    engine._check(engine.lib.otsdb_agg_finalize_device(
        engine.ctx, C.byref(spec), G, nb, gp_i.shape[0], gp_i.data_ptr(),
        ge.data_ptr(), C.byref(r), None))
    torch.cuda.synchronize()
    return _host(res, G)


def _same_bits(a, b, where):
    assert len(a) == len(b), where
    for g, (x, y) in enumerate(zip(a, b)):
        w = "%s/g%d" % (where, g)
        assert np.array_equal(x.ts, y.ts), w + ": timestamps"
        assert np.array_equal(x.is_int, y.is_int), w + ": is_int"
        assert np.array_equal(x.bits, y.bits), w + ": bits"


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("n", [40, 90])
@pytest.mark.parametrize("aggs", SETS, ids=["-".join(s) for s in SETS])
def test_scalar_sets_across_ranks(engines, batches, aggs, n, world):
    """Every output of the shared-partials path against the oracle; one
    downsample pass on every rank."""
    hb = batches[n]
    shards = _shards(hb, world)
    for ds, fill in DOWNSAMPLERS:
        spec = _spec(aggs[0], ds, fill)
        passes = []
        gp, ge, nb = _multi_partials(engines, spec, aggs, shards, hb.n_groups,
                                     passes)
        assert passes == [1] * world, passes
        outs = _multi_finalize(engines[0], spec, aggs, hb.n_groups, nb, gp, ge)
        for agg, got in zip(aggs, outs):
            ref = _ref((n, agg, ds, fill), _spec(agg, ds, fill), hb)
            compare(got, ref, agg in ORDER_FREE and ds == "max",
                    where="w%d/n%d/%s/%s/%s" % (world, n, agg, ds, fill))


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("n", [40, 90])
def test_consistent_with_the_single_entries(engines, batches, n, world):
    """Slice i of the multi partials with the one emit mask is a valid input
    of otsdb_agg_finalize_device and gives the bits of output i (a wrong
    slot in k_finalize_ranks_multi's dispatch shows here); order-free
    aggregators also have the bits of the single partials entry."""
    hb = batches[n]
    aggs = sorted({a for s in SETS for a in s})
    spec = _spec(aggs[0], "max", "nan")
    G = hb.n_groups
    gp, ge, nb = _multi_partials(engines, spec, aggs, _shards(hb, world), G)
    outs = _multi_finalize(engines[0], spec, aggs, G, nb, gp, ge)
    for i, agg in enumerate(aggs):
        si = _spec(agg, "max", "nan")
        one = _single_finalize(engines[0], si, G, nb, gp[:, i], ge)
        _same_bits(outs[i], one, "w%d/n%d/%s" % (world, n, agg))
        if agg in ORDER_FREE:
            _same_bits(outs[i], _partials_emulated(engines, si, hb, world),
                       "w%d/n%d/%s vs single partials" % (world, n, agg))


def test_one_output_and_explicit_interpolations(engines, batches):
    """n_out == 1 runs the single entry's path (one pass, the single
    entry's bits); interps[i] replaces the aggregator's own interpolation
    (two classes over the same aggregator)."""
    import torch
    hb, world = batches[40], 2
    G = hb.n_groups
    spec = _spec("sum", "avg", "none")
    passes = []
    gp, ge, nb = _multi_partials(engines, spec, ["sum"], _shards(hb, world),
                                 G, passes)
    assert passes == [1] * world
    outs = _multi_finalize(engines[0], spec, ["sum"], G, nb, gp, ge)
    _same_bits(outs[0], _partials_emulated(engines, spec, hb, world), "n1")
    its = [core.Interpolation.LERP, core.Interpolation.ZIM]
    res = [DeviceResult(torch, G, G * nb, "cuda") for _ in its]
    parts, emits = [], []
    for r, sh in enumerate(_shards(hb, world)):
        p = torch.zeros((2, G * nb, 4), dtype=torch.int64, device="cuda")
        m = torch.zeros(G * nb, dtype=torch.uint8, device="cuda")
        partials_multi_device(engines[r], spec, ["sum", "sum"],
                              odist.to_device(sh), p, m, interps=its)
        assert engines[r].multi_counters() == dict(
            downsample_passes=1, group_passes=2, key_transposes=0,
            transform_passes=2)
        parts.append(p)
        emits.append(m)
    finalize_multi_device(engines[0], spec, ["sum", "sum"], G, nb, world,
                          torch.stack(parts).contiguous(),
                          torch.stack(emits).contiguous(), res, interps=its)
    torch.cuda.synchronize()
    for it, r in zip(its, res):
        si = _spec("sum", "avg", "none", interp=it)
        compare(_host(r, G), pyoracle.group_by(si, hb), False,
                where="interp %d" % int(it))


def _one_sided(hb):
    """90 series regrouped and cut so that rank 1 holds no series at all,
    group 0 (60 members: tiles of 8, k_combine) lives wholly on rank 0 —
    an empty group with local series on rank 2 — and group 1 spans ranks 0
    and 2."""
    gid = np.where(np.arange(90) < 60, 0, 1)
    g_off, members = groups_from_ids(gid, 2)
    hb2 = HostBatch(hb.offsets, hb.ts, hb.val, hb.is_float, None, g_off,
                    members)
    return hb2, [_slice(hb2, 0, 70), _slice(hb2, 70, 70), _slice(hb2, 70, 90)]


def test_empty_rank_and_one_rank_groups(engines, batches):
    hb, shards = _one_sided(batches[90])
    G = hb.n_groups
    assert shards[1].n_series == 0
    assert shards[2].group_offsets[1] == 0  # group 0: no member on rank 2
    for aggs in SETS:
        for ds, fill in DOWNSAMPLERS:
            spec = _spec(aggs[0], ds, fill)
            passes = []
            gp, ge, nb = _multi_partials(engines, spec, aggs, shards, G,
                                         passes)
            # a rank without series shares no rows: its outputs run one
            # after another (n_out passes over no points)
            assert passes == [1, len(aggs), 1], passes
            outs = _multi_finalize(engines[0], spec, aggs, G, nb, gp, ge)
            for i, (agg, got) in enumerate(zip(aggs, outs)):
                si = _spec(agg, ds, fill)
                ref = _ref(("one-sided", agg, ds, fill), si, hb)
                compare(got, ref, agg in ORDER_FREE and ds == "max",
                        where="one-sided/%s/%s/%s" % (agg, ds, fill))
                one = _single_finalize(engines[0], si, G, nb, gp[:, i], ge)
                _same_bits(got, one, "one-sided/%s/%s" % (agg, ds))


def _select_multi_emulated(engines, spec0, aggs, hb, world):
    """One otsdb_sel_* session per rank for all of `aggs`: one prepare, the
    three all-reduces once, then per aggregator (retargeted) the pass loop,
    pick and finish.  Returns one host result per aggregator."""
    import torch
    G = hb.n_groups
    before = [e.sel_sessions() for e in engines[:world]]
    sels = [odist.ShardedSelect(
        engines[r], spec0, odist.to_device(odist.shard_host_batch(hb, world, r)),
        G) for r in range(world)]
    cs, es, ks = zip(*[s.prepare() for s in sels])
    counts = torch.stack(cs).sum(0)
    emit = torch.stack(es).max(0).values
    krange = torch.stack(ks).min(0).values
    for s in sels:
        s.counts.copy_(counts)
        s.emit.copy_(emit)
        s.krange.copy_(krange)
    results = []
    for k, agg in enumerate(aggs):
        if k:
            for s in sels:
                s.retarget(agg)
        p = 0
        while True:
            more = [s.hist_pass(p) for s in sels]
            assert len(set(more)) == 1, "ranks planned different passes"
            if not more[0]:
                break
            h = torch.stack([s.hist for s in sels]).sum(0)
            for s in sels:
                s.hist.copy_(h.to(torch.int32))
            p += 1
            assert p <= odist.MAX_SEL_PASSES
        picks = torch.stack([s.pick().clone() for s in sels]).sum(0)
        for s in sels:
            s.picks.copy_(picks)
        outs = [_host(s.finish(), G) for s in sels]
        for o in outs[1:]:  # every rank ends with the same bits
            _same_bits(outs[0], o, "ranks/%s" % agg)
        results.append(outs[0])
    after = [e.sel_sessions() for e in engines[:world]]
    assert [b - a for a, b in zip(before, after)] == [1] * world
    return results


PCTS = ["p99", "p999", "median", "ep95r3"]


@pytest.mark.parametrize("world", [2, 3])
def test_percentiles_from_one_session(engines, world):
    """Retargeted sessions: the bits of a fresh single session and of the
    oracle, for every aggregator; one prepare per rank for the whole set."""
    hb = datasets.random_batch(203, n_series=90, n_groups=2, nan_frac=0.05,
                               span_ms=3600 * 1000, cadence_ms=20000)
    for ds, fill in (("avg", "none"), ("max", "nan")):
        spec0 = _spec(PCTS[0], ds, fill, end=H1)
        got = _select_multi_emulated(engines, spec0, PCTS, hb, world)
        for agg, g in zip(PCTS, got):
            si = _spec(agg, ds, fill, end=H1)
            _same_bits(g, _select_emulated(engines, si, hb, world),
                       "w%d/%s/%s vs fresh session" % (world, agg, fill))
            compare(g, pyoracle.group_by(si, hb), ds == "max",
                    where="w%d/%s/%s" % (world, agg, fill))


@pytest.mark.parametrize("world", [2, 3])
def test_percentiles_from_one_session_fill_and_rate(engines, world):
    """The other paths into the key matrix (fixed-interval shapes of
    test_percentiles_across_ranks_fills_rate_calendar): a zero fill, where
    the transpose applies the fill and counts the keys, and counter rates."""
    aggs = ["p99", "median", "ep95r3"]
    hb = datasets.random_batch(211, n_series=70, n_groups=2, nan_frac=0.03,
                               span_ms=3 * 3600 * 1000, cadence_ms=20000)
    hc = datasets.random_batch(213, n_series=60, n_groups=2, counter=True,
                               span_ms=3 * 3600 * 1000, cadence_ms=20000)
    ro = core.RateOptions(True, 2**63 - 1, 0)
    for name, b, kw in (("fill", hb, dict(ds="sum", fill="zero")),
                        ("rate", hc, dict(ds="sum", fill="none", rate=True,
                                          ro=ro))):
        got = _select_multi_emulated(engines, _spec(aggs[0], **kw), aggs, b,
                                     world)
        for agg, g in zip(aggs, got):
            si = _spec(agg, **kw)
            _same_bits(g, _select_emulated(engines, si, b, world),
                       "w%d/%s/%s vs fresh session" % (world, name, agg))
            compare(g, pyoracle.group_by(si, b), False,
                    where="w%d/%s/%s" % (world, name, agg))


def test_retarget_status_codes(batches):
    """No session: illegal state; not a selection: illegal argument; a query
    run on the context in between ends the session: illegal state."""
    import torch
    e = Engine(0)
    try:
        p999 = core.Aggregators.get("p999").id
        with pytest.raises(core.IllegalStateException):
            e._check(e.lib.otsdb_sel_retarget(e.ctx, p999))
        hb = batches[40]
        db = odist.to_device(hb)
        sel = odist.ShardedSelect(e, _spec("p99", "avg", "none"), db,
                                  hb.n_groups)
        sel.prepare()
        with pytest.raises(core.IllegalArgumentException):
            sel.retarget("sum")
        sel.retarget("p999")  # the session is still there
        spec = _spec("sum", "avg", "none")
        sz = e.plan(spec, db)
        res = DeviceResult(torch, hb.n_groups, int(sz.max_out_points), "cuda")
        run_device(e, spec, db, res)
        with pytest.raises(core.IllegalStateException):
            sel.retarget("p999")
        with pytest.raises(core.IllegalStateException):
            sel.hist_pass(0)
    finally:
        e.close()


def test_partials_entry_refusals(engines, batches):
    import torch
    e = engines[0]
    hb = batches[40]
    db = odist.to_device(hb)
    spec = _spec("sum", "avg", "none")
    nb = int(e.plan(spec, db).n_buckets)
    GB = hb.n_groups * nb
    p = torch.zeros((33, GB, 4), dtype=torch.int64, device="cuda")
    m = torch.zeros(GB, dtype=torch.uint8, device="cuda")
    with pytest.raises(core.IllegalArgumentException):  # a selection
        partials_multi_device(e, spec, ["sum", "p99"], db, p, m)
    t0, t1 = datasets.T0, datasets.T0 + 3 * 3600 * 1000
    raw = core.make_spec(t0, t1, core.Aggregators.get("sum"), None, t0, t1)
    with pytest.raises(core.UnsupportedOperationException):
        partials_multi_device(e, raw, ["sum", "max"], db, p, m)
    b = db.as_abi()
    ids = np.zeros(33, np.int32)
    for n_out in (0, 33):
        assert e.lib.otsdb_agg_partials_multi_device(
            e.ctx, C.byref(spec), n_out, ids.ctypes.data, None, C.byref(b),
            p.data_ptr(), m.data_ptr(), None) == abi.E_ILLEGAL_ARGUMENT
        r = DeviceResult(torch, hb.n_groups, GB, "cuda").as_abi()
        assert e.lib.otsdb_agg_finalize_multi_device(
            e.ctx, C.byref(spec), n_out, ids.ctypes.data, None, hb.n_groups,
            nb, 1, p.data_ptr(), m.data_ptr(), C.byref(r), None) == \
            abi.E_ILLEGAL_ARGUMENT


GLOO_SETS = [(["sum", "dev", "max", "avg"], "avg", "none"),
             (["p99", "p999"], "max", "nan"),
             (["min", "p99", "count"], "max", "nan")]  # mixed: both paths


def _rank_main(rank, world, port, q):
    import torch
    import torch.distributed as tdist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    tdist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    e = Engine(0)
    hb = datasets.random_batch(205, n_series=50, n_groups=3, nan_frac=0.02)
    out = []
    for aggs, ds, fill in GLOO_SETS:
        db = odist.to_device(odist.shard_host_batch(hb, world, rank))
        res = odist.run_sharded_multi(e, _spec(aggs[0], ds, fill), aggs, db,
                                      hb.n_groups)
        torch.cuda.synchronize()
        out.append([{g: tuple(a.copy() for a in v)
                     for g, v in r.host_groups().items()} for r in res])
    q.put((rank, out))
    tdist.barrier()
    tdist.destroy_process_group()
    e.close()


def test_two_processes_gloo():
    """dist.run_sharded_multi as two ranks run it (gloo, both on cuda:0):
    a scalar set with dev, a percentile set and a mixed one."""
    import queue
    import time
    import torch.multiprocessing as mp
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_rank_main, args=(r, world, port, q))
          for r in range(world)]
    for p in ps:
        p.start()
    outs = []
    deadline = time.time() + 240
    while len(outs) < world:  # stop early if a rank died
        assert time.time() < deadline, "ranks did not report"
        try:
            outs.append(q.get(timeout=5))
        except queue.Empty:
            assert all(p.is_alive() or p.exitcode == 0 for p in ps), \
                [p.exitcode for p in ps]
    for p in ps:
        p.join(timeout=120)
        assert p.exitcode == 0
    hb = datasets.random_batch(205, n_series=50, n_groups=3, nan_frac=0.02)
    for k, (aggs, ds, fill) in enumerate(GLOO_SETS):
        for i, agg in enumerate(aggs):
            ref = pyoracle.group_by(_spec(agg, ds, fill), hb)
            merged = {}
            for _, out in outs:
                merged.update(out[k][i])
            assert sorted(merged) == list(range(hb.n_groups))
            got = [DataPoints(*merged[g]) for g in range(hb.n_groups)]
            exact = ds == "max" and (agg in ORDER_FREE or agg.startswith("p"))
            compare(got, ref, exact, where="gloo/%s/%s" % (agg, ds))
