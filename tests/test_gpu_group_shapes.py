"""Group-shape edges through every path of the main query: group sizes on
both sides of each rule that spreads a query's series over fold tiles, row
chunks, ordered chains, combine slices and the selections' kernels, and the
members that stream nothing placed at the edges of those pieces
(tests/group_shapes.py).  Needs an MI355X.

Every comparison is against the CPU oracle through the suite's compare(), bit
for bit: the batches' values make every sum, interpolation and rate exact in
any reduction order (tests/test_group_shapes_cpu.py asserts it, pins the
oracle to a plain model on the same batches and shows that the batches catch
the mistakes these boundaries invite).  The one exception is dev one member
past the exact chain without OTSDB_SPEC_EXACT_ORDER, held to the contract of
test_dev_offset_gauge_past_one_chain; a percentile that is +-0.0 compares by
value (zero_sign_blind, the rule of tests/test_gpu_value_domain.py).
"""
import ctypes
import time

import numpy as np
import pytest

from opentsdb_amd import abi
from opentsdb_amd.batch import HostBatch
from opentsdb_amd.engine import Engine
from oracle import pyoracle
from tests import group_shapes as GS
from tests.test_gpu_multi import with_agg
from tests.test_gpu_panel import with_query
from tests.test_gpu_parity import compare

pytestmark = pytest.mark.gpu

C = GS.C
PANEL = [("sum", "sum"), ("min", "min"), ("max", "max"), ("count", "count"),
         ("avg", "avg")]
# the aggregator sets of one interpolation class a multi-aggregator fold takes
LERP_SET = ["sum", "avg", "min", "max"]
ZIM_SET = ["zimsum", "count"]
FIVE = ["sum", "avg", "min", "max", "count"]


@pytest.fixture(scope="module")
def engine():
    from opentsdb_amd import build
    build.build()
    e = Engine(0)
    yield e
    e.close()


class Oracle:
    """The oracle's result per spec of one batch, computed once."""

    def __init__(self, batch):
        self.batch, self.kept = batch, {}

    def __call__(self, spec):
        key = bytes(spec)
        if key not in self.kept:
            self.kept[key] = pyoracle.group_by(spec, self.batch)
        return self.kept[key]


def held(engine, b, aggs, fills, where, ds="sum", rate=False, ora=None,
         blind=False):
    """engine.run against the oracle, bit for bit."""
    ora = ora or Oracle(b.batch)
    for fill in fills:
        for agg in aggs:
            spec = GS.spec_of(b, agg, ds, fill, rate)
            got, ref = engine.run(spec, b.batch), ora(spec)
            if blind and agg != "median":
                from tests.test_gpu_value_domain import zero_sign_blind
                got = zero_sign_blind(got, ref)
            compare(got, ref, True, "%s/%s:%s-%s" % (where, agg, ds, fill))


# ------------------------------------------------------ the unordered fold
@pytest.mark.parametrize("n", GS.fold_ladder())
def test_fold_ladder(engine, n):
    """One tile | tiles of kFoldChunkLarge | k_combine | k_combine_l1 with
    every slice used | with the last slice short: plain, and with the members
    that stream nothing at every placement the size has."""
    for name, b in GS.fold_batches(n):
        held(engine, b, GS.FOLD_AGGS, GS.FILLS, "fold/%d/%s" % (n, name))


# ------------------------------------------------------- the ordered fold
@pytest.mark.parametrize("n", GS.ordered_ladder())
def test_ordered_fold(engine, n):
    """dev: one chain per (group, bucket) — one fold tile up to
    kOrderedFoldChunk members (member contexts preloaded up to FOLD_CTX_MAX,
    alone and beside small groups), the row path's chain one member later."""
    for name, b in GS.ordered_batches(n):
        held(engine, b, ("dev",), GS.FILLS, "dev/%d/%s" % (n, name))
    # which path ran: the route is the cells entry's too, and its walker
    # counters move only when the cells fold runs
    from tests.test_gpu_cells_panel import cells_single
    b = GS.build([GS.Group(n)], form="double")
    case = DeviceEncoded(engine, b.batch)
    for fill in GS.FILLS:
        spec = GS.spec_of(b, "dev", "sum", fill)
        c0 = engine.counters()
        got = cells_single(engine, case, spec)
        assert (cells_folds(engine, c0) >= 1) == (n <= C.kOrderedFoldChunk), \
            "dev/%d-%s: the fold up to kOrderedFoldChunk members" % (n, fill)
        compare(got, pyoracle.group_by(spec, b.batch), True,
                "dev/%d/cells-%s" % (n, fill))


# ------------------------------------------------------------ the row path
@pytest.mark.parametrize("n", GS.row_ladder())
def test_row_path(engine, n):
    """k_group's chunks of kChunk members, reached through a rate over
    counters and through a percentile downsampler."""
    held(engine, GS.single(n, counter=True), GS.ROW_AGGS, ("none",),
         "rate/%d" % n, ds="max", rate=True)
    for name, b in GS.row_batches(n):
        held(engine, b, GS.ROW_AGGS, GS.FILLS, "p90/%d/%s" % (n, name),
             ds="p90")


def test_row_path_two_level_combine(engine):
    """kCombineL1 chunks of kChunk members and one member more: k_combine |
    k_combine_l1 on the row path."""
    for n in GS.row_two_level():
        t = time.perf_counter()
        held(engine, GS.single(n, nb=2), ("sum", "min", "first", "last"),
             ("none",), "p90/%d" % n, ds="p90")
        print("row path, %d members: %.1f s" % (n, time.perf_counter() - t))


# ---------------------------------------------------------- dev past the fold
def test_dev_at_and_past_the_exact_chain(engine):
    """kOrderedChunk members are one chain: bit for bit.  One member more:
    bit for bit with OTSDB_SPEC_EXACT_ORDER; without it the in-order chunk
    states merge (Chan), inside the contract test_dev_offset_gauge_past_one_
    chain asserts (<= 1e-9 relative; the measured figure is printed)."""
    n = C.kOrderedChunk
    held(engine, GS.single(n, nb=2), ("dev",), ("none",), "dev/%d" % n)
    t = time.perf_counter()
    b = GS.single(n + 1, nb=2)
    spec = GS.spec_of(b, "dev", "sum", "none")
    ref = pyoracle.group_by(spec, b.batch)
    got = engine.run(spec, b.batch)
    assert np.array_equal(got[0].ts, ref[0]["ts"]) and len(ref[0]) == 2
    g = got[0].bits.view(np.float64)
    r = ref[0]["bits"].view(np.float64)
    rel = float(np.max(np.abs(g - r) / np.abs(r)))
    print("dev over %d members, chunk-merged: max rel err %.3e" % (n + 1, rel))
    assert rel <= 1e-9
    spec.flags = abi.SPEC_EXACT_ORDER
    compare(engine.run(spec, b.batch), ref, True, "dev/%d/exact" % (n + 1))
    print("dev, %d members: %.1f s" % (n + 1, time.perf_counter() - t))


# ------------------------------------------------------------ mixed batches
@pytest.fixture(scope="module")
def mixed():
    return {name: (b, Oracle(b.batch)) for name, b in GS.mixed_batches()}


MIXED = ("mixed", "mixed-inter", "large-first", "large-last", "singletons")


@pytest.mark.parametrize("name", MIXED)
def test_mixed_single_query(engine, mixed, name):
    """Two-level groups beside two-tile and one-tile groups (every multi-tile
    group of the call goes through k_combine_l1), member-less groups first
    but one, doubled in the middle and last, a group whose members all
    stream nothing between groups that emit."""
    b, ora = mixed[name]
    held(engine, b, GS.FOLD_AGGS + ("dev",), GS.FILLS, name, ora=ora)
    held(engine, b, ("sum", "max"), GS.FILLS, name, ds="avg", ora=ora)
    # no group without effective members emits anything
    spec = GS.spec_of(b, "sum", "sum", "zero")
    got = engine.run(spec, b.batch)
    for g, grp in enumerate(b.groups):
        if grp.n == len(grp.quiet):
            assert len(got[g].ts) == 0, "%s/g%d" % (name, g)


@pytest.mark.parametrize("fold", [False, True])
@pytest.mark.parametrize("name", MIXED)
def test_mixed_multi(engine, mixed, name, fold):
    """run_multi with and without OTSDB_SPEC_MULTI_FOLD: the multi fold's
    tiles leave one partial an envelope member."""
    b, ora = mixed[name]
    for fill, sets in (("none", (LERP_SET, ZIM_SET)), ("zero", (FIVE,))):
        for aggs in sets:
            spec = GS.spec_of(b, aggs[0], "sum", fill)
            got = engine.run_multi(spec, aggs, b.batch, fold=fold)
            assert engine.multi_fold_counters() == dict(
                fold_launches=1 if fold else 0)
            for i, agg in enumerate(aggs):
                compare(got[i], ora(with_agg(spec, agg)), True,
                        "multi/%s/%s-%s/fold%d" % (name, agg, fill, fold))


@pytest.mark.parametrize("name", MIXED)
def test_mixed_panel(engine, mixed, name):
    b, ora = mixed[name]
    for fill in GS.FILLS:
        spec = GS.spec_of(b, "sum", "sum", fill)
        got = engine.run_panel(spec, PANEL, b.batch)
        for i, q in enumerate(PANEL):
            compare(got[i], ora(with_query(spec, q)), True,
                    "panel/%s/%s:%s-%s" % ((name,) + q + (fill,)))


class DeviceEncoded:
    """A batch of doubles as columnar device arrays and as cells that
    otsdb_encode_cells_device wrote (one value type a series is what the
    device encoder takes): what tests.test_gpu_cells_panel.Case is for
    host-encoded cells."""

    def __init__(self, engine, hb):
        from opentsdb_amd import workload
        from tests.test_gpu_decode import _device_batch
        assert (hb.is_float == 1).all() and (hb.ts % 1000 == 0).all()
        self.b = hb
        self.db = _device_batch(hb, "float")
        self.dc = workload.encode_cells_device(engine, self.db)

    def cap(self, spec):
        return (4 + (spec.end_ms - spec.start_ms) // spec.ds_interval_ms) * \
            self.b.n_groups + 8


def cells_folds(engine, c0):
    """Cells folds launched since the counters c0."""
    c1 = engine.counters()
    return sum(c1[k] - c0[k] for k in ("cells_uniform", "cells_general"))


ENCODERS = ("device", "host")


@pytest.fixture(scope="module")
def mixed_cells(engine, mixed):
    """{(name, encoder): (Built, oracle, case)}: the mixed batches as cells
    encoded on the device (all doubles) and on the host (values of mixed
    types, tests/cells.py), 2-byte qualifiers both."""
    from tests.test_gpu_cells_panel import Case
    out = {}
    for name, b in GS.mixed_batches("double"):
        out[name, "device"] = (b, Oracle(b.batch),
                               DeviceEncoded(engine, b.batch))
    for name in MIXED:
        b, ora = mixed[name]
        out[name, "host"] = (b, ora, Case(b.batch))
    return out


def folds_dev(b):
    """Whether dev takes the fold on this batch: no group past one tile."""
    return max(g.n for g in b.groups) <= C.kOrderedFoldChunk


@pytest.mark.parametrize("enc", ENCODERS)
@pytest.mark.parametrize("name", MIXED)
def test_mixed_cells_fold(engine, mixed_cells, name, enc):
    """The cells fold from device-encoded and from host-encoded cells: every
    query of an unordered aggregator runs it (the walker counters move per
    query); dev runs it where no group is past kOrderedFoldChunk members and
    takes the row pipeline otherwise."""
    from tests.test_gpu_cells_panel import cells_single
    b, ora, case = mixed_cells[name, enc]
    for fill in GS.FILLS:
        for agg in GS.FOLD_AGGS + ("dev",):
            spec = GS.spec_of(b, agg, "sum", fill)
            w = "cells/%s/%s/%s-%s" % (name, enc, agg, fill)
            c0 = engine.counters()
            got = cells_single(engine, case, spec)
            assert (cells_folds(engine, c0) >= 1) == \
                (agg != "dev" or folds_dev(b)), w + ": cells folds"
            compare(got, ora(spec), True, w)


@pytest.mark.parametrize("enc", ENCODERS)
@pytest.mark.parametrize("name", MIXED)
def test_mixed_cells_multi_fold(engine, mixed_cells, name, enc):
    from tests.test_gpu_cells_multi_fold import cells_multi_fold
    b, ora, case = mixed_cells[name, enc]
    for fill, sets in (("none", (LERP_SET, ZIM_SET)), ("zero", (FIVE,))):
        for aggs in sets:
            spec = GS.spec_of(b, aggs[0], "sum", fill)
            got = cells_multi_fold(engine, case, spec, aggs, None)
            assert engine.multi_fold_counters()["fold_launches"] >= 1
            for i, agg in enumerate(aggs):
                compare(got[i], ora(with_agg(spec, agg)), True,
                        "cells-multi/%s/%s/%s-%s" % (name, enc, agg, fill))


# ------------------------------------------------------------ emulated ranks
def _shard(hb, a, b):
    """Series [a, b) of a batch with group offsets over every global group
    (dist.shard_host_batch with the cut chosen)."""
    offs = hb.offsets[a:b + 1] - hb.offsets[a]
    p0, p1 = hb.offsets[a], hb.offsets[b]
    g_off, members = [0], []
    for g in range(hb.n_groups):
        m = hb.group_members[hb.group_offsets[g]:hb.group_offsets[g + 1]]
        members.extend((m[(m >= a) & (m < b)] - a).tolist())
        g_off.append(len(members))
    return HostBatch(offs, hb.ts[p0:p1], hb.val[p0:p1], hb.is_float[p0:p1],
                     None, np.array(g_off, np.int64),
                     np.array(members, np.int64))


def _partials_at(engine, spec, hb, cuts):
    """tests/test_gpu_sharded.py::_partials_emulated with the ranks' series
    ranges given: otsdb_agg_partials_device per rank, then
    otsdb_agg_finalize_device over them in rank order."""
    import torch
    from opentsdb_amd import dist as odist
    from opentsdb_amd.engine import DeviceResult
    from tests.test_gpu_sharded import _host
    G, world = hb.n_groups, len(cuts) - 1
    parts, emits, nb = [], [], None
    for r in range(world):
        db = odist.to_device(_shard(hb, cuts[r], cuts[r + 1]))
        nb = int(engine.plan(spec, db).n_buckets)
        GB = G * nb
        p = torch.zeros((max(GB, 1), 4), dtype=torch.int64, device="cuda")
        m = torch.zeros(max(GB, 1), dtype=torch.uint8, device="cuda")
        ab = db.as_abi()
        engine._check(engine.lib.otsdb_agg_partials_device(
            engine.ctx, ctypes.byref(spec), ctypes.byref(ab), p.data_ptr(),
            m.data_ptr(), None))
        parts.append(p[:GB])
        emits.append(m[:GB])
    gp = torch.stack(parts).contiguous()
    ge = torch.stack(emits).contiguous()
    res = DeviceResult(torch, G, max(G * nb, 1), "cuda")
    r = res.as_abi()
    engine._check(engine.lib.otsdb_agg_finalize_device(
        engine.ctx, ctypes.byref(spec), G, nb, world, gp.data_ptr(),
        ge.data_ptr(), ctypes.byref(r), None))
    torch.cuda.synchronize()
    return _host(res, G)


def shard_cuts():
    """{name: series cuts} over the contiguous mixed batch: on a tile boundary
    of the larger two-level group, one member past it, and three ranks of
    which the middle one holds no member of either two-level group."""
    sizes = GS.mixed_sizes()
    S = sum(sizes)
    big = sizes.index(max(sizes))
    at = sum(sizes[:big])
    L = C.kFoldChunkLarge
    return {"tile": [0, at + 5 * L, S],
            "tile+1": [0, at + 5 * L + 1, S],
            "none-of-large": [0, sizes[0], at, S],
            "three": [0, sizes[0] - L - 1, at + 64 * L + 1, S]}


@pytest.mark.parametrize("cut", sorted(shard_cuts()))
def test_mixed_partials_across_ranks(engine, mixed, cut):
    b, ora = mixed["mixed"]
    cuts = shard_cuts()[cut]
    assert all(x < y for x, y in zip(cuts, cuts[1:]))
    for fill in GS.FILLS:
        for agg in GS.FOLD_AGGS:
            spec = GS.spec_of(b, agg, "sum", fill)
            compare(_partials_at(engine, spec, b.batch, cuts), ora(spec),
                    True, "ranks/%s/%s-%s" % (cut, agg, fill))


@pytest.mark.parametrize("world", [2, 3])
def test_mixed_interleaved_partials_across_ranks(engine, mixed, world):
    """The interleaved batch: every rank holds members of every group, and a
    rank's tiles are cut over its own members (the cuts above are member
    positions of the contiguous batch; here they are series indices)."""
    b, ora = mixed["mixed-inter"]
    S = b.batch.n_series
    cuts = [0] + [r * S // world + r for r in range(1, world)] + [S]
    for fill in GS.FILLS:
        for agg in GS.FOLD_AGGS:
            spec = GS.spec_of(b, agg, "sum", fill)
            compare(_partials_at(engine, spec, b.batch, cuts), ora(spec),
                    True, "ranks/inter%d/%s-%s" % (world, agg, fill))


# -------------------------------------------- host and device entry in turn
def test_entries_large_small_large(engine):
    """build_tiles caches on the group offsets: the host and the device entry
    on one context, a two-level batch, a small one and the first again."""
    from tests.test_gpu_call_sequence import _device, _run_device
    large = GS.mixed(GS.mixed_sizes(), GS.mixed_quiet())
    small = GS.build(GS.groups_of([3, C.kFoldChunkLarge + 1, 0,
                                   C.kFoldChunk + 1]))
    inter = GS.mixed(GS.mixed_sizes(), GS.mixed_quiet(), order="inter")
    # (the interleaved batch has the same group offsets as `large` and other
    # members: the cached tiles hold, the member list is the call's own)
    for k, b in enumerate((large, small, large, inter)):
        ora = Oracle(b.batch)
        db = _device(b.batch)
        for agg, fill in (("sum", "none"), ("min", "zero"), ("last", "none"),
                          ("dev", "none"), ("max", "none")):
            spec = GS.spec_of(b, agg, "sum", fill)
            w = "entries/%d/%s-%s" % (k, agg, fill)
            compare(engine.run(spec, b.batch), ora(spec), True, w + "/host")
            compare(_run_device(engine, spec, db), ora(spec), True,
                    w + "/device")


# --------------------------------------------------------------- selections
@pytest.mark.parametrize("n", GS.selection_ladder())
def test_selections(engine, n):
    """The LDS sort up to SEL_K members, the key transpose (tiles of
    OTSDB_KT_M members) and k_seg_select past it."""
    held(engine, GS.selection_group(n), GS.SEL_AGGS, GS.SEL_FILLS,
         "sel/%d" % n, blind=True)


def test_selections_both_kernels_in_one_batch(engine):
    b = GS.build(GS.groups_of([C.SEL_K, C.SEL_K + 1]), form="double")
    held(engine, b, GS.SEL_AGGS, GS.SEL_FILLS, "sel/both", blind=True)


def test_selection_candidates_at_the_gather_cap(engine):
    """SS_CAP candidates in one bucket (the direct gather) and SS_CAP + 1 in
    its neighbour (a digit pass first): NaN values take the rest of the
    SS_CAP + 6 members out."""
    held(engine, GS.ss_cap_batch(), GS.SEL_AGGS, GS.SEL_FILLS, "sel/ss_cap",
         blind=True)


# ------------------------------------------------------------ raw group-by
@pytest.mark.parametrize("form", ["long", "double"])
def test_raw_group_by(engine, form):
    """No downsampler: groups of 1, SEL_K, SEL_K + 1 and kChunk + 1 members
    with member-less groups between them."""
    b = GS.build(GS.groups_of(GS.raw_sizes()), form=form, raw=True)
    held(engine, b, GS.RAW_AGGS, ("none",), "raw/" + form)
