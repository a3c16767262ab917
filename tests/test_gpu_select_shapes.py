"""Key-shape edges through every selection kernel: keys built from bit
patterns so that k_seg_select takes its digit passes (two, shared and copied
histograms, a short last pass), its shift == 0 exits, the corrected offset
shift and shift == 64, for_keys' head, tail and unrolled body; wave_select
under k_ds_select and k_raw_select sees keys that differ in one byte, heavy
ties and NaN keys that outnumber the values; the k_xsel_* protocol more than
a bin's worth of keys a rank and a second SEL_CHUNK (tests/select_shapes.py).
Needs an MI355X.

Every comparison is against the CPU oracle through the suite's compare(),
bit for bit (selection is exact by construction: the same keys, the same
order statistics).  tests/test_select_shapes_cpu.py pins the oracle to a
plain model on the same batches, shows from a restatement of the kernels'
plans that each batch reaches the branch it is there for, and that the
batches catch the mistakes those branches invite.  A percentile that is
+-0.0 compares by value (zero_sign_blind, the rule of
tests/test_gpu_value_domain.py); median never does.
"""
import time

import numpy as np
import pytest

from opentsdb_amd import dist as odist
from opentsdb_amd.engine import Engine
from oracle import pyoracle
from tests import select_shapes as SS
from tests.test_gpu_group_shapes import DeviceEncoded, Oracle
from tests.test_gpu_multi import with_agg
from tests.test_gpu_parity import compare
from tests.test_gpu_sharded import _select_emulated, engines  # noqa: F401
from tests.test_gpu_value_domain import zero_sign_blind
from tests.value_domain import PERCENTILES

pytestmark = pytest.mark.gpu

K = SS.K


@pytest.fixture(scope="module")
def engine():
    from opentsdb_amd import build
    build.build()
    e = Engine(0)
    t = time.perf_counter()
    yield e
    print("select shapes, the whole file: %.1f s" % (time.perf_counter() - t))
    e.close()


def exact(got, ref, blind, where):
    if blind:
        got = zero_sign_blind(got, ref)
    compare(got, ref, True, where)


def held(engine, b, fills, where, ds="max", aggs=SS.SEL_AGGS, multi=True):
    """engine.run of every aggregator, and one run_multi of four of them (one
    transpose, then the selections over the kept keys), against the
    oracle."""
    ora = Oracle(b.batch)
    for fill in fills:
        for agg in aggs:
            spec = SS.spec_of(b, agg, fill, ds)
            exact(engine.run(spec, b.batch), ora(spec), agg in PERCENTILES,
                  "%s/%s:%s-%s" % (where, agg, ds, fill))
        if multi:
            spec = SS.spec_of(b, SS.MULTI_AGGS[0], fill, ds)
            got = engine.run_multi(spec, SS.MULTI_AGGS, b.batch)
            for i, agg in enumerate(SS.MULTI_AGGS):
                exact(got[i], ora(with_agg(spec, agg)), agg in PERCENTILES,
                      "%s/multi/%s:%s-%s" % (where, agg, ds, fill))


# ------------------------------------------------- across series, one GPU
@pytest.mark.parametrize("name", list(SS.POPULATIONS))
def test_across_series(engine, name):
    """Every size and layout of one population: more than SS_CAP keys (the
    offset pass, the digit passes, the exits), the for_keys ladder, and the
    cuts to SEL_K (k_group_select's sort) and SEL_K + 1 (the direct
    gather); fills none (k_sel_init's counts) and nan."""
    for w, pop, n, how in SS.across_cases():
        if pop == name:
            held(engine, SS.layout(pop, n, how), SS.SEL_FILLS, w)
    # the downsampler `first`: the same bucket values by another kernel
    b = SS.layout(name, SS.big_sizes()[0], "after")
    held(engine, b, ("none",), name + "/first", ds="first", multi=False)


def test_fill_layouts(engine):
    """Every group large under zero / nan: k_keys_transpose<true> applies
    the fill, k_seg_select derives n from the tile counts; under zero the
    fill value is a tie of more than SS_CAP keys between both signs."""
    for w, n, how in SS.fill_cases():
        held(engine, SS.fill_layout(n, how), SS.FILL_FILLS, w)


@pytest.mark.parametrize("name", SS.CELLS_POPULATIONS)
def test_from_cells(engine, name):
    """The same batches as 2-byte-qualifier cells (points on whole
    seconds), through the cells entry."""
    from tests.test_gpu_cells_panel import cells_single
    for n in SS.big_sizes():
        b = SS.layout(name, n, "after")
        case, ora = DeviceEncoded(engine, b.batch), Oracle(b.batch)
        for fill in SS.SEL_FILLS:
            for agg in SS.SEL_AGGS:
                spec = SS.spec_of(b, agg, fill)
                exact(cells_single(engine, case, spec), ora(spec),
                      agg in PERCENTILES,
                      "cells/%s/%d/%s-%s" % (name, n, agg, fill))


# ------------------------------------- as the downsampling function
@pytest.mark.parametrize("interval", ["1m", "0all"])
def test_downsampling(engine, interval):
    """k_ds_select: consecutive buckets of DS_SMALL .. 1000 points (one
    wave's lanes mix the insertion sort and wave_select), 70 buckets (a
    second round of lanes), a series that starts in bucket 3; every count
    meets every bucket population.  One group of the three series, and each
    series alone so that every bucket value shows."""
    from tests.test_select_shapes_cpu import DS_QUERIES
    for grouping, agg in DS_QUERIES:
        b = SS.ds_batch(grouping)
        ora = Oracle(b.batch)
        for fill in SS.SEL_FILLS:
            for fn in SS.DS_FNS:
                spec = SS.ds_spec(b, agg, fn, fill, interval)
                exact(engine.run(spec, b.batch), ora(spec),
                      fn in PERCENTILES, "ds/%s/%s:%s-%s-%s" % (
                          grouping, agg, interval, fn, fill))


# ------------------------------------------------------------ raw group-by
def as_ref(model, is_int):
    """A plain model's result in the oracle's form."""
    out = []
    for ts, vals in model:
        r = np.zeros(len(ts), pyoracle.POINT)
        r["ts"] = ts
        r["bits"] = vals if is_int else \
            np.array(vals, np.float64).view(np.int64)
        r["is_int"] = is_int
        out.append(r)
    return out


@pytest.mark.parametrize("form", ["double", "long"])
def test_raw(engine, form):
    """k_raw_select: groups of 1 .. 300 members (one wave, a wave and one
    key, several rounds) holding the bucket populations at one timestamp
    each."""
    b = SS.raw_batch(form)
    ora = Oracle(b.batch)
    for agg in SS.SEL_AGGS:
        spec = SS.raw_spec(b, agg)
        exact(engine.run(spec, b.batch), ora(spec),
              agg in PERCENTILES and form == "double",
              "raw/%s/%s" % (form, agg))


def test_raw_long_estimators(engine):
    """Every percentile of the registry over 1 .. 41 longs: R_3's rint to
    even and its p <= 0.5 / n, R_7's 1 + (n - 1) p.  The reference is the
    plain model of tests/test_select_shapes_cpu.py (to which that file pins
    the oracle)."""
    from tests.test_select_shapes_cpu import raw_model
    b = SS.raw_long_batch()
    for agg in sorted(PERCENTILES) + ["median"]:
        spec = SS.raw_spec(b, agg)
        got = engine.run(spec, b.batch)
        compare(got, as_ref(raw_model(b, agg), 1), True, "rawlong/" + agg)
        compare(got, pyoracle.group_by(spec, b.batch), True,
                "rawlong/oracle/" + agg)


# ------------------------------------------------------------ across ranks
def ranks_held(engines, b, world, where, aggs=SS.SEL_AGGS):
    ora = Oracle(b.batch)
    for agg in aggs:
        spec = SS.spec_of(b, agg, "none")
        stats = []
        got = _select_emulated(engines, spec, b.batch, world, stats)
        exact(got, ora(spec), agg in PERCENTILES,
              "w%d/%s/%s" % (world, where, agg))
        for reads, passes in stats:
            assert reads <= 2 and passes <= odist.MAX_SEL_PASSES, (
                where, agg, reads, passes)


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("name", SS.RANK_POPULATIONS)
def test_across_ranks(engines, name, world):
    """The otsdb_sel_* protocol with more than a bin's worth of keys a rank:
    the ballot append into the pool, the 2 x 1,024-bin split pass and the
    pool passes; at most two reads of a rank's keys."""
    ranks_held(engines, SS.build([SS.population(name, SS.big_sizes()[0])]),
               world, name)


def test_across_ranks_each_half_on_one_rank(engines):
    b = SS.build([SS.population("straddle_halves", SS.big_sizes()[0])])
    a, e = odist.shard_range(b.batch.n_series, 2, 0, b.batch.offsets)
    v = b.v[0][0]
    assert v[a:e].max() < 1.25 < v[e:].min()
    ranks_held(engines, b, 2, "straddle_halves")


def test_across_ranks_second_chunk(engines):
    """One group of 2 * SEL_CHUNK + 3 members over two ranks: one of them
    holds more than SEL_CHUNK, k_xsel_scan's chunk index c > 0."""
    t = time.perf_counter()
    b = SS.chunk_batch()
    held_by = [len(odist.shard_host_batch(b.batch, 2, r).group_members)
               for r in range(2)]
    assert max(held_by) > K.SEL_CHUNK, held_by
    ranks_held(engines, b, 2, "chunk", aggs=("median", "p50"))
    print("SEL_CHUNK case, %d members: %.1f s" % (
        b.batch.n_series, time.perf_counter() - t))
