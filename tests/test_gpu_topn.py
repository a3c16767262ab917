"""highestMax / highestCurrent on the GPU (otsdb_topn_*) against the
plain-Python model (tests/topn_model.py), bit for bit: the picked series'
numbers, their keys and their point lists.  The batches are
tests/topn_cases.py's, which tests/test_topn_model_cpu.py shows to notice
every mutation of the model."""
import numpy as np
import pytest

from opentsdb_amd import abi, core
from opentsdb_amd.batch import HostBatch
from opentsdb_amd.engine import DataPoints
from tests import topn_cases as TC
from tests import topn_model as TM

pytestmark = pytest.mark.gpu

FUNCTIONS = (TM.HIGHEST_MAX, TM.HIGHEST_CURRENT)


@pytest.fixture(scope="module")
def eng():
    from opentsdb_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def to_datapoints(series):
    ts = np.array([p[0] for p in series], np.int64)
    bits = np.array([p[1] if p[2] else TM.bits_of(p[1]) for p in series],
                    np.int64)
    isint = np.array([1 if p[2] else 0 for p in series], np.uint8)
    return DataPoints(ts, bits, isint)


def host_inputs(results):
    return [[to_datapoints(s) for s in res] for res in results]


def as_points(dp):
    return [(int(t), int(b), bool(i)) for t, b, i in zip(dp.ts, dp.bits,
                                                         dp.is_int)]


def model_points(series):
    return [(t, v if i else TM.bits_of(v), i) for t, v, i in series]


def check(eng, case, fn, topn, grid):
    st, picked, keys, series = TM.evaluate(fn, topn, case.start, case.end,
                                           case.results)
    assert st == TM.OK, case
    got_p, got_k, got_s = eng.run_topn(fn, topn, case.start, case.end,
                                       host_inputs(case.results),
                                       grid_interval_ms=grid)
    assert got_p.tolist() == picked
    assert got_k.view(np.int64).tolist() == keys
    assert [as_points(d) for d in got_s] == [model_points(s) for s in series]
    return eng.topn_counters()


GRID = dict(grid=1, general=0, grid_miss=0)
GENERAL = dict(grid=0, general=1, grid_miss=0)
MISSED = dict(grid=1, general=1, grid_miss=1)


@pytest.mark.parametrize("fn", FUNCTIONS)
@pytest.mark.parametrize("case", TC.CASES, ids=lambda c: c.name)
def test_against_the_model(eng, case, fn):
    """Every case against the model; a grid-eligible one twice, first with
    the caller's promise (the grid path answers), then without (the general
    path): both equal the model, so they equal each other bit for bit."""
    for topn in case.topns:
        if case.grid:
            assert check(eng, case, fn, topn, case.grid) == GRID
        assert check(eng, case, fn, topn, 0) == GENERAL


@pytest.mark.parametrize("fn", FUNCTIONS)
@pytest.mark.parametrize("name", ["long_ragged", "mixed_ragged", "off_grid",
                                  "two_grids", "long_then_double"])
def test_a_promise_that_does_not_hold(eng, fn, name):
    """Long and mixed inputs, an off-grid timestamp and two grids under a
    promise they do not keep: the grid path notices on the device (miss
    counter = 1) and the general path answers in the same call."""
    case = TC.BY_NAME[name]
    assert case.grid == 0
    for topn in case.topns:
        assert check(eng, case, fn, topn, TC.IV) == MISSED


@pytest.mark.parametrize("fn", FUNCTIONS)
def test_a_window_past_the_bucket_cap_goes_general(eng, fn):
    """A kept promise of 1 ms over a window of 120,001 grid timestamps (the
    cap is 65,536): the general path, same answer."""
    case = TC.BY_NAME["lerp_gaps"]
    assert check(eng, case, fn, 3, 1) == GENERAL
    assert check(eng, case, fn, 3, TC.IV) == GRID


# ------------------------------------------------------------------ end to end
def test_downsampled_query_straight_into_topn(eng):
    """A small downsampled query (`none` fill, outages) through run_device;
    its DeviceResult goes straight into run_topn_device.  The model runs over
    the CPU oracle's group_by output of the same query."""
    import torch
    from opentsdb_amd.engine import (DeviceBatch, DeviceResult, DeviceTopN,
                                     run_device, run_topn_device)
    from oracle import pyoracle
    rng = np.random.RandomState(7)
    t0, n_series, n_groups = 1_600_000_020_000, 24, 8
    spans = []
    for s in range(n_series):
        ts = t0 + np.arange(0, 600_000, 10_000) + int(rng.randint(0, 9_000))
        keep = np.ones(len(ts), bool)
        a = int(rng.randint(0, len(ts)))
        keep[a:a + int(rng.randint(0, 30))] = False         # an outage
        if s % 5 == 0:
            keep[:int(rng.randint(0, 30))] = False          # a late start
        # quarters: every bucket's sum is exact, so the producing query's
        # values do not depend on the order the engine adds a bucket's points
        # in (the oracle adds them one by one) and the two top-N inputs are
        # the same bits
        spans.append([(int(t), float(rng.randint(0, 400)) / 4.0, True)
                      for t in ts[keep]])
    groups = [spans[g::n_groups] for g in range(n_groups)]
    hb = HostBatch.from_groups(groups)
    start, end = t0, t0 + 599_999
    ds = core.DownsamplingSpecification("1m-avg")
    spec = core.make_spec(start, end, core.Aggregators.get("sum"), ds,
                          start, end)
    want_groups = pyoracle.group_by(spec, hb)
    model_in = [[[(int(p["ts"]),
                   int(p["bits"]) if p["is_int"] else TM.double_of(int(p["bits"])),
                   bool(p["is_int"])) for p in g] for g in want_groups]]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    db = DeviceBatch(dev(hb.offsets), dev(hb.ts), dev(hb.val),
                     dev(hb.group_offsets), dev(hb.group_members),
                     is_float=dev(hb.is_float))
    sz = eng.plan(spec, hb)
    dres = DeviceResult(torch, n_groups, int(sz.max_out_points), "cuda")
    run_device(eng, spec, db, dres)
    n_pts = int(dres.offsets[-1].item())
    for fn in FUNCTIONS:
        for topn in (1, 3, n_groups):
            st, picked, keys, series = TM.evaluate(fn, topn, start, end,
                                                   model_in)
            assert st == TM.OK
            dtop = DeviceTopN(torch, min(topn, n_groups), n_pts, "cuda")
            run_topn_device(eng, fn, topn, start, end, [dres], dtop,
                            grid_interval_ms=core.topn_grid_interval_ms(ds))
            assert eng.topn_counters() == GRID
            assert dtop.n_picked == len(picked)
            assert dtop.picked[:dtop.n_picked].tolist() == picked
            assert dtop.key[:dtop.n_picked].tolist() == keys
            assert ([as_points(d) for d in dtop.points()] ==
                    [model_points(s) for s in series])


# -------------------------------------------------------------------- statuses
@pytest.mark.parametrize("grid", [0, TC.IV])
def test_statuses(eng, grid):
    case = TC.BY_NAME["lerp_gaps"]
    inp = host_inputs(case.results)
    # topn = 0 through the C-ABI itself (the binding refuses it earlier)
    import ctypes as C
    from opentsdb_amd.engine import _topn_host_inputs
    rs, ng, keep, S, N = _topn_host_inputs(inp)
    offs = np.zeros(S + 1, np.int64)
    out = abi.TopNResult(abi.Result(0, offs.ctypes.data, None, None, None),
                         None, None, 0)
    spec = abi.TopNSpec(0, 0, case.start, case.end, 0)
    assert eng.lib.otsdb_topn_run(eng.ctx, C.byref(spec), len(inp), rs,
                                  ng.ctypes.data,
                                  C.byref(out)) == abi.E_ILLEGAL_ARGUMENT
    # no emission in the window: the reference's NullPointerException
    for fn in FUNCTIONS:
        assert TM.evaluate(fn, 1, TC.T0 + 100 * TC.IV, TC.T0 + 101 * TC.IV,
                           case.results)[0] == TM.ILLEGAL_STATE
        with pytest.raises(core.IllegalStateException):
            eng.run_topn(fn, 1, TC.T0 + 100 * TC.IV, TC.T0 + 101 * TC.IV, inp,
                         grid_interval_ms=grid)
    # a repeated timestamp
    bad = [[[TC.dpt(0, 1), TC.dpt(1, 2), TC.dpt(1, 3)], [TC.dpt(0, 5)]]]
    for fn in FUNCTIONS:
        assert TM.evaluate(fn, 1, case.start, case.end, bad)[0] == TM.UNSUPPORTED
        with pytest.raises(core.UnsupportedOperationException):
            eng.run_topn(fn, 1, case.start, case.end, host_inputs(bad),
                         grid_interval_ms=grid)
    # nothing to number: OK, nothing picked
    for fn, empty in ((TM.HIGHEST_MAX, []), (TM.HIGHEST_MAX, [[], []]),
                      (TM.HIGHEST_CURRENT, [[[], []], [[]]])):
        p, k, s = eng.run_topn(fn, 3, case.start, case.end, host_inputs(empty),
                                 grid_interval_ms=grid)
        assert (len(p), len(k), s) == (0, 0, [])
    # highestMax numbers empty series: they can be picked
    st, picked, keys, series = TM.evaluate(TM.HIGHEST_MAX, 3, case.start,
                                           case.end, [[[], []], [[]]])
    assert st == TM.ILLEGAL_STATE
    with pytest.raises(core.IllegalStateException):
        eng.run_topn(TM.HIGHEST_MAX, 3, case.start, case.end,
                     host_inputs([[[], []], [[]]]),
                     grid_interval_ms=grid)


@pytest.mark.parametrize("grid", [0, TC.IV])
def test_capacity_then_retry(eng, grid):
    """An under-sized result: E_CAPACITY with offsets, picked, key and
    n_picked whole; the retry with offsets[n_picked] succeeds."""
    import ctypes as C
    from opentsdb_amd.engine import _topn_host_inputs
    case = TC.BY_NAME["lerp_gaps"]
    fn, topn = TM.HIGHEST_MAX, 3
    st, picked, keys, series = TM.evaluate(fn, topn, case.start, case.end,
                                           case.results)
    rs, ng, keep, S, N = _topn_host_inputs(host_inputs(case.results))
    spec = abi.TopNSpec(0, topn, case.start, case.end, grid)
    need = sum(len(s) for s in series)
    assert need > 2

    def run(cap):
        offs = np.full(topn + 1, -1, np.int64)
        ts = np.zeros(max(cap, 1), np.int64)
        bits = np.zeros(max(cap, 1), np.int64)
        isint = np.zeros(max(cap, 1), np.uint8)
        pk = np.full(topn, -1, np.int64)
        key = np.zeros(topn, np.int64)
        out = abi.TopNResult(abi.Result(cap, offs.ctypes.data, ts.ctypes.data,
                                        bits.ctypes.data, isint.ctypes.data),
                             pk.ctypes.data, key.ctypes.data, 0)
        st = eng.lib.otsdb_topn_run(eng.ctx, C.byref(spec), len(case.results),
                                    rs, ng.ctypes.data, C.byref(out))
        return st, int(out.n_picked), offs, pk, key, ts, bits, isint

    st, k, offs, pk, key, _, _, _ = run(2)
    assert st == abi.E_CAPACITY
    assert k == len(picked) and pk.tolist() == picked and key.tolist() == keys
    assert offs.tolist() == np.cumsum([0] + [len(s) for s in series]).tolist()
    st, k, offs, pk, key, ts, bits, isint = run(int(offs[k]))
    assert st == abi.OK and pk.tolist() == picked
    got = [[(int(ts[j]), int(bits[j]), bool(isint[j]))
            for j in range(offs[i], offs[i + 1])] for i in range(k)]
    assert got == [model_points(s) for s in series]


def test_both_entries_large_small_large_on_one_context(eng):
    """The host and the device entry on one context, inputs of very
    different sizes in turn: workspaces grow and are reused."""
    import torch
    from opentsdb_amd.engine import DeviceResult, DeviceTopN, run_topn_device
    T = TC.round_size()
    order = ["shape_s%d_nb3" % (2 * T + 1), "ragged_small", "shape_s65_nb65",
             "signed_zero", "shape_s%d_nb3" % (2 * T + 1)]
    for name in order:
        case = TC.BY_NAME[name]
        for fn in FUNCTIONS:
            topn = case.topns[-1]
            check(eng, case, fn, topn, 0)
            # the same through the device entry
            st, picked, keys, series = TM.evaluate(fn, topn, case.start,
                                                   case.end, case.results)
            dres = []
            for res in case.results:
                dps = [to_datapoints(s) for s in res]
                n = sum(len(d.ts) for d in dps)
                r = DeviceResult(torch, len(dps), max(n, 1), "cuda")
                offs = np.cumsum([0] + [len(d.ts) for d in dps]).astype(np.int64)
                r.offsets.copy_(torch.from_numpy(offs))
                if n:
                    cat = lambda k: torch.from_numpy(  # noqa: E731
                        np.concatenate([getattr(d, k) for d in dps]))
                    r.ts[:n].copy_(cat("ts"))
                    r.val[:n].copy_(cat("bits"))
                    r.is_int[:n].copy_(cat("is_int"))
                dres.append(r)
            S = sum(len(r) for r in case.results)
            dtop = DeviceTopN(torch, min(topn, S),
                              sum(len(s) for s in series), "cuda")
            run_topn_device(eng, fn, topn, case.start, case.end, dres, dtop,
                            grid_interval_ms=case.grid)
            assert eng.topn_counters() == (GRID if case.grid else GENERAL)
            assert dtop.picked[:dtop.n_picked].tolist() == picked
            assert dtop.key[:dtop.n_picked].tolist() == keys
            assert ([as_points(d) for d in dtop.points()] ==
                    [model_points(s) for s in series])
