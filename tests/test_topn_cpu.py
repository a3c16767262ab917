"""The host side of the top-N functions without a GPU: core.py's parameter
rules (HighestMax.java:49-73), the spec builder's checks, the ctypes structs
and the C-ABI's own argument checks (otsdb_topn_plan does no device work)."""
import ctypes as C

import numpy as np
import pytest

from opentsdb_amd import abi, core
from opentsdb_amd import engine as E


@pytest.fixture(scope="module")
def lib():
    from opentsdb_amd import build
    build.build()
    return abi.load()


def test_parse_topn_follows_the_reference():
    assert core.parse_topn(["1"]) == 1
    assert core.parse_topn(["0010"]) == 10
    assert core.parse_topn(["2147483647", "ignored"]) == 2 ** 31 - 1
    for bad in (None, [], [None], [""], ["0"], ["000"], ["-1"], ["+1"],
                ["1.0"], [" 1"], ["1 "], ["ten"], ["not a number"],
                ["2147483648"], ["99999999999999999999"], [1]):
        with pytest.raises(core.IllegalArgumentException):
            core.parse_topn(bad)


def test_function_names():
    assert core.topn_function("highestMax") == abi.TOPN_HIGHEST_MAX == 0
    assert core.topn_function("highestCurrent") == abi.TOPN_HIGHEST_CURRENT == 1
    assert core.topn_function(1) == 1
    for bad in ("highestmax", "HighestMax", "lowestMax", "", None, 2):
        with pytest.raises(core.IllegalArgumentException):
            core.topn_function(bad)


def test_grid_interval_of_a_downsampler():
    g = core.topn_grid_interval_ms
    assert g("5m-avg") == 300000
    assert g("10s-sum-nan") == 10000
    assert g(core.DownsamplingSpecification("1h-max")) == 3600000
    assert g(None) == 0
    assert g("1dc-sum") == 0      # calendar buckets: no fixed grid
    assert g("0all-sum") == 0


def test_spec_builder_checks_before_the_device():
    s = E.topn_spec("highestMax", "10", 1000, 2000, 500)
    assert (s.function, s.topn, s.start_ms, s.end_ms, s.grid_interval_ms) == (
        0, 10, 1000, 2000, 500)
    assert E.topn_spec("highestCurrent", 3, 0, 1).function == 1
    for args in (("highestMax", 0, 0, 1), ("highestMax", -1, 0, 1),
                 ("highestMax", "0", 0, 1), ("highestMax", "x", 0, 1),
                 ("highestMax", 2 ** 31, 0, 1), ("nosuch", 1, 0, 1),
                 ("highestMax", 1, -1, 1), ("highestMax", 1, 0, 1, -5)):
        with pytest.raises(core.IllegalArgumentException):
            E.topn_spec(*args)


def test_struct_layout():
    assert C.sizeof(abi.TopNSpec) == 4 + 4 + 3 * 8
    assert C.sizeof(abi.TopNResult) == C.sizeof(abi.Result) + 3 * 8
    assert abi.TopNResult.picked.offset == C.sizeof(abi.Result)


def _plan(lib, fn, topn, start, end, grid, groups, points):
    s = abi.TopNSpec(fn, topn, start, end, grid)
    ng = np.asarray(groups, np.int64)
    npnt = np.asarray(points, np.int64)
    sz = abi.Sizes()
    st = lib.otsdb_topn_plan(None, C.byref(s), len(groups),
                             ng.ctypes.data if len(groups) else None,
                             npnt.ctypes.data if len(groups) else None,
                             C.byref(sz))
    return st, sz


def test_plan_sizes_and_statuses(lib):
    st, sz = _plan(lib, 0, 10, 0, 1000, 0, [3, 0, 40], [30, 0, 400])
    assert st == abi.OK
    assert (sz.n_buckets, sz.max_out_points) == (10, 430)
    assert sz.workspace_bytes > 430 * 17
    st, sz = _plan(lib, 1, 100, 0, 1000, 60000, [3], [30])
    assert (st, sz.n_buckets) == (abi.OK, 3)           # min(topn, series)
    st, sz = _plan(lib, 0, 1, 0, 1000, 0, [], [])
    assert (st, sz.n_buckets, sz.max_out_points) == (abi.OK, 0, 0)
    assert _plan(lib, 0, 0, 0, 1000, 0, [3], [30])[0] == abi.E_ILLEGAL_ARGUMENT
    assert b"greater than zero" in lib.otsdb_last_error()
    assert _plan(lib, 0, -4, 0, 1000, 0, [3], [30])[0] == abi.E_ILLEGAL_ARGUMENT
    assert _plan(lib, 2, 1, 0, 1000, 0, [3], [30])[0] == abi.E_ILLEGAL_ARGUMENT
    assert _plan(lib, 0, 1, -1, 1000, 0, [3], [30])[0] == abi.E_ILLEGAL_ARGUMENT
    assert _plan(lib, 0, 1, 0, 1000, -1, [3], [30])[0] == abi.E_ILLEGAL_ARGUMENT
    assert _plan(lib, 0, 1, 0, 1000, 0, [-1], [30])[0] == abi.E_ILLEGAL_ARGUMENT
    assert _plan(lib, 0, 1, 0, 1000, 0, [3], [-2])[0] == abi.E_ILLEGAL_ARGUMENT
    assert _plan(lib, 0, 1, 0, 2 ** 47, 0, [3], [30])[0] == abi.E_UNSUPPORTED


def test_run_entries_refuse_null_and_bad_specs_before_the_device(lib):
    s = abi.TopNSpec(0, 0, 0, 1000, 0)
    offs = np.zeros(2, np.int64)
    out = abi.TopNResult(abi.Result(0, offs.ctypes.data, None, None, None),
                         None, None, 0)
    # no context: refused before anything else is read
    assert lib.otsdb_topn_run(None, C.byref(s), 0, None, None,
                              C.byref(out)) == abi.E_ILLEGAL_ARGUMENT
    assert lib.otsdb_topn_run_device(None, C.byref(s), 0, None, None,
                                     C.byref(out), None) == abi.E_ILLEGAL_ARGUMENT
