"""CPU-side checks of the multi-aggregator entries: the library exports and
binds them, and Engine.run_multi's argument checks run before anything
touches the device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from opentsdb_amd import abi, core
from opentsdb_amd.engine import multi_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("otsdb_agg_plan_multi", "otsdb_agg_run_multi_device",
           "otsdb_agg_run_multi", "otsdb_agg_run_cells_multi_device")


@pytest.fixture(scope="module")
def lib():
    from opentsdb_amd import build
    build.build()
    return abi.load()


def test_entries_bound_with_argtypes(lib):
    vp, i32 = C.c_void_p, C.c_int32
    PS, PB, PR = (C.POINTER(abi.QuerySpec), C.POINTER(abi.Batch),
                  C.POINTER(abi.Result))
    want = {
        "otsdb_agg_plan_multi": [vp, PS, i32, vp, vp, PB,
                                 C.POINTER(abi.Sizes)],
        "otsdb_agg_run_multi_device": [vp, PS, i32, vp, vp, PB, PR, vp],
        "otsdb_agg_run_multi": [vp, PS, i32, vp, vp, PB, PR],
        "otsdb_agg_run_cells_multi_device": [vp, PS, i32, vp, vp,
                                             C.POINTER(abi.Cells), PB, PR, vp],
    }
    for name in ENTRIES:
        assert name in abi.EXPORTS
        f = getattr(lib, name)
        assert list(f.argtypes) == want[name], name
        assert f.restype is C.c_int


def test_header_declares_the_entries_and_the_limit():
    with open(os.path.join(ROOT, "include", "otsdb_agg.h")) as f:
        src = f.read()
    for name in ENTRIES:
        assert re.search(r"^otsdb_status %s\(" % name, src, re.M), name
    m = re.search(r"^#define OTSDB_MULTI_MAX (\d+)", src, re.M)
    assert m and int(m.group(1)) == abi.MULTI_MAX == 32
    assert re.search(r"^#define OTSDB_ABI_VERSION 6$", src, re.M)


def test_argument_checks_reach_no_device(lib):
    """n_out outside [1, OTSDB_MULTI_MAX], an unknown id and a bad
    interpolation are refused by the plan entry, which needs no context."""
    spec = core.make_spec(0, 3600000, core.Aggregators.get("sum"),
                          core.DownsamplingSpecification("1m-avg"), 0, 3600000)
    b = abi.Batch()
    b.n_series, b.n_points, b.n_groups = 4, 100, 2
    sz = abi.Sizes()

    def plan(ids, interps=None):
        ids = np.array(ids, np.int32)
        it = (np.full(len(ids), -1, np.int32) if interps is None
              else np.array(interps, np.int32))
        return lib.otsdb_agg_plan_multi(None, C.byref(spec), len(ids),
                                        ids.ctypes.data, it.ctypes.data,
                                        C.byref(b), C.byref(sz))
    assert lib.otsdb_agg_plan_multi(None, C.byref(spec), 0, None, None,
                                    C.byref(b), C.byref(sz)) == \
        abi.E_ILLEGAL_ARGUMENT
    assert plan([0] * 33) == abi.E_ILLEGAL_ARGUMENT
    assert plan([0, 99]) == abi.E_NO_SUCH_ELEMENT
    assert plan([0, -1]) == abi.E_NO_SUCH_ELEMENT
    assert plan([0, 3], [0, 7]) == abi.E_ILLEGAL_ARGUMENT
    assert plan([0] * 32) == abi.OK
    assert sz.n_buckets == 61 and sz.max_out_points == 2 * 61
    single = abi.Sizes()
    assert lib.otsdb_agg_plan(None, C.byref(spec), C.byref(b),
                              C.byref(single)) == abi.OK
    # max_out_points bounds each output; the workspace covers the whole call
    assert sz.max_out_points == single.max_out_points
    assert sz.workspace_bytes > single.workspace_bytes


def test_plan_bounds_a_very_wide_none_window_by_its_points(lib):
    """Past 4e9 series x buckets a NONE-fill window is planned by what it can
    emit, groups x n_points (a group emits only at buckets its members have
    points in), not by groups x buckets of the window as given: the host
    entries stage their results by this figure.  A fill policy emits every
    bucket, and smaller windows keep groups x buckets."""
    b = abi.Batch()
    b.n_series, b.n_points, b.n_groups = 43, 100000, 3
    hour = 3600000

    def sizes(fill, end, entry="single"):
        spec = core.make_spec(0, end, core.Aggregators.get("sum"),
                              core.DownsamplingSpecification("1h-avg-" + fill),
                              0, end)
        sz = abi.Sizes()
        if entry == "single":
            st = lib.otsdb_agg_plan(None, C.byref(spec), C.byref(b),
                                    C.byref(sz))
        else:
            ids = np.array([0, 3], np.int32)
            it = np.full(2, -1, np.int32)
            st = lib.otsdb_agg_plan_multi(None, C.byref(spec), 2,
                                          ids.ctypes.data, it.ctypes.data,
                                          C.byref(b), C.byref(sz))
        assert st == abi.OK
        return sz
    end = core.LONG_MAX // 2
    for entry in ("single", "multi"):
        sz = sizes("none", end, entry)
        assert sz.n_buckets == end // hour + 1
        assert 43 * sz.n_buckets > 4e9
        assert sz.max_out_points == 3 * 100000, entry
    # the largest NONE window at or below 4e9 series x buckets, and the next
    nb = int(4e9) // 43
    assert sizes("none", nb * hour - 1).max_out_points == 3 * nb
    assert sizes("none", (nb + 1) * hour - 1).max_out_points == 3 * 100000
    # few points: groups x buckets where that is the smaller
    b.n_points = 10**13
    sz = sizes("none", (nb + 1) * hour - 1)
    assert sz.max_out_points == 3 * (nb + 1)
    b.n_points = 100000
    sz = sizes("nan", 10**8 * hour)  # a fill policy emits every bucket
    assert sz.n_buckets == 10**8 and sz.max_out_points == 3 * 10**8


def test_multi_args():
    n, ids, it = multi_args(["min", core.Aggregators.get("avg"), 3, "p99"])
    assert n == 4 and ids.dtype == np.int32 and it.dtype == np.int32
    assert list(ids) == [core.Aggregators.get(a).id
                         for a in ("min", "avg", "max", "p99")]
    assert list(it) == [-1] * 4
    n, ids, it = multi_args(["sum", "sum"], [core.Interpolation.ZIM, None])
    assert list(it) == [int(core.Interpolation.ZIM), -1]
    with pytest.raises(core.IllegalArgumentException):
        multi_args([])
    with pytest.raises(core.IllegalArgumentException):
        multi_args(["sum"] * 33)
    with pytest.raises(core.NoSuchElementException):
        multi_args(["sum", "nosuch"])
    with pytest.raises(core.IllegalArgumentException):
        multi_args(["sum", "max"], [0])
    with pytest.raises(core.IllegalArgumentException):
        multi_args(["sum"], [9])
