"""CPU-side checks of the multi-aggregator entries of the series-sharded
path: the library exports and binds them, their null / argument checks
touch no device, and dist.run_sharded_multi's argument checks raise before
any collective."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from opentsdb_amd import abi, core, dist as odist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("otsdb_agg_partials_multi_device",
           "otsdb_agg_finalize_multi_device", "otsdb_sel_retarget")


@pytest.fixture(scope="module")
def lib():
    from opentsdb_amd import build
    build.build()
    return abi.load()


def _spec(agg="sum"):
    return core.make_spec(0, 3600000, core.Aggregators.get(agg),
                          core.DownsamplingSpecification("1m-avg"), 0, 3600000)


def test_entries_declared_exported_and_bound(lib):
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    PS, PB, PR = (C.POINTER(abi.QuerySpec), C.POINTER(abi.Batch),
                  C.POINTER(abi.Result))
    want = {
        "otsdb_agg_partials_multi_device": [vp, PS, i32, vp, vp, PB, vp, vp,
                                            vp],
        "otsdb_agg_finalize_multi_device": [vp, PS, i32, vp, vp, i64, i64,
                                            i32, vp, vp, PR, vp],
        "otsdb_sel_retarget": [vp, i32],
    }
    with open(os.path.join(ROOT, "include", "otsdb_agg.h")) as f:
        src = f.read()
    assert lib.otsdb_abi_version() == 6
    for name in ENTRIES:
        assert re.search(r"^otsdb_status %s\(" % name, src, re.M), name
        assert name in abi.EXPORTS
        f = getattr(lib, name)
        assert list(f.argtypes) == want[name], name
        assert f.restype is C.c_int


def test_null_arguments_reach_no_device(lib):
    spec = _spec()
    b = abi.Batch()
    ids = np.array([0, 3], np.int32)
    p99 = core.Aggregators.get("p99").id
    assert lib.otsdb_sel_retarget(None, p99) == abi.E_ILLEGAL_ARGUMENT
    assert lib.otsdb_sel_retarget(None, 0) == abi.E_ILLEGAL_ARGUMENT
    assert lib.otsdb_agg_partials_multi_device(
        None, C.byref(spec), 2, ids.ctypes.data, None, C.byref(b), None,
        None, None) == abi.E_ILLEGAL_ARGUMENT
    assert lib.otsdb_agg_partials_multi_device(
        None, None, 2, None, None, None, None, None, None) == \
        abi.E_ILLEGAL_ARGUMENT
    assert lib.otsdb_agg_finalize_multi_device(
        None, C.byref(spec), 2, ids.ctypes.data, None, 2, 61, 2, None, None,
        None, None) == abi.E_ILLEGAL_ARGUMENT
    assert lib.otsdb_agg_finalize_multi_device(
        None, None, 2, None, None, 2, 61, 2, None, None, None, None) == \
        abi.E_ILLEGAL_ARGUMENT


def test_session_counter_is_not_in_the_older_views():
    """Engine.counters() / multi_counters() keep their keys; the session
    counter has its own method."""
    from opentsdb_amd.engine import Engine
    assert callable(Engine.sel_sessions)
    assert callable(odist.ShardedSelect.retarget)


def test_run_sharded_multi_checks_arguments_first():
    """multi_args raises before the engine, the batch or a process group is
    touched (none exists here)."""
    spec = _spec()
    with pytest.raises(core.IllegalArgumentException):
        odist.run_sharded_multi(None, spec, [], None, 3)
    with pytest.raises(core.IllegalArgumentException):
        odist.run_sharded_multi(None, spec, ["sum"] * 33, None, 3)
    with pytest.raises(core.NoSuchElementException):
        odist.run_sharded_multi(None, spec, ["sum", "nosuch"], None, 3)
    with pytest.raises(core.IllegalArgumentException):
        odist.run_sharded_multi(None, spec, ["sum", "max"], None, 3,
                                interps=[0])
    with pytest.raises(core.IllegalArgumentException):
        odist.run_sharded_select_multi(None, spec, [], None, 3)
    with pytest.raises(core.IllegalArgumentException):  # sum: no selection
        odist.run_sharded_select_multi(None, spec, ["p99", "sum"], None, 3)
