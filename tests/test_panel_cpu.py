"""CPU-side checks of the panel entries (otsdb_agg_*_panel*): the header
declares them, the library exports and binds them, null arguments are refused
without a device, and Engine.run_panel's argument checks run before an engine
is needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from opentsdb_amd import abi, core
from opentsdb_amd.engine import Engine, panel_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("otsdb_agg_plan_panel", "otsdb_agg_run_panel_device",
           "otsdb_agg_run_panel")


@pytest.fixture(scope="module")
def lib():
    from opentsdb_amd import build
    build.build()
    return abi.load()


def _spec(ds="1m-avg"):
    d = core.DownsamplingSpecification(ds) if ds else None
    return core.make_spec(0, 3600000, core.Aggregators.get("sum"), d, 0,
                          3600000)


def test_entries_declared_exported_and_bound(lib):
    with open(os.path.join(ROOT, "include", "otsdb_agg.h")) as f:
        src = f.read()
    vp, i32 = C.c_void_p, C.c_int32
    PS, PB, PR = (C.POINTER(abi.QuerySpec), C.POINTER(abi.Batch),
                  C.POINTER(abi.Result))
    want = {
        "otsdb_agg_plan_panel": [vp, PS, i32, vp, vp, vp, PB,
                                 C.POINTER(abi.Sizes)],
        "otsdb_agg_run_panel_device": [vp, PS, i32, vp, vp, vp, PB, PR, vp],
        "otsdb_agg_run_panel": [vp, PS, i32, vp, vp, vp, PB, PR],
    }
    for name in ENTRIES:
        m = re.search(r"^otsdb_status %s\(([^;]*)\);" % name, src, re.M)
        assert m, name
        # ds_agg_ids comes before agg_ids, as the multi entries order theirs
        assert m.group(1).index("ds_agg_ids") < m.group(1).index(" agg_ids")
        assert name in abi.EXPORTS
        f = getattr(lib, name)
        assert list(f.argtypes) == want[name], name
        assert f.restype is C.c_int
    assert re.search(r"^#define OTSDB_ABI_VERSION 6$", src, re.M)
    assert lib.otsdb_abi_version() == 6


def test_null_arguments_reach_no_device(lib):
    spec = _spec()
    b = abi.Batch()
    b.n_series, b.n_points, b.n_groups = 4, 100, 2
    sz = abi.Sizes()
    rs = (abi.Result * 2)()
    ids = np.zeros(2, np.int32)
    p = ids.ctypes.data
    E = abi.E_ILLEGAL_ARGUMENT
    # null context / spec / batch / results
    assert lib.otsdb_agg_run_panel(None, C.byref(spec), 2, p, p, None,
                                   C.byref(b), rs) == E
    assert lib.otsdb_agg_run_panel_device(None, C.byref(spec), 2, p, p, None,
                                          C.byref(b), rs, None) == E
    assert lib.otsdb_agg_plan_panel(None, None, 2, p, p, None, C.byref(b),
                                    C.byref(sz)) == E
    assert lib.otsdb_agg_plan_panel(None, C.byref(spec), 2, p, p, None, None,
                                    C.byref(sz)) == E
    # null id arrays
    assert lib.otsdb_agg_plan_panel(None, C.byref(spec), 2, None, p, None,
                                    C.byref(b), C.byref(sz)) == E
    assert lib.otsdb_agg_plan_panel(None, C.byref(spec), 2, p, None, None,
                                    C.byref(b), C.byref(sz)) == E


def test_plan_checks_follow_the_multi_entries(lib):
    spec = _spec()
    b = abi.Batch()
    b.n_series, b.n_points, b.n_groups = 4, 100, 2
    sz = abi.Sizes()
    A = core.Aggregators

    def plan(ds, aggs, interps=None, s=spec):
        ds, aggs = np.array(ds, np.int32), np.array(aggs, np.int32)
        it = None if interps is None else np.array(interps, np.int32)
        return lib.otsdb_agg_plan_panel(
            None, C.byref(s), len(aggs), ds.ctypes.data, aggs.ctypes.data,
            None if it is None else it.ctypes.data, C.byref(b), C.byref(sz))
    mn, av, mx = A.get("min").id, A.get("avg").id, A.get("max").id
    assert plan([], []) == abi.E_ILLEGAL_ARGUMENT
    assert plan([mn] * 33, [mn] * 33) == abi.E_ILLEGAL_ARGUMENT
    assert plan([mn, 99], [mn, mx]) == abi.E_NO_SUCH_ELEMENT
    assert plan([mn, -1], [mn, mx]) == abi.E_NO_SUCH_ELEMENT
    assert plan([mn, mx], [mn, 99]) == abi.E_NO_SUCH_ELEMENT
    assert plan([mn, A.NONE.id], [mn, mx]) == abi.E_ILLEGAL_ARGUMENT
    assert plan([mn, mx], [mn, mx], [0, 7]) == abi.E_ILLEGAL_ARGUMENT
    # raw group-by has no downsampler: the functions are ignored
    assert plan([99, -1], [mn, mx], s=_spec(None)) == abi.OK
    assert plan([mn, av, mx], [mn, av, mx]) == abi.OK
    single = abi.Sizes()
    assert lib.otsdb_agg_plan(None, C.byref(spec), C.byref(b),
                              C.byref(single)) == abi.OK
    assert sz.n_buckets == single.n_buckets == 61
    assert sz.max_out_points == single.max_out_points
    assert sz.workspace_bytes > single.workspace_bytes


def test_panel_args():
    A, I = core.Aggregators, core.Interpolation
    n, ds, ids, it = panel_args([("min", "min"), (A.get("avg"), "avg"),
                                 ("max", A.get("max").id, I.ZIM),
                                 ("p99", "zimsum", None)])
    assert n == 4 and all(a.dtype == np.int32 for a in (ds, ids, it))
    assert list(ids) == [A.get(a).id for a in ("min", "avg", "max", "p99")]
    assert list(ds) == [A.get(a).id for a in ("min", "avg", "max", "zimsum")]
    assert list(it) == [-1, -1, int(I.ZIM), -1]


@pytest.mark.parametrize("queries,exc", [
    ([], core.IllegalArgumentException),
    ([("sum", "avg")] * 33, core.IllegalArgumentException),
    ([("sum", "avg"), ("nosuch", "avg")], core.NoSuchElementException),
    ([("sum", "avg"), ("sum", "nosuch")], core.NoSuchElementException),
    ([("sum", "avg"), ("sum", "none")], core.IllegalArgumentException),
    ([("sum", "avg"), ("sum",)], core.IllegalArgumentException),
    ([("sum", "avg", 0, 0)], core.IllegalArgumentException),
    ([("sum", "avg", 9)], core.IllegalArgumentException),
])
def test_run_panel_argument_checks_need_no_engine(queries, exc):
    with pytest.raises(exc):
        panel_args(queries)
    # the methods check before they touch the context or the library
    for f in (Engine.run_panel, Engine.plan_panel):
        with pytest.raises(exc):
            f(None, _spec(), queries, None)
