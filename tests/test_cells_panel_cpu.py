"""CPU-side checks of the panel entry from compacted cells
(otsdb_agg_run_cells_panel_device): the header declares it, the library
exports and binds it, the ABI version stays, null arguments are refused
without a device, and workload.run_cells_panel_device's argument checks run
before an engine or the library is needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from opentsdb_amd import abi, core, workload

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "otsdb_agg_run_cells_panel_device"


@pytest.fixture(scope="module")
def lib():
    from opentsdb_amd import build
    build.build()
    return abi.load()


def _spec(ds="1m-avg"):
    d = core.DownsamplingSpecification(ds) if ds else None
    return core.make_spec(0, 3600000, core.Aggregators.get("sum"), d, 0,
                          3600000)


def test_entry_declared_exported_and_bound(lib):
    with open(os.path.join(ROOT, "include", "otsdb_agg.h")) as f:
        src = f.read()
    m = re.search(r"^otsdb_status %s\(([^;]*)\);" % NAME, src, re.M)
    assert m, NAME
    args = [a.strip() for a in m.group(1).split(",")]
    names = [re.split(r"[\s*]+", a)[-1] for a in args]
    # otsdb_agg_run_cells_multi_device's, ds_agg_ids before agg_ids
    assert names == ["ctx", "spec", "n_out", "ds_agg_ids", "agg_ids",
                     "interps", "cells", "batch", "outs", "hip_stream"]
    assert NAME in abi.EXPORTS
    vp, i32 = C.c_void_p, C.c_int32
    f = getattr(lib, NAME)
    assert list(f.argtypes) == [vp, C.POINTER(abi.QuerySpec), i32, vp, vp, vp,
                                C.POINTER(abi.Cells), C.POINTER(abi.Batch),
                                C.POINTER(abi.Result), vp]
    assert f.restype is C.c_int
    assert re.search(r"^#define OTSDB_ABI_VERSION 6$", src, re.M)
    assert lib.otsdb_abi_version() == 6


def test_null_arguments_reach_no_device(lib):
    spec = _spec()
    b = abi.Batch()
    b.n_series, b.n_points, b.n_groups = 4, 0, 2
    cells = abi.Cells()
    rs = (abi.Result * 2)()
    ids = np.zeros(2, np.int32)
    p = ids.ctypes.data
    E = abi.E_ILLEGAL_ARGUMENT
    f = getattr(lib, NAME)
    S, Cl, B = C.byref(spec), C.byref(cells), C.byref(b)
    assert f(None, S, 2, p, p, None, Cl, B, rs, None) == E       # ctx
    # the other checks come before the context is looked at: a placeholder
    # that is no context stands in for it
    blank = C.create_string_buffer(1 << 16)
    ctx = C.cast(blank, C.c_void_p)
    assert f(ctx, None, 2, p, p, None, Cl, B, rs, None) == E     # spec
    assert f(ctx, S, 2, p, p, None, None, B, rs, None) == E      # cells
    assert f(ctx, S, 2, p, p, None, Cl, None, rs, None) == E     # batch
    assert f(ctx, S, 2, p, p, None, Cl, B, None, None) == E      # results
    assert f(ctx, S, 2, None, p, None, Cl, B, rs, None) == E     # ds_agg_ids
    assert f(ctx, S, 2, p, None, None, Cl, B, rs, None) == E     # agg_ids
    assert f(ctx, S, 0, p, p, None, Cl, B, rs, None) == E        # n_out
    assert f(ctx, S, 33, p, p, None, Cl, B, rs, None) == E


@pytest.mark.parametrize("queries,exc", [
    ([], core.IllegalArgumentException),
    ([("sum", "avg")] * 33, core.IllegalArgumentException),
    ([("sum", "avg"), ("nosuch", "avg")], core.NoSuchElementException),
    ([("sum", "avg"), ("sum", "nosuch")], core.NoSuchElementException),
    ([("sum", "avg"), ("sum", "none")], core.IllegalArgumentException),
    ([("sum", "avg"), ("sum",)], core.IllegalArgumentException),
    ([("sum", "avg", 9)], core.IllegalArgumentException),
])
def test_wrapper_argument_checks_need_no_engine(queries, exc):
    with pytest.raises(exc):
        workload.run_cells_panel_device(None, _spec(), queries, None, None,
                                        [None] * len(queries))


def test_wrapper_counts_results_before_the_library():
    with pytest.raises(core.IllegalArgumentException):
        workload.run_cells_panel_device(
            None, _spec(), [("min", "min"), ("max", "max")], None, None,
            [None])
