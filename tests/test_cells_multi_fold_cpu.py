"""CPU-side checks of the cells multi-aggregator fold's interface
(OTSDB_SPEC_CELLS_MULTI_FOLD): the flag's value in the header and the Python
mirror, run_cells_multi_device's fold argument and the spec it hands to the
library, and that the plan entry does not depend on the flag."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from opentsdb_amd import abi, core, workload
from opentsdb_amd import engine as eng_mod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from opentsdb_amd import build
    build.build()
    return abi.load()


def _make_spec():
    return core.make_spec(0, 3600000, core.Aggregators.get("sum"),
                          core.DownsamplingSpecification("1m-avg"), 0, 3600000)


def test_flag_value_in_header_and_mirror():
    with open(os.path.join(ROOT, "include", "otsdb_agg.h")) as f:
        src = f.read()
    m = re.search(r"^#define OTSDB_SPEC_CELLS_MULTI_FOLD (\d+)\b", src, re.M)
    assert m and int(m.group(1)) == abi.SPEC_CELLS_MULTI_FOLD == 4
    # a bit of its own beside the two there were
    m = re.search(r"^#define OTSDB_SPEC_MULTI_FOLD (\d+)\b", src, re.M)
    assert m and int(m.group(1)) == abi.SPEC_MULTI_FOLD == 2
    assert abi.SPEC_EXACT_ORDER == 1
    # no new entry, no struct change
    assert re.search(r"^#define OTSDB_ABI_VERSION 6$", src, re.M)


def test_abi_version_stays(lib):
    assert lib.otsdb_abi_version() == 6


def test_fold_argument():
    p = inspect.signature(workload.run_cells_multi_device).parameters
    assert "fold" in p and p["fold"].default is False
    assert list(p)[:7] == ["engine", "spec", "aggs", "cells", "db_groups",
                           "results", "interps"]


def test_fold_spec_keeps_its_two_argument_form():
    spec = _make_spec()
    assert eng_mod._fold_spec(spec, False) is spec
    assert eng_mod._fold_spec(spec, True).flags == abi.SPEC_MULTI_FOLD
    s = eng_mod._fold_spec(spec, True, abi.SPEC_CELLS_MULTI_FOLD)
    assert s is not spec and s.flags == abi.SPEC_CELLS_MULTI_FOLD
    assert eng_mod._fold_spec(spec, False, abi.SPEC_CELLS_MULTI_FOLD) is spec
    assert spec.flags == 0


class _Ptr:
    def data_ptr(self):
        return 0


class _Groups:
    n_groups = 1
    group_offsets = _Ptr()
    group_members = _Ptr()


class _Cells:
    n_series = 1

    def as_abi(self):
        return abi.Cells()


class _Result:
    def as_abi(self):
        return abi.Result()


class _Lib:
    """Records the flags of the spec the cells multi entry is handed."""

    def __init__(self):
        self.flags = []

    def otsdb_agg_run_cells_multi_device(self, ctx, spec, n, ids, interps,
                                         cells, batch, results, stream):
        self.flags.append(int(spec._obj.flags))
        return abi.OK


class _Engine:
    ctx = None

    def __init__(self):
        self.lib = _Lib()

    def _check(self, rc):
        assert rc == abi.OK


@pytest.mark.parametrize("other", [0, abi.SPEC_EXACT_ORDER,
                                   abi.SPEC_MULTI_FOLD,
                                   abi.SPEC_EXACT_ORDER | abi.SPEC_MULTI_FOLD])
def test_fold_sets_bit_4_on_a_copy(other):
    spec = _make_spec()
    spec.flags = other
    e = _Engine()
    args = (["min", "max"], _Cells(), _Groups(), [_Result(), _Result()])
    workload.run_cells_multi_device(e, spec, *args)
    workload.run_cells_multi_device(e, spec, *args, fold=False)
    workload.run_cells_multi_device(e, spec, *args, fold=True)
    workload.run_cells_multi_device(e, spec, *args, None, True)
    assert e.lib.flags == [other, other, other | abi.SPEC_CELLS_MULTI_FOLD,
                           other | abi.SPEC_CELLS_MULTI_FOLD]
    assert spec.flags == other  # the caller's spec is not written


@pytest.mark.parametrize("ds", ["1m-avg", "1m-max-nan", None])
def test_plan_multi_does_not_depend_on_the_flag(lib, ds):
    d = core.DownsamplingSpecification(ds) if ds else None
    spec = core.make_spec(0, 3600000, core.Aggregators.get("sum"), d, 0,
                          3600000)
    b = abi.Batch()
    b.n_series, b.n_points, b.n_groups = 40, 1000, 3
    ids = np.array([core.Aggregators.get(a).id
                    for a in ("min", "avg", "max", "sum", "count")], np.int32)
    it = np.full(len(ids), -1, np.int32)

    def plan(s):
        sz = abi.Sizes()
        assert lib.otsdb_agg_plan_multi(None, C.byref(s), len(ids),
                                        ids.ctypes.data, it.ctypes.data,
                                        C.byref(b), C.byref(sz)) == abi.OK
        return sz.n_buckets, sz.max_out_points, sz.workspace_bytes
    flagged = eng_mod._fold_spec(spec, True, abi.SPEC_CELLS_MULTI_FOLD)
    assert plan(spec) == plan(flagged)
    flagged.flags |= abi.SPEC_MULTI_FOLD
    assert plan(spec) == plan(flagged)
