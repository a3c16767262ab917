"""CPU-side checks of the rollup entries (otsdb_agg_run_rollup*): the model
(tests/rollup_model.py) reproduces the reference's rollup KATs, the header
declares the entries, the library exports and binds them, null arguments are
refused without a device, and Engine.run_rollup's argument checks run before
an engine is needed."""
import ctypes as C
import json
import math
import os
import re

import numpy as np
import pytest

from opentsdb_amd import abi, core
from opentsdb_amd.engine import Engine, rollup_args
from tests import kat, rollup_model as RM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("otsdb_agg_run_rollup_device", "otsdb_agg_run_rollup")


load_rollup_kats, kat_kind, kat_query = RM.load_kats, RM.kat_kind, RM.kat_query


@pytest.fixture(scope="module")
def lib():
    from opentsdb_amd import build
    build.build()
    return abi.load()


def _spec(ds="1m-avg", agg="sum"):
    d = core.DownsamplingSpecification(ds) if ds else None
    return core.make_spec(0, 3600000, core.Aggregators.get(agg), d, 0, 3600000)


def test_kat_file_is_current():
    import runpy
    mod = runpy.run_path(os.path.join(ROOT, "tests", "golden",
                                      "make_rollup_kats.py"))
    assert json.loads(json.dumps(mod["cases"])) == load_rollup_kats()
    names = [c["name"] for c in load_rollup_kats()]
    assert len(names) == len(set(names)) == 12
    assert all(c["cite"].startswith("test/core/") for c in load_rollup_kats())


@pytest.mark.parametrize("c", [c for c in load_rollup_kats()
                               if "error" not in c and kat_kind(c)],
                         ids=lambda c: c["name"])
def test_model_reproduces_kat(c):
    """The model's bucket points of the case's one series: over a filling
    grid the present buckets (the KAT's non-NaN points), else every point."""
    spec, batch, counts = kat_query(c)
    got = RM.series_buckets(spec, kat_kind(c), batch.ts, batch.val,
                            batch.is_float, counts)
    exp = [(e[0], kat.dec(e[1])) for e in c["expect"]]
    if c["spec"].get("fill"):
        exp = [e for e in exp if not math.isnan(e[1])]
    assert len(got) == len(exp)
    for (t, v), (et, ev) in zip(got, exp):
        assert t == et
        assert abs(v - ev) <= c["tol"]


def test_model_count_wraps_like_a_long():
    # 2^62 + 2^62 = 2^63 wraps to -2^63: 3.0 / -9.223372036854775808e18
    v = RM.bucket_value(RM.AVG, [1.0, 2.0], [2 ** 62, 2 ** 62])
    assert v == 3.0 / -9223372036854775808.0
    assert RM.wrap_long(2 ** 63) == -2 ** 63
    assert RM.wrap_long(-2 ** 63 - 1) == 2 ** 63 - 1
    # ... and on to zero: a present 0.0
    assert RM.bucket_value(RM.AVG, [5.0, 7.0, 1.0, 1.0],
                           [2 ** 62] * 4) == 0.0
    assert RM.bucket_value(RM.AVG, [5.0], [0]) == 0.0
    assert math.copysign(1.0, RM.bucket_value(RM.AVG, [-0.0], [1])) == 1.0
    # NaN is not skipped
    assert math.isnan(RM.bucket_value(RM.AVG, [1.0, math.nan], [1, 1]))
    assert math.isnan(RM.bucket_value(RM.COUNT, [1.0, math.nan], None))
    assert RM.bucket_value(RM.COUNT, [1.0, 2.0, 4.0], None) == 7.0


def test_entries_declared_exported_and_bound(lib):
    with open(os.path.join(ROOT, "include", "otsdb_agg.h")) as f:
        src = f.read()
    vp, i32 = C.c_void_p, C.c_int32
    PS, PB, PR = (C.POINTER(abi.QuerySpec), C.POINTER(abi.Batch),
                  C.POINTER(abi.Result))
    want = {
        "otsdb_agg_run_rollup_device": [vp, PS, PB, i32, vp, PR, vp],
        "otsdb_agg_run_rollup": [vp, PS, PB, i32, vp, PR],
    }
    for name in ENTRIES:
        m = re.search(r"^otsdb_status %s\(([^;]*)\);" % name, src, re.M)
        assert m, name
        args = m.group(1)
        assert args.index("rollup_agg_id") < args.index("value_count") < \
            args.index("otsdb_result")
        assert name in abi.EXPORTS
        f = getattr(lib, name)
        assert list(f.argtypes) == want[name], name
        assert f.restype is C.c_int
    assert re.search(r"^#define OTSDB_ABI_VERSION 6$", src, re.M)
    assert lib.otsdb_abi_version() == 6


def test_null_arguments_reach_no_device(lib):
    spec = _spec("1m-avg")
    b = abi.Batch()
    b.n_series, b.n_points, b.n_groups = 4, 100, 2
    r = abi.Result()
    cnt = np.ones(100, np.int64)
    avg = core.Aggregators.AVG.id
    E = abi.E_ILLEGAL_ARGUMENT
    S, B, R, p = C.byref(spec), C.byref(b), C.byref(r), cnt.ctypes.data
    # null context / spec / batch / result
    assert lib.otsdb_agg_run_rollup(None, S, B, avg, p, R) == E
    assert lib.otsdb_agg_run_rollup_device(None, S, B, avg, p, R, None) == E
    assert lib.otsdb_agg_run_rollup(None, None, B, avg, p, R) == E
    assert lib.otsdb_agg_run_rollup(None, S, None, avg, p, R) == E
    assert lib.otsdb_agg_run_rollup(None, S, B, avg, p, None) == E
    assert lib.otsdb_agg_run_rollup_device(None, S, B, avg, p, None,
                                           None) == E


def test_rollup_args():
    A = core.Aggregators
    cnt = np.ones(4, np.int64)
    r, vc = rollup_args(_spec("1m-avg"), "avg", cnt)
    assert r == A.AVG.id and vc is cnt
    assert rollup_args(_spec("1m-avg"), A.AVG, cnt)[0] == A.AVG.id
    # the counts are ignored unless the rollup aggregator is avg
    assert rollup_args(_spec("1m-count"), "sum", cnt) == (A.SUM.id, None)
    assert rollup_args(_spec("1m-avg"), A.SUM.id, None) == (A.SUM.id, None)
    assert rollup_args(_spec("0all-avg"), "avg", cnt)[0] == A.AVG.id


@pytest.mark.parametrize("ds,rollup,counts,exc", [
    ("1m-avg", "nosuch", True, core.NoSuchElementException),
    ("1m-avg", 99, True, core.NoSuchElementException),
    ("1m-dev", "dev", True, core.UnsupportedOperationException),
    ("1m-avg", "dev", True, core.UnsupportedOperationException),
    ("1m-max", "avg", True, core.UnsupportedOperationException),
    (None, "avg", True, core.UnsupportedOperationException),
    (None, "sum", False, core.UnsupportedOperationException),
    ("1m-avg", "avg", False, core.IllegalArgumentException),
])
def test_run_rollup_argument_checks_need_no_engine(ds, rollup, counts, exc):
    cnt = np.ones(4, np.int64) if counts else None
    with pytest.raises(exc):
        rollup_args(_spec(ds), rollup, cnt)
    # the method checks before it touches the context or the library
    with pytest.raises(exc):
        Engine.run_rollup(None, _spec(ds), None, rollup, cnt)


def test_run_rollup_refuses_anchored_calendars():
    spec = _spec("1m-avg")
    spec.n_cal_anchors = 2
    with pytest.raises(core.UnsupportedOperationException):
        rollup_args(spec, "avg", np.ones(4, np.int64))
