"""CPU-side checks of the histogram entries (otsdb_hist_*): the header
declares them, the library exports and binds them, the ABI is still 6, and
null arguments and the limits are refused before any device work (no context
is needed to reach them)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from opentsdb_amd import abi, core

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("otsdb_hist_plan", "otsdb_hist_run", "otsdb_hist_run_device",
           "otsdb_hist_partials_device", "otsdb_hist_finalize_device")


@pytest.fixture(scope="module")
def lib():
    from opentsdb_amd import build
    build.build()
    return abi.load()


def _spec(ds="1m-sum", start=60000, end=3600000):
    d = core.DownsamplingSpecification(ds) if ds else None
    return core.make_spec(start, end, core.Aggregators.get("sum"), d, start, end)


class Call:
    """One otsdb_hist_run / _run_device call's arguments, kept alive."""

    def __init__(self, K=3, n_pct=2, spec=None, lower=None, upper=None,
                 counts_out=False):
        self.spec = spec if spec is not None else _spec()
        self.b = abi.Batch()
        self.b.n_series, self.b.n_points, self.b.n_groups = 4, 100, 2
        self.lower = np.arange(K, dtype=np.float32) if lower is None else \
            np.asarray(lower, np.float32)
        self.upper = self.lower + 1 if upper is None else \
            np.asarray(upper, np.float32)
        self.counts = np.zeros((100, K + 2), np.int64)
        self.h = abi.HistColumns(K, self.lower.ctypes.data,
                                 self.upper.ctypes.data,
                                 self.counts.ctypes.data)
        self.p = np.full(max(n_pct, 1), 50.0, np.float32)
        self.n_pct = n_pct
        self.offs = np.zeros(3, np.int64)
        self.ts = np.zeros(8, np.int64)
        self.pct = np.zeros((max(n_pct, 1), 8), np.float64)
        self.cnt = np.zeros((8, K + 2), np.int64)
        self.r = abi.HistResult(8, self.offs.ctypes.data, self.ts.ctypes.data,
                                self.pct.ctypes.data,
                                self.cnt.ctypes.data if counts_out else None)

    def run(self, lib, ctx=None):
        return lib.otsdb_hist_run(ctx, C.byref(self.spec), C.byref(self.b),
                                  C.byref(self.h), self.p.ctypes.data,
                                  self.n_pct, C.byref(self.r))

    def run_device(self, lib):
        return lib.otsdb_hist_run_device(
            None, C.byref(self.spec), C.byref(self.b), C.byref(self.h),
            self.p.ctypes.data, self.n_pct, C.byref(self.r), None)

    def plan(self, lib):
        sz = abi.Sizes()
        st = lib.otsdb_hist_plan(None, C.byref(self.spec), C.byref(self.b),
                                 C.byref(self.h), C.byref(sz))
        return st, sz


def test_entries_declared_exported_and_bound(lib):
    with open(os.path.join(ROOT, "include", "otsdb_agg.h")) as f:
        src = f.read()
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    PS, PB = C.POINTER(abi.QuerySpec), C.POINTER(abi.Batch)
    PH, PR = C.POINTER(abi.HistColumns), C.POINTER(abi.HistResult)
    want = {
        "otsdb_hist_plan": [vp, PS, PB, PH, C.POINTER(abi.Sizes)],
        "otsdb_hist_run": [vp, PS, PB, PH, vp, i32, PR],
        "otsdb_hist_run_device": [vp, PS, PB, PH, vp, i32, PR, vp],
        "otsdb_hist_partials_device": [vp, PS, PB, PH, vp, vp, vp],
        "otsdb_hist_finalize_device": [vp, PS, PH, i64, i64, vp, vp, vp, i32,
                                       PR, vp],
    }
    for name in ENTRIES:
        assert re.search(r"^otsdb_status %s\(([^;]*)\);" % name, src, re.M), name
        assert name in abi.EXPORTS
        f = getattr(lib, name)
        assert list(f.argtypes) == want[name], name
        assert f.restype is C.c_int
    assert re.search(r"^int32_t otsdb_hist_window\(int32_t n_bins\);", src, re.M)
    assert "otsdb_hist_window" in abi.EXPORTS
    for t in ("otsdb_hist_columns", "otsdb_hist_result"):
        assert re.search(r"^} %s;" % t, src, re.M), t
    assert re.search(r"^#define OTSDB_ABI_VERSION 6$", src, re.M)
    assert lib.otsdb_abi_version() == 6
    assert abi.HIST_MAX_ROW == int(re.search(
        r"#define OTSDB_HIST_MAX_ROW (\d+)", src).group(1))
    assert abi.HIST_MAX_PCT == int(re.search(
        r"#define OTSDB_HIST_MAX_PCT (\d+)", src).group(1))
    # the E_UNSUPPORTED comment no longer lists histograms as a whole
    m = re.search(r"/\* Valid in the reference but not implemented by this "
                  r"engine \((.*?)\)", src, re.S)
    assert m and not m.group(1).startswith("histograms,")


def test_window_planning_is_host_only(lib):
    assert lib.otsdb_hist_window(0) == 0
    assert lib.otsdb_hist_window(255) == 0  # K + 2 = 257
    for K in (1, 2, 61, 100, 126, 254):
        w = lib.otsdb_hist_window(K)
        row = (K + 3) & ~1
        assert w >= 16
        assert 64 + w * (row * 8 + 4) <= 34816  # the fold's LDS budget


def test_null_arguments_reach_no_device(lib):
    E = abi.E_ILLEGAL_ARGUMENT
    c = Call()
    S, B, H, R = (C.byref(c.spec), C.byref(c.b), C.byref(c.h), C.byref(c.r))
    p = c.p.ctypes.data
    assert c.run(lib) == E            # everything valid but the context
    assert b"context" in lib.otsdb_last_error()
    assert c.run_device(lib) == E
    assert lib.otsdb_hist_run(None, None, B, H, p, 2, R) == E
    assert lib.otsdb_hist_run(None, S, None, H, p, 2, R) == E
    assert lib.otsdb_hist_run(None, S, B, None, p, 2, R) == E
    assert lib.otsdb_hist_run(None, S, B, H, None, 2, R) == E
    assert lib.otsdb_hist_run(None, S, B, H, p, 2, None) == E
    assert lib.otsdb_hist_run_device(None, S, B, H, p, 2, None, None) == E
    assert lib.otsdb_hist_partials_device(None, S, B, H, None, None, None) == E
    assert lib.otsdb_hist_partials_device(None, S, B, H, p, p, None) == E
    assert lib.otsdb_hist_finalize_device(None, S, H, 2, 60, None, None, p, 2,
                                          R, None) == E
    assert lib.otsdb_hist_finalize_device(None, S, H, 2, 60, p, p, p, 2, R,
                                          None) == E
    assert lib.otsdb_hist_plan(None, S, B, H, None) == E
    # a schema without arrays, no buckets, a negative percentile count
    c2 = Call()
    c2.h.lower = None
    assert c2.run(lib) == E
    assert Call(K=3, n_pct=-1).run(lib) == E
    c3 = Call()
    c3.h.n_bins = 0
    assert c3.run(lib) == E


def test_limits_are_checked_before_any_device_work(lib):
    U, E, CAP = abi.E_UNSUPPORTED, abi.E_ILLEGAL_ARGUMENT, abi.E_CAPACITY
    for call in (lambda c: c.run(lib), lambda c: c.run_device(lib)):
        assert call(Call(K=255)) == U  # K + 2 = 257
        assert b"257" in lib.otsdb_last_error()
        assert call(Call(K=254)) == E  # in range: stops at the null context
        assert call(Call(n_pct=17)) == U
        assert b"17" in lib.otsdb_last_error()
        assert call(Call(n_pct=16)) == E
        assert call(Call(n_pct=0)) == E  # no percentile, no counts output
        assert b"counts" in lib.otsdb_last_error()
        assert call(Call(n_pct=0, counts_out=True)) == E  # (null context)
        assert b"context" in lib.otsdb_last_error()
        # schema order: Float.compare on lower, then upper, strictly
        assert call(Call(lower=[0, 2, 1])) == E
        assert b"ascend" in lib.otsdb_last_error()
        assert call(Call(lower=[0, 1, 1], upper=[1, 2, 2])) == E  # a repeat
        assert b"ascend" in lib.otsdb_last_error()
        assert call(Call(lower=[0, 1, 1], upper=[1, 3, 2])) == E
        assert b"ascend" in lib.otsdb_last_error()
        assert call(Call(lower=[0, 1, 1], upper=[1, 2, 3])) == E
        assert b"context" in lib.otsdb_last_error()
        assert call(Call(lower=[0.0, -0.0, 1.0])) == E  # -0.0 sorts first
        assert b"ascend" in lib.otsdb_last_error()
        assert call(Call(lower=[-0.0, 0.0, np.nan])) == E
        assert b"context" in lib.otsdb_last_error()
        assert call(Call(spec=_spec("0all-sum"))) == U
        assert b"0all" in lib.otsdb_last_error()
        s = _spec("1m-sum")
        s.use_calendar = 1
        assert call(Call(spec=s)) == U
        assert b"calendar" in lib.otsdb_last_error()
        assert call(Call(spec=_spec(None))) == U
        assert b"downsampler" in lib.otsdb_last_error()
        assert call(Call(spec=_spec("1m-sum", start=-5))) == E
        assert call(Call(spec=_spec("1m-sum", start=0, end=10))) == U
    # the dense budget, through the plan: 2 groups x buckets x 5 counts x 8 B
    st, sz = Call().plan(lib)
    assert st == abi.OK and sz.n_buckets == 60 and sz.max_out_points == 120
    big = Call(spec=_spec("1ms-sum", start=1, end=1 + (8 << 30) // 80))
    assert big.plan(lib)[0] == CAP
    assert b"bytes" in lib.otsdb_last_error()
    assert big.run(lib) == CAP
    assert Call(K=255).plan(lib)[0] == U


def test_python_percentile_limit_needs_no_engine():
    from opentsdb_amd.histogram import percentile_spec
    assert len(percentile_spec(range(1, 17))) == 16
    with pytest.raises(core.UnsupportedOperationException):
        percentile_spec(range(1, 18))
