"""CPU-side checks of the histogram entries over storage rows
(otsdb_hist_*rows*): the header declares them, the library exports and binds
them, the ABI is still 6, and null arguments and the argument limits are
refused before any device work (every call here passes a null context)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from opentsdb_amd import abi, core
from opentsdb_amd import histogram as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("otsdb_hist_rows_schema_device", "otsdb_hist_decode_rows_device",
           "otsdb_hist_run_rows_device", "otsdb_hist_run_rows")
T0 = 1356998400


@pytest.fixture(scope="module")
def lib():
    from opentsdb_amd import build
    build.build()
    return abi.load()


def _spec(ds="1m-sum", start=T0 * 1000 + 60000, end=T0 * 1000 + 3600000):
    d = core.DownsamplingSpecification(ds) if ds else None
    return core.make_spec(start, end, core.Aggregators.get("sum"), d, start, end)


class Call:
    """The arguments of one call over two small rows, kept alive."""

    def __init__(self, K=3, n_pct=2, spec=None, lower=None, counts_out=False):
        self.spec = spec if spec is not None else _spec()
        pts = [[((T0 + 60 * i) * 1000, H.Histogram({(0, 1): i + 1}, 0, 0))
                for i in range(3)] for _ in range(2)]
        self.rows = H.hist_rows(pts, 0)
        self.raw = self.rows.as_abi()
        self.b = abi.Batch()
        self.b.n_series, self.b.n_points, self.b.n_groups = 2, 0, 1
        self.goff = np.array([0, 2], np.int64)
        self.mem = np.array([0, 1], np.int64)
        self.b.group_offsets = self.goff.ctypes.data
        self.b.group_members = self.mem.ctypes.data
        self.lower = np.arange(K, dtype=np.float32) if lower is None else \
            np.asarray(lower, np.float32)
        self.upper = self.lower + 1
        self.h = abi.HistColumns(K, self.lower.ctypes.data,
                                 self.upper.ctypes.data, None)
        self.p = np.full(max(n_pct, 1), 50.0, np.float32)
        self.n_pct = n_pct
        self.offs = np.zeros(3, np.int64)
        self.ts = np.zeros(64, np.int64)
        self.pct = np.zeros((max(n_pct, 1), 64), np.float64)
        self.cnt = np.zeros((64, K + 2), np.int64)
        self.r = abi.HistResult(64, self.offs.ctypes.data, self.ts.ctypes.data,
                                self.pct.ctypes.data,
                                self.cnt.ctypes.data if counts_out else None)

    def run(self, lib, codec=0):
        return lib.otsdb_hist_run_rows(
            None, C.byref(self.spec), C.byref(self.raw), codec, C.byref(self.b),
            C.byref(self.h), self.p.ctypes.data, self.n_pct, C.byref(self.r))

    def run_device(self, lib, codec=0):
        return lib.otsdb_hist_run_rows_device(
            None, C.byref(self.spec), C.byref(self.raw), codec, C.byref(self.b),
            C.byref(self.h), self.p.ctypes.data, self.n_pct, C.byref(self.r),
            None)

    def decode(self, lib, codec=0, n_series=2):
        return lib.otsdb_hist_decode_rows_device(
            None, C.byref(self.raw), codec, n_series, C.byref(self.h),
            self.offs.ctypes.data, None, None, 0, None)

    def schema(self, lib, codec=0):
        n = C.c_int32()
        lo = np.zeros(254, np.float32)
        return lib.otsdb_hist_rows_schema_device(
            None, C.byref(self.raw), codec, lo.ctypes.data, lo.ctypes.data,
            C.byref(n), None)


def test_entries_declared_exported_and_bound(lib):
    with open(os.path.join(ROOT, "include", "otsdb_agg.h")) as f:
        src = f.read()
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    PS, PB = C.POINTER(abi.QuerySpec), C.POINTER(abi.Batch)
    PH, PR = C.POINTER(abi.HistColumns), C.POINTER(abi.HistResult)
    PW = C.POINTER(abi.RawRows)
    want = {
        "otsdb_hist_rows_schema_device": [vp, PW, i32, vp, vp,
                                          C.POINTER(i32), vp],
        "otsdb_hist_decode_rows_device": [vp, PW, i32, i64, PH, vp, vp, vp,
                                          i64, vp],
        "otsdb_hist_run_rows_device": [vp, PS, PW, i32, PB, PH, vp, i32, PR,
                                       vp],
        "otsdb_hist_run_rows": [vp, PS, PW, i32, PB, PH, vp, i32, PR],
    }
    for name in ENTRIES:
        assert re.search(r"^otsdb_status %s\(([^;]*)\);" % name, src, re.M), name
        assert name in abi.EXPORTS
        f = getattr(lib, name)
        assert list(f.argtypes) == want[name], name
        assert f.restype is C.c_int
    assert re.search(r"^#define OTSDB_ABI_VERSION 6$", src, re.M)
    assert lib.otsdb_abi_version() == 6
    # the deviations stand next to the entries
    sec = src[src.index("histogram queries from storage rows"):]
    for word in ("bucketCount > 254", "64", "SKIPPED", "[15]", "[16]", "[17]",
                 "pinned"):
        assert word in sec, word


def test_null_arguments_reach_no_device(lib):
    E = abi.E_ILLEGAL_ARGUMENT
    c = Call()
    S, W, B, Hh, R = (C.byref(c.spec), C.byref(c.raw), C.byref(c.b),
                      C.byref(c.h), C.byref(c.r))
    p = c.p.ctypes.data
    for call in (c.run, c.run_device, c.decode, c.schema):
        assert call(lib) == E  # everything valid but the context
        assert b"context" in lib.otsdb_last_error()
    f = lib.otsdb_hist_run_rows
    assert f(None, None, W, 0, B, Hh, p, 2, R) == E
    assert f(None, S, None, 0, B, Hh, p, 2, R) == E
    assert f(None, S, W, 0, None, Hh, p, 2, R) == E
    assert f(None, S, W, 0, B, None, p, 2, R) == E
    assert f(None, S, W, 0, B, Hh, None, 2, R) == E
    assert f(None, S, W, 0, B, Hh, p, 2, None) == E
    g = lib.otsdb_hist_run_rows_device
    assert g(None, S, None, 0, B, Hh, p, 2, R, None) == E
    assert g(None, S, W, 0, B, None, p, 2, R, None) == E
    d = lib.otsdb_hist_decode_rows_device
    o = c.offs.ctypes.data
    assert d(None, None, 0, 2, Hh, o, None, None, 0, None) == E
    assert d(None, W, 0, 2, None, o, None, None, 0, None) == E
    assert d(None, W, 0, 2, Hh, None, None, None, 0, None) == E
    assert d(None, W, 0, 2, Hh, o, o, None, 0, None) == E  # ts without counts
    assert d(None, W, 0, -1, Hh, o, None, None, 0, None) == E
    s = lib.otsdb_hist_rows_schema_device
    n = C.c_int32()
    assert s(None, None, 0, o, o, C.byref(n), None) == E
    assert s(None, W, 0, None, o, C.byref(n), None) == E
    assert s(None, W, 0, o, o, None, None) == E
    # a row array missing, a schema without arrays, no buckets
    c2 = Call()
    c2.raw.col_val_off = None
    for call in (c2.run, c2.run_device, c2.decode, c2.schema):
        assert call(lib) == E
        assert b"raw row" in lib.otsdb_last_error()
    c3 = Call()
    c3.h.lower = None
    assert c3.run(lib) == E and c3.run_device(lib) == E and c3.decode(lib) == E
    c4 = Call()
    c4.h.n_bins = 0
    assert c4.run(lib) == E and c4.run_device(lib) == E and c4.decode(lib) == E
    assert b"0 buckets" in lib.otsdb_last_error()


def test_limits_are_checked_before_any_device_work(lib):
    U, E = abi.E_UNSUPPORTED, abi.E_ILLEGAL_ARGUMENT
    for codec in (-1, 256):
        c = Call()
        for call in (c.run, c.run_device, c.decode, c.schema):
            assert call(lib, codec) == E
            assert b"codec" in lib.otsdb_last_error()
    c = Call()
    for call in (c.run, c.run_device, c.decode, c.schema):
        assert call(lib, 255) == E  # in range: stops at the null context
        assert b"context" in lib.otsdb_last_error()
    for call in (lambda c: c.run(lib), lambda c: c.run_device(lib)):
        assert call(Call(K=255)) == U  # K + 2 = 257
        assert b"257" in lib.otsdb_last_error()
        assert call(Call(K=254)) == E
        assert b"context" in lib.otsdb_last_error()
        assert call(Call(n_pct=17)) == U
        assert call(Call(n_pct=0)) == E  # no percentile, no counts output
        assert b"counts" in lib.otsdb_last_error()
        assert call(Call(n_pct=0, counts_out=True)) == E
        assert b"context" in lib.otsdb_last_error()
        assert call(Call(lower=[0, 2, 1])) == E
        assert b"ascend" in lib.otsdb_last_error()
        assert call(Call(spec=_spec("0all-sum"))) == U
        assert call(Call(spec=_spec(None))) == U
        assert b"downsampler" in lib.otsdb_last_error()
    assert Call(K=255).decode(lib) == U
    assert Call(lower=[0, 2, 1]).decode(lib) == E
    assert b"ascend" in lib.otsdb_last_error()
    assert Call(lower=[0.0, -0.0, 1.0]).decode(lib) == E  # -0.0 sorts first
    assert b"ascend" in lib.otsdb_last_error()
