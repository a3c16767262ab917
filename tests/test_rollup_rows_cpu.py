"""CPU-side checks of the rollup rows entries (otsdb_rollup_decode_rows_device,
otsdb_agg_run_rollup_rows*): the iterator-faithful model
(tests/rollup_rows_model.py) reproduces every transcribed reference test, it
replays the seek example of DESIGN.md §4.3.1, the library exports and binds
the entries, and their argument checks run without a device."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from opentsdb_amd import abi, core
from opentsdb_amd.engine import Engine, rollup_rows_args
from tests import kat, rollup_model as RM, rollup_rows_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("otsdb_rollup_decode_rows_device",
           "otsdb_agg_run_rollup_rows_device", "otsdb_agg_run_rollup_rows")
KATS = M.load_kats()


@pytest.fixture(scope="module")
def lib():
    from opentsdb_amd import build
    build.build()
    return abi.load()


def test_kat_file_is_current():
    import runpy
    mod = runpy.run_path(os.path.join(ROOT, "tests", "golden",
                                      "make_rollup_rows_kats.py"))
    for k in ("seq", "query", "skipped"):
        assert json.loads(json.dumps(mod[k])) == KATS[k], k
    names = [c["name"] for c in KATS["seq"] + KATS["query"]]
    assert len(names) == len(set(names))
    assert len(KATS["seq"]) == 51 and len(KATS["query"]) == 16
    assert all(c["cite"].startswith("test/") for c in
               KATS["seq"] + KATS["query"] + KATS["skipped"])
    assert all(c["reason"] for c in KATS["skipped"])


def _value(p):
    """(ts, value, is_float, count) of a model point."""
    return (p[0], RM.to_double(p[1], p[2]) if p[2] else int(p[1]), p[2], p[3])


@pytest.mark.parametrize("c", KATS["seq"], ids=lambda c: c["name"])
def test_model_reproduces_seq_kat(c):
    """RollupSeq.size() and what the iterator yields (after the seek), or the
    exception, cell for cell as the test builds the seq."""
    table, rows = M.kat_table(c), M.kat_rows(c)
    span = M.RollupSpan(table)
    if "error" in c:
        with pytest.raises(M.ERRORS[c["error"]]):
            for _, base_s, cells in rows:
                span.add_row(base_s, cells)
        return
    for _, base_s, cells in rows:
        span.add_row(base_s, cells)
    assert len(span.rows) == 1
    assert span.rows[0].size() == c["size"]
    got = [_value(p) for p in span.iterate(c.get("seek_ms"))]
    if "expect_count" in c:
        assert len(got) == c["expect_count"]
        return
    assert got == [tuple(e) for e in c["expect"]]
    for g, e in zip(got, c["expect"]):
        assert type(g[1]) is type(e[1])  # a long stays a long


def _query_points(c):
    table, rows = M.kat_table(c), M.kat_rows(c)
    spec = kat.spec_from_case(c["spec"])
    return spec, table, M.decode_rows(table, rows, 1, M.query_seek_ms(spec))


@pytest.mark.parametrize("c", KATS["query"], ids=lambda c: c["name"])
def test_model_reproduces_query_kat(c):
    """The whole query over the model's points: the rollup model's buckets
    through the oracle (avg), or the oracle's own single query."""
    from oracle import pyoracle
    if "error" in c:
        with pytest.raises(M.ERRORS[c["error"]]):
            _query_points(c)
        return
    spec, table, (offs, ts, bits, isf, cnt) = _query_points(c)
    batch = M.points_batch(offs, ts, bits, isf)
    if table.need_count:
        ref = RM.expect_query(spec, RM.AVG, batch, cnt)
    else:
        ref = pyoracle.group_by(spec, batch)
    kat.check_points(ref[0], [[e[0], e[1], 1] for e in c["expect"]], c["tol"],
                     c["name"])


def test_model_replays_the_seek_example():
    """Values {1, 2, 3, 5}, counts {1, 3, 5}, seek to 3: the plain
    intersection holds 3 and 5, the iterator yields only 5 — the two cursors
    advance together past the value cells 1 and 2, so count 3 is behind the
    count cursor when the iterator syncs again."""
    t = M.Table("avg", 600, 0, 1)
    rows = M.build_rows(t, [[(1, 10, 1), (2, 20, None), (3, 30, 3),
                             (5, 50, 5)]])
    span = M.RollupSpan(t)
    for _, base_s, cells in rows:
        span.add_row(base_s, cells)
    iv = 600000
    assert [p[0] // iv for p in span.iterate()] == [1, 3, 5]
    assert [p[0] // iv for p in span.iterate(3 * iv)] == [5]
    assert [p[0] // iv for p in span.iterate(3 * iv - 1)] == [5]
    assert [p[0] // iv for p in span.iterate(1 * iv)] == [1, 3, 5]
    # the decode keeps the plain pairs before the seek
    assert [p[0] // iv for p in M.decode_series(t, [(0, rows[0][2])],
                                                3 * iv)] == [1, 5]
    # a count cursor that runs off the end: nothing from the seek on
    rows = M.build_rows(t, [[(1, 10, 1), (2, 20, None), (3, 30, None),
                             (4, 40, None), (5, 50, 5)]])
    assert [p[0] // iv for p in M.decode_series(t, [(0, rows[0][2])],
                                                5 * iv)] == [1]


def test_model_seek_row_passes_rows_without_pairs():
    t = M.Table("avg", 600, 0, 1)
    # rows of 4 offsets: row 0 pairs, row 1 holds sums only, row 2 pairs
    rows = M.build_rows(t, [[(0, 1, 1), (1, 2, 2), (4, 3, None), (5, 4, None),
                             (8, 5, 5), (9, 6, 6)]], cells_per_row=4)
    span = M.RollupSpan(t)
    for _, base_s, cells in rows:
        span.add_row(base_s, cells)
    iv = 600000
    assert [r.size() for r in span.rows] == [2, 0, 2]
    assert span.seek_row(0) == 0 and span.seek_row(2 * iv) == 2
    assert span.seek_row(9 * iv) == 2 and span.seek_row(99 * iv) == 2
    assert [p[0] // iv for p in span.iterate(5 * iv)] == [8, 9]


def test_model_duplicate_runs():
    t = M.Table("sum", 600, 0, 1, fix_duplicates=True)
    q = lambda o: M.qualifier(o, 0, 0)  # noqa: E731
    # the last cell whose timestamp is >= every earlier one's wins the run
    cells = [(q(3), b"\x01", 5), (q(3), b"\x02", 7), (q(3), b"\x03", 6),
             (q(3), b"\x04", 7), (q(3), b"\x05", 2), (q(4), b"\x06", 1)]
    assert [p[1] for p in M.decode_series(t, [(0, cells)])] == [4, 6]
    t.fix_duplicates = False
    with pytest.raises(core.IllegalDataException):
        M.decode_series(t, [(0, cells)])


def test_entries_declared_exported_and_bound(lib):
    with open(os.path.join(ROOT, "include", "otsdb_agg.h")) as f:
        src = f.read()
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    PS, PB, PR = (C.POINTER(abi.QuerySpec), C.POINTER(abi.Batch),
                  C.POINTER(abi.Result))
    PW, PT = C.POINTER(abi.RawRows), C.POINTER(abi.RollupTable)
    want = {
        "otsdb_rollup_decode_rows_device": [vp, PW, PT, i32, i64, i64, vp, vp,
                                            vp, vp, vp, i64, vp],
        "otsdb_agg_run_rollup_rows_device": [vp, PS, PW, PT, i32, PB, PR, vp],
        "otsdb_agg_run_rollup_rows": [vp, PS, PW, PT, i32, PB, PR],
    }
    for name in ENTRIES:
        assert re.search(r"^otsdb_status %s\(" % name, src, re.M), name
        assert name in abi.EXPORTS
        f = getattr(lib, name)
        assert list(f.argtypes) == want[name], name
        assert f.restype is C.c_int
    m = re.search(r"typedef struct \{([^}]*)\} otsdb_rollup_table;", src)
    assert re.findall(r"int32_t (\w+);", m.group(1)) == \
        [f[0] for f in abi.RollupTable._fields_]
    assert C.sizeof(abi.RollupTable) == 16
    assert re.search(r"^#define OTSDB_ABI_VERSION 6$", src, re.M)
    assert lib.otsdb_abi_version() == 6


def _spec(ds="10m-avg", agg="sum"):
    d = core.DownsamplingSpecification(ds) if ds else None
    return core.make_spec(0, 3600000, core.Aggregators.get(agg), d, 0, 3600000)


def _raw():
    t = M.Table("avg", 600, 0, 1)
    return M.host_rows(M.build_rows(t, [[(0, 1, 1), (1, 2, 2)]]))


def test_argument_checks_reach_no_device(lib):
    """raw / table NULL, interval_s <= 0, an unknown rollup aggregator and
    check_rollup's refusals, all with a null context: the checks come before
    anything touches the device."""
    A = core.Aggregators
    hr = _raw()
    raw, tab = hr.as_abi(), abi.RollupTable(600, 0, 1, 0)
    b, r = abi.Batch(), abi.Result()
    b.n_series, b.n_groups = 1, 1
    S, W, T, B, R = (C.byref(_spec()), C.byref(raw), C.byref(tab), C.byref(b),
                     C.byref(r))
    run, dev, dec = (lib.otsdb_agg_run_rollup_rows,
                     lib.otsdb_agg_run_rollup_rows_device,
                     lib.otsdb_rollup_decode_rows_device)
    offs = np.zeros(2, np.int64)
    O = offs.ctypes.data  # noqa: E741

    def all3(raw_, tab_, agg, spec_=S):
        return {run(None, spec_, raw_, tab_, agg, B, R),
                dev(None, spec_, raw_, tab_, agg, B, R, None)}
    E = abi.E_ILLEGAL_ARGUMENT
    assert all3(None, T, A.AVG.id) == {E}
    assert all3(W, None, A.AVG.id) == {E}
    assert dec(None, None, T, A.AVG.id, 1, 0, O, None, None, None, None, 0,
               None) == E
    assert dec(None, W, None, A.AVG.id, 1, 0, O, None, None, None, None, 0,
               None) == E
    for iv in (0, -600):
        bad = abi.RollupTable(iv, 0, 1, 0)
        assert all3(W, C.byref(bad), A.AVG.id) == {E}
        assert dec(None, W, C.byref(bad), A.AVG.id, 1, 0, O, None, None, None,
                   None, 0, None) == E
    for agg in (-1, 35, 99):
        assert all3(W, T, agg) == {abi.E_NO_SUCH_ELEMENT}
        assert dec(None, W, T, agg, 1, 0, O, None, None, None, None, 0,
                   None) == abi.E_NO_SUCH_ELEMENT
    U = abi.E_UNSUPPORTED
    # check_rollup's refusals: R = dev, R = avg with F != avg, no downsampler,
    # per-series calendar anchors
    assert all3(W, T, A.DEV.id, C.byref(_spec("10m-dev"))) == {U}
    assert dec(None, W, T, A.DEV.id, 1, 0, O, None, None, None, None, 0,
               None) == U
    assert all3(W, T, A.AVG.id, C.byref(_spec("10m-max"))) == {U}
    assert all3(W, T, A.AVG.id, C.byref(_spec(None))) == {U}
    assert all3(W, T, A.SUM.id, C.byref(_spec(None))) == {U}
    anch = _spec()
    anch.n_cal_anchors = 2
    assert all3(W, T, A.AVG.id, C.byref(anch)) == {U}
    # valid arguments and no context: the null is the only thing left
    assert all3(W, T, A.AVG.id) == {E}
    assert all3(W, T, A.SUM.id, C.byref(_spec("10m-sum"))) == {E}


@pytest.mark.parametrize("ds,rollup,table,exc", [
    ("10m-avg", "nosuch", (600, 0, 1, 0), core.NoSuchElementException),
    ("10m-avg", "dev", (600, 0, 1, 0), core.UnsupportedOperationException),
    ("10m-max", "avg", (600, 0, 1, 0), core.UnsupportedOperationException),
    (None, "avg", (600, 0, 1, 0), core.UnsupportedOperationException),
    ("10m-avg", "avg", (0, 0, 1, 0), core.IllegalArgumentException),
])
def test_run_rollup_rows_argument_checks_need_no_engine(ds, rollup, table,
                                                        exc):
    with pytest.raises(exc):
        rollup_rows_args(_spec(ds), rollup, table)
    with pytest.raises(exc):
        Engine.run_rollup_rows(None, _spec(ds), None, table, rollup, None)


def test_builder_round_trips_through_the_model():
    """build_rows' knobs (old-style qualifiers, widths, floats, float counts,
    split rows, duplicates) decode to the points they were built from."""
    t = M.Table("avg", 600, 0, 1, fix_duplicates=True)
    pts = [(0, 5, 1), (3, 1.5, 2.0), (7, np.float32(2.25), 3), (3839, -9, 4),
           (3840, 70000, 1e30), (3841, 2 ** 40, float("nan"))]
    rows = M.build_rows(t, [pts], cells_per_row=3840, split=3,
                        old_style=lambda s, o: o % 2 == 1,
                        dup={(0, 7): [(99, 9, 50)]}, with_ts=True)
    assert len(rows) == 5 and rows[0][1] == rows[2][1] != rows[3][1]
    offs, ts, bits, isf, cnt = M.decode_rows(t, rows, 1)
    assert list(ts // 600000) == [0, 3, 7, 3839, 3840, 3841]
    assert list(isf) == [0, 1, 0, 0, 0, 0]
    assert list(bits[[0, 2, 3, 4, 5]]) == [5, 99, -9, 70000, 2 ** 40]
    assert list(cnt) == [1, 2, 9, 4, 2 ** 63 - 1, 0]
