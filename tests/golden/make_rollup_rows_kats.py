"""Writes tests/golden/kat_rollup_rows.json: the reference's JUnit tests over
rollup CELLS as known-answer vectors (data only: cell bytes, timestamps,
values, expected exceptions; every case cites its test, paths under the
reference's tree).

"seq" cases (test/rollup/TestRollupSeq.java): `table` (R, the interval, the
RollupConfig ids, fix_duplicates), `rows` as [series, base_s, [[qualifier hex,
value hex(, HBase timestamp)], ...]] — every KeyValue the test hands to setRow
/ addRow is its own one-column scanner row of the same key, in call order —
`seek_ms` where the test seeks (seconds timestamps written as the milliseconds
RollupIterator.seek turns them into), `size` (RollupSeq.size()) and `expect`
as [ts_ms, value, is_float, value_count]: what the iterator yields (after the
seek), or `expect_count` where the test only counts, or `error`.

"query" cases (test/core/TestTsdbQueryRollup.java): the cells MockBase holds
after the test's writes — one scanner row per row key, columns in qualifier
order — with `spec` (tests/kat.py spec_from_case fields) and `expect` as
[ts_ms, value].

"skipped": the tests not transcribed, each with its reason.

Run:  python tests/golden/make_rollup_rows_kats.py
"""
import json
import os
import struct

TS = "test/rollup/TestRollupSeq.java"
TQ = "test/core/TestTsdbQueryRollup.java"
IDS = {"sum": 0, "count": 1, "max": 2, "min": 3, "avg": 4}

seq, query, skipped = [], [], []


def table(rollup_agg, interval_s, value="sum", fix=False):
    return dict(rollup_agg=rollup_agg, interval_s=interval_s,
                value_id=IDS[value], count_id=IDS["count"], fix_duplicates=fix)


def vle(v):
    """Internal.vleEncodeLong."""
    for w in (1, 2, 4, 8):
        if -(1 << (8 * w - 1)) <= v < (1 << (8 * w - 1)):
            return v.to_bytes(w, "big", signed=True)


def kv(ts_s, value, agg, interval_s, span_s, kind="long"):
    """getRollupKeyValue / TSDB.addAggregatePoint: [base_s, qualifier hex,
    value hex].  kind: long (vle), float (4 bytes), double (8 bytes)."""
    base = ts_s - ts_s % span_s
    if kind == "long":
        val = vle(value)
        flags = len(val) - 1
    elif kind == "float":
        val, flags = struct.pack(">f", value), 0x8 | 0x3
    else:
        val, flags = struct.pack(">d", value), 0x8 | 0x7
    off = (ts_s - base) // interval_s
    q = bytes([IDS[agg]]) + struct.pack(">H", off << 4 | flags)
    return [base, q.hex(), val.hex()]


def one_col_rows(cells):
    """Every KeyValue its own scanner row (cells: [base_s, q, v(, ts)])."""
    return [[0, c[0], [c[1:]]] for c in cells]


def P(ts_ms, v, is_float=0, count=1):
    return [ts_ms, v, is_float, count]


def S(**kw):
    seq.append(kw)


# ---------------------------------------------------- 1 s table, raw bytes
B1 = 1356998400
SUMQ = lambda b: bytes([0x73, 0x75, 0x6D, 0x3A, 0x00, b]).hex()  # noqa: E731
CNTQ = lambda b: bytes([0x63, 0x6F, 0x75, 0x6E, 0x74, 0x3A, 0x00, b]).hex()  # noqa
L8 = lambda v: v.to_bytes(8, "big", signed=True).hex()  # noqa: E731 Bytes.fromLong
H10, H6, D1 = 600, 21600, 86400


def raw(quals, first=4, ts=None):
    """cells (qualifier, Bytes.fromLong(first + i)[, HBase ts])."""
    out = []
    for i, q in enumerate(quals):
        out.append([B1, q, L8(first + i)] + ([] if ts is None else [ts[i]]))
    return out


S(name="setRow", cite=TS + ":198-213", table=table("sum", 1),
  rows=one_col_rows([kv(B1, 4, "sum", 1, 3600)]), size=1,
  expect=[P(B1 * 1000, 4)])
S(name="addRow", cite=TS + ":229-258", table=table("sum", 1),
  rows=one_col_rows([kv(B1, 4, "sum", 1, 3600),
                     kv(B1 + 100, 5, "sum", 1, 3600)]), size=2,
  expect=[P(B1 * 1000, 4), P((B1 + 100) * 1000, 5)])
S(name="addRowMergeLater", cite=TS + ":260-292", table=table("sum", 1),
  rows=one_col_rows(raw([SUMQ(0x07), SUMQ(0x17), SUMQ(0x27), SUMQ(0x37)])),
  size=4, expect=[P((B1 + i) * 1000, 4 + i) for i in range(4)])
S(name="addRowMergeEarlier", cite=TS + ":294-309", table=table("sum", 1),
  rows=one_col_rows([[B1, SUMQ(0x27), L8(6)], [B1, SUMQ(0x37), L8(7)],
                     [B1, SUMQ(0x07), L8(4)]]),
  error="IllegalDataException")
S(name="addRowMergeMiddle", cite=TS + ":311-334", table=table("sum", 1),
  rows=one_col_rows([[B1, SUMQ(0x07), L8(4)], [B1, SUMQ(0x17), L8(5)],
                     [B1, SUMQ(0x47), L8(8)], [B1, SUMQ(0x57), L8(9)],
                     [B1, SUMQ(0x27), L8(6)]]),
  error="IllegalDataException")
S(name="addRowMergeDuplicateLater", cite=TS + ":336-351",
  table=table("sum", 1),
  rows=one_col_rows(raw([SUMQ(0x07), SUMQ(0x17), SUMQ(0x27)]) +
                    [[B1, SUMQ(0x27), L8(6)]]),
  error="IllegalDataException")
S(name="addRowMergeDuplicateLaterRepair", cite=TS + ":353-395",
  table=table("sum", 1, fix=True),
  rows=one_col_rows(raw([SUMQ(0x07), SUMQ(0x17), SUMQ(0x27)], ts=[1, 2, 3]) +
                    [[B1, SUMQ(0x27), L8(7), 8]]),
  size=3, expect=[P(B1 * 1000, 4), P((B1 + 1) * 1000, 5),
                  P((B1 + 2) * 1000, 7)])
S(name="addRowMergeDuplicateEarlier", cite=TS + ":397-415",
  table=table("sum", 1),
  rows=one_col_rows([[B1, SUMQ(0x17), L8(5)], [B1, SUMQ(0x27), L8(6)],
                     [B1, SUMQ(0x37), L8(7)], [B1, SUMQ(0x07), L8(4)]]),
  error="IllegalDataException")
S(name="addRowMergeDuplicateEarlierRepair", cite=TS + ":417-456",
  table=table("sum", 1, fix=True),
  rows=one_col_rows(raw([SUMQ(0x07), SUMQ(0x17), SUMQ(0x27)], ts=[1, 2, 3]) +
                    [[B1, SUMQ(0x27), L8(7), 1]]),
  size=3, expect=[P((B1 + i) * 1000, 4 + i) for i in range(3)])
S(name="addRowMergeDuplicateCountLater", cite=TS + ":458-473",
  table=table("avg", 1),
  rows=one_col_rows(raw([CNTQ(0x07), CNTQ(0x17), CNTQ(0x27)]) +
                    [[B1, CNTQ(0x27), L8(6)]]),
  error="IllegalArgumentException")
# (the test then reads count_values[23]; no point comes of count cells alone)
S(name="addRowMergeDuplicateCountLaterRepair", cite=TS + ":475-494",
  table=table("avg", 1, fix=True),
  rows=one_col_rows(raw([CNTQ(0x07), CNTQ(0x17), CNTQ(0x27)], ts=[1, 2, 3]) +
                    [[B1, CNTQ(0x27), L8(7), 8]]),
  size=0, expect=[])
S(name="addRowMergeDuplicateCountEarlier", cite=TS + ":496-514",
  table=table("avg", 1),
  rows=one_col_rows([[B1, CNTQ(0x17), L8(5)], [B1, CNTQ(0x27), L8(6)],
                     [B1, CNTQ(0x37), L8(7)], [B1, CNTQ(0x07), L8(4)]]),
  error="IllegalArgumentException")
S(name="addRowMergeDuplicateCountEarlierRepair", cite=TS + ":516-535",
  table=table("avg", 1, fix=True),
  rows=one_col_rows(raw([CNTQ(0x07), CNTQ(0x17), CNTQ(0x27)], ts=[1, 2, 3]) +
                    [[B1, CNTQ(0x27), L8(7), 1]]),
  size=0, expect=[])
# rollup_query_sum_mimmax over a cell of id "max": the table's value id
S(name="timestamp", cite=TS + ":633-650", table=table("mimmax", 1, "max"),
  rows=one_col_rows([kv(B1, 7, "max", 1, 3600)]), size=1,
  expect=[P(B1 * 1000, 7)])

# ------------------------------------------------------------ 10 m table
B2 = 1420070400
T10 = [B2 + 600 * i for i in range(8)]


def ten(vals, agg="sum", kind="long"):
    return [kv(T10[i], v, agg, H10, H6, kind) for i, v in enumerate(vals)]


def pts10(vals, is_float=0, count=1, first=0):
    return [P(T10[first + i] * 1000, v, is_float, count)
            for i, v in enumerate(vals)]


S(name="rollup10m", cite=TS + ":653-682", table=table("sum", H10),
  rows=one_col_rows(ten([1, 2, 3, 4, 5])), size=5,
  expect=pts10([1, 2, 3, 4, 5]))
S(name="rollup10mDouble", cite=TS + ":684-713", table=table("sum", H10),
  rows=one_col_rows(ten([0.25, 0.5, 0.75, 1.0, 1.25], kind="double")), size=5,
  expect=pts10([0.25, 0.5, 0.75, 1.0, 1.25], 1))
S(name="rollup10mFloat", cite=TS + ":715-743", table=table("sum", H10),
  rows=one_col_rows(ten([10.25, 10.75, 11.25, 11.75, 12.25], kind="float")),
  size=5, expect=pts10([10.25, 10.75, 11.25, 11.75, 12.25], 1))
S(name="rollup10mMixFloatAndLong", cite=TS + ":745-785",
  table=table("sum", H10),
  rows=one_col_rows([kv(T10[0], 20, "sum", H10, H6),
                     kv(T10[1], 10.5, "sum", H10, H6, "float"),
                     kv(T10[2], 21, "sum", H10, H6),
                     kv(T10[3], 11.5, "sum", H10, H6, "float"),
                     kv(T10[4], 22, "sum", H10, H6),
                     kv(T10[5], 12.5, "sum", H10, H6, "float")]),
  size=6, expect=[P(T10[0] * 1000, 20), P(T10[1] * 1000, 10.5, 1),
                  P(T10[2] * 1000, 21), P(T10[3] * 1000, 11.5, 1),
                  P(T10[4] * 1000, 22), P(T10[5] * 1000, 12.5, 1)])


def avg_cells(sums, counts, count_first=False):
    """The test's call order: offset i's sum cell then its count cell (None:
    the commented-out call)."""
    out = []
    for i in range(max(len(sums), len(counts))):
        pair = []
        if i < len(sums) and sums[i] is not None:
            pair.append(kv(T10[i], sums[i], "sum", H10, H6))
        if i < len(counts) and counts[i] is not None:
            pair.append(kv(T10[i], counts[i], "count", H10, H6))
        out += pair[::-1] if count_first else pair
    return out


def A(name, cite, sums, counts, size, expect, seek_ms=None, count_first=False,
      **kw):
    d = dict(name=name, cite=TS + ":" + cite, table=table("avg", H10),
             rows=one_col_rows(avg_cells(sums, counts, count_first)),
             size=size, expect=expect)
    if seek_ms is not None:
        d["seek_ms"] = seek_ms
    d.update(kw)
    seq.append(d)


FULL_S, FULL_C = [20, 21, 22, 23], [2, 2, 2, 2]
A("rollupAvg10mWithCount", "787-821", FULL_S, FULL_C, 4,
  pts10([20, 21, 22, 23], 0, 2))
A("rollupAvg10mWithCountFirst", "823-857", FULL_S, FULL_C, 4,
  pts10([20, 21, 22, 23], 0, 2), count_first=True)
A("rollupAvg10mMissingCount", "859-876", FULL_S, [], 0, [])
A("rollupAvg10mSkipFirstCount", "878-912", FULL_S, [None, 2, 2, 2], 3,
  pts10([21, 22, 23], 0, 2, first=1))
A("rollupAvg10mSkipLastCount", "914-948", FULL_S, [2, 2, 2, None], 3,
  pts10([20, 21, 22], 0, 2))
A("rollupAvg10mSkipMiddleCount", "950-988", FULL_S, [2, None, 2, 2], 3,
  [P(T10[0] * 1000, 20, 0, 2), P(T10[2] * 1000, 22, 0, 2),
   P(T10[3] * 1000, 23, 0, 2)])
A("rollupAvg10mMissingSum", "990-1006", [], FULL_C, 0, [])
# (not annotated @Test in the reference; its first call is addRow on an unset
# seq — transcribed as the cells it means to hold)
A("rollupAvg10mSkipFirstSum", "1008-1040", [None, 21, 22, 23], FULL_C, 3,
  pts10([21, 22, 23], 0, 2, first=1))
A("rollupAvg10mSkipLastSum", "1042-1075", [20, 21, 22, None], FULL_C, 3,
  pts10([20, 21, 22], 0, 2))
A("rollupAvg10mSkipMiddleSum", "1077-1116", [20, None, 22, 23], FULL_C, 3,
  [P(T10[0] * 1000, 20, 0, 2), P(T10[2] * 1000, 22, 0, 2),
   P(T10[3] * 1000, 23, 0, 2)])
A("rollupAvg10mUnaligned", "1118-1143", [20, None, 22, None],
  [None, 2, None, 2], 0, [])

# endOfArrayDivergence / arrayOverflowAvoidance set the seq's arrays directly
# (Whitebox): the literal qualifier and value bytes, as the cells that hold
# them — value cells first, then count cells.  The first test's arrays end
# with a zero entry inside indices (offset 0 after offset 23), which no cell
# can append; it is left out (the count of 22 is reached before it).
Q_DIV = [0, 11, 0, 27, 0, 43, 0, 59, 0, 75, 0, 91, 0, 107, 0, 123, 0, -117, 0,
         -101, 0, -85, 0, -69, 0, -53, 0, -37, 0, -21, 0, -5, 1, 11, 1, 27, 1,
         43, 1, 59, 1, 75, 1, 91, 1, 123]
V_DIV = [67, 10, 71, -82, 66, -10, -108, 123, 66, -52, -52, -51, 66, -56, 97,
         72, 66, -78, 5, 31, 66, -79, -31, 72, 66, 101, 0, 0, 67, 1, 99, -41,
         66, -17, -77, 51, 66, -48, 10, 61, 66, -48, -118, 61, 66, -77, -47,
         -20, 66, -79, 81, -20, 66, -33, -118, 61, 67, 6, -31, 72, 66, -22,
         -26, 102, 66, -51, -103, -102, 66, -65, 51, 51, 66, -73, 112, -92, 66,
         -71, -47, -20, 66, -25, -6, -31, 67, 10, 10, 61, 65, -115, 92, 41]
CQ_DIV = Q_DIV[:-2] + [1, 107]
CV_DIV = [66, 112, 0, 0] * 6 + [65, -16, 0, 0, 66, 100, 0, 0] + \
    [66, 112, 0, 0] * 14 + [65, 32, 0, 0]
Q_OVF = Q_DIV[:-2] + [1, 107, 1, 123]
V_OVF = [75, 29, -83, 11, 75, 28, -40, -13, 75, 23, -115, 8, 75, 9, -84, 94,
         75, 11, 55, -77, 75, 12, -115, 111, 75, 8, -21, -48, 75, 12, 66, 76,
         75, 8, 118, -48, 75, 11, -65, 121, 75, 26, 64, -100, 75, 69, -15,
         -114, 75, 95, 85, -64, 75, 109, 28, 40, 75, 118, 100, -32, 75, 110,
         -119, 20, 75, 100, -71, -94, 75, 100, -94, 50, 75, 90, -53, 44, 75,
         90, 47, 70, 75, 82, 80, 40, 75, 66, 106, 121, 75, 57, -102, -34, 75,
         53, 69, 4]
CV_OVF = [65, 64, 0, 0] * 10 + [65, 48, 0, 0] + [65, 64, 0, 0] * 13


def array_cells(quals, vals, agg):
    """The cells behind a qualifier / value array pair (4-byte floats)."""
    u = lambda b: b & 0xFF  # noqa: E731
    assert len(vals) == 2 * len(quals)
    return [[B2, bytes([IDS[agg], u(quals[2 * i]), u(quals[2 * i + 1])]).hex(),
             bytes(u(b) for b in vals[4 * i:4 * i + 4]).hex()]
            for i in range(len(quals) // 2)]


S(name="endOfArrayDivergence", cite=TS + ":1145-1170", table=table("avg", H10),
  rows=one_col_rows(array_cells(Q_DIV, V_DIV, "sum") +
                    array_cells(CQ_DIV, CV_DIV, "count")),
  size=22, expect_count=22)
S(name="arrayOverflowAvoidance", cite=TS + ":1172-1196",
  table=table("avg", H10),
  rows=one_col_rows(array_cells(Q_OVF, V_OVF, "sum") +
                    array_cells(Q_OVF, CV_OVF, "count")),
  size=24, expect_count=24)

# ------------------------------------------------------------- 1 h table
T1H = [B2 + 3600 * i for i in range(5)]
S(name="rollup1hLong", cite=TS + ":1198-1227", table=table("sum", 3600),
  rows=one_col_rows([kv(t, i + 1, "sum", 3600, D1)
                     for i, t in enumerate(T1H)]),
  size=5, expect=[P(t * 1000, i + 1) for i, t in enumerate(T1H)])
S(name="rollup1hFloat", cite=TS + ":1229-1258", table=table("sum", 3600),
  rows=one_col_rows([kv(t, 0.25 * (i + 1), "sum", 3600, D1, "double")
                     for i, t in enumerate(T1H)]),
  size=5, expect=[P(t * 1000, 0.25 * (i + 1), 1) for i, t in enumerate(T1H)])
S(name="rollup1hLongWithCount", cite=TS + ":1260-1299",
  table=table("avg", 3600),
  rows=one_col_rows([c for i, t in enumerate(T1H) for c in
                     (kv(t, i + 1, "sum", 3600, D1),
                      kv(t, 2, "count", 3600, D1))]),
  size=5, expect=[P(t * 1000, i + 1, 0, 2) for i, t in enumerate(T1H)])
S(name="rollup1hLongWithCountWithDoubles", cite=TS + ":1301-1340",
  table=table("avg", 3600),
  rows=one_col_rows([c for i, t in enumerate(T1H) for c in
                     (kv(t, i + 1, "sum", 3600, D1),
                      kv(t, 2.0, "count", 3600, D1, "double")
                      if i in (1, 2, 3) else kv(t, 2, "count", 3600, D1))]),
  size=5, expect=[P(t * 1000, i + 1, 0, 2) for i, t in enumerate(T1H)])

# ------------------------------------------------------------------ seeks
EIGHT = one_col_rows(ten([1, 2, 3, 4, 5, 6, 7, 8]))


def K(name, cite, seek_ms, first, **kw):
    S(name=name, cite=TS + ":" + cite, table=table("sum", H10), rows=EIGHT,
      size=8, seek_ms=seek_ms,
      expect=pts10(list(range(first + 1, 9)), first=first), **kw)


K("rollup10mSeekTop", "1342-1378", T10[0] * 1000, 0)
K("rollup10mSeek", "1380-1416", T10[3] * 1000, 3)
S(name="rollup10mSeekOOB", cite=TS + ":1418-1444", table=table("sum", H10),
  rows=EIGHT, size=8, seek_ms=1420075200000, expect=[])
K("rollup10mSeekSeconds", "1446-1482", T10[3] * 1000, 3, seek_in_seconds=True)
K("rollup10mSeekUnaligned", "1484-1520", 1420072123456, 3)

UNAL_S, UNAL_C = [20, None, 22, 23], [2, 2, None, 2]
EMPTY_S, EMPTY_C = [20, None, 22, None], [None, 2, None, 2]
A("rollup10mAvgSeekTopAligned", "1522-1559", FULL_S, FULL_C, 4,
  pts10([20, 21, 22, 23], 0, 2), seek_ms=T10[0] * 1000)
A("rollup10mAvgSeekTopUnaligned", "1561-1595", UNAL_S, UNAL_C, 2,
  [P(T10[0] * 1000, 20, 0, 2), P(T10[3] * 1000, 23, 0, 2)],
  seek_ms=T10[0] * 1000)
A("rollup10mAvgSeekTopUnalignedMissingTop", "1597-1633", FULL_S,
  [None, 2, 2, 2], 3, pts10([21, 22, 23], 0, 2, first=1),
  seek_ms=T10[0] * 1000)
A("rollup10mAvgSeekAligned", "1635-1672", FULL_S, FULL_C, 4,
  pts10([22, 23], 0, 2, first=2), seek_ms=T10[2] * 1000, seek_in_seconds=True)
A("rollup10mAvgSeekUnaligned", "1674-1709", UNAL_S, UNAL_C, 2,
  [P(T10[3] * 1000, 23, 0, 2)], seek_ms=T10[2] * 1000, seek_in_seconds=True)
A("rollup10mAvgSeekUnalignedEmpty", "1711-1733", EMPTY_S, EMPTY_C, 0, [],
  seek_ms=T10[2] * 1000, seek_in_seconds=True)
A("rollup10mAvgSeekTopAlignedOOB", "1735-1761", FULL_S, FULL_C, 4, [],
  seek_ms=1420075200000)
A("rollup10mAvgSeekTopUnalignedOOB", "1763-1787", UNAL_S, UNAL_C, 2, [],
  seek_ms=1420075200000)
A("rollup10mAvgSeekTopUnalignedEmptyOOB", "1789-1811", EMPTY_S, EMPTY_C, 0, [],
  seek_ms=1420075200000)
# (timestamp(i) of the three points; the index checks are object state)
S(name="rollup10mTimestamp", cite=TS + ":1813-1838", table=table("sum", H10),
  rows=one_col_rows(ten([1, 2, 3])), size=3, expect=pts10([1, 2, 3]))
S(name="rollupRowWithDifferentAggregators", cite=TS + ":1840-1872",
  table=table("avg", 3600),
  rows=one_col_rows([kv(t, i + 1, "sum", 3600, D1)
                     for i, t in enumerate(T1H[:3])] +
                    [kv(t, i + 1, "count", 3600, D1)
                     for i, t in enumerate(T1H[:3])]),
  size=3, seek_ms=B2 * 1000, seek_in_seconds=True,
  expect=[P(t * 1000, i + 1, 0, i + 1) for i, t in enumerate(T1H[:3])])

skipped += [
    dict(name="setRowAlreadySet", cite=TS + ":215-227",
         reason="Java object state: setRow called twice on one RollupSeq"),
    dict(name="addRowNotSet", cite=TS + ":557-567",
         reason="Java object state: addRow before setRow"),
    dict(name="addRowDiffBaseTime", cite=TS + ":537-555",
         reason="RollupSeq.addRow's key check: RollupSpan.addRow starts a new "
                "RollupSeq for another key and never reaches it"),
    dict(name="addRowMergeDifferentKey", cite=TS + ":569-588",
         reason="as addRowDiffBaseTime (another tag value: another series)"),
    dict(name="addRowMergeDifferentKeyAndSalt", cite=TS + ":590-610",
         reason="as addRowDiffBaseTime"),
    dict(name="addRowMergeDifferentTime", cite=TS + ":612-631",
         reason="as addRowDiffBaseTime"),
]

# ------------------------------------------------------------- TsdbQuery
T0S, T1S = 1356998400, 1357041600
SPEC = dict(start_ms=T0S * 1000, end_ms=T1S * 1000,
            query_start_ms=T0S * 1000, query_end_ms=T1S * 1000,
            ds_interval_ms=600000)


def scanner_rows(cells):
    """MockBase's rows: one per row key, columns sorted by qualifier."""
    by = {}
    for c in cells:
        by.setdefault(c[0], []).append(c[1:])
    return [[0, b, sorted(by[b], key=lambda c: bytes.fromhex(c[0]))]
            for b in sorted(by)]


def Q(name, cite, rollup, cells, expect, value=None, fix=False, tol=0.0001,
      **spec):
    t = table(rollup, H10, value or ("sum" if rollup == "avg" else rollup), fix)
    d = dict(name=name, cite=TQ + ":" + cite, table=t,
             rows=scanner_rows(cells),
             spec=dict(SPEC, agg=rollup, ds_agg=rollup, **spec), tol=tol)
    d.update(expect)
    query.append(d)


def stored(agg, kind="long", n=73):
    """storeLongRollup / storeFloatRollup's web01 series."""
    return [kv(T0S + 600 * i, 600 * (i + 1) + (0.5 if kind == "float" else 0),
               agg, H10, H6, kind) for i in range(n)]


def every(vals, first=0):
    return dict(expect=[[(T0S + 600 * (first + i)) * 1000, v]
                        for i, v in enumerate(vals)])


Q("run10mSumLongSingleTS", "220-250", "sum", stored("sum"),
  every([600.0 * (i + 1) for i in range(73)]))
Q("run10mSumLongSingleTSRate", "264-293", "sum", stored("sum"),
  every([1.0] * 72, first=1), rate=True, tol=0.00001)
Q("run10mSumFloatSingleTS", "295-324", "sum", stored("sum", "float"),
  every([600.5 + 600 * i for i in range(73)]), tol=0.00001)
Q("run10mSumFloatSingleTSRate", "326-355", "sum", stored("sum", "float"),
  every([1.0] * 72, first=1), rate=True, tol=0.00001)
Q("run10mMaxLongSingleTS", "459-489", "max", stored("max"),
  every([600.0 * (i + 1) for i in range(73)]))
Q("run10mMinLongSingleTS", "491-521", "min", stored("min"),
  every([600.0 * (i + 1) for i in range(73)]))
Q("run10mAvgLongSingleTSMissingCount", "556-576", "avg", stored("sum"),
  dict(expect=[]))
Q("run10mAvgLongSingleTSMissingSum", "578-597", "avg",
  [kv(T0S + 600 * i, 1, "count", H10, H6) for i in range(73)],
  dict(expect=[]))


def sp(ts, v, agg):
    return kv(ts, v, agg, H10, H6)


Q("run10mAvgLongSingleTSMissingACount", "599-635", "avg",
  [sp(1356998400, 20, "sum"), sp(1356998400, 2, "count"),
   sp(1356999000, 40, "sum"),
   sp(1356999600, 60, "sum"), sp(1356999600, 3, "count"),
   sp(1357000200, 80, "sum"), sp(1357000200, 4, "count")],
  dict(expect=[[1356998400000, 10.0], [1356999600000, 20.0],
               [1357000200000, 20.0]]))
Q("run10mAvgLongSingleTSMissingASum", "637-673", "avg",
  [sp(1356998400, 20, "sum"), sp(1356998400, 2, "count"),
   sp(1356999000, 5, "count"),
   sp(1356999600, 60, "sum"), sp(1356999600, 3, "count"),
   sp(1357000200, 80, "sum"), sp(1357000200, 4, "count")],
  dict(expect=[[1356998400000, 10.0], [1356999600000, 20.0],
               [1357000200000, 20.0]]))
Q("run10mAvgLongSingleTSMissingToZero", "675-702", "avg",
  [sp(1356998400, 20, "sum"), sp(1356999000, 5, "count"),
   sp(1356999600, 60, "sum"), sp(1357000200, 4, "count")],
  dict(expect=[]))
LONG_END = dict(end_ms=1359590400000, query_end_ms=1359590400000)
Q("run10mAvgLongSingleTSMissingToZeroOneSpan", "704-752", "avg",
  [sp(1356998400, 20, "sum"), sp(1356998400, 2, "count"),
   sp(1356999000, 40, "sum"), sp(1356999000, 5, "count"),
   sp(1357084800, 60, "sum"), sp(1357085400, 4, "count"),
   sp(1357171200, 90, "sum"), sp(1357171200, 3, "count"),
   sp(1357171800, 100, "sum"), sp(1357171800, 5, "count")],
  dict(expect=[[1356998400000, 10.0], [1356999000000, 8.0],
               [1357171200000, 30.0], [1357171800000, 20.0]]), **LONG_END)
Q("run10mAvgLongSingleTSMissingToZeroBookends", "754-796", "avg",
  [sp(1356998400, 20, "sum"), sp(1356999000, 5, "count"),
   sp(1357084800, 60, "sum"), sp(1357084800, 3, "count"),
   sp(1357085400, 80, "sum"), sp(1357085400, 4, "count"),
   sp(1357171200, 3, "count"), sp(1357171800, 100, "sum")],
  dict(expect=[[1357084800000, 20.0], [1357085400000, 20.0]]), **LONG_END)
# runDupes: Integer.MAX_VALUE (4-byte long) then 42.5F at one timestamp — two
# qualifiers of one offset, the long's sorting first
DUPES = [kv(1357026600, 2 ** 31 - 1, "sum", H10, H6),
         kv(1357026600, 42.5, "sum", H10, H6, "float")]
Q("runDupes", "798-815", "sum", DUPES, dict(error="IllegalDataException"))
Q("runDupes_fix_duplicates", "817-822", "sum", DUPES,
  dict(expect=[[1357026600000, 42.5]]), fix=True)
Q("oldStringPrefix", "825-852", "sum",
  [[T0S, bytes([0x73, 0x75, 0x6D, 0x3A, 0, 0]).hex(), "2a"]],
  dict(expect=[[T0S * 1000, 42.0]]), tol=0.001)

skipped += [
    dict(name="run15mSumLongSingleTS / run30mSumLongSingleTS / "
              "run10mZimSumLongSingleTS / run10mMaxLongSingleTSNotFound",
         cite=TQ + ":101-218",
         reason="the choice of table (raw fallback, a coarser downsampler over "
                "the 10m table, an aggregator without a table) is "
                "TsdbQuery's, before any cell is read"),
    dict(name="run10mSumLongSingleTSInMS", cite=TQ + ":252-262",
         reason="the write path refuses a millisecond timestamp; nothing is "
                "stored"),
    dict(name="run10mSumLongDoubleTS* (three tests)", cite=TQ + ":357-457",
         reason="series filtering and grouping by tags happen before the "
                "engine is called; the aggregation over two series is "
                "test_gpu_rollup_rows's generated ground"),
    dict(name="run10mAvgLongSingleTS", cite=TQ + ":523-554",
         reason="already in kat_rollup.json as points; its cells are the "
                "stored sums of run10mSumLongSingleTS beside a count of 2"),
]

if __name__ == "__main__":
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                       "kat_rollup_rows.json")
    with open(out, "w") as f:
        json.dump({"seq": seq, "query": query, "skipped": skipped}, f,
                  indent=None, separators=(",", ":"))
        f.write("\n")
    print("%d seq + %d query cases -> %s" % (len(seq), len(query), out))
