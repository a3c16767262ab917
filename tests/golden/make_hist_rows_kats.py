"""Writes tests/golden/kat_hist_rows.json: known answers for the stored form
of histogram points and for span assembly.

Nothing here is computed by the code under test: the byte vectors are
hand-derived from Kryo 3.0.0's documented encoding (the issue "Histogram
queries from storage rows" pins them; the Kryo jar is not available, so no run
of the reference stands behind them), the other cases are the reference's own
unit tests written down as data — the Output call sequence of each test and
the map or timestamps the test expects.

  python tests/golden/make_hist_rows_kats.py
"""
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))


def buckets8():
    """verifyE2EKryo / testToFromBytes: (1,2) .. (8,9), 5 5 5 0 0 0 0 0."""
    calls = [["writeShort", 8]]
    for i in range(8):
        calls += [["writeFloat", float(i + 1)], ["writeFloat", float(i + 2)],
                  ["writeLong", 5 if i < 3 else 0]]
    calls += [["writeLong", 0], ["writeLong", 2]]
    expect = [[float(i + 1), float(i + 2), 5 if i < 3 else 0] for i in range(8)]
    return calls, expect


def percentile_calls(n):
    b = [[1.0, 6.0, 5], [6.0, 10.0, 10], [10.0, 20.0, 1], [20.0, 40.0, 0]][:n]
    calls = [["writeShort", n]]
    for lo, up, c in b:
        calls += [["writeFloat", lo], ["writeFloat", up], ["writeLong", c]]
    calls += [["writeLong", 0], ["writeLong", 5]]
    return calls, b


def main():
    c8, e8 = buckets8()
    c3, e3 = percentile_calls(3)
    c4, e4 = percentile_calls(4)
    doc = {
        "source": "hand-derived; pinned by the issue 'Histogram queries from "
                  "storage rows: decode blobs on the GPU' (Kryo 3.0.0, "
                  "third_party/kryo/include.mk; parity unpinned at the byte "
                  "level)",
        "vectors": {
            "writeShort": [[8, "00 08"]],
            "writeFloat": [[1.0, "3F 80 00 00"], [-0.0, "80 00 00 00"]],
            "writeLong": [
                ["0", "00"], ["127", "7F"], ["128", "80 01"],
                ["300", "AC 02"], ["16383", "FF 7F"], ["16384", "80 80 01"],
                ["72057594037927936", "80 80 80 80 80 80 80 80 01"],
                ["9223372036854775807", "FF FF FF FF FF FF FF FF 7F"],
                ["-1", "FF FF FF FF FF FF FF FF FF"]],
            "value": {
                "codec_id": 0,
                "buckets": [[1.0, 2.0, 5], [2.0, 3.0, 300]],
                "underflow": 0, "overflow": 2,
                "bytes": "00 00 02 3F 80 00 00 40 00 00 00 05 40 00 00 00 "
                         "40 40 00 00 AC 02 00 02"},
            "qualifier": [
                {"ts": 1356998400, "ms": False, "base_s": 1356998400,
                 "bytes": "06 00 00",
                 "cite": "test/core/TestTSDBAddHistogramPoint.java:39-43, "
                         "Internal.getQualifier (Internal.java:1027-1049)"},
                {"ts": 1356998400500, "ms": True, "base_s": 1356998400,
                 "bytes": "06 00 00 01 F4",
                 "cite": "Internal.getQualifier (Internal.java:1034-1040)"}],
        },
        "blobs": [
            {"name": "e2e_kryo_8_buckets", "include_id": False, "calls": c8,
             "expect": {"buckets": e8, "underflow": 0, "overflow": 2},
             "cite": "test/core/TestSimpleHistogram.java:66-128, :131-207"},
            {"name": "e2e_kryo_8_buckets_with_id", "include_id": True,
             "calls": [["writeByte", 0]] + c8,
             "expect": {"buckets": e8, "underflow": 0, "overflow": 2},
             "cite": "test/core/TestSimpleHistogram.java:131-169"},
            {"name": "single_percentile_3_buckets", "include_id": False,
             "calls": c3,
             "expect": {"buckets": e3, "underflow": 0, "overflow": 5},
             "cite": "test/core/TestSimpleHistogram.java:280-303"},
            {"name": "percentile_list_4_buckets", "include_id": False,
             "calls": c4,
             "expect": {"buckets": e4, "underflow": 0, "overflow": 5},
             "cite": "test/core/TestSimpleHistogram.java:306-337, :340-442"},
            {"name": "incomplete_byte_array", "include_id": False,
             "calls": [["writeShort", 4]], "expect": "throws",
             "cite": "test/core/TestSimpleHistogram.java:238-254"},
        ],
        "spans": [
            {"name": "addRow",
             "rows": [[1356998400, [100, 105]]],
             "expect_ts": [100, 105],
             "cite": "test/core/TestHistogramSpan.java:89-101"},
            {"name": "addRowOutOfOrder",
             "rows": [[1357002000, [110, 115]], [1356998400, [100, 105]]],
             "expect_ts": [100, 105, 110, 115],
             "engine": "E_UNSUPPORTED",
             "cite": "test/core/TestHistogramSpan.java:197-222"},
        ],
        "left_out": [
            ["TestSimpleHistogram.testHistogramSerialization, "
             "testInvalidHistogramLength",
             "they go through SimpleHistogram.write / read (Kryo's "
             "KryoSerializable form), not the stored bytes"],
            ["TestSimpleHistogram percentile, merge, JSON and constructor "
             "cases", "no bytes involved; the percentile and merge cases are "
             "tests/golden/kat_histogram.json's"],
            ["TestHistogramSpan.addRowNull / BadKeyLength / MissMatched* / "
             "addDifferentKey", "row keys of another series: the rows here "
             "carry a series index, not a key"],
            ["TestHistogramSpan.getTagUids*, getAggregatedTagUids*, "
             "timestampsOutOfBounds", "UID lookups and index errors, no "
             "decode or assembly"],
            ["TestTSDBAddHistogramPoint beyond the qualifier",
             "the write path"],
        ],
    }
    with open(os.path.join(HERE, "kat_hist_rows.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
