"""The model of the stored histogram form (tests/hist_rows_model.py) and the
host encoders (opentsdb_amd.histogram) against the known answers of
tests/golden/kat_hist_rows.json, and against each other."""
import numpy as np
import pytest

from opentsdb_amd import core
from opentsdb_amd import histogram as H
from tests import hist_model as HM
from tests import hist_rows_model as M

KATS = M.load_kats()
T0 = 1356998400  # an hour base, seconds


def unhex(s):
    return bytes.fromhex(s.replace(" ", ""))


def replay(calls):
    out = M.Output()
    for name, arg in calls:
        getattr(out, name)(arg)
    return out.toBytes()


def test_pinned_vectors():
    v = KATS["vectors"]
    for x, b in v["writeShort"]:
        assert replay([["writeShort", x]]) == unhex(b)
    for x, b in v["writeFloat"]:
        assert replay([["writeFloat", x]]) == unhex(b)
    for x, b in v["writeLong"]:
        assert replay([["writeLong", int(x)]]) == unhex(b), x
        assert H.write_var_long(int(x)) == unhex(b), x
        assert M.Input(unhex(b)).readLong(True) == int(x), x
    val = v["value"]
    h = H.Histogram({(lo, up): c for lo, up, c in val["buckets"]},
                    val["underflow"], val["overflow"])
    assert H.encode_simple(h, val["codec_id"]) == unhex(val["bytes"])
    got = M.from_histogram(unhex(val["bytes"]), True)
    assert got.buckets == HM.Hist.of(val["buckets"]).buckets
    assert (got.underflow, got.overflow) == (0, 2)
    for q in v["qualifier"]:
        assert H.hist_qualifier(q["ts"]) == (q["base_s"], unhex(q["bytes"]))
        assert H.hist_qualifier(q["ts"], ms=q["ms"])[1] == unhex(q["bytes"])
        ms = q["ts"] if q["ms"] else q["ts"] * 1000
        assert M.timestamp_from_non_dp(q["base_s"], unhex(q["bytes"])) == ms
    with pytest.raises(core.IllegalArgumentException):
        H.hist_qualifier(0)


@pytest.mark.parametrize("c", KATS["blobs"], ids=lambda c: c["name"])
def test_blob_kat(c):
    raw = replay(c["calls"])
    if c["expect"] == "throws":
        with pytest.raises(Exception):
            M.from_histogram(raw, c["include_id"])
        return
    e = c["expect"]
    got = M.from_histogram(raw, c["include_id"])
    assert got.buckets == HM.Hist.of(e["buckets"]).buckets
    assert (got.underflow, got.overflow) == (e["underflow"], e["overflow"])
    # and the encoder writes the same bytes back (testToFromBytes)
    h = H.Histogram({(lo, up): n for lo, up, n in e["buckets"]},
                    e["underflow"], e["overflow"])
    enc = H.encode_simple(h, 0)
    assert (enc if c["include_id"] else enc[1:]) == raw


@pytest.mark.parametrize("c", KATS["spans"], ids=lambda c: c["name"])
def test_span_kat(c):
    sp = M.Span()
    for base, ts in c["rows"]:
        sp.addRow((0, base), [(t, None) for t in ts])
    assert [t for t, _ in sp.points()] == c["expect_ts"]


def test_left_out_is_listed():
    assert all(len(x) == 2 and x[1] for x in KATS["left_out"])
    assert "unpinned" in KATS["source"]


def test_var_long_round_trips():
    vals = [-(1 << 63), (1 << 63) - 1, 0, -1]
    for k in range(1, 10):
        vals += [(1 << (7 * k)) - 1, 1 << (7 * k), (1 << (7 * k)) + 1]
    for v in vals:
        w = HM.wrap_long(v)
        b = H.write_var_long(w)
        assert b == replay([["writeLong", w]])
        assert 1 <= len(b) <= 9
        assert M.Input(b).readLong(True) == w
        if w < 0:
            assert len(b) == 9
        elif w:
            assert len(b) == min(9, (w.bit_length() + 6) // 7)
        # every byte but the last carries the continuation bit
        assert all(x & 0x80 for x in b[:-1]) and (len(b) == 9 or b[-1] < 0x80)
        for cut in range(len(b)):
            with pytest.raises(M.KryoException):
                M.Input(b[:cut]).readLong(True)


def test_an_empty_histogram_does_not_survive_its_stored_form():
    """id + short + two one-byte var-longs is 5 bytes: fromHistogram refuses
    anything under 6, so the scanner skips such a point."""
    v = H.encode_simple(H.Histogram({}, 1, 2), 0)
    assert len(v) == 5
    with pytest.raises(ValueError):
        M.from_histogram(v, True)
    got = M.from_histogram(H.encode_simple(H.Histogram({}, 128, 2), 0), True)
    assert (got.buckets, got.underflow, got.overflow) == ({}, 128, 2)


def test_merge_keeps_the_earlier_rows_point():
    a, b = M.RowSeq(), [(2, "b2"), (3, "b3"), (9, "b9")]
    a.setRow((0, T0), [(1, "a1"), (3, "a3"), (5, "a5")])
    a.addRow(b)
    assert a.seq == [(1, "a1"), (2, "b2"), (3, "a3"), (5, "a5"), (9, "b9")]
    with pytest.raises(RuntimeError):
        a.setRow((0, T0), [])
    with pytest.raises(RuntimeError):
        M.RowSeq().addRow(b)


def random_points(rng, n_series, per_series=5):
    """Sparse histograms over a pool of keys, one a minute."""
    pool = [(float(i) * 0.5 - 3.0, float(i) * 0.5 - 2.5) for i in range(24)]
    series = []
    for s in range(n_series):
        pts = []
        for i in range(per_series):
            ks = [pool[j] for j in
                  rng.choice(len(pool), size=int(rng.integers(1, 9)),
                             replace=False)]
            cnt = {k: int(rng.integers(0, 1 << int(rng.integers(1, 40))))
                   for k in ks}
            ts = (T0 + 3540 + 60 * i) * 1000 + (0 if (s + i) % 3 else 250)
            pts.append((ts, H.Histogram(cnt, int(rng.integers(0, 300)),
                                        int(rng.integers(0, 3)))))
        series.append(pts)
    return series


def test_decode_of_encoded_points_is_densify():
    rng = np.random.default_rng(60)
    series = random_points(rng, 12)  # 60 histograms
    rows = H.hist_rows(series, 7)
    assert rows.n_series == 12
    schema = H.union_schema([h for p in series for _, h in p])
    keys = M.union_keys(M.series_points(rows, 12, 7)[0])
    lo, up = M.schema_of(keys)
    assert np.array_equal(lo.view(np.int32), schema[0].view(np.int32))
    assert np.array_equal(up.view(np.int32), schema[1].view(np.int32))
    offs, ts, cnt = M.decode_rows(rows, 12, 7, schema)
    assert np.array_equal(cnt, H.densify([[h for _, h in p] for p in series],
                                         schema))
    assert list(ts) == [t for p in series for t, _ in p]
    assert list(offs) == [5 * i for i in range(13)]
    assert M.refusal(rows, 12, 7, schema) == (M.OK, -1)
    # another codec's id: skipped by the reference, refused by the engine
    pts, c = M.series_points(rows, 12, 8)
    assert c["skipped"] == 60 and not any(pts)
    assert M.refusal(rows, 12, 8, schema) == (M.E_UNSUPPORTED, 1)


def test_query_over_decoded_rows_is_the_query_over_the_source():
    rng = np.random.default_rng(61)
    series = random_points(rng, 9, per_series=6)
    rows = H.hist_rows(series, 0)
    src = [[(t, HM.Hist.of([(k.lower, k.upper, v)
                            for k, v in h.buckets.items()],
                           h.underflow, h.overflow)) for t, h in p]
           for p in series]
    dec, _ = M.series_points(rows, 9, 0)
    groups = [[0, 1, 2, 3], [4], [5, 6, 7, 8]]
    start, end = (T0 + 3500) * 1000, (T0 + 3900) * 1000
    for agg in (HM.SUM, None):
        a = HM.group_query(start, end, 120000, agg, src, groups)
        b = HM.group_query(start, end, 120000, agg, dec, groups)
        assert len(a) == len(b)
        for ga, gb in zip(a, b):
            assert [(t, h.buckets, h.underflow, h.overflow) for t, h in ga] == \
                   [(t, h.buckets, h.underflow, h.overflow) for t, h in gb]
