"""The histogram model (tests/hist_model.py) against the reference's JUnit
expectations (tests/golden/kat_histogram.json), the padding claim of the
dense schema, and the float percentiles."""
import json
import os
import random

import numpy as np
import pytest

from opentsdb_amd import core, histogram as H
from tests import hist_model as HM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KATS = HM.load_kats()


def test_kat_file_is_current():
    import runpy
    mod = runpy.run_path(os.path.join(ROOT, "tests", "golden",
                                      "make_hist_kats.py"))
    assert json.loads(json.dumps(mod["cases"])) == KATS
    names = [c["name"] for c in KATS]
    assert len(names) == len(set(names)) == 29
    assert all(c["cite"].startswith("test/core/") for c in KATS)


@pytest.mark.parametrize("c", [c for c in KATS if c["kind"] == "percentile"],
                         ids=lambda c: c["name"])
def test_model_percentile_kat(c):
    h = HM.hist_of_case(c["hist"])
    for p, e in zip(c["percentiles"], c["expect"]):
        assert abs(h.percentile(float(np.float32(p))) - e) <= c["tol"]


@pytest.mark.parametrize("c", [c for c in KATS if c["kind"] == "merge"],
                         ids=lambda c: c["name"])
def test_model_merge_kat(c):
    hs = [HM.hist_of_case(h) for h in c["hists"]]
    for o in hs[1:]:
        hs[0].aggregate(o, HM.SUM)
    for lo, up, n in c["expect"]:
        assert hs[0].buckets[HM.make_key(lo, up)] == n
    if c["overflow"] is not None:
        assert hs[0].overflow == c["overflow"]
    if c["underflow"] is not None:
        assert hs[0].underflow == c["underflow"]


@pytest.mark.parametrize("c", [c for c in KATS if c["kind"] == "query"],
                         ids=lambda c: c["name"])
def test_model_query_kat(c):
    ds = core.DownsamplingSpecification(c["ds"])
    assert ds.histogram_aggregation == "SUM"
    pts = HM.kat_query_points(c)
    one = HM.make_key(0.0, 1.0)
    # the downsampler alone, as the downsampler tests drive it
    if c["cite"].startswith("test/core/TestHistogramDownsampler") and pts[0]:
        d = HM.Downsampler(HM.SpanView(pts[0]), ds.getInterval(),
                           ds.histogram_aggregation)
        if c["seek"] is not None:
            d.seek(c["seek"])
        out = []
        while d.hasNext():
            t, h = d.next()
            out.append([t, h.buckets[one]])
        assert out[:len(c["expect"])] == c["expect"]
    # ... and the group's iterator over the case's window
    res = HM.group_query(c["start_ms"], c["end_ms"], ds.getInterval(),
                         ds.histogram_aggregation, pts,
                         [list(range(len(pts)))])[0]
    assert [[t, h.buckets[one]] for t, h in res] == c["expect"]


def test_histogram_aggregation_is_sum_only_for_sum():
    assert core.DownsamplingSpecification("5m-sum").histogram_aggregation == "SUM"
    for f in ("avg", "max", "zimsum", "count"):
        assert core.DownsamplingSpecification(
            "5m-" + f).histogram_aggregation is None


def test_non_sum_keeps_the_first_histogram():
    pts = [(1000, HM.Hist.of([(0.0, 1.0, 3)])), (1500, HM.Hist.of([(0.0, 1.0, 4)])),
           (2100, HM.Hist.of([(0.0, 1.0, 5)]))]
    k = HM.make_key(0.0, 1.0)
    s = HM.group_query(1000, 3000, 1000, HM.SUM, [pts], [[0]])[0]
    f = HM.group_query(1000, 3000, 1000, None, [pts], [[0]])[0]
    assert [(t, h.buckets[k]) for t, h in s] == [(1000, 7), (2000, 5)]
    assert [(t, h.buckets[k]) for t, h in f] == [(1000, 3), (2000, 5)]


def test_float_percentile_is_widened():
    p = H.percentile_spec([99.9])
    assert p.dtype == np.float32
    wide = float(p[0])
    assert wide != 99.9 and wide == 99.90000152587890625
    # counts 999, 1: area of the first key is exactly 99.9 as a double
    # quotient (99900.0 / 1000), which is below the widened float
    h = HM.Hist.of([(0.0, 2.0, 999), (2.0, 4.0, 1)])
    assert h.percentile(99.9) == 1.0      # the double the test writer meant
    assert h.percentile(wide) == 3.0      # what the reference computes


def test_wrapping_and_int_value():
    assert HM.wrap_long(2 ** 63) == -2 ** 63
    assert HM.int_value(2 ** 31) == -2 ** 31
    assert HM.int_value(2 ** 32 + 5) == 5
    # int sum 0 with nonzero counts: every area is -inf or NaN -> 0.0
    h = HM.Hist.of([(0.0, 1.0, 2 ** 31), (1.0, 2.0, 2 ** 31)])
    assert h.percentile(50.0) == 0.0
    # a tie: area == p picks the first key
    assert HM.Hist.of([(0.0, 2.0, 1), (2.0, 4.0, 1)]).percentile(50.0) == 1.0
    assert HM.Hist.of([(0.0, 2.0, 1)]).percentile(float("nan")) == 0.0
    assert HM.Hist.of([(0.0, 2.0, 1)]).percentile(0.5) == -1.0


def test_bucket_order_is_float_compare():
    ks = [H.HistogramBucket(0.0, 1.0), H.HistogramBucket(-0.0, 1.0),
          H.HistogramBucket(float("nan"), 0.0), H.HistogramBucket(-1.0, 5.0),
          H.HistogramBucket(-1.0, 2.0), H.HistogramBucket(float("inf"), 0.0)]
    got = [(float(k.lower), float(k.upper)) for k in sorted(ks)]
    assert str(got) == str([(-1.0, 2.0), (-1.0, 5.0), (-0.0, 1.0), (0.0, 1.0),
                            (float("inf"), 0.0), (float("nan"), 0.0)])
    assert H.float_compare(float("nan"), float("nan")) == 0
    model = sorted([(k.lower, k.upper) for k in ks], key=HM.key_order)
    assert str([(float(a), float(b)) for a, b in model]) == str(got)


def test_densified_union_schema_gives_the_sparse_percentiles():
    """A histogram padded with zero counts to the query's union schema has
    the percentiles of its sparse map: a zero-count key never qualifies."""
    rng = random.Random(7)
    edges = [float(np.float32(x)) for x in
             (-5.0, -0.0, 0.0, 0.5, 1.0, 2.5, 7.0, 20.0, 1e9, float("inf"))]
    keys = [(a, b) for i, a in enumerate(edges) for b in edges[i + 1:]]
    pcts = [float(x) for x in H.percentile_spec(
        [1.0, 25, 50, 90, 99, 99.9, 100.0])]
    for _ in range(40):
        hs = []
        for _ in range(5):
            ks = rng.sample(keys, rng.randint(1, 8))
            hs.append(H.Histogram(
                {k: rng.choice([0, 1, 3, 17, 2 ** 31, 2 ** 32 + 5, -4])
                 for k in ks}, rng.randint(0, 9), rng.randint(0, 9)))
        schema = H.union_schema(hs)
        dense = H.densify([hs], schema)
        assert dense.shape == (5, len(schema[0]) + 2)
        for i, h in enumerate(hs):
            sparse = HM.Hist.of([(k.lower, k.upper, v)
                                 for k, v in h.buckets.items()])
            padded = HM.Hist.of([(lo, up, int(dense[i, j])) for j, (lo, up)
                                 in enumerate(zip(*schema))])
            assert len(padded.buckets) == len(schema[0])
            assert dense[i, -2] == h.underflow and dense[i, -1] == h.overflow
            for p in pcts:
                assert padded.percentile(p) == sparse.percentile(p)
