"""The stream-shape cases (tests/stream_shapes.py) without a GPU: the case
list reaches every structure class of reduce_step for each kernel shape, the
classifier is held to two profiles classified by hand, the shapes the cases
are written for are the ones the sources state, and the CPU oracle gives
expected_single on every case bit for bit — the reference the GPU file
(tests/test_gpu_stream_shapes.py) holds the kernels to.
"""
import numpy as np
import pytest

from opentsdb_amd import core
from oracle import pyoracle
from tests import stream_shapes as SS

SHAPES = [(8, SS.RING_ROW), (8, SS.RING_FOLD), (8, SS.RING_RATE),
          (6, SS.RING_ROW)]


def spec_of(built, agg, ds, fill, interval="10s", rate=False, ro=None):
    s, e = SS.window(built, fill)
    d = core.DownsamplingSpecification("%s-%s-%s" % (interval, ds, fill))
    return core.make_spec(s, e, core.Aggregators.get(agg), d, s, e, rate, ro,
                          None)


@pytest.fixture(scope="module", params=[8, 6], ids=["K8", "K6"])
def built(request):
    return {f: SS.build(list(SS.case_list(request.param)), f)
            for f in SS.FORMS}


def test_shapes_are_the_kernels():
    """K, WIN and FL as ds_tu.hip, panel.hip and fold.hip state them."""
    ks = SS.kernel_shapes()
    assert ks["row"] == (SS.K_COLUMNS,) + SS.RING_ROW
    assert ks["panel"] == (SS.K_COLUMNS,) + SS.RING_ROW
    assert ks["rate"] == (SS.K_COLUMNS,) + SS.RING_RATE
    assert ks["fold"] == (SS.K_COLUMNS,) + SS.RING_FOLD
    assert ks["cells"] == (SS.K_CELLS,) + SS.RING_ROW


@pytest.mark.parametrize("K,ring", SHAPES,
                         ids=["K%d-W%d" % (k, r[0]) for k, r in SHAPES])
def test_cases_reach_every_class(K, ring):
    cases = list(SS.case_list(K))
    b = SS.build(cases, "long")
    got = SS.classify(b.batch.ts, b.spans, K, ring[0], ring[1], b.interval,
                      b.start)
    want = SS.all_classes(SS.RING_KIND[ring])
    assert not want - got, "no case reaches %s" % sorted(want - got)
    assert not got - want, "unlisted classes %s" % sorted(got - want)


def test_cases_are_short_and_placed():
    for K in (8, 6):
        b = SS.build(list(SS.case_list(K)), "mixed")
        for c, (lo, hi) in zip(b.cases, b.spans):
            assert lo % 2 == c.odd and hi - lo == SS.n_points(c.profile)
            # (the longest: a 3-step bucket, singles, a 3-step bucket)
            assert hi - lo <= 7 * 64 * K, c.name
            assert np.all(b.batch.ts[lo:hi] >= b.start)
            assert lo == 0 or c.pre is None or np.all(
                b.batch.ts[lo - c.pre:lo] < b.start)
        lens = {hi - lo for c, (lo, hi) in zip(b.cases, b.spans)
                if c.name.startswith("len")}
        assert lens == {1, K - 1, K, K + 1, 64 * K - 1, 64 * K, 64 * K + 1}
    # the helper's two means: a filler in front, or points before the window
    assert SS.with_parity(4, 1) == (False, 1)
    assert SS.with_parity(4, 1, pre=2) == (True, 2)
    assert SS.with_parity(5, 1, pre=2) == (False, 2)


def _one(profile, odd, K=8, ring=SS.RING_ROW):
    b = SS.build([SS.Case("hand", profile, odd, pre=3 if odd else 0)], "long")
    return SS.classify(b.batch.ts, b.spans, K, ring[0], ring[1], b.interval,
                       b.start)


def test_classifier_on_two_profiles_by_hand():
    # 12 points from an even index: lane 0 holds buckets 0 0 0 1 2 2 2 2 (a
    # bucket wholly inside it, head and tail both close), lane 1 four points
    # of bucket 5, lanes 2 .. 63 nothing; one step, a tail step
    assert _one([(0, 3), (1, 1), (2, 4), (5, 4)], 0) == {
        "lane:3+mid", "lane:1", "step:has3", "tail:nv0", "tail:partial",
        "first+last", "L:16-63", "step:both"}
    # 13 points from an odd index: base = lo - 1, so lane 0 holds 7 points,
    # buckets 0 3 4 4 9 9 9, and lane 1 six, buckets 9 9 10 10 10 10: lane
    # 0's tail runs on into lane 1, whose own tail closes (with its head)
    assert _one([(0, 1), (3, 1), (4, 2), (9, 5), (10, 4)], 1) == {
        "lane:4+", "lane:2", "step:no3", "first:base<lo", "first+last",
        "L:16-63", "step:both"}


@pytest.mark.parametrize("fill", ["none", "zero"])
@pytest.mark.parametrize("form", SS.FORMS)
def test_oracle_is_the_profile(built, form, fill):
    """pyoracle.group_by over one single-series group per case equals
    expected_single for the seven functions."""
    b = built[form]
    for fn in SS.FUNCS:
        ref = pyoracle.group_by(spec_of(b, "sum", fn, fill), b.batch)
        SS.check_expected(ref, b, fn, fill, "oracle/" + form)
