"""tests/topn_model.py against what pins it: its iterator bit for bit against
the CPU oracle's raw group-by, its functions against the transcribed value
tests of TestHighestMax / TestHighestCurrent, and its mutation switches
against the batches the GPU tests run (tests/topn_cases.py)."""
import json
import os

import numpy as np
import pytest

from opentsdb_amd import core
from opentsdb_amd.batch import HostBatch
from oracle import pyoracle
from tests import topn_cases as TC
from tests import topn_model as TM

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "kat_gexp_topn.json")) as f:
    KAT = json.load(f)


# ------------------------------------------------- iterator against the oracle
def _ragged_batch(seed, kind, n_series=9, n_ts=40):
    """Seeded ragged series on irregular timestamps; every series has a point
    on both sides of... at least inside [start, end] (the oracle's raw path
    applies SpanGroup.add's filter, which the top-N iterator does not have:
    a series wholly outside the window would differ in isInteger only)."""
    rng = np.random.RandomState(seed)
    base = 1_500_000_000_000
    grid = base + np.cumsum(rng.randint(1, 2000, n_ts))
    start, end = int(grid[5]), int(grid[n_ts - 6])
    series = []
    for s in range(n_series):
        while True:
            keep = np.sort(rng.choice(n_ts, rng.randint(1, n_ts), replace=False))
            if any(start <= grid[k] <= end for k in keep):
                break
        pts = []
        for k in keep:
            isl = kind == "long" or (kind == "mixed" and rng.rand() < 0.6)
            if isl:
                v = int(rng.randint(-10 ** 6, 10 ** 6))
                if rng.rand() < 0.1:
                    v = int(rng.choice([2 ** 62, -2 ** 62, 2 ** 63 - 1]))
                pts.append((int(grid[k]), v, True))
            else:
                pts.append((int(grid[k]), float(rng.uniform(-1e3, 1e3)), False))
        series.append(pts)
    return series, start, end


def _agg(name, is_int, values):
    vs = [v for _, v in values]
    if is_int:
        acc = vs[0]
        for v in vs[1:]:
            acc = TM.jlong(acc + v) if name == "sum" else max(acc, v)
        return acc
    acc = vs[0]
    for v in vs[1:]:
        acc = acc + v if name == "sum" else max(acc, v)
    return TM.bits_of(acc)


@pytest.mark.parametrize("kind", ["long", "double", "mixed"])
@pytest.mark.parametrize("agg", ["sum", "max"])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_iterator_matches_the_oracle_raw_group_by(kind, agg, seed):
    series, start, end = _ragged_batch(seed, kind)
    spans = [[(t, v, not isl) for t, v, isl in pts] for pts in series]
    hb = HostBatch.from_groups([spans])
    spec = core.make_spec(start, end, core.Aggregators.get(agg))
    want = pyoracle.group_by(spec, hb)[0]
    got = TM.iterate(series, start, end)
    assert [x for x, _, _ in got] == want["ts"].tolist()
    assert [int(i) for _, i, _ in got] == want["is_int"].tolist()
    assert [_agg(agg, i, vals) for _, i, vals in got] == want["bits"].tolist()


# ------------------------------------------------------------ transcribed KATs
def _series(entry):
    return [(int(t), (int(v) if i else float(v)), bool(i))
            for t, v, i in entry["points"]]


@pytest.mark.parametrize("case", KAT["cases"], ids=lambda c: c["test"])
def test_transcribed_value_tests(case):
    results = [[_series(e) for e in res] for res in case["results"]]
    names = [e["name"] for res in case["results"] for e in res]
    flat = [s for res in results for s in res]
    topn = core.parse_topn([case["topn"]])
    st, picked, keys, series = TM.evaluate(
        case["function"], topn, KAT["start_ms"], KAT["end_ms"], results)
    assert st == TM.OK
    assert [names[i] for i in picked] == case["expect"], case["test"]
    assert series == [flat[i] for i in picked]   # whole, untouched lists


@pytest.mark.parametrize("case", KAT["errors"], ids=lambda c: c["test"])
def test_transcribed_argument_tests(case):
    if case["expect"] == "IllegalArgumentException":
        with pytest.raises(core.IllegalArgumentException):
            core.parse_topn(case["params"])
        return
    topn = core.parse_topn(case["params"])
    st, picked, _, _ = TM.evaluate(case["function"], topn, KAT["start_ms"],
                                   KAT["end_ms"], case["results"])
    assert (st, picked) == (TM.OK, case["expect"])


# ---------------------------------------------------------- mutation switches
def _answers(mut):
    out = {}
    for c in TC.CASES:
        if not c.small:
            continue
        for fn in (TM.HIGHEST_MAX, TM.HIGHEST_CURRENT):
            for n in c.topns:
                out[(c.name, fn, n)] = TM.evaluate(fn, n, c.start, c.end,
                                                   c.results, mut)[:3]
    return out


@pytest.fixture(scope="module")
def reference_answers():
    return _answers(None)


@pytest.mark.parametrize("mut", TM.MUTATIONS)
def test_the_gpu_batches_tell_the_model_from_each_mutation(mut,
                                                           reference_answers):
    got = _answers(mut)
    differ = [k for k in got if got[k] != reference_answers[k]]
    assert differ, "no batch of tests/topn_cases.py notices " + mut


def test_case_names_are_unique_and_cover_the_issue_shapes():
    assert len(TC.BY_NAME) == len(TC.CASES)
    T = TC.round_size()
    sizes = {sum(len(r) for r in c.results) for c in TC.CASES}
    assert {1, 2, T - 1, T, T + 1, 2 * T + 1} <= sizes
    T = TC.tile_size()
    assert {T - 1, T, T + 1, 2 * T + 1} <= sizes
    # a grid promise is only ever attached to all-double, on-grid batches
    for c in TC.CASES:
        if c.grid:
            assert all(not p[2] and p[0] % c.grid == 0
                       for r in c.results for s in r for p in s), c.name
