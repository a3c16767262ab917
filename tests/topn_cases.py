"""The batches of the top-N tests: tests/test_gpu_topn.py runs every one on
the GPU against tests/topn_model.py, tests/test_topn_model_cpu.py shows that
they tell the model from each of its mutations.

A case: name, results (a list of sub-query results, each a list of series,
each a list of (ts, value, is_int) points), start, end, grid (the interval
every timestamp is a multiple of when all points are doubles — what a caller
may promise — else 0), topns (the N values to run; None = (1, n))."""
import os
import re

import numpy as np

T0 = 1_600_000_020_000   # a multiple of IV
IV = 60_000
NAN = float("nan")

_SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    "opentsdb_amd", "csrc", "topn.hip")


def round_size():
    """kTopnRound of topn.hip: the series one round of k_topn_current's
    workgroup takes; positions carry a base from round to round."""
    with open(_SRC) as f:
        m = re.search(r"constexpr\s+int\s+kTopnRound\s*=\s*(\d+)\s*;", f.read())
    return int(m.group(1))


def tile_size():
    """kTopnTile of topn.hip: the series of one position tile of the grid
    path (one row of its count table; in-tile ranks are counted beyond)."""
    with open(_SRC) as f:
        m = re.search(r"constexpr\s+int\s+kTopnTile\s*=\s*(\d+)\s*;", f.read())
    return int(m.group(1))


class Case:
    def __init__(self, name, results, start, end, grid=0, topns=None,
                 small=True):
        self.name, self.results = name, results
        self.start, self.end, self.grid = start, end, grid
        self.small = small
        n = sum(len(r) for r in results)
        self.topns = tuple(topns) if topns else tuple(sorted({1, max(n, 1)}))

    def __repr__(self):
        return self.name


def dpt(b, v):
    return (T0 + b * IV, float(v), False)


def lpt(b, v):
    return (T0 + b * IV, int(v), True)


def ragged(rng, S, NB, p_gap=0.2, kind="double", late=0.4):
    """S series on a grid of NB buckets: random first / last bucket, random
    inner gaps.  kind: double | long | mixed."""
    out = []
    for s in range(S):
        a, b = 0, NB - 1
        if NB > 1 and rng.rand() < late:
            a = int(rng.randint(0, NB))
        if NB > 1 and rng.rand() < late:
            b = int(rng.randint(a, NB))
        pts = []
        for k in range(a, b + 1):
            if a < k < b and rng.rand() < p_gap:
                continue
            if kind == "double" or (kind == "mixed" and rng.rand() < 0.5):
                pts.append(dpt(k, np.round(rng.uniform(-50, 100), 3)))
            else:
                pts.append(lpt(k, int(rng.randint(-50, 100))))
        out.append(pts)
    return out


def window(NB):
    return T0, T0 + (NB - 1) * IV


def build_cases():
    T = round_size()
    rng = np.random.RandomState(20240611)
    cases = []

    def add(name, results, start, end, grid=IV, **kw):
        cases.append(Case(name, results, start, end, grid, **kw))

    # ---- batch shapes: bucket counts over a few series, series counts over
    # a few buckets (the model is O(series x buckets) in plain Python)
    for NB in (1, 2, 63, 64, 65, 130):
        s, e = window(NB)
        add("shape_s3_nb%d" % NB, [ragged(rng, 3, NB)], s, e)
    for S in (1, 2, T - 1, T, T + 1, 2 * T + 1):
        s, e = window(3)
        add("shape_s%d_nb3" % S, [ragged(rng, S, 3)], s, e,
            topns=(1, 10, S), small=S <= 64)
    s, e = window(65)
    add("shape_s65_nb65", [ragged(rng, 65, 65)], s, e)
    # the grid path's position tile: T - 1, T, T + 1, 2T + 1 series
    TT = tile_size()
    for S in (TT - 1, TT, TT + 1, 2 * TT + 1):
        for NB in (2, 5, 65):
            if (S, NB) == (65, 65):
                continue
            s, e = window(NB)
            add("tile_s%d_nb%d" % (S, NB), [ragged(rng, S, NB, p_gap=0.3)], s, e,
                topns=(1, 10, S), small=NB <= 5)
    S = 2 * TT + 1
    for tag, who in (("first", [0]), ("last", [S - 1]), ("edge_lo", [TT - 1]),
                     ("edge_hi", [TT]), ("tile", list(range(TT, 2 * TT)))):
        for mode in ("late", "early"):
            vals = np.round(rng.uniform(1, 100, (S, 4)), 3)
            ser = []
            for i in range(S):
                ks = (0, 1, 3)                      # an inner gap: LERP at 2
                if i % 3 == 0:
                    ks = (0, 1, 2, 3)
                if i in set(who):
                    ks = (1, 2, 3) if mode == "late" else (0, 1, 2)
                ser.append([dpt(k, vals[i, k]) for k in ks])
            add("tile_ragged_%s_%s" % (tag, mode), [ser], *window(4),
                topns=(1, 7, S), small=False)
    # ---- ragged placement: late starts / early ends at the first and last
    # slot, either side of a round edge, a whole round
    S = 2 * T + 1
    for tag, who in (("first", [0]), ("last", [S - 1]), ("edge_lo", [T - 1]),
                     ("edge_hi", [T]), ("round", list(range(T, 2 * T)))):
        for mode in ("late", "early"):
            vals = np.round(rng.uniform(1, 100, (S, 3)), 3)
            ser = []
            for i in range(S):
                ks = (0, 1, 2)
                if i in set(who):
                    ks = (1, 2) if mode == "late" else (0, 1)
                ser.append([dpt(k, vals[i, k]) for k in ks])
            s, e = window(3)
            add("ragged_%s_%s" % (tag, mode), [ser], s, e, topns=(1, 7, S),
                small=False)
    # the same idea small enough for the mutation tests
    ser = [[dpt(1, 5), dpt(2, 6)], [dpt(0, 9), dpt(1, 1), dpt(2, 2)],
           [dpt(0, 3), dpt(1, 7)], [dpt(0, 4), dpt(1, 4), dpt(2, 8)]]
    add("ragged_small", [ser], *window(3), topns=(1, 2, 4))
    # ---- LERP and window
    ser = [
        [dpt(0, 1), dpt(2, 30), dpt(6, 2), dpt(7, 3)],            # gaps 1, 3
        [dpt(k, 10 + k) for k in range(8)],
        [dpt(3, 50)],                                             # one point
        [],                                                       # empty
        [dpt(1, -5), dpt(5, 40)],
        [dpt(k, 20 - k) for k in range(2, 7)],
    ]
    add("lerp_gaps", [ser], *window(8), topns=(1, 3, 5, 6, 106))
    # points before start and after end; the latter are LERP ends
    ser = [
        [dpt(k, k) for k in range(0, 11)],
        [dpt(0, 99), dpt(1, 98), dpt(5, 3), dpt(9, 80)],          # LERP past end
        [dpt(4, 7), dpt(6, 8), dpt(10, 500)],
        [dpt(0, 1000), dpt(1, 1000)],                             # all before
        [dpt(9, 1000), dpt(10, 1000)],                            # all after
        [dpt(2, 5), dpt(7, 6)],
    ]
    add("window_in_out", [ser], T0 + 2 * IV, T0 + 7 * IV, topns=(1, 3, 6))
    add("window_bounds_off_grid", [ser], T0 + 2 * IV + 1, T0 + 7 * IV - 1,
        topns=(1, 3, 6))
    add("window_one_bucket", [ser], T0 + 3 * IV - 5, T0 + 3 * IV + 5,
        topns=(1, 6))
    # a series whose last point before `end` is followed by one past it,
    # while others still emit: the point past `end` is a LERP end
    ser = [[dpt(0, 1), dpt(2, 2), dpt(6, 90)],
           [dpt(0, 5), dpt(3, 6), dpt(4, 7)],
           [dpt(1, 3), dpt(4, 4)]]
    add("lerp_past_end", [ser], T0, T0 + 4 * IV, topns=(1, 2, 3))
    # ---- special values
    ser = [[dpt(0, NAN), dpt(1, 5)], [dpt(0, 3), dpt(1, 9)],
           [dpt(0, 1), dpt(1, NAN)], [dpt(0, 7), dpt(1, 7)]]
    add("nan_values", [ser], *window(2), topns=(1, 2, 4))
    ser = [[dpt(0, -0.0)], [dpt(0, 0.0)], [dpt(0, -0.0)], [dpt(0, 0.0)],
           [dpt(0, -1.0)]]
    add("signed_zero", [ser], *window(1), topns=(1, 2, 5))
    ser = [[dpt(0, -5), dpt(1, -1)], [dpt(0, -2), dpt(1, -3)],
           [dpt(0, -9), dpt(1, -8)]]
    add("all_negative", [ser], *window(2), topns=(1, 2, 3))
    ser = [[dpt(0, -5), dpt(1, -1)], [dpt(0, 2), dpt(1, 3)],
           [dpt(0, -9), dpt(1, -8)], [dpt(0, 1), dpt(1, 3)]]
    add("some_negative", [ser], *window(2), topns=(1, 2, 4))
    ser = [[dpt(0, 4), dpt(1, 6)], [dpt(0, 6), dpt(1, 4)], [dpt(0, 6), dpt(1, 6)],
           [dpt(0, 1), dpt(1, 2)], [dpt(0, 6), dpt(1, 5)]]
    add("exact_ties", [ser], *window(2), topns=(1, 2, 4, 5))
    # ---- topn: 1, n - 1, n, n + 100
    s, e = window(6)
    add("topn_values", [ragged(rng, 9, 6)], s, e, topns=(1, 8, 9, 109))
    # ---- sub-queries: one above; three (an empty series, an empty result)
    r = ragged(rng, 7, 5)
    add("three_subqueries", [r[:2] + [[]], [], r[2:4], [[]] + r[4:]], *window(5),
        topns=(1, 4, 9, 50))
    # ---- the general path's own: longs, mixed, off-grid, two grids
    ser = [[lpt(0, -7), lpt(1, -3), lpt(2, -4)], [lpt(0, -2), lpt(1, -9)],
           [lpt(1, -6), lpt(2, -8)], [lpt(0, -5), lpt(2, -1)]]
    add("long_negative_pad", [ser], *window(3), grid=0, topns=(1, 2, 4))
    s, e = window(9)
    add("long_ragged", [ragged(rng, 12, 9, kind="long")], s, e, grid=0,
        topns=(1, 5, 12))
    big = 2 ** 62
    ser = [[lpt(0, big), lpt(4, -big)], [lpt(0, 1), lpt(1, 2), lpt(2, 3),
                                         lpt(3, 4), lpt(4, 5)],
           [lpt(0, -big + 1), lpt(3, big - 1)]]
    add("long_lerp_wraps", [ser], *window(5), grid=0, topns=(1, 3))
    add("mixed_ragged", [ragged(rng, 10, 9, kind="mixed")], s, e, grid=0,
        topns=(1, 4, 10))
    add("mixed_three_subqueries",
        [ragged(rng, 3, 6, kind="long"), ragged(rng, 3, 6),
         ragged(rng, 2, 6, kind="mixed")], *window(6), grid=0, topns=(1, 8))
    # a late double after long-only emissions: both kinds of emission seen
    ser = [[lpt(0, 5), lpt(1, 6), lpt(2, 7)], [lpt(0, 9), lpt(1, 1)],
           [dpt(2, 6.5), dpt(3, 2.5)]]
    add("long_then_double", [ser], *window(4), grid=0, topns=(1, 2, 3))
    ser = [[dpt(0, 1), (T0 + IV + 1, 8.0, False), dpt(3, 2)],
           [dpt(0, 5), dpt(1, 6), dpt(2, 1)], [dpt(1, 3), dpt(3, 4)]]
    add("off_grid", [ser], *window(4), grid=0, topns=(1, 3))
    g2 = IV * 3 // 2
    ser = [[dpt(k, 3 * k) for k in range(7)],
           [(T0 + k * g2, float(10 - k), False) for k in range(5)],
           [(T0 + k * g2, float(k * k), False) for k in range(1, 4)]]
    add("two_grids", [ser[:1], ser[1:]], T0, T0 + 6 * IV, grid=0, topns=(1, 3))
    return cases


CASES = build_cases()
BY_NAME = {c.name: c for c in CASES}
