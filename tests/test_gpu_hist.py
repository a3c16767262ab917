"""Histogram queries on the GPU (otsdb_hist_*) against the plain-Python model
of the reference's iterators (tests/hist_model.py).  Everything is bit-exact:
timestamps, offsets, merged counts, percentile bits."""
import ctypes as C

import numpy as np
import pytest

from opentsdb_amd import abi, core, dist
from opentsdb_amd import histogram as H
from opentsdb_amd.batch import HostBatch
from tests import hist_model as HM

pytestmark = pytest.mark.gpu

T0 = 1_600_000_020_000  # a multiple of 1 s and 1 min
IV = 1000
PCTS = [50.0, 99.0]


@pytest.fixture(scope="module")
def eng():
    from opentsdb_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def spec_of(ds, start, end):
    return core.make_spec(start, end, core.Aggregators.get("sum"),
                          core.DownsamplingSpecification(ds), start, end)


def schema(K):
    lo = np.arange(K, dtype=np.float32) * np.float32(1.5)
    return lo, lo + np.float32(1.5)


class Case:
    """series: per series (ts int64 [n], counts int64 [n][K + 2]); groups:
    lists of series indices."""

    def __init__(self, series, groups, lower, upper):
        self.series, self.groups = series, groups
        self.lower = np.asarray(lower, np.float32)
        self.upper = np.asarray(upper, np.float32)
        self.K = len(self.lower)
        R = self.K + 2
        offs = np.zeros(len(series) + 1, np.int64)
        for i, (t, c) in enumerate(series):
            assert c.shape == (len(t), R)
            offs[i + 1] = offs[i] + len(t)
        self.offsets = offs
        self.ts = (np.concatenate([t for t, _ in series]) if series
                   else np.zeros(0)).astype(np.int64)
        self.counts = (np.concatenate([c for _, c in series]) if series
                       else np.zeros((0, R))).astype(np.int64).reshape(-1, R)
        self.goff = np.zeros(len(groups) + 1, np.int64)
        for g, m in enumerate(groups):
            self.goff[g + 1] = self.goff[g] + len(m)
        self.members = np.array([s for m in groups for s in m], np.int64)

    def host(self):
        hb = HostBatch(self.offsets, self.ts, np.zeros(0, np.int64), None,
                       None, self.goff, self.members)
        return hb, H.HistColumns(self.lower, self.upper, self.counts)

    def model(self, spec, ds):
        keys = [HM.make_key(a, b) for a, b in zip(self.lower, self.upper)]
        K = self.K
        pts = [[(int(t), HM.Hist(dict(zip(keys, row[:K].tolist())),
                                 int(row[K]), int(row[K + 1])))
                for t, row in zip(ts, cnt)] for ts, cnt in self.series]
        d = core.DownsamplingSpecification(ds)
        res = HM.group_query(spec.start_ms, spec.end_ms, d.getInterval(),
                             d.histogram_aggregation, pts, self.groups)
        return res, keys

    def device(self, lo=None, hi=None):
        """The batch (or the shard of series [lo, hi)) in HBM."""
        import torch
        from opentsdb_amd.engine import DeviceBatch, DeviceHist
        S = len(self.series)
        lo, hi = (0, S) if lo is None else (lo, hi)
        p0, p1 = int(self.offsets[lo]), int(self.offsets[hi])
        R = self.K + 2

        def dev(a, shape):
            t = torch.zeros(shape, dtype=torch.int64, device="cuda")
            if a.size:
                t[:len(a)] = torch.from_numpy(np.ascontiguousarray(a)).cuda()
            return t
        n = p1 - p0
        ts = dev(self.ts[p0:p1], (max(n, 2),))[:n]
        cnt = dev(self.counts[p0:p1], (max(n, 2), R))[:n]
        goff, mem = [0], []
        for m in self.groups:
            mem += [s - lo for s in m if lo <= s < hi]
            goff.append(len(mem))
        mem_t = dev(np.array(mem, np.int64), (max(len(mem), 2),))[:len(mem)]
        db = DeviceBatch(dev(self.offsets[lo:hi + 1] - p0, (hi - lo + 1,)), ts,
                         None, dev(np.array(goff, np.int64), (len(goff),)),
                         mem_t)
        return db, DeviceHist(self.lower, self.upper, cnt)


def expected(case, spec, ds, pcts):
    """Per group: ts [n], counts [n][K + 2], pct bits [P][n]."""
    res, keys = case.model(spec, ds)
    wide = [float(np.float32(p)) for p in pcts]
    out = []
    for g in res:
        ts = np.array([t for t, _ in g], np.int64)
        cnt = np.array([[h.buckets[k] for k in keys] + [h.underflow, h.overflow]
                        for _, h in g], np.int64).reshape(len(g), case.K + 2)
        pct = np.array([[h.percentile(p) for _, h in g] for p in wide],
                       np.float64).reshape(len(wide), len(g))
        out.append((ts, cnt, pct))
    return out


def assert_same(got, exp):
    assert len(got) == len(exp)
    for g, (r, (ts, cnt, pct)) in enumerate(zip(got, exp)):
        assert np.array_equal(r.ts, ts), g
        if r.counts is not None:
            assert np.array_equal(r.counts, cnt), g
        assert np.array_equal(np.asarray(r.pct).view(np.int64),
                              pct.view(np.int64)), (g, r.pct, pct)


def run_device(eng, spec, case, pcts, want_counts=True, dev=None):
    import torch
    from opentsdb_amd.engine import (DeviceHistResult, HistPoints,
                                     run_hist_device)
    db, dh = dev or case.device()
    sz = eng.plan_hist(spec, *case.host())
    G = len(case.groups)
    res = DeviceHistResult(torch, G, int(sz.max_out_points), case.K, len(pcts),
                           want_counts, "cuda")
    run_hist_device(eng, spec, db, dh, pcts, res)
    return slices(res, G, len(pcts)), res


def slices(res, G, n_pct):
    from opentsdb_amd.engine import HistPoints
    offs = res.offsets.cpu().numpy()
    ts = res.ts.cpu().numpy()
    pct = res.pct.cpu().numpy()
    cnt = None if res.counts is None else res.counts.cpu().numpy()
    return [HistPoints(ts[offs[g]:offs[g + 1]],
                       pct[:n_pct, offs[g]:offs[g + 1]],
                       None if cnt is None else cnt[offs[g]:offs[g + 1]])
            for g in range(G)]


def check(eng, case, ds, start, end, pcts=PCTS, device=True):
    spec = spec_of(ds, start, end)
    exp = expected(case, spec, ds, pcts)
    hb, hc = case.host()
    got = eng.run_hist(spec, hb, hc, pcts, want_counts=True)
    assert_same(got, exp)
    if device:
        assert_same(run_device(eng, spec, case, pcts)[0], exp)
    return exp


def rand_series(rng, K, buckets, per_bucket=(1, 3), hi=50, t0=T0, iv=IV):
    """Points in the given buckets (indices from t0), sorted by time."""
    ts = []
    for b in buckets:
        n = int(rng.integers(per_bucket[0], per_bucket[1] + 1))
        ts += sorted(int(t0 + b * iv + x)
                     for x in rng.choice(iv, size=n, replace=False))
    cnt = rng.integers(0, hi, size=(len(ts), K + 2)).astype(np.int64)
    cnt[rng.random(cnt.shape) < 0.3] = 0
    return np.array(ts, np.int64), cnt


# ---------------------------------------------------------------- the KATs
QUERY_KATS = [c for c in HM.load_kats() if c["kind"] == "query"]


@pytest.mark.parametrize("c", QUERY_KATS, ids=lambda c: c["name"])
def test_query_kat(eng, c):
    series = [(np.array([t for t, _ in s], np.int64),
               np.array([[v, 0, 0] for _, v in s], np.int64).reshape(-1, 3))
              for s in c["series"]]
    case = Case(series, [list(range(len(series)))], [0.0], [1.0])
    spec = spec_of(c["ds"], c["start_ms"], c["end_ms"])
    hb, hc = case.host()
    for got in (eng.run_hist(spec, hb, hc, [50.0], want_counts=True),
                run_device(eng, spec, case, [50.0])[0]):
        assert [[int(t), int(v[0])] for t, v in
                zip(got[0].ts, got[0].counts)] == c["expect"]
    check(eng, case, c["ds"], c["start_ms"], c["end_ms"])


@pytest.mark.parametrize("c", [c for c in HM.load_kats()
                               if c["kind"] != "query"],
                         ids=lambda c: c["name"])
def test_simple_histogram_kat(eng, c):
    """The percentile and merge KATs as one bucket of a query: the case's
    histograms are the points of as many series at one timestamp."""
    hs = [c["hist"]] if c["kind"] == "percentile" else c["hists"]
    hh = [H.Histogram({(lo, up): n for lo, up, n in h["buckets"]},
                      h["underflow"], h["overflow"]) for h in hs]
    sch = H.union_schema(hh)
    dense = H.densify([hh], sch)
    series = [(np.array([T0 + 5], np.int64), dense[i:i + 1])
              for i in range(len(hh))]
    case = Case(series, [list(range(len(hh)))], *sch)
    pcts = c.get("percentiles", [50.0])
    check(eng, case, "1s-sum", T0, T0 + 999, pcts)
    hb, hc = case.host()
    got = eng.run_hist(spec_of("1s-sum", T0, T0 + 999), hb, hc, pcts,
                       want_counts=True)[0]
    assert list(got.ts) == [T0]
    if c["kind"] == "percentile":
        for q, e in enumerate(c["expect"]):
            assert abs(got.pct[q, 0] - e) <= c["tol"]
    else:
        col = {(float(a), float(b)): j for j, (a, b) in enumerate(zip(*sch))}
        for lo, up, n in c["expect"]:
            assert got.counts[0, col[(lo, up)]] == n
        if c["underflow"] is not None:
            assert got.counts[0, -2] == c["underflow"]
        if c["overflow"] is not None:
            assert got.counts[0, -1] == c["overflow"]


# -------------------------------------------------------- lane-mapping edges
@pytest.mark.parametrize("R", [3, 4, 63, 64, 65, 102, 127, 128, 129, 255, 256])
def test_bin_widths(eng, R):
    rng = np.random.default_rng(R)
    K = R - 2
    series = [rand_series(rng, K, [0, 1, 3], (1, 6)) for _ in range(3)]
    series.append(rand_series(rng, K, [2, 3], (1, 2)))
    case = Case(series, [[0, 1, 2], [3], [1, 3]], *schema(K))
    check(eng, case, "1s-sum", T0, T0 + 3999)


@pytest.mark.parametrize("R", [102, 256])
def test_even_row_on_an_8_byte_aligned_matrix(eng, R):
    """An even row length whose matrix starts 8 bytes off a 16-byte boundary
    takes the 8-byte loads (the header promises 8-byte alignment only)."""
    import torch
    from opentsdb_amd.engine import DeviceHist
    rng = np.random.default_rng(R + 1)
    K = R - 2
    series = [rand_series(rng, K, [0, 1, 3], (1, 6)) for _ in range(3)]
    case = Case(series, [[0, 1, 2], [1]], *schema(K))
    spec = spec_of("1s-sum", T0, T0 + 3999)
    exp = expected(case, spec, "1s-sum", PCTS)
    db, dh = case.device()
    n = dh.counts.shape[0]
    flat = torch.zeros(n * R + 2, dtype=torch.int64, device="cuda")
    base = 1 if flat.data_ptr() % 16 == 0 else 2  # 8 mod 16 either way
    off = flat[base:base + n * R].view(n, R)
    off.copy_(dh.counts)
    assert off.data_ptr() % 16 == 8
    assert_same(run_device(eng, spec, case, PCTS,
                           dev=(db, DeviceHist(case.lower, case.upper, off)))[0],
                exp)


# ------------------------------------------------ tile edges and the combine
def group_size_case(rng, K=4):
    sizes = [1, 2, 63, 64, 65, 130]
    series, groups = [], []
    for n in sizes:
        m = []
        for _ in range(n):
            m.append(len(series))
            series.append(rand_series(
                rng, K, sorted(rng.choice(6, size=2, replace=False)), (1, 2)))
        groups.append(m)
    groups.append([])  # an empty group
    R = K + 2
    special = [
        (np.zeros(0, np.int64), np.zeros((0, R), np.int64)),  # 0 points
        rand_series(rng, K, [0, 1], t0=T0 - 100 * IV),  # wholly before
        rand_series(rng, K, [0, 1], t0=T0 + 100 * IV),  # wholly after
        rand_series(rng, K, [1, 4]),
    ]
    groups.append(list(range(len(series), len(series) + 4)))
    series += special
    groups.append([len(series) - 4, len(series) - 3])  # nothing in the window
    return Case(series, groups, *schema(K))


def test_group_sizes(eng):
    case = group_size_case(np.random.default_rng(11))
    exp = check(eng, case, "1s-sum", T0, T0 + 5999)
    assert len(exp[6][0]) == 0 and len(exp[8][0]) == 0
    assert len(exp[5][0]) > 0


# --------------------------------------------------------------- grid lengths
def window_of(eng, R):
    w = eng.lib.otsdb_hist_window(R - 2)
    assert w >= 16
    return w


@pytest.mark.parametrize("R", [256, 102])
@pytest.mark.parametrize("which", ["1", "W-1", "W", "W+1", "2W+1", "300"])
def test_grid_lengths(eng, R, which):
    W = window_of(eng, R)
    nb = {"1": 1, "W-1": W - 1, "W": W, "W+1": W + 1, "2W+1": 2 * W + 1,
          "300": 300}[which]
    rng = np.random.default_rng(nb * 1000 + R)
    K = R - 2

    def pick(n):
        n = min(n, nb)
        return sorted(int(b) for b in rng.choice(nb, size=n, replace=False))
    edge = sorted({0, nb - 1, min(W - 1, nb - 1), min(W, nb - 1)})
    series = [rand_series(rng, K, edge, (1, 2)),
              rand_series(rng, K, pick(5), (1, 2)),
              rand_series(rng, K, pick(3), (1, 1))]
    series += [rand_series(rng, K, pick(2), (1, 1)) for _ in range(65)]
    case = Case(series, [[0, 1], [2], list(range(3, 68))], *schema(K))
    check(eng, case, "1s-sum", T0, T0 + nb * IV - 1, [50.0], device=False)


# --------------------------------------------------------- points per bucket
def test_points_per_bucket(eng):
    rng = np.random.default_rng(5)
    K = 4
    one = rand_series(rng, K, range(8), (1, 1))
    six = rand_series(rng, K, range(8), (6, 6))
    ts = np.concatenate([T0 + 2 * 60000 + np.sort(
        rng.choice(60000, size=5000, replace=False)), [T0 + 5 * 60000 + 7]])
    big = (ts.astype(np.int64),
           rng.integers(0, 2 ** 40, size=(5001, K + 2)).astype(np.int64))
    check(eng, Case([one, six], [[0, 1], [0], [1]], *schema(K)), "1s-sum", T0,
          T0 + 7999)
    check(eng, Case([big, one], [[0], [0, 1]], *schema(K)), "1m-sum", T0,
          T0 + 6 * 60000)


# ------------------------------------------------------- start and end edges
@pytest.mark.parametrize("end", [T0 + 5000, T0 + 4999])
def test_start_and_end_edges(eng, end):
    """start_ms off the grid: the partial first bucket is skipped; a point
    exactly at align(start + interval - 1) is the first taken; a bucket
    starting at end_ms is emitted with its points past end_ms, one starting
    at end_ms + 1 is not."""
    K = 3
    R = K + 2
    rng = np.random.default_rng(3)

    def s(ts):
        return (np.array(ts, np.int64),
                rng.integers(1, 9, size=(len(ts), R)).astype(np.int64))
    series = [s([T0 + 400, T0 + 999, T0 + 1000, T0 + 1001, T0 + 5000,
                 T0 + 5500, T0 + 5999, T0 + 6000]),
              s([T0 + 350, T0 + 4999, T0 + 5999]),
              s([T0 + 700])]  # kept by the filter, nothing after the seek
    case = Case(series, [[0, 1, 2], [2], [1]], *schema(K))
    exp = check(eng, case, "1s-sum", T0 + 300, end)
    ts0 = list(exp[0][0])
    assert ts0[0] == T0 + 1000 and T0 not in ts0
    assert (T0 + 5000 in ts0) == (end == T0 + 5000)
    assert len(exp[1][0]) == 0
    if end == T0 + 5000:  # the points past end_ms count
        assert np.array_equal(
            exp[0][1][-1], series[0][1][4:7].sum(0) + series[1][1][2])


def test_wide_grid(eng):
    """A fixed grid past 2^32 ms: 40 buckets of 2^27 ms, 3 series."""
    iv = 1 << 27
    t0 = (T0 // iv + 1) * iv
    rng = np.random.default_rng(9)
    K = 5
    series = [rand_series(rng, K, sorted(rng.choice(40, 12, replace=False)),
                          (1, 3), t0=t0, iv=iv) for _ in range(3)]
    case = Case(series, [[0, 1, 2], [1]], *schema(K))
    assert 40 * iv > 2 ** 32
    exp = check(eng, case, "%dms-sum" % iv, t0 - 5, t0 + 40 * iv - 1)
    assert exp[0][0][-1] - exp[0][0][0] > 2 ** 32


# ------------------------------------------------------------------- counts
def test_count_values(eng):
    K = 2
    big = [2 ** 31, 2 ** 32 + 5, 2 ** 63 - 1]

    def s(t, rows):
        return (np.array(t, np.int64), np.array(rows, np.int64))
    series = [
        # longs that wrap when summed (bucket 0), underflow / overflow too
        s([T0 + 1, T0 + 2], [[big[2], big[0], big[2], 1],
                             [big[2], big[1], 5, big[2]]]),
        s([T0 + 3], [[big[2], big[1], big[2], big[2]]]),
        # int sum 0 with nonzero counts (bucket 1): 2^31 + 2^31
        s([T0 + 1001], [[big[0], big[0], 0, 0]]),
        # a negative int sum (bucket 2)
        s([T0 + 2001], [[big[0], 5, 0, 0]]),
        # all-zero rows (bucket 3)
        s([T0 + 3001, T0 + 3002], [[0, 0, 0, 0], [0, 0, 0, 0]]),
        # the tie: counts 1, 1 at p = 50 picks the first bin (bucket 4)
        s([T0 + 4001], [[1, 1, 0, 0]]),
        # +1, -1: int sum 0, first area +inf (bucket 5)
        s([T0 + 5001], [[1, -1, 0, 0]]),
    ]
    groups = [[0, 1], [2], [3], [4], [5], [6], list(range(7))]
    case = Case(series, groups, [0.0, 2.0], [2.0, 6.0])
    pcts = [1.0, 50.0, 100.0]
    exp = check(eng, case, "1s-sum", T0, T0 + 5999, pcts)
    assert exp[0][1][0].tolist() == [
        HM.wrap_long(3 * big[2]), HM.wrap_long(big[0] + 2 * big[1]),
        HM.wrap_long(2 * big[2] + 5), HM.wrap_long(2 * big[2] + 1)]
    assert exp[1][2][:, 0].tolist() == [0.0, 0.0, 0.0]
    assert exp[4][2][1, 0] == 1.0  # the tie
    assert exp[3][2][:, 0].tolist() == [0.0, 0.0, 0.0]  # NaN areas
    assert exp[5][2][1, 0] == 1.0  # +inf >= p


# -------------------------------------------------------------- percentiles
def pct_case():
    rng = np.random.default_rng(21)
    K = 70
    series = [rand_series(rng, K, [0, 1, 2, 4], (1, 3), hi=1000)
              for _ in range(5)]
    return Case(series, [[0, 1, 2], [3, 4], [0, 4]], *schema(K))


def test_percentile_set_in_one_call(eng):
    pcts = [1.0, 50, 99, np.float32(99.9), 100.0, 0.5, 1000, float("nan")]
    exp = check(eng, pct_case(), "1s-sum", T0, T0 + 4999, pcts)
    assert (exp[0][2][5] == -1.0).all() and (exp[0][2][6] == -1.0).all()
    assert (exp[0][2][7] == 0.0).all()
    assert eng.hist_counters() == dict(fold_launches=1, percentile_passes=1)


def test_percentile_counts_and_counters(eng):
    case = pct_case()
    spec = spec_of("1s-sum", T0, T0 + 4999)
    hb, hc = case.host()
    launches = {}
    for pcts in ([], [75.0], [float(q) for q in range(10, 26)]):
        exp = expected(case, spec, "1s-sum", pcts)
        got = eng.run_hist(spec, hb, hc, pcts, want_counts=True)
        assert_same(got, exp)
        c = eng.hist_counters()
        launches[len(pcts)] = c["fold_launches"]
        assert c["percentile_passes"] == (1 if pcts else 0)
        assert_same(run_device(eng, spec, case, pcts)[0], exp)
    # one aggregation for every percentile
    assert launches[1] == launches[16] == launches[0] == 1
    # no percentile and no counts output: refused
    with pytest.raises(core.IllegalArgumentException):
        eng.run_hist(spec, hb, hc, [], want_counts=False)
    # percentiles alone (no counts output)
    got = eng.run_hist(spec, hb, hc, [75.0])
    assert got[0].counts is None
    assert_same(got, expected(case, spec, "1s-sum", [75.0]))


# ---------------------------------------------------- downsampling function
@pytest.mark.parametrize("fn", ["avg", "max"])
def test_non_sum_function_keeps_the_first_histogram(eng, fn):
    rng = np.random.default_rng(2)
    K = 6
    series = [rand_series(rng, K, [0, 1, 2], (2, 4)) for _ in range(3)]
    series[0][1][:] += 1  # (every record differs from zero)
    case = Case(series, [[0, 1, 2], [0]], *schema(K))
    a = check(eng, case, "1s-sum", T0, T0 + 2999)
    b = check(eng, case, "1s-" + fn, T0, T0 + 2999)
    assert np.array_equal(a[0][0], b[0][0])
    assert not np.array_equal(a[0][1], b[0][1])
    # the first record of series 0's first bucket alone
    assert np.array_equal(b[1][1][0], series[0][1][0])


# ------------------------------------------------------------------ sharding
def test_sharded_partials_sum_to_the_single_run(eng):
    import torch
    from opentsdb_amd.engine import (DeviceHistResult, DeviceHist,
                                     hist_finalize_device,
                                     hist_partials_device)
    case = group_size_case(np.random.default_rng(11))
    spec = spec_of("1s-sum", T0, T0 + 5999)
    pcts = [50.0, 99.0, 99.9]
    exp = expected(case, spec, "1s-sum", pcts)
    single, sres = run_device(eng, spec, case, pcts)
    assert_same(single, exp)
    S, G, R = len(case.series), len(case.groups), case.K + 2
    nb = int(eng.plan_hist(spec, *case.host()).n_buckets)
    for shards in (2, 3, 5):
        cuts = [S * i // shards for i in range(shards + 1)]
        dense = torch.zeros((G, nb, R), dtype=torch.int64, device="cuda")
        emit = torch.zeros((G, nb), dtype=torch.uint8, device="cuda")
        for a, b in zip(cuts, cuts[1:]):
            db, dh = case.device(a, b)
            d = torch.full((G, nb, R), -1, dtype=torch.int64, device="cuda")
            e = torch.full((G, nb), 7, dtype=torch.uint8, device="cuda")
            hist_partials_device(eng, spec, db, dh, d, e)
            dense += d
            emit = torch.maximum(emit, e)
        res = DeviceHistResult(torch, G, G * nb, case.K, len(pcts), True,
                               "cuda")
        hist_finalize_device(eng, spec, DeviceHist(case.lower, case.upper),
                             G, nb, dense, emit, pcts, res)
        for name in ("offsets", "ts", "pct", "counts"):
            n = int(sres.offsets[-1].item())
            x, y = getattr(res, name), getattr(sres, name)
            if name == "pct":
                x, y = x[:, :n].contiguous().view(torch.int64), \
                    y[:, :n].contiguous().view(torch.int64)
            elif name != "offsets":
                x, y = x[:n], y[:n]
            assert torch.equal(x, y), (shards, name)
    # the distributed wrapper, the one rank being the whole world
    db, dh = case.device()
    res = dist.run_sharded_hist(eng, spec, dh, db, pcts, G, want_counts=True)
    assert_same(slices(res, G, len(pcts)), exp)


def test_same_call_twice_gives_identical_bytes(eng):
    case = group_size_case(np.random.default_rng(12))
    spec = spec_of("1s-sum", T0, T0 + 5999)
    dev = case.device()
    outs = []
    for _ in range(2):
        _, res = run_device(eng, spec, case, PCTS, dev=dev)
        n = int(res.offsets[-1].item())
        outs.append([res.offsets.cpu().numpy().tobytes(),
                     res.ts[:n].cpu().numpy().tobytes(),
                     res.pct[:, :n].cpu().numpy().tobytes(),
                     res.counts[:n].cpu().numpy().tobytes()])
    assert outs[0] == outs[1]
