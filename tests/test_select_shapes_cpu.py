"""Key-shape edges of the selections without a GPU (tests/select_shapes.py):

a. a plain model of the answer in Python floats (a sort by Double.compareTo
   for median, by value for the percentiles; the LEGACY estimator for
   runDouble, commons-math's R_3 / R_7 positions on the raw long path) and
   the CPU oracle pinned to it bit for bit on every batch
   tests/test_gpu_select_shapes.py runs;
b. a numpy restatement of k_seg_select's plan (min / max, shift, the offset
   digit with its s1 correction, the digit passes with two / shared
   histograms, the exits by shift == 0 and by gather, for_keys' head, tail
   and unrolled body), parameterised by the constants, that returns the
   branch trace of a key column: every case is asserted to reach the branch
   it is there for, and the union of the cases to reach every branch the
   suite did not hold exactly before.  No counter is added to the kernels;
   this model carries the coverage argument;
c. the restatement run to completion equals the plain model on every case,
   and with the mistakes these branches invite switched on, one at a time,
   it does not: the cases tell a wrong kernel from a right one;
d. the same for wave_select (8 passes of 8 bits, four bins a lane) on the
   bucket populations of k_ds_select / k_raw_select, and for the cross-rank
   protocol through tests/test_sel_protocol_cpu.py's select().
"""
import math
import re
import struct

import numpy as np
import pytest

from opentsdb_amd import dist as odist
from oracle import pyoracle
from tests import select_shapes as SS
from tests.test_sel_protocol_cpu import select as xsel_select
from tests.value_domain import PERCENTILES

K = SS.K
BROKEN = "broken"  # a mutant read a value the kernel never wrote


# ------------------------------------------------------- a. the plain model
def fbits(x):
    return struct.unpack("<q", struct.pack("<d", x))[0]


def pct_of(name):
    """(percent, estimation type) of a percentile's registry name."""
    m = re.match(r"^(e?)p(\d+)(?:r(\d))?$", name)
    assert m, name
    p = 99.9 if m.group(2) == "999" else float(m.group(2))
    return p, int(m.group(3)) if m.group(1) else 0


def java_order(x):
    """Double.compareTo on non-NaN doubles: by value, -0.0 before 0.0."""
    return (x, math.copysign(1.0, x))


def estimate(a, percent, est=0):
    """commons-math3 Percentile.evaluate over the sorted doubles a."""
    n = len(a)
    if n == 1:
        return a[0]
    p = percent / 100.0
    if est == 3:
        pos = 0.0 if p <= 0.5 / float(n) else float(round(float(n) * p))
    elif est == 7:
        pos = 0.0 if p == 0.0 else (float(n) if p == 1.0 else
                                    1 + float(n - 1) * p)
    else:
        pos = 0.0 if p == 0.0 else (float(n) if p == 1.0 else
                                    p * float(n + 1))
    fpos = math.floor(pos)
    if pos < 1:
        return a[0]
    if pos >= n:
        return a[n - 1]
    lower, upper = a[int(fpos) - 1], a[int(fpos)]
    return lower + (pos - fpos) * (upper - lower)


def select_double(agg, vals):
    """Median / PercentileAgg.runDouble: NaNs dropped; LEGACY whatever the
    name says."""
    v = [x for x in vals if not math.isnan(x)]
    if not v:
        return math.nan
    if agg == "median":
        return sorted(v, key=java_order)[len(v) // 2]
    return estimate(sorted(v), pct_of(agg)[0], 0)


def d2l(r):
    """Java's (long) of a double."""
    if math.isnan(r):
        return 0
    if r >= 2.0**63:
        return 2**63 - 1
    if r <= -2.0**63:
        return -2**63
    return int(r)


def select_long(agg, vals):
    """Median / PercentileAgg.runLong over Python ints."""
    if agg == "median":
        return sorted(vals)[len(vals) // 2]
    p, est = pct_of(agg)
    return d2l(estimate(sorted(float(x) for x in vals), p, est))


def same(agg, x, y):
    """Bit for bit; a percentile (never median) that is +-0.0 on both sides
    by value, the rule of tests/test_gpu_value_domain.py::zero_sign_blind."""
    if isinstance(x, str) or isinstance(y, str):
        return x == y
    if math.isnan(x) or math.isnan(y):
        return math.isnan(x) and math.isnan(y)
    if agg in PERCENTILES and x == 0.0 and y == 0.0:
        return True
    return fbits(x) == fbits(y)


def across_model(b, agg, fill):
    """[(ts, values)] per group of a select_shapes.build batch."""
    out = []
    for g, k in enumerate(b.sizes):
        ts, vals = [], []
        for bucket in range(b.nb):
            v = b.v[bucket][g].tolist()
            if fill == "zero" and bucket == 1:
                v = [x if h else 0.0 for x, h in zip(v, b.has1[g].tolist())]
            real = [x for x in v if not math.isnan(x)]
            if k == 0 or (fill == "none" and not real):
                continue
            ts.append(b.start + bucket * b.interval)
            vals.append(select_double(agg, real))
        out.append((ts, vals))
    return out


def oracle_points(ref):
    """The oracle's groups as (ts, values): doubles as floats, longs as
    ints."""
    out = []
    for r in ref:
        vals = [int(x) if i else struct.unpack("<d", struct.pack("<q", int(x)))[0]
                for x, i in zip(r["bits"].tolist(), r["is_int"].tolist())]
        out.append((r["ts"].tolist(), vals))
    return out


def pin(model, ref, agg, where):
    got = oracle_points(ref)
    assert len(got) == len(model), where
    for g, ((tm, vm), (to, vo)) in enumerate(zip(model, got)):
        assert tm == to, "%s/g%d: emission %s vs oracle %s" % (
            where, g, tm[:6], to[:6])
        for t, x, y in zip(tm, vm, vo):
            assert type(x) is type(y), "%s/g%d @%d: type" % (where, g, t)
            ok = x == y if isinstance(x, int) else same(agg, x, y)
            assert ok, "%s/g%d @%d: model %r vs oracle %r" % (where, g, t, x, y)


ACROSS = SS.across_cases()


@pytest.fixture(scope="module")
def layouts():
    return {w: SS.layout(name, n, how) for w, name, n, how in ACROSS}


@pytest.mark.parametrize("name", list(SS.POPULATIONS))
def test_oracle_is_the_model_across_series(layouts, name):
    for w, pop, n, how in ACROSS:
        if pop != name:
            continue
        b = layouts[w]
        for fill in SS.SEL_FILLS:
            for agg in SS.SEL_AGGS:
                ref = pyoracle.group_by(SS.spec_of(b, agg, fill), b.batch)
                pin(across_model(b, agg, fill), ref, agg,
                    "%s/%s-%s" % (w, agg, fill))
    # the downsampler `first` leaves the same bucket values
    b = layouts["%s/%d/after" % (name, SS.big_sizes()[0])]
    ref = pyoracle.group_by(SS.spec_of(b, "p50", "none", ds="first"), b.batch)
    pin(across_model(b, "p50", "none"), ref, "p50", name + "/first")


def test_oracle_is_the_model_fill_layouts():
    for w, n, how in SS.fill_cases():
        b = SS.fill_layout(n, how)
        for fill in SS.FILL_FILLS:
            for agg in SS.SEL_AGGS:
                ref = pyoracle.group_by(SS.spec_of(b, agg, fill), b.batch)
                pin(across_model(b, agg, fill), ref, agg,
                    "%s/%s-%s" % (w, agg, fill))


def test_oracle_is_the_model_chunk_case():
    b = SS.chunk_batch()
    for agg in ("median", "p50"):
        ref = pyoracle.group_by(SS.spec_of(b, agg, "none"), b.batch)
        pin(across_model(b, agg, "none"), ref, agg, "chunk/" + agg)


def ds_model(b, agg, fn, fill, interval):
    """The downsampling selections: per series and bucket fn over the
    bucket's points as doubles, then `agg` (max / mimmax / mimmin: the
    largest or smallest of the members' own non-NaN bucket values; no value
    is interpolated into the result) across each group."""
    hb = b.batch
    nb = 1 if interval == "0all" else b.nb
    streams = []
    for s in range(hb.n_series):
        a, e = int(hb.offsets[s]), int(hb.offsets[s + 1])
        isf = hb.is_float[a:e]
        v = np.where(isf == 1, hb.val[a:e].view(np.float64),
                     hb.val[a:e].astype(np.float64))
        bk = np.zeros(e - a, np.int64) if nb == 1 else \
            (hb.ts[a:e] - b.start) // b.interval
        st = {}
        for k in np.unique(bk).tolist():
            st[k] = select_double(fn, v[bk == k].tolist())
        streams.append(st)
    out = []
    for g in range(hb.n_groups):
        mem = hb.group_members[hb.group_offsets[g]:hb.group_offsets[g + 1]]
        ts, vals = [], []
        for k in range(nb):
            own = [streams[s][k] for s in mem.tolist() if k in streams[s]]
            real = [x for x in own if not math.isnan(x)]
            # (a bucket whose points are all NaN is a point of its series,
            # of value NaN: it is emitted under `none` too)
            if fill == "none" and not own:
                continue
            ts.append(b.start + k * b.interval)
            if not real:
                vals.append(math.nan)
            else:
                vals.append(min(real) if agg == "mimmin" else max(real))
        out.append((ts, vals))
    return out


DS_QUERIES = (("one", "mimmax"), ("one", "mimmin"), ("each", "max"))


@pytest.mark.parametrize("interval", ["1m", "0all"])
def test_oracle_is_the_model_downsampling(interval):
    for grouping, agg in DS_QUERIES:
        b = SS.ds_batch(grouping)
        for fill in SS.SEL_FILLS:
            for fn in SS.DS_FNS:
                ref = pyoracle.group_by(SS.ds_spec(b, agg, fn, fill, interval),
                                        b.batch)
                pin(ds_model(b, agg, fn, fill, interval), ref, fn,
                    "ds/%s/%s:%s-%s-%s" % (grouping, agg, interval, fn, fill))


def raw_model(b, agg):
    hb = b.batch
    T = b.nb
    out = []
    for g in range(hb.n_groups):
        mem = hb.group_members[hb.group_offsets[g]:hb.group_offsets[g + 1]]
        ts, vals = [], []
        for t in range(T):
            at = hb.offsets[mem] + t
            if b.form == "long":
                vals.append(select_long(agg, hb.val[at].tolist()))
            else:
                vals.append(select_double(
                    agg, hb.val[at].view(np.float64).tolist()))
            ts.append(b.start + t * b.interval)
        out.append((ts, vals))
    return out


@pytest.mark.parametrize("form", ["double", "long"])
def test_oracle_is_the_model_raw(form):
    b = SS.raw_batch(form)
    for agg in SS.SEL_AGGS:
        ref = pyoracle.group_by(SS.raw_spec(b, agg), b.batch)
        pin(raw_model(b, agg), ref, agg, "raw/%s/%s" % (form, agg))


def test_oracle_is_the_model_raw_long_estimators():
    """Every percentile of the registry over 1 .. 41 longs: R_3 rounds n p
    half to even and returns the minimum up to p <= 0.5 / n; R_7 reads
    1 + (n - 1) p."""
    b = SS.raw_long_batch()
    for agg in sorted(PERCENTILES) + ["median"]:
        ref = pyoracle.group_by(SS.raw_spec(b, agg), b.batch)
        pin(raw_model(b, agg), ref, agg, "rawlong/" + agg)
    # the sizes do reach what they are there for
    p = 0.5
    assert any((n * p) % 1 == 0.5 and round(n * p) % 2 == 0 and
               round(n * p) != math.floor(n * p + 0.5)
               for n in SS.RAW_LONG_SIZES), "rint: a half that rounds down"
    assert any(0.5 <= 0.5 / n for n in SS.RAW_LONG_SIZES)      # p50, n = 1
    assert any(0.75 > 0.5 / n for n in SS.RAW_LONG_SIZES)
    assert any(abs(0.95 * n - round(0.95 * n)) == 0.5 or
               (0.9 * n) % 1 == 0.5 for n in SS.RAW_LONG_SIZES)


# ------------------------------------------- b. k_seg_select's plan, restated
MUTANTS = ("no_rank_sub", "no_carry", "dm_full", "no_copy", "tie_eq",
           "head_skipped")
M64 = 2**64 - 1


def ranks_of(agg, n):
    """sel_state_of: the one or two order statistics, and pos."""
    if agg == "median":
        return [n // 2], 0.0
    if n == 1:
        return [0], 0.0
    pos = (pct_of(agg)[0] / 100.0) * float(n + 1)
    if pos < 1:
        return [0], pos
    if pos >= float(n):
        return [n - 1], pos
    ip = int(math.floor(pos))
    return [ip - 1, ip], pos


def scan(h, r):
    """One wave over a histogram: the bin whose cumulative count passes the
    rank -> (digit, keys below it, keys in it); None: no lane finds it and
    the kernel would read what it never wrote."""
    cum = np.cumsum(h)
    d = int(np.searchsorted(cum, r, side="right"))
    if d >= len(h):
        return None
    return d, int(cum[d - 1]) if d else 0, int(h[d])


def seg_select(col, agg, head=0, mutant=None, k=K):
    """k_seg_select over one key column (KEY_NONE: no contribution) ->
    (value, trace).  trace: the branches taken, in order."""
    tr = []
    col = np.asarray(col, np.uint64)
    kk = len(col)
    BITS, BINS, CAP, T = k.SS_BITS, k.SS_BINS, k.SS_CAP, k.SS_THREADS
    # for_keys: the head key, pairs (four a thread in flight), the odd tail
    npairs = (kk - head) >> 1
    if head and kk > 0:
        tr.append("fk:head")
    if (kk - head) & 1:
        tr.append("fk:tail")
    ent = max(0, min(T, npairs - 3 * T))
    if ent:
        tr.append("fk:unrolled:all" if ent == T else "fk:unrolled:%d" % ent)
    seen = col[1:] if (mutant == "head_skipped" and head) else col
    seen = seen[seen != SS.KEY_NONE]
    real = col[col != SS.KEY_NONE]
    n = len(real)  # (k_sel_init: from the count query, not from for_keys)
    if n == 0:
        return math.nan, tr
    ranks, pos = ranks_of(agg, n)
    nt = len(ranks)
    mn, mx = int(real.min()), int(real.max())
    shift = (mn ^ mx).bit_length()
    if mn == mx:
        tr.append("mn==mx")
    if shift == 64:
        tr.append("shift64")
    mask = [0 if shift >= 64 else (M64 << shift) & M64] * 2
    prefix = [mn & mask[0]] * 2
    rank = list(ranks) + [0] * (2 - nt)
    cnt = [n] * 2
    h = [np.zeros(BINS, np.int64), np.zeros(BINS, np.int64)]

    def many():
        return cnt[0] > CAP or (nt == 2 and cnt[1] > CAP)

    def digit_of(x, s):
        return x >> np.uint64(s) if s < 64 else np.zeros(len(x), np.uint64)
    if shift > 0 and many():
        tr.append("offset")
        s1 = max((mx - mn).bit_length() - BITS, 0)
        bumps = 0
        while s1 < 64 and (mx >> s1) - (mn >> s1) >= BINS and \
                mutant != "no_carry":
            s1 += 1
            bumps += 1
        if bumps:
            tr.append("offset:carry%d" % bumps)
        b1 = mn >> s1
        d = (digit_of(seen, s1) - np.uint64(b1)).astype(np.int64)
        h[0] = np.bincount(d[d < BINS], minlength=BINS)  # (past it: lost)
        if nt == 2:
            h[1] = h[0].copy()
        for t in range(nt):
            f = scan(h[t], rank[t])
            if f is None:
                return BROKEN, tr
            mask[t] = (M64 << s1) & M64 if s1 < 64 else 0
            prefix[t] = ((b1 + f[0]) << s1) & M64 if s1 < 64 else 0
            if mutant != "no_rank_sub":
                rank[t] -= f[1]
            cnt[t] = f[2]
        shift = s1
        if shift == 0:
            tr.append("offset:all-bits")
    while shift > 0 and many():
        w = min(shift, BITS)
        shift -= w
        dm = (1 << w) - 1
        if mutant == "dm_full":
            dm = BINS - 1
        two = nt == 2 and prefix[1] != prefix[0]
        tr.append("digit")
        tr.append("digit:two" if two else
                  ("digit:copy" if nt == 2 else "digit:one"))
        if two and (cnt[0] <= CAP or cnt[1] <= CAP):
            tr.append("digit:two:one-small")
        if w < BITS:
            tr.append("digit:short%d" % w)
        d = (digit_of(seen, shift) & np.uint64(dm)).astype(np.int64)
        for t in range(2 if two else 1):
            m = (seen & np.uint64(mask[t])) == np.uint64(prefix[t])
            h[t] = np.bincount(d[m], minlength=BINS)
        if nt == 2 and not two and mutant != "no_copy":
            h[1] = h[0].copy()
        for t in range(nt):
            f = scan(h[t], rank[t])
            if f is None:
                return BROKEN, tr
            prefix[t] |= f[0] << shift
            mask[t] |= dm << shift
            rank[t] -= f[1]
            cnt[t] = f[2]
    val = [None, None]
    if shift == 0:
        tr.append("exit:shift0")
        if many():
            tr.append("exit:shift0:ties>cap")
        val = list(prefix)
    else:
        tr.append("gather")
        if shift < BITS:
            tr.append("gather:shift<bits")
        if shift == 64:
            tr.append("gather:shift64")
        if nt == 2:
            tr.append("gather:same" if prefix[0] == prefix[1] else
                      "gather:two")
        for t in range(nt):
            cand = seen[(seen & np.uint64(mask[t])) == np.uint64(prefix[t])]
            cand = cand[:CAP]
            tr.append("gather:nc=%d" % len(cand))
            pick = None
            for x in np.unique(cand).tolist():
                less, eq = int((cand < x).sum()), int((cand == x).sum())
                hit = (less == rank[t]) if mutant == "tie_eq" else \
                    (less <= rank[t] < less + eq)
                if hit:
                    pick = x
            if pick is None:
                return BROKEN, tr
            val[t] = pick
    if nt == 1:
        val[1] = val[0]
    lo, hi = SS.key_value(val[0]), SS.key_value(val[1])
    if agg == "median" or n == 1:
        return lo, tr
    if 1 <= pos < float(n):
        return lo + (pos - math.floor(pos)) * (hi - lo), tr
    return lo, tr


def digit_passes(tr):
    return tr.count("digit")


def plan(name, n, agg, how="alone", bucket=0):
    b = SS.layout(name, n, how)
    g = len(b.sizes) - 1
    return seg_select(SS.keys_of(b, g, bucket, "none"), agg,
                      b.edges[g, bucket][0])[1]


BIG = SS.big_sizes()


@pytest.mark.parametrize("n", BIG)
def test_each_population_reaches_its_branch(n):
    assert n > K.SS_CAP
    for agg in SS.SEL_AGGS:
        tr = plan("onekey", n, agg)
        assert "mn==mx" in tr and "exit:shift0" in tr, tr
        assert "offset" not in tr and "digit" not in tr and "gather" not in tr
        tr = plan("lowbits", n, agg)
        assert "offset" in tr and "offset:all-bits" in tr and \
            "exit:shift0" in tr and "digit" not in tr and "gather" not in tr
        tr = plan("carry", n, agg)
        assert "offset:carry1" in tr, tr
        tr = plan("cluster", n, agg)
        assert "offset" in tr and digit_passes(tr) >= 2 and \
            "gather:shift<bits" in tr, tr
        tr = plan("cluster_ties", n, agg)
        assert "digit:short3" in tr and tr[-1] == "exit:shift0" and \
            "gather" not in tr, tr
        tr = plan("signed", n, agg)
        assert "offset" in tr and "digit" not in tr and "gather" in tr, tr
        tr = plan("zeros", n, agg)
        assert "shift64" in tr and "offset:all-bits" in tr and \
            "exit:shift0" in tr and "gather" not in tr, tr
    # straddle: p50's order statistics lie in two bins of more than SS_CAP
    tr = plan("straddle", n, "p50")
    assert digit_passes(tr) >= 2 and tr.count("digit:two") == \
        digit_passes(tr) and "digit:two:one-small" not in tr and \
        "gather:two" in tr, tr
    tr = plan("straddle", n, "median")
    assert digit_passes(tr) >= 2 and tr.count("digit:one") == digit_passes(tr)
    tr = plan("straddle", n, "p99")
    assert digit_passes(tr) >= 2 and tr.count("digit:copy") == \
        digit_passes(tr), tr
    tr = plan("straddle_wide", n, "p50")
    assert "digit:two:one-small" in tr, tr
    # heavytie: inside the tie down to the last bit; past it a few candidates
    for agg in ("median", "p50"):
        tr = plan("heavytie", n, agg)
        assert "exit:shift0:ties>cap" in tr and any(
            x.startswith("digit:short") for x in tr), tr
    for agg in ("p99", "p999"):
        tr = plan("heavytie", n, agg)
        nc = [int(x[10:]) for x in tr if x.startswith("gather:nc=")]
        assert nc and max(nc) < 8 and "digit" not in tr, tr


def test_small_cuts_take_the_direct_gather():
    """SEL_K + 1 members: k_seg_select with no pass at all; the two zeros
    leave shift = 64 (mask 0) for the gather."""
    n = K.SEL_K + 1
    for name in SS.POPULATIONS:
        tr = plan(name, n, "p50")
        assert "offset" not in tr and "digit" not in tr
        if name != "onekey":
            assert "gather" in tr, (name, tr)
    assert "gather:shift64" in plan("zeros", n, "p50")
    v = SS.population("zeros", n)
    assert set(SS.dkey(v).tolist()) == {2**63 - 1, 2**63}   # mx - mn = 1


def test_for_keys_ladder_and_edges():
    T = K.SS_THREADS
    lad = SS.for_keys_ladder()
    assert lad[:4] == [6 * T - 1, 6 * T, 6 * T + 1, 6 * T + 2]
    unrolled = lambda tr: [x for x in tr if x.startswith("fk:unrolled")]
    for name in SS.LADDER_POPULATIONS:
        got = [unrolled(plan(name, n, "p99")) for n in lad]
        assert got == [[], [], [], ["fk:unrolled:1"], ["fk:unrolled:all"],
                       ["fk:unrolled:%d" % (T // 2)]], got
        # behind an odd group the head key takes one key off the pairs
        got = [unrolled(plan(name, n, "p99", "after")) for n in lad[:5]]
        assert got == [[], [], [], [], ["fk:unrolled:all"]], got
    # all four (head, tail) pairs, in the large segments of the layouts
    pairs = set()
    for w, name, n, how in ACROSS:
        if n <= K.SS_CAP:
            continue
        b = SS.layout(name, n, how)
        g = len(b.sizes) - 1
        for bucket in range(2):
            e = b.edges[g, bucket]
            assert e == ((bucket * b.M + int(b.off[g])) & 1,
                         (n - e[0]) & 1)
            pairs.add(e)
    assert pairs == {(0, 0), (0, 1), (1, 0), (1, 1)}
    # bucket 1: fewer keys than members, and an odd count under an even one
    for n in BIG + lad:
        b = SS.layout("cluster", n, "alone")
        n1 = int((SS.keys_of(b, 0, 1, "none") != SS.KEY_NONE).sum())
        assert n1 < n and n1 % 2 == 1
    b = SS.layout("cluster", BIG[0], "after")
    assert b.sizes[0] == K.SEL_K + 1 and b.sizes[0] % 2 == 1 and \
        b.sizes[0] > K.SEL_K


def every_segment():
    """(where, keys, head, fill) of every large segment of every across-
    series and fill case."""
    for w, name, n, how in ACROSS:
        if n <= K.SEL_K:
            continue
        b = SS.layout(name, n, how)
        g = len(b.sizes) - 1
        for bucket in range(2):
            yield ("%s/b%d" % (w, bucket), SS.keys_of(b, g, bucket, "none"),
                   b.edges[g, bucket][0], "none")
    for w, n, how in SS.fill_cases():
        b = SS.fill_layout(n, how)
        g = len(b.sizes) - 1
        for fill in SS.FILL_FILLS:
            yield ("%s-%s/b1" % (w, fill), SS.keys_of(b, g, 1, fill),
                   b.edges[g, 1][0], fill)


@pytest.fixture(scope="module")
def truth():
    """Per segment and aggregator: the plain model's value and the true
    restatement's (value, trace)."""
    out = []
    for w, keys, head, fill in every_segment():
        vals = [SS.key_value(x) for x in keys[keys != SS.KEY_NONE].tolist()]
        for agg in SS.SEL_AGGS:
            out.append((w, agg, keys, head, select_double(agg, vals),
                        seg_select(keys, agg, head)))
    return out


def test_the_cases_reach_every_branch(truth):
    seen = set()
    for w, agg, keys, head, want, (got, tr) in truth:
        seen.update(tr)
    need = {"mn==mx", "shift64", "offset", "offset:carry1", "offset:all-bits",
            "digit:one", "digit:two", "digit:copy", "digit:two:one-small",
            "digit:short3", "exit:shift0", "exit:shift0:ties>cap", "gather",
            "gather:shift<bits", "gather:shift64", "gather:same",
            "gather:two", "fk:head", "fk:tail", "fk:unrolled:all",
            "fk:unrolled:1", "fk:unrolled:%d" % (K.SS_THREADS // 2)}
    assert need <= seen, sorted(need - seen)
    # under the zero fill the tie of more than SS_CAP keys is the fill value
    assert any("-zero/" in w and "exit:shift0:ties>cap" in tr and
               want == 0.0 for w, agg, keys, head, want, (got, tr) in truth)


# --------------------------------------------------------- c. the mutants
def test_the_restatement_is_the_model(truth):
    for w, agg, keys, head, want, (got, tr) in truth:
        assert same(agg, got, want), "%s/%s: %r vs %r (%s)" % (
            w, agg, got, want, tr)


# dm_full: see test_a_wide_mask_on_the_last_pass_changes_nothing
@pytest.mark.parametrize("mutant", [m for m in MUTANTS if m != "dm_full"])
def test_the_cases_catch(truth, mutant):
    caught = []
    for w, agg, keys, head, want, (got, tr) in truth:
        bad = seg_select(keys, agg, head, mutant)[0]
        if not same(agg, bad, want):
            caught.append("%s/%s" % (w, agg))
    assert caught, mutant + ": no case tells it from the true plan"
    if mutant == "no_carry":
        assert all(c.startswith("carry/") for c in caught), caught[:4]
    if mutant == "head_skipped":
        assert all("/after/b0" in c or "/b1" in c for c in caught)


def test_a_wide_mask_on_the_last_pass_changes_nothing(truth):
    """`dm` taken as SS_BINS - 1 on a pass of w < SS_BITS bits is no mistake
    a result can show: such a pass is the last one (shift ends at 0), the
    keys it counts already agree with the target's prefix in every bit from
    w up, so the extra digit bits are the prefix's own bits: the bins keep
    their order and `prefix |= digit` adds nothing.  Held here so that a
    change to the passes that makes the mask matter shows up."""
    short = 0
    for w, agg, keys, head, want, (got, tr) in truth:
        if any(x.startswith("digit:short") for x in tr):
            short += 1
            bad = seg_select(keys, agg, head, "dm_full")[0]
            assert same(agg, bad, got), (w, agg)
    assert short > 20


# ------------------------------------------------------- d. wave_select
def wave_select(keys, r, mutant=None):
    """select.hip wave_select: 8 MSB passes of 8 bits; each of 64 lanes owns
    four bins, a wave scan finds the lane, the lane its bin."""
    keys = np.asarray(keys, np.uint64)
    prefix = mask = 0
    tr = set()
    for shift in range(56, -1, -8):
        m = (keys & np.uint64(mask)) == np.uint64(prefix)
        d = ((keys[m] >> np.uint64(shift)) & np.uint64(255)).astype(np.int64)
        c = np.bincount(d, minlength=256).reshape(64, 4)
        tot = c.sum(1)
        incl = np.cumsum(tot)
        excl = incl - tot
        mine = np.nonzero((r >= excl) & (r < incl))[0]
        if mutant and len(mine) == 0:
            return -1, tr  # (no lane holds the rank: lane 0's leftovers)
        assert len(mine) == 1
        lane = int(mine[0])
        cum, j = int(excl[lane]), 0
        while j < 3:
            if r < cum + c[lane, j]:
                break
            cum += int(c[lane, j])
            j += 1
        if j == 3:
            tr.add("fourth-bin")
        if (c > 0).sum() == 1:
            tr.add("one-bin")
        if c.max() > 1 and (c > 0).sum() > 1:
            tr.add("ties")
        if (c > 0).sum() == 256:
            tr.add("all-bins")
        if mutant != "rank_kept":
            r = r - cum
        prefix |= (4 * lane + j) << shift
        mask |= 0xFF << shift
    return prefix, tr


def bucket_keys(name, n, seed=0):
    """The keys wave_select sees in k_ds_select: NaN -> ~0."""
    v, f = SS.bucket_population(name, n, seed)
    d = v.view(np.float64) if f else v.astype(np.float64)
    return SS.dkey(d)


def test_wave_select_is_a_sort():
    seen = set()
    caught = 0
    for name in SS.BUCKET_POPULATIONS:
        for n in SS.ds_counts()[1:] + [300]:
            keys = bucket_keys(name, n)
            srt = np.sort(keys)
            nn = int((keys != SS.KEY_NONE).sum())
            for agg in SS.SEL_AGGS:
                if nn == 0:
                    continue
                for r in ranks_of(agg, nn)[0]:
                    got, tr = wave_select(keys, r)
                    seen |= tr
                    assert got == int(srt[r]), (name, n, agg, r)
                    caught += wave_select(keys, r, "rank_kept")[0] != got
    assert {"fourth-bin", "one-bin", "ties", "all-bins"} <= seen, seen
    assert caught > 0
    # the NaN keys outnumber the values and never reach a rank below nn
    keys = bucket_keys("mostly_nan", 40)
    assert (keys == SS.KEY_NONE).sum() == 30 > (keys != SS.KEY_NONE).sum()
    neg = SS.bucket_population("mostly_nan", 40)[0]
    assert (neg[np.isnan(neg.view(np.float64))] < 0).any()
    # longs beyond 2^53 do fold into ties as doubles
    v, f = SS.bucket_population("longs", 257)
    assert f == 0 and len(set(v.tolist())) > len(set(
        v.astype(np.float64).tolist()))
    # the lowest byte: every digit used, with ties, from 256 points on
    low = bucket_keys("lowbyte", 257)
    assert len(set((low & np.uint64(255)).tolist())) == 256 and \
        len(set((low >> np.uint64(8)).tolist())) == 1
    top = bucket_keys("topbyte", 257)
    assert len(set((top & np.uint64(2**56 - 1)).tolist())) <= 2 and \
        len(set((top >> np.uint64(56)).tolist())) > 100


def test_downsampling_buckets_mix_the_two_sorts():
    b = SS.ds_batch()
    hb = b.batch
    c = SS.ds_counts()
    assert c[0] == K.DS_SMALL and c[1] == K.DS_SMALL + 1
    assert SS.DS_NB > 64
    for s in range(SS.DS_SERIES):
        a, e = int(hb.offsets[s]), int(hb.offsets[s + 1])
        bk = (hb.ts[a:e] - b.start) // b.interval
        n = np.bincount(bk, minlength=SS.DS_NB)
        first = 3 if s == SS.DS_SERIES - 1 else 0
        assert (n[:first] == 0).all() and (n[first:] > 0).all()
        small = n[first:first + 64] <= K.DS_SMALL
        assert small.any() and (~small).any()   # within one wave's lanes
    assert int((hb.ts - b.start).max()) < SS.DS_NB * b.interval


# ------------------------------------------------------ the cross-rank half
def rank_parts(b, world, fill="none", bucket=0):
    """The segment's keys as dist.shard_host_batch deals the series."""
    keys = SS.keys_of(b, 0, bucket, fill)
    hb = b.batch
    cuts = [odist.shard_range(hb.n_series, world, r, hb.offsets)
            for r in range(world)]
    return [keys[a:e][keys[a:e] != SS.KEY_NONE] for a, e in cuts]


@pytest.mark.parametrize("world", [2, 3])
def test_protocol_plan_on_the_rank_populations(world):
    n = BIG[0]
    for name in SS.RANK_POPULATIONS + ("straddle_halves",):
        b = SS.build([SS.population(name, n)])
        for bucket in range(2):
            parts = rank_parts(b, world, bucket=bucket)
            allk = np.sort(np.concatenate(parts))
            for agg in SS.SEL_AGGS:
                ranks = ranks_of(agg, len(allk))[0]
                got, reads, passes, psz = xsel_select(parts, ranks)
                assert got == [int(allk[r]) for r in ranks], (name, agg)
                # (select() reads the keys once per target it picks where
                # no pool was built; k_xsel_scan picks both in one read)
                once = len(ranks) - 1 if passes == 1 else 0
                assert max(reads) - once <= 2, (name, agg, reads)
                assert passes <= odist.MAX_SEL_PASSES
                if name == "onekey":
                    assert passes == 0 and max(reads) == 0
                if name in ("cluster", "straddle", "straddle_halves") and \
                        agg != "median":
                    # more than a wave's ballot of candidates a rank
                    assert max(psz) > 64, (name, agg, psz)
        if name in ("straddle", "straddle_halves"):
            # p50's two targets leave the offset pass in different bins of
            # more than one key each: xs_plan splits the next pass into two
            # halves of XS_BINS / 2 bins
            allk = np.sort(SS.keys_of(b, 0, 0, "none"))
            mn, mx = int(allk[0]), int(allk[-1])
            s1 = max((mx - mn).bit_length() - 11, 0)
            while (mx >> s1) - (mn >> s1) >= K.XS_BINS:
                s1 += 1
            bins = (allk >> np.uint64(s1)).tolist()
            r0, r1 = ranks_of("p50", len(allk))[0]
            assert bins[r0] != bins[r1] and bins.count(bins[r0]) > 1 and \
                bins.count(bins[r1]) > 1, name
        if name == "straddle_halves" and world == 2:
            v = b.v[0][0]
            a, e = odist.shard_range(n, 2, 0, b.batch.offsets)
            assert v[a:e].max() < 1.25 < v[e:].min()


def test_chunk_case_puts_a_second_chunk_on_one_rank():
    b = SS.chunk_batch()
    held = [e - a for a, e in (odist.shard_range(
        b.batch.n_series, 2, r, b.batch.offsets) for r in range(2))]
    assert max(held) > K.SEL_CHUNK and sum(held) == 2 * K.SEL_CHUNK + 3
    assert K.XS_BINS == K.SS_BINS
