"""Shared by tests/test_select_shapes_cpu.py and
tests/test_gpu_select_shapes.py: batches whose *keys* sit on purpose on every
branch the median / percentile kernels take from what the keys look like as
64-bit patterns (select.hip k_seg_select, wave_select, k_xsel_*; kernels.hip
k_group_select; raw.hip k_raw_select).  tests/group_shapes.py walks the other
axis, how many keys a segment holds.  Imports nothing that needs a GPU.

Every threshold is read from the sources (K, and group_shapes.C), so a
retune moves the tests with it.

    POPULATIONS    (n, rng) -> float64[n]: finite doubles of magnitude
                   <= 1e150 built from bit patterns; with B(x) the bits of x,
                   most are B(1.0) + j
    sizes_of       the segment sizes of a population
    build          groups of such keys -> a batch of 2 buckets, one point per
                   member and bucket on the bucket's start, and per (group,
                   bucket) the (head, tail) for_keys sees
    keys_of        the key column k_seg_select reads for a (group, bucket)
    ds_batch       3 series whose buckets hold DS_SMALL .. 1000 points of
                   the BUCKET_POPULATIONS (k_ds_select)
    raw_batch ..   groups of 1 .. 300 members on common timestamps
                   (k_raw_select)
"""
import collections
import os
import re
import zlib

import numpy as np

from opentsdb_amd import core
from opentsdb_amd.batch import HostBatch, groups_from_ids
from tests import datasets
from tests import group_shapes as GS

C = GS.C
START = GS.START
INTERVAL = GS.INTERVAL
KEY_NONE = np.uint64(2**64 - 1)

Constants = collections.namedtuple("Constants", (
    "SS_BITS", "SS_BINS", "SS_CAP", "SS_THREADS", "DS_SMALL", "SEL_CHUNK",
    "XS_BINS", "OTSDB_KT_M", "SEL_K"))


def constants():
    d = os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir,
                     "opentsdb_amd", "csrc")
    text = open(os.path.join(d, "select.hip")).read()

    def const(name):
        m = re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, text)
        assert m, name
        return int(m.group(1))
    assert re.search(r"SS_BINS = 1 << SS_BITS;", text)
    m = re.search(r"constexpr int SEL_CHUNK = 1 << (\d+);", text)
    assert m
    return Constants(
        SS_BITS=const("SS_BITS"), SS_BINS=1 << const("SS_BITS"),
        SS_CAP=C.SS_CAP, SS_THREADS=const("SS_THREADS"),
        DS_SMALL=const("DS_SMALL"), SEL_CHUNK=1 << int(m.group(1)),
        XS_BINS=const("XS_BINS"), OTSDB_KT_M=C.OTSDB_KT_M, SEL_K=C.SEL_K)


K = constants()
CARRY_S = 20


# ------------------------------------------------------------------ the keys
def bits(x):
    return int(np.float64(x).view(np.int64))


def from_bits(b):
    return np.ascontiguousarray(b, dtype=np.int64).view(np.float64)


def dkey(v):
    """select.hip dkey: the order-preserving key of doubles (-0.0 < 0.0);
    NaN -> KEY_NONE."""
    v = np.ascontiguousarray(v, dtype=np.float64)
    u = v.view(np.uint64)
    k = np.where(u >> np.uint64(63) == 1, ~u, u | np.uint64(1 << 63))
    return np.where(np.isnan(v), KEY_NONE, k)


def key_value(k):
    k = int(k)
    u = (k & (2**63 - 1)) if k >> 63 else (~k & (2**64 - 1))
    return float(np.uint64(u).view(np.float64))


def _around(base, j):
    return from_bits(bits(base) + np.asarray(j, np.int64))


def _shuffled(rng, *parts):
    v = np.concatenate([np.asarray(p, np.float64) for p in parts])
    rng.shuffle(v)
    return v


def p_onekey(n, rng):
    return np.full(n, 42.0)


def p_lowbits(n, rng):
    j = rng.integers(0, K.SS_BINS - 1, n)
    j[:2] = (0, K.SS_BINS - 2)  # (the range is the table's, whatever n)
    rng.shuffle(j)
    return _around(1.0, j)


def p_carry(n, rng):
    """min = B(1) + 2^s - 1, max = min + (SS_BINS - 1) 2^s + 1, the rest
    uniform between.  The maximum is held by three members: a percentile of
    more than SS_CAP keys never reads the very last order statistic, so one
    key in the bin the dropped correction loses would go unnoticed."""
    s = CARRY_S
    lo = (1 << s) - 1
    hi = lo + (K.SS_BINS - 1) * (1 << s) + 1
    j = rng.integers(lo + 1, hi, n)
    j[0] = lo
    j[1:4] = hi
    rng.shuffle(j)
    return _around(1.0, j)


def p_cluster(n, rng):
    return _shuffled(rng, _around(1.0, rng.integers(0, 4096, n - 2)),
                     [1e-6, 1e6])


def p_cluster_ties(n, rng):
    j = np.arange(n - 2) % 8
    return _shuffled(rng, _around(1.0, j), [1e-6, 1e6])


def p_straddle(n, rng):
    lo = (n + 1) // 2  # p50's two order statistics: the halves' inner ends
    return _shuffled(rng, _around(1.0, rng.integers(0, 4096, lo)),
                     _around(1.5, rng.integers(0, 4096, n - lo)))


def p_straddle_halves(n, rng):
    """straddle, the lower half first: dealt over two ranks, each half lies
    wholly on one of them."""
    lo = (n + 1) // 2
    return np.concatenate([_around(1.0, rng.integers(0, 4096, lo)),
                           _around(1.5, rng.integers(0, 4096, n - lo))])


def p_straddle_wide(n, rng):
    lo = (n + 1) // 2
    return _shuffled(rng, _around(1.0, rng.integers(0, 4096, lo)),
                     _around(1.5, rng.integers(0, 2**50, n - lo)))


def p_heavytie(n, rng):
    t = (6 * n + 9) // 10
    a = (n - t) // 2
    below = _around(1.0, rng.integers(1, bits(1.5) - bits(1.0), a))
    above = _around(1.5, rng.integers(1, bits(1.75) - bits(1.5), n - t - a))
    return _shuffled(rng, np.full(t, 1.5), below, above)


def p_zeros(n, rng):
    return _shuffled(rng, np.full(n // 2, -0.0), np.full(n - n // 2, 0.0))


def p_signed(n, rng):
    b, _ = datasets.edge_values("signed", rng, n)
    return from_bits(b)


POPULATIONS = collections.OrderedDict([
    ("onekey", p_onekey), ("lowbits", p_lowbits), ("carry", p_carry),
    ("cluster", p_cluster), ("cluster_ties", p_cluster_ties),
    ("straddle", p_straddle), ("straddle_wide", p_straddle_wide),
    ("heavytie", p_heavytie), ("zeros", p_zeros), ("signed", p_signed)])


def population(name, n):
    """The first n keys of the population drawn at its largest size: the
    small cuts keep the ties of the large ones."""
    fn = p_straddle_halves if name == "straddle_halves" else POPULATIONS[name]
    top = max(n, 2 * K.SS_CAP + 2)
    if n <= K.SEL_K + 1:
        # (a cut of the 2 * SS_CAP + 2 draw)
        rng = np.random.default_rng(zlib.crc32(("%s/%d" % (name, top)).encode()))
        v = fn(top, rng)[:n]
    else:
        rng = np.random.default_rng(zlib.crc32(("%s/%d" % (name, n)).encode()))
        v = fn(n, rng)
    assert len(v) == n and np.isfinite(v).all() and (np.abs(v) <= 1e150).all()
    return v


def big_sizes():
    return [2 * K.SS_CAP + 2, 3 * K.SS_CAP + 1]


def small_sizes():
    return [K.SEL_K, K.SEL_K + 1]


def for_keys_ladder():
    """for_keys: the four-way unrolled body runs past 6 * SS_THREADS keys;
    the last size leaves it to the first half of the threads only."""
    T = K.SS_THREADS
    return [6 * T - 1, 6 * T, 6 * T + 1, 6 * T + 2, 8 * T + 3,
            2 * (3 * T + T // 2) + 1]


LADDER_POPULATIONS = ("cluster", "signed")
LAYOUTS = ("alone", "after")
SEL_AGGS = ("median", "p50", "p99", "p999", "ep95r3")
MULTI_AGGS = ["median", "p50", "p99", "p999"]
PCT = {"p50": 50.0, "p99": 99.0, "p999": 99.9, "ep95r3": 95.0}
SEL_FILLS = ("none", "nan")
FILL_FILLS = ("zero", "nan")
RANK_POPULATIONS = ("cluster", "cluster_ties", "straddle", "straddle_wide",
                    "heavytie", "zeros", "onekey")
CELLS_POPULATIONS = ("cluster", "heavytie")


# --------------------------------------------------------------- the layouts
class Built:
    """batch, nb, start, interval, raw; per group g: v[b][g] the members'
    values of bucket b in member order (NaN: a NaN point; absent members are
    in lack[g]); edges[g, b] = (head, tail) of the segment's key column."""


def nan_positions(k):
    """The members whose bucket-1 value is NaN: n < k, and n odd."""
    q = 3 if k % 2 == 0 else 2
    if k < 8:
        return []
    return [1, k // 2, k - 2][:q]


def build(groups, nans=True, lack=None):
    """groups: float64 arrays, the members' bucket-0 values in member order.
    Bucket 1 carries the same values in reversed member order, NaN at
    nan_positions (nans).  lack[g] (bool per member): the member has no
    point in bucket 1."""
    G = len(groups)
    sizes = [len(v) for v in groups]
    S = sum(sizes)
    v0 = np.concatenate(groups) if S else np.zeros(0)
    v1 = np.concatenate([v[::-1] for v in groups]) if S else np.zeros(0)
    v1 = v1.copy()
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    if nans:
        for g, k in enumerate(sizes):
            for p in nan_positions(k):
                v1[off[g] + p] = np.nan
    has1 = np.ones(S, bool)
    if lack is not None:
        has1 = ~np.concatenate([np.asarray(x, bool) for x in lack])
    npts = 1 + has1.astype(np.int64)
    offsets = np.concatenate([[0], np.cumsum(npts)]).astype(np.int64)
    P = int(offsets[-1])
    ts = np.full(P, START, np.int64)
    val = np.zeros(P, np.float64)
    val[offsets[:-1]] = v0
    second = offsets[:-1][has1] + 1
    ts[second] = START + INTERVAL
    val[second] = v1[has1]
    gid = np.repeat(np.arange(G, dtype=np.int64), sizes)
    g_off, members = groups_from_ids(gid, G)
    out = Built()
    out.batch = HostBatch(offsets, ts, val.view(np.int64),
                          np.ones(P, np.uint8), None, g_off, members)
    out.nb, out.start, out.interval, out.raw = 2, START, INTERVAL, False
    out.sizes, out.off, out.M = sizes, off, S
    v1 = np.where(has1, v1, np.nan)
    out.v = [[v0[off[g]:off[g + 1]] for g in range(G)],
             [v1[off[g]:off[g + 1]] for g in range(G)]]
    out.has1 = [has1[off[g]:off[g + 1]] for g in range(G)]
    out.edges = {}
    for g, k in enumerate(sizes):
        for b in range(2):
            head = int(b * S + off[g]) & 1 if k > 0 else 0
            out.edges[g, b] = (head, (k - head) & 1)
    return out


def first_group():
    """The group ahead of the one under test: SEL_K + 1 members, so it is
    large too and its odd size makes the next group's lg_off odd."""
    return population("signed", K.SEL_K + 1)


def layout(name, n, how, **kw):
    v = population(name, n)
    return build([v] if how == "alone" else [first_group(), v], **kw)


def fill_layout(n, how):
    """Every group large, fill zero / nan (the fused k_keys_transpose<true>
    path): cluster, negated for half the members; more than SS_CAP of them
    lack bucket 1, so that under `zero` the fill value is a tie of more than
    SS_CAP keys between keys of both signs."""
    v = population("cluster", n).copy()
    v[1::2] = -v[1::2]
    lack = np.zeros(n, bool)
    lack[np.arange(K.SS_CAP + 3) * 2 % n] = True
    assert lack.sum() > K.SS_CAP
    groups, lacks = [v], [lack]
    if how == "after":
        groups.insert(0, first_group())
        lacks.insert(0, np.arange(K.SEL_K + 1) % 3 == 1)
    return build(groups, nans=False, lack=lacks)


def keys_of(b, g, bucket, fill):
    """The key column of segment (g, bucket) as k_seg_select reads it."""
    v = b.v[bucket][g]
    k = dkey(v)
    if bucket == 1 and fill == "zero":
        k = np.where(b.has1[g], k, dkey(np.zeros(1))[0])
    return k


def spec_of(b, agg, fill, ds="max"):
    return GS.spec_of(b, agg, ds, fill)


def across_cases():
    """(where, population, n, layout) of the across-series tests."""
    out = []
    for name in POPULATIONS:
        for n in big_sizes() + small_sizes():
            for how in LAYOUTS:
                out.append(("%s/%d/%s" % (name, n, how), name, n, how))
    for name in LADDER_POPULATIONS:
        for n in for_keys_ladder():
            for how in LAYOUTS:
                out.append(("%s/%d/%s" % (name, n, how), name, n, how))
    return out


def fill_cases():
    return [("fill/%d/%s" % (n, how), n, how) for n in big_sizes()
            for how in LAYOUTS]


def chunk_batch():
    """One group of 2 * SEL_CHUNK + 3 one-point series over 1 bucket: over
    two ranks one of them holds more than SEL_CHUNK members."""
    n = 2 * K.SEL_CHUNK + 3
    v = population("signed", n)
    offsets = np.arange(n + 1, dtype=np.int64)
    out = Built()
    out.batch = HostBatch(offsets, np.full(n, START, np.int64),
                          v.view(np.int64), np.ones(n, np.uint8), None,
                          np.array([0, n], np.int64),
                          np.arange(n, dtype=np.int64))
    out.nb, out.start, out.interval, out.raw = 1, START, INTERVAL, False
    out.sizes, out.off, out.M = [n], np.array([0, n]), n
    out.v = [[v]]
    return out


# ------------------------------------------- buckets of k_ds_select / raw
def _spread(rng, n, choices):
    c = np.asarray(choices)
    v = c[rng.integers(0, len(c), n)]
    v[:min(n, len(c))] = c[:n]
    rng.shuffle(v)
    return v


NAN_BITS = (0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001,
            0x7FFFFFFFFFFFFFFF, 0xFFF4DEAD0BADF00D)


def b_equal(n, rng):
    return np.full(n, 42.0), 1


def b_lowbyte(n, rng):
    """keys that differ in the lowest byte only; from 256 points on every
    digit is used, with ties"""
    return _around(1.0, _spread(rng, n, np.arange(256))), 1


def b_topbyte(n, rng):
    """keys that differ in the top byte only: both signs, wide exponents"""
    top = np.array([e << 56 for e in range(0x01, 0x60)] +
                   [(0x80 | e) << 56 for e in range(0x01, 0x60)], np.uint64)
    top = top[np.abs(top.view(np.float64)) <= 1e150]
    return _spread(rng, n, top.view(np.int64)).view(np.float64), 1


def b_allbutone(n, rng):
    """all keys equal through seven passes but one"""
    j = np.zeros(n, np.int64)
    j[int(rng.integers(0, n))] = 1 + int(rng.integers(0, 255))
    return _around(1.0, j), 1


def b_mostly_nan(n, rng):
    """a quarter of the points (at most DS_SMALL - 6) are values, the rest
    NaNs of several payloads, a negative NaN among them: the count is past
    DS_SMALL where the values are not"""
    nv = max(1, min(n // 4, K.DS_SMALL - 6))
    v = np.array(NAN_BITS, np.uint64)[np.arange(n) % len(NAN_BITS)]
    at = rng.permutation(n)[:nv]
    v[at] = rng.standard_normal(nv).view(np.uint64)
    return v.view(np.float64), 1


def b_all_nan(n, rng):
    return np.array(NAN_BITS, np.uint64)[np.arange(n) % len(NAN_BITS)].view(
        np.float64), 1


def b_longs(n, rng):
    """longs of both signs beyond 2^53: (double) folds neighbours into
    ties"""
    base = np.array([2**53, -2**53, 2**60, -2**60, 2**62], np.int64)
    v = base[rng.integers(0, len(base), n)] + rng.integers(-3, 4, n)
    return v, 0


BUCKET_POPULATIONS = collections.OrderedDict([
    ("equal", b_equal), ("lowbyte", b_lowbyte), ("topbyte", b_topbyte),
    ("allbutone", b_allbutone), ("mostly_nan", b_mostly_nan),
    ("all_nan", b_all_nan), ("longs", b_longs)])


def bucket_population(name, n, seed=0):
    """(int64 bits, is_float) of n points."""
    rng = np.random.default_rng(zlib.crc32(("%s/%d/%d" % (name, n, seed))
                                           .encode()))
    v, f = BUCKET_POPULATIONS[name](n, rng)
    v = np.ascontiguousarray(v)
    return (v.view(np.int64) if f else v.astype(np.int64)), f


def ds_counts():
    s = K.DS_SMALL
    return [s, s + 1, 40, 63, 64, 65, 255, 256, 257, 1000]


DS_NB = 70          # > 64 non-empty buckets: a second round of lanes
DS_SERIES = 3
DS_FNS = SEL_AGGS


def ds_batch(grouping="one"):
    """3 series over DS_NB buckets of 1 m.  Bucket b of series s holds
    ds_counts()[(b + s) % 10] points of BUCKET_POPULATIONS[(b + 3 * s) % 7]:
    consecutive buckets (one wave's lanes) mix the insertion sort and the
    wave select, and every count meets every population.  The last series
    has no point in buckets 0 .. 2.  grouping "one": one group of the three;
    "each": every series its own group (every bucket value shows)."""
    counts, names = ds_counts(), list(BUCKET_POPULATIONS)
    assert len(counts) * len(names) == DS_NB
    offs, ts, val, isf = [0], [], [], []
    for s in range(DS_SERIES):
        n = 0
        for b in range(3 if s == DS_SERIES - 1 else 0, DS_NB):
            c = counts[(b + s) % len(counts)]
            v, f = bucket_population(names[(b + 3 * s) % len(names)], c, s)
            step = INTERVAL // c
            ts.append(START + b * INTERVAL + np.arange(c, dtype=np.int64) *
                      step)
            val.append(v)
            isf.append(np.full(c, f, np.uint8))
            n += c
        offs.append(offs[-1] + n)
    if grouping == "one":
        g_off, members = np.array([0, DS_SERIES], np.int64), \
            np.arange(DS_SERIES, dtype=np.int64)
    else:
        g_off, members = groups_from_ids(np.arange(DS_SERIES))
    out = Built()
    out.batch = HostBatch(np.array(offs, np.int64), np.concatenate(ts),
                          np.concatenate(val), np.concatenate(isf), None,
                          g_off, members)
    out.nb, out.start, out.interval, out.raw = DS_NB, START, INTERVAL, False
    return out


def ds_spec(b, agg, ds, fill, interval):
    s, e = GS.window(b, fill)
    d = core.DownsamplingSpecification("%s-%s-%s" % (interval, ds, fill))
    return core.make_spec(s, e, core.Aggregators.get(agg), d, s, e, False,
                          None, None)


RAW_SIZES = (1, 2, 3, 63, 64, 65, 128, 129, 300)


def raw_batch(form):
    """Groups of RAW_SIZES members, every series with one point on each of
    the same timestamps; at timestamp t the members of a group hold the t-th
    bucket population (form "double": all seven; "long": those of longs, the
    doubles' bit patterns taken as longs where that keeps their order
    shape)."""
    names = list(BUCKET_POPULATIONS) if form == "double" else \
        ["equal", "lowbyte", "topbyte", "allbutone", "longs"]
    T = len(names)
    cols = []
    for g, m in enumerate(RAW_SIZES):
        per_t = []
        for name in names:
            v, f = bucket_population(name, m, 100 + g)
            if form == "double" and not f:
                v = v.astype(np.float64).view(np.int64)
            per_t.append(v)
        cols.append(np.stack(per_t, 1))  # [m][T]
    val = np.concatenate(cols).reshape(-1)
    S = sum(RAW_SIZES)
    out = Built()
    out.batch = HostBatch(
        np.arange(S + 1, dtype=np.int64) * T,
        np.tile(START + np.arange(T, dtype=np.int64) * 1000, S), val,
        np.full(S * T, form == "double", np.uint8), None,
        *groups_from_ids(np.repeat(np.arange(len(RAW_SIZES)), RAW_SIZES)))
    out.nb, out.start, out.interval, out.raw = T, START, 1000, True
    out.names, out.form = names, form
    return out


RAW_LONG_SIZES = tuple(range(1, 42))


def raw_long_batch():
    """Groups of 1 .. 41 series of longs, two timestamps each: R_3's rint
    half-to-even at n p = x.5 and p <= 0.5 / n, R_7's 1 + (n - 1) p."""
    rng = np.random.default_rng(4141)
    S = sum(RAW_LONG_SIZES)
    val = rng.integers(-10**6, 10**6, (S, 2))
    val[:, 1] = np.where(rng.random(S) < 0.5, val[:, 1] // 1000,
                         2**53 + rng.integers(-40, 40, S))
    out = Built()
    out.batch = HostBatch(
        np.arange(S + 1, dtype=np.int64) * 2,
        np.tile(START + np.arange(2, dtype=np.int64) * 1000, S),
        val.reshape(-1), np.zeros(S * 2, np.uint8), None,
        *groups_from_ids(np.repeat(np.arange(len(RAW_LONG_SIZES)),
                                   RAW_LONG_SIZES)))
    out.nb, out.start, out.interval, out.raw = 2, START, 1000, True
    out.form = "long"
    return out


def raw_spec(b, agg):
    s, e = b.start, b.start + b.nb * b.interval
    return core.make_spec(s, e, core.Aggregators.get(agg), None, s, e, False,
                          None, None)
