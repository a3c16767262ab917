"""Shared by tests/test_stream_shapes_cpu.py and tests/test_gpu_stream_shapes.py:
point streams whose bucket boundaries fall on purpose against the lanes, DPP
rows, steps and rings of reduce_step (kernels.hip).  Imports nothing that
needs a GPU.

A series is written as a *run profile*: [(bucket index, point count), ...]
with strictly increasing indices.  Bucket b's points sit at
start + b * interval + j ms, j = 0 .. count - 1.  Values are distinct integers
of [-2^20, 2^20] and no bucket holds more than 2^13 points: every sum is
below 2^33, exact in a double in any order, so every comparison built on
this file is bit for bit.

    expected_single   the downsampled series straight from the profile
    classify          the lane mapping alone, restated: which structure
                      classes of reduce_step a stream [lo, hi) reaches
    case_list         the profiles, per K
"""
import functools
import os
import re
import zlib

import numpy as np

from opentsdb_amd.batch import HostBatch
from tests import datasets

START = datasets.T0
INTERVAL = 10_000          # > 2^13: a bucket's points keep distinct ms
HOUR = 3_600_000
MAX_RUN = 2**13
VMAX = 2**20
FORMS = ("long", "double", "mixed")
FUNCS = ("sum", "avg", "min", "max", "count", "first", "last")

K_COLUMNS, K_CELLS = 8, 6
RING_ROW, RING_FOLD, RING_RATE = (256, 64), (128, 32), (1024, 512)
RING_KIND = {RING_ROW: "row", RING_FOLD: "fold", RING_RATE: "rate"}
WINS = (128, 256, 1024)


# ------------------------------------------------- the kernels' shapes, read
def kernel_shapes():
    """K, WIN and FL of every consumer as the sources state them."""
    d = os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir,
                     "opentsdb_amd", "csrc")
    text = {n: open(os.path.join(d, n)).read()
            for n in ("ds_tu.hip", "panel.hip", "fold.hip")}

    def define(src, name):
        m = re.search(r"#define\s+%s\s+(\d+)" % name, text[src])
        assert m, (src, name)
        return int(m.group(1))

    def grab(src, pat):
        m = re.search(pat, text[src])
        assert m, (src, pat)
        return int(m.group(1))

    return {
        "row": (grab("ds_tu.hip", r"case DS_RING:[^\n]*\n\s*hipLaunchKernelGGL"
                     r"\(\(k_bucketize_k<M, (\d+),"),
                define("ds_tu.hip", "OTSDB_RING_WIN"),
                define("ds_tu.hip", "OTSDB_RING_FL")),
        "rate": (define("ds_tu.hip", "OTSDB_RATE_K"),
                 define("ds_tu.hip", "OTSDB_RATE_WIN"),
                 define("ds_tu.hip", "OTSDB_RATE_FL")),
        "cells": (define("ds_tu.hip", "OTSDB_CELLS_K"),
                  define("ds_tu.hip", "OTSDB_RING_WIN"),
                  define("ds_tu.hip", "OTSDB_RING_FL")),
        "fold": (grab("ds_tu.hip", r"k_fold<M, A, (\d+)>"),
                 grab("fold.hip", r"constexpr int FOLD_WIN = (\d+);"),
                 define("fold.hip", "OTSDB_FOLD_FL")),
        "panel": (grab("panel.hip", r"k_bucketize_k<M, (\d+),"),
                  define("ds_tu.hip", "OTSDB_RING_WIN"),
                  define("ds_tu.hip", "OTSDB_RING_FL")),
    }


# ------------------------------------------------------------------ profiles
def check_profile(profile):
    assert len(profile) > 0
    b = [p[0] for p in profile]
    assert b[0] >= 0 and all(x < y for x, y in zip(b, b[1:])), "indices"
    assert all(1 <= c <= MAX_RUN for _, c in profile), "counts"


def n_points(profile):
    return sum(c for _, c in profile)


def profile_values(profile):
    """The profile's values, one a point in time order: distinct integers of
    [-2^20, 2^20], a function of the profile alone."""
    return _values(tuple(map(tuple, profile)))


@functools.lru_cache(maxsize=None)
def _values(profile):
    n = n_points(profile)
    seed = zlib.crc32(np.asarray(profile, np.int64).tobytes())
    rng = np.random.default_rng(seed)
    # a shuffled ladder of n rungs over the range, each value anywhere on
    # its own rung
    stride = (2 * VMAX + 1) // n
    assert stride >= 1
    v = rng.permutation(n) * stride + rng.integers(0, stride, n) - VMAX
    v = v.astype(np.int64)
    v.setflags(write=False)
    return v


def profile_ts(profile, interval=INTERVAL, start=START, spacing=1):
    return np.concatenate([start + b * interval +
                           spacing * np.arange(c, dtype=np.int64)
                           for b, c in profile])


def series_of(profile, form, pre=0, interval=INTERVAL, start=START,
              spacing=1, counter=False):
    """(ts, bits, is_float) of a profile in one of FORMS, with `pre` points
    (0 to 3) just before the window start.  spacing: ms between a bucket's
    points.  counter: the running sum of the values' magnitudes + 1 (a
    counter that only rises, below 2^33)."""
    assert form in FORMS and 0 <= pre <= 3
    check_profile(profile)
    assert max(c for _, c in profile) * spacing <= interval
    ts = profile_ts(profile, interval, start, spacing)
    v = profile_values(profile)
    if counter:
        v = np.cumsum(np.abs(v) + 1)
    if pre:  # never read: outside every value the window holds
        ts = np.concatenate([start + spacing * np.arange(-pre, 0,
                                                         dtype=np.int64), ts])
        v = np.concatenate([3 * VMAX + np.arange(pre, dtype=np.int64), v])
    if form == "long":
        f = np.zeros(len(v), np.uint8)
    elif form == "double":
        f = np.ones(len(v), np.uint8)
    else:
        f = ((np.arange(len(v)) * 2654435761 >> 7) & 1).astype(np.uint8)
    bits = np.where(f == 1, v.astype(np.float64).view(np.int64), v)
    return ts, bits, f


def with_parity(offset, parity, pre=None):
    """How a series that would start at index `offset` of the batch's ts
    column gets a first in-window point of absolute index parity `parity`:
    (filler, pre) — a one-point filler series in front or not, and the
    number of points before the window start.  pre given (0 to 3): kept, the
    filler makes up the parity; else no filler and pre is 0 or 1."""
    if pre is None:
        return False, (parity - offset) % 2
    assert 0 <= pre <= 3
    return (offset + pre) % 2 != parity % 2, pre


class Case:
    """A profile, the parity of its first in-window point's absolute index
    and, optionally, the number of points before the window (else the
    helper's choice)."""

    def __init__(self, name, profile, odd=0, pre=None):
        check_profile(profile)
        self.name, self.profile, self.odd, self.pre = name, profile, odd, pre

    def __repr__(self):
        return "Case(%s)" % self.name


class Built:
    """A batch of cases, one single-series group per case (filler series, if
    any, share one last group): batch, spans[i] = (lo, hi) of case i's
    in-window points in the ts column, and the grid."""


def build(cases, form, interval=INTERVAL, start=START, pad=0, mixed=0,
          spacing=1, counter=False, nb_min=0):
    """pad: that many further one-point single-series groups behind the
    cases (the fold's plan keeps full windows when there are many tiles).
    mixed > 0: instead, `mixed` groups that each hold one member of every
    case (the form rotates from group to group).  nb_min: the grid has at
    least that many buckets."""
    offs, tss, vals, isf = [0], [], [], []
    spans, case_series, fillers = [], [], []

    def add(t, v, f):
        tss.append(t), vals.append(v), isf.append(f)
        offs.append(offs[-1] + len(t))
        return len(offs) - 2

    reps = max(mixed, 1)
    for r in range(reps):
        for c in cases:
            fm = FORMS[(FORMS.index(form) + r) % 3]
            filler, pre = with_parity(offs[-1], c.odd, c.pre)
            if filler:
                fillers.append(add(np.array([start], np.int64),
                                   np.array([7], np.int64),
                                   np.zeros(1, np.uint8)))
            t, v, f = series_of(c.profile, fm, pre, interval, start, spacing,
                                counter)
            lo = offs[-1] + pre
            assert lo % 2 == c.odd % 2
            case_series.append(add(t, v, f))
            if r == 0:
                spans.append((lo, offs[-1]))
    pads = [add(np.array([start + (i % 64) * interval], np.int64),
                np.array([i], np.int64), np.zeros(1, np.uint8))
            for i in range(pad)]
    n = len(cases)
    if mixed:
        groups = [[case_series[r * n + i] for i in range(n)]
                  for r in range(reps)]
    else:
        groups = [[s] for s in case_series]
    groups += [[s] for s in pads]
    if fillers:
        groups.append(fillers)
    g_off = np.cumsum([0] + [len(g) for g in groups]).astype(np.int64)
    members = np.array([s for g in groups for s in g], np.int64)
    out = Built()
    out.cases, out.form, out.interval, out.start = cases, form, interval, start
    out.batch = HostBatch(np.array(offs, np.int64), np.concatenate(tss),
                          np.concatenate(vals), np.concatenate(isf), None,
                          g_off, members)
    out.spans = spans
    out.mixed = mixed
    out.nb = max(nb_min, 1 + max(c.profile[-1][0] for c in cases))
    return out


def window(built, fill):
    """The grid's nb buckets from start: under NONE the iterator's window
    ends 1 ms before the next bucket's start, a filling grid ends on it."""
    end = built.start + built.nb * built.interval
    return built.start, end - (1 if fill == "none" else 0)


# ------------------------------------------------------- the plain reference
def expected_single(profile, fn, fill="none", nb=None):
    """(bucket indices int64[], values float64[]) of the profile downsampled
    with fn.  fill "zero": every bucket of 0 .. nb - 1, absent ones 0."""
    assert fn in FUNCS
    v = profile_values(profile).astype(np.float64)
    idx = np.array([b for b, _ in profile], np.int64)
    cnt = np.array([c for _, c in profile], np.int64)
    a = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    if fn == "sum":
        out = np.add.reduceat(v, a)
    elif fn == "avg":
        out = np.add.reduceat(v, a) / cnt.astype(np.float64)
    elif fn == "min":
        out = np.minimum.reduceat(v, a)
    elif fn == "max":
        out = np.maximum.reduceat(v, a)
    elif fn == "count":
        out = cnt.astype(np.float64)
    elif fn == "first":
        out = v[a]
    else:
        out = v[a + cnt - 1]
    if fill == "none":
        return idx, out
    assert fill == "zero" and nb is not None and nb > idx[-1]
    full = np.zeros(nb, np.float64)
    full[idx] = out
    return np.arange(nb, dtype=np.int64), full


# ------------------------------------------------------------ the classifier
# (the scan branches at L > 0, > 1, > 3 and > 7: both sides of each)
L_CLASSES = ("L:0", "L:1", "L:2", "L:3", "L:4", "L:5-7", "L:8", "L:9-15",
             "L:16-63", "L:64")
L_TOPS = (0, 1, 2, 3, 4, 7, 8, 15, 63, 64)
COMMON_CLASSES = (
    "lane:1", "lane:2", "lane:3+mid", "lane:3-nomid", "lane:4+",
    "step:no3", "step:has3", "tail:nv0", "tail:partial", "first:base<lo",
    "first+last") + L_CLASSES + (
    "cross:15|16", "cross:31|32", "cross:47|48",
    "start:16", "start:32", "start:48", "bucket:2steps",
    "carry:join1", "carry:joinhead", "carry:closed",
    "step:both", "step:noboth",
    "ring:WIN-1", "ring:WIN", "ring:gap>WIN",
    "drain:FL-1", "drain:FL", "drain:FL+1")
FOLD_CLASSES = ("fold:cut-odd",)


def all_classes(kind):
    return set(COMMON_CLASSES + (FOLD_CLASSES if kind == "fold" else ()))


def _l_class(n):
    for name, top in zip(L_CLASSES, L_TOPS):
        if n <= top:
            return name
    raise AssertionError(n)


def classify(ts, spans, K, WIN, FL, interval, start, kind=None):
    """The structure classes the streams [lo, hi) of `spans` reach, from the
    lane mapping alone: base0 = lo & ~1, lane l of step j holds the points
    from base0 + 64 K j + K l on.  No value is computed.

    The span of a lane or step is the difference of its last and first
    bucket index (fold_fast's test): "lane:3-nomid" is a lane over buckets k
    and k + 2.  "ring:WIN-1" / "ring:WIN": the step's last bucket lies
    WIN - 1 / WIN past the open one (the first fits the ring, the second is
    the first that does not).  "drain:n": n final buckets stand undrained
    when the step is done.

    kind: which ring bookkeeping surrounds the steps — "row" (the step goes
    direct), "rate" (the series is handed back: classification ends) or
    "fold" (the step is cut at the ring's end and the stream re-based on
    hi_step & ~1); default by (WIN, FL)."""
    kind = kind or RING_KIND.get((WIN, FL), "row")
    out = set()
    for lo, hi in spans:
        if lo < hi:
            out |= _classify_stream(np.asarray(ts), lo, hi, K, WIN, FL,
                                    interval, start, kind)
    return out


def _classify_stream(ts, lo, hi, K, WIN, FL, interval, start, kind):
    PTS = 64 * K
    out = set()
    key = (ts - start) // interval
    base0 = lo & ~1
    flushed = int(key[lo])
    carry = None           # the open bucket's key after the previous step
    prev_whole = None      # the previous step's key when one bucket fills it
    prev_hi = -1
    lo_eff, base, first = lo, base0, True
    while base < hi:
        last_i = min(base + PTS, hi) - 1
        first_i = max(base, lo_eff)
        k_hi, k_first = int(key[last_i]), int(key[first_i])
        hi_step = hi
        # ---- the ring before the step
        k_open = carry if carry is not None else k_first
        if kind == "fold":
            limit = carry if carry is not None else prev_hi + 1
            if not first:
                _drain_class(out, limit - flushed, FL)
            if limit - flushed >= FL:
                flushed = limit
            if k_hi >= flushed + WIN:
                if carry is not None and carry < k_first:
                    carry, limit = None, k_first
                elif carry is None:
                    limit = k_first
                flushed = max(flushed, limit)
                if k_hi >= flushed + WIN:
                    hi_step = first_i + int(np.count_nonzero(
                        key[first_i:last_i + 1] < flushed + WIN))
                    if hi_step & 1:
                        out.add("fold:cut-odd")
            k_open = carry if carry is not None else k_first
        direct = False
        if k_hi - k_open == WIN - 1:
            out.add("ring:WIN-1")
        if k_hi - k_open == WIN:
            out.add("ring:WIN")
        if kind != "fold" and k_hi >= flushed + WIN:
            flushed = max(flushed, k_open)
            direct = k_hi >= flushed + WIN
        e = min(last_i + 1, hi_step)
        kk = key[first_i:last_i + 1]  # (the fold: before the cut)
        gaps = np.nonzero(np.diff(kk) > WIN + 1)[0]
        if len(gaps) and len(np.unique(kk[gaps[0] + 1:])) >= 2:
            out.add("ring:gap>WIN")
        if direct and kind == "rate":
            return out
        # ---- the lanes
        if first and base < lo_eff:
            out.add("first:base<lo")
        if first and base + PTS >= hi:
            out.add("first+last")
        is_tail = base >= lo_eff and base + PTS > hi_step
        nseg, head, tail = [], [], []
        has3 = False
        for lane in range(64):
            a = max(base + K * lane, lo_eff)
            b = min(base + K * lane + K, hi_step)
            k = key[a:b] if a < b else key[:0]
            nv = len(k)
            if is_tail:
                if nv == 0:
                    out.add("tail:nv0")
                elif nv < K:
                    out.add("tail:partial")
            u = np.unique(k)
            nseg.append(len(u))
            head.append(int(k[0]) if nv else None)
            tail.append(int(k[-1]) if nv else None)
            if nv == 0:
                continue
            d = int(k[-1] - k[0])
            if d == 0:
                out.add("lane:1")
            elif d == 1:
                out.add("lane:2")
            elif d == 2:
                has3 = True
                out.add("lane:3+mid" if len(u) == 3 else "lane:3-nomid")
            else:
                out.add("lane:4+")
        out.add("step:has3" if has3 else "step:no3")
        run = best = 0
        for n in nseg:
            run = run + 1 if n <= 1 else 0
            best = max(best, run)
        out.add(_l_class(best))
        for edge in (16, 32, 48):
            if tail[edge - 1] is not None and head[edge] is not None:
                if tail[edge - 1] == head[edge]:
                    out.add("cross:%d|%d" % (edge - 1, edge))
                else:
                    out.add("start:%d" % edge)
        both = False
        for lane in range(64):
            nxt = head[lane + 1] if lane < 63 else None
            put_tail = nseg[lane] >= 1 and lane < 63 and nxt != tail[lane]
            both |= nseg[lane] >= 2 and put_tail
        out.add("step:both" if both else "step:noboth")
        whole = (nseg == [1] * 64 and head[0] == tail[63] and
                 e - first_i == PTS)
        if whole and prev_whole == head[0]:
            out.add("bucket:2steps")
        prev_whole = head[0] if whole else None
        if carry is not None and nseg[0] >= 1:
            if carry != head[0]:
                out.add("carry:closed")
            else:
                out.add("carry:join1" if nseg[0] == 1 else "carry:joinhead")
        # ---- the ring after the step
        carry = tail[63]
        if kind == "fold":
            if hi_step < hi:
                prev_hi = int(key[hi_step - 1])
                lo_eff, base = hi_step, hi_step & ~1
            else:
                prev_hi = k_hi
                base += PTS
        else:
            limit = carry if carry is not None else k_hi + 1
            if direct:
                flushed = max(flushed, limit)
            else:
                _drain_class(out, limit - flushed, FL)
                flushed += (limit - flushed) // FL * FL
            base += PTS
        first = False
    return out


def _drain_class(out, n, FL):
    if n in (FL - 1, FL, FL + 1):
        out.add("drain:FL%+d" % (n - FL) if n != FL else "drain:FL")


# -------------------------------------------------------------- the case list
def runs(length, total, first=0):
    """Buckets of `length` points, adjacent, `total` points in all (the last
    bucket takes what is left)."""
    p, b = [], first
    while total > 0:
        p.append((b, min(length, total)))
        total -= length
        b += 1
    return p


def then(profile, more, gap=0):
    """`more` behind `profile`, `gap` empty buckets between them."""
    b0 = profile[-1][0] + 1 + gap
    return profile + [(b0 + b, c) for b, c in more]


MULTIPLES = (2, 3, 4, 7, 8, 15, 16, 17, 31, 32, 63, 64, 65, 129)


@functools.lru_cache(maxsize=None)
def case_list(K):
    PTS = 64 * K
    cs = []

    def add(name, profile, odd=0, pre=None):
        cs.append(Case(name, profile, odd, pre))

    add("singles", runs(1, 3 * PTS), 1)
    for r in (2, 3, 4):
        add("runs%d" % r, runs(r, 3 * PTS + r + 1), r & 1, pre=r - 1)
    for d in (-1, 0, 1):
        add("runsK%+d" % d, runs(K + d, 3 * PTS + 5), d & 1)
    for m in MULTIPLES:
        for d in (-1, 0, 1):
            n = m * K + d
            add("runs%dK%+d" % (m, d), runs(n, min(4 * PTS, max(4 * n, PTS + n))),
                (m + d) & 1)
    up, tot, r = [], 0, 1
    while tot < 4 * PTS:
        up.append(r)
        tot += r
        r += 1
    add("stairs-up", [(i, c) for i, c in enumerate(up)], 0)
    add("stairs-down", [(i, c) for i, c in enumerate(reversed(up))], 1, pre=2)
    big = [(0, 3 * PTS)]
    add("3steps-singles-3steps",
        then(then(big, runs(1, PTS // 2 + 3)), big), 0)
    for n in (1, K - 1, K, K + 1, PTS - 1, PTS, PTS + 1):
        for odd in (0, 1):
            add("len%d-%s" % (n, "odd" if odd else "even"), runs(3, n), odd,
                pre=3 if odd else 0)
    for W in WINS:
        for g in (W - 1, W, W + 1, 2 * W + 5):
            add("gap%d-in-step/W%d" % (g, W),
                then(runs(1, 40), runs(2, PTS + 9), g), 0, pre=0)
            add("gap%d-on-step/W%d" % (g, W),
                then(runs(K, PTS), runs(3, PTS // 2), g), 0, pre=0)
    # ---- cases written for one class each (the class test names them)
    for W, FL in (RING_ROW, RING_FOLD, RING_RATE):
        # a step of one bucket, then a step that begins in that open bucket
        # and whose last bucket lies W - 1 / W past it
        for d in (W - 1, W):
            add("ring-span%d/W%d" % (d, W),
                then([(0, PTS + 2)], _span_step(PTS - 2, d)), 0, pre=0)
        # a first step that leaves FL - 1, FL and FL + 1 final buckets
        for d in (FL - 1, FL, FL + 1):
            add("drain%d/W%d" % (d, W), [(0, PTS // 2), (d, PTS // 2 + K)],
                0, pre=0)
    # a step of the fold cut at the ring's end on an odd point index
    add("fold-cut-odd", then(runs(3, 9), runs(1, PTS), RING_FOLD[0] + 3), 0,
        pre=0)
    # a head that closes inside lane 0 and continues the carry
    add("carry-into-head", [(0, PTS + K // 2)] + runs(K, PTS, 1), 0, pre=0)
    # three-bucket lanes with nothing in their middle bucket
    add("lane3-nomid", _nomid(K), 0, pre=0)
    # L on both sides of every row step the scan skips: stretches of whole
    # lanes in one bucket
    for ln in (1, 2, 3, 4, 5, 7, 8, 9, 20):
        add("stretch%d" % ln, _stretch(K, ln), 0, pre=0)
    # runs that start exactly at lanes 16, 32 and 48, then whole steps
    add("rows", [(i, 16 * K) for i in range(8)] + [(8, 2 * PTS + 3)], 0, pre=0)
    names = [c.name for c in cs]
    assert len(set(names)) == len(names)
    return tuple(cs)


def _span_step(PTS, d):
    """One step of PTS points over the d buckets behind the open one: one
    point each while they last, the rest in the d-th."""
    n1 = min(d - 1, PTS - 1)
    return [(i, 1) for i in range(n1)] + [(d - 1, PTS - n1)]


def _nomid(K):
    """Lanes of K points: half in bucket 3 i, half in bucket 3 i + 2."""
    p = []
    for i in range(2 * 64):
        p += [(3 * i, K // 2), (3 * i + 2, K - K // 2)]
    return p


def _stretch(K, ln):
    """More than one full step with a bucket boundary inside every lane
    (half-lane buckets) but for stretches of `ln` whole lanes that lie inside
    one bucket — begun at lanes 1, 13 (across the rows' edge 15|16 when it
    is long enough) and 36 while they fit the step: the step's L is ln."""
    sizes, lane = [], 0
    for at in (1, 13, 36):
        if at < lane or at + ln + 2 > 64:
            continue
        sizes += [K // 2] * (2 * (at - lane)) + [K // 2,
                                                 K // 2 + ln * K + K // 2,
                                                 K // 2]
        lane = at + ln + 2
    sizes += [K // 2] * (2 * (64 - lane + 3))
    return list(enumerate(sizes))


# ------------------------------------------------- results against the profile
def as_doubles(p):
    """(ts, float64 values) of one group's points: a record array of the
    oracle's POINT or anything with ts / bits / is_int."""
    if isinstance(p, np.ndarray):
        ts, bits, ii = p["ts"], p["bits"], p["is_int"]
    else:
        ts, bits, ii = (np.asarray(p.ts), np.asarray(p.bits),
                        np.asarray(p.is_int))
    bits = np.ascontiguousarray(bits, np.int64)
    return np.asarray(ts, np.int64), np.where(
        np.asarray(ii).astype(bool), bits.astype(np.float64),
        bits.view(np.float64))


def check_expected(groups, built, fn, fill, where=""):
    """Every case's group of a result (one single-series group per case) is
    expected_single, bit for bit: the same buckets, the same double bits."""
    assert len(groups) >= len(built.cases), where
    for c, g in zip(built.cases, groups):
        w = "%s/%s/%s-%s" % (where, c.name, fn, fill)
        idx, want = expected_single(c.profile, fn, fill, built.nb)
        ts, got = as_doubles(g)
        assert len(ts) == len(idx), "%s: %d points, expected %d" % (
            w, len(ts), len(idx))
        assert np.array_equal(ts, built.start + idx * built.interval), \
            w + ": timestamps"
        bad = got.view(np.int64) != want.view(np.int64)
        assert not bad.any(), "%s: bucket %s: %r, expected %r" % (
            w, idx[bad][:4], got[bad][:4], want[bad][:4])


# ------------------------------------------------ which case reaches what
CONSUMERS = (("k_bucketize_k / panel ring", K_COLUMNS, RING_ROW),
             ("rate ring", K_COLUMNS, RING_RATE),
             ("k_fold / k_fold_multi / cells fold", K_COLUMNS, RING_FOLD),
             ("k_bucketize_cells / cells panel", K_CELLS, RING_ROW))


def coverage_table(K, ring, most=3):
    """{class: the first `most` cases that reach it, and how many do}."""
    cases = list(case_list(K))
    b = build(cases, "long")
    reach = {}
    for c, span in zip(cases, b.spans):
        for k in classify(b.batch.ts, [span], K, ring[0], ring[1], b.interval,
                          b.start):
            reach.setdefault(k, []).append(c.name)
    return {k: (v[:most], len(v)) for k, v in sorted(reach.items())}


if __name__ == "__main__":
    for name, K, ring in CONSUMERS:
        print("\n%s (K = %d, WIN = %d, FL = %d)" % ((name, K) + ring))
        for k, (names, n) in coverage_table(K, ring).items():
            print("  %-14s %3d cases: %s%s" % (k, n, ", ".join(names),
                                                ", ..." if n > len(names)
                                                else ""))
