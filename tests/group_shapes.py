"""Shared by tests/test_group_shapes_cpu.py and tests/test_gpu_group_shapes.py:
batches whose *group sizes* sit on purpose on both sides of every rule that
spreads the series of a query over tiles, chunks, chains and combine slices
(foldplan.h cut_tiles / two_level_combine / fold_plan, the selections' SEL_K
and SS_CAP).  Imports nothing that needs a GPU.

Every size is derived from the constants as the sources state them
(constants()), so a retune moves the tests with it.

The data compares bit for bit in any reduction order.  A grid of NB = 6 (some
tests 2) buckets of 1 m; points on whole seconds (the same batches encode as
2-byte-qualifier cells); values are integers, multiples of 4, of
[-2^20, 2^20], positive in even buckets and negative in odd ones (so that a
minimum and a maximum both have a side on which a stray 0 or identity
shows); at most 2 points a bucket; a gappy member misses runs of exactly 1 or
3 buckets, so that the LERP expression y0 + (x - x0) (y1 - y0) / (x1 - x0)
has an exact product and an exact quotient.  Every contribution is an
integer (or a multiple of 1/8 under `avg` downsampling) and every sum stays
far below 2^53: sum, zimsum, avg (one division), min, max, mimmin, mimmax,
count, first, last and diff are exact in any order, dev wherever the engine
promises one chain.  build() asserts the preconditions on the points;
tests/test_group_shapes_cpu.py holds the exact-integer model that asserts
them on every contribution.

    constants      the thresholds, read from the sources
    Group          one group: its size and the positions (in member order) of
                   the members that stream nothing
    placements     the named placements of such members that exist at a size
    build          groups -> batch, contiguous or interleaved member order
    fold_ladder .. the sizes, from the constants
"""
import collections
import os
import re
import zlib

import numpy as np

from opentsdb_amd import core
from opentsdb_amd.batch import HostBatch, groups_from_ids
from tests import datasets

START = datasets.T0
INTERVAL = 60_000
NB = 6
VMAX = 2**20
FORMS = ("long", "double", "mixed")
EFFECTIVE = ("full", "gappy", "late", "early", "one", "straddle")
# members that stream nothing and that the span group does not even keep
QUIET = ("empty", "before", "after")
# the buckets a gappy member has: every run it misses is 1 or 3 buckets long
GAPPY = ((0, 2, 3, 5), (0, 4, 5), (0, 1, 5), (1, 3, 4), (0, 2, 4), (1, 5),
         (0, 2), (1, 2, 4), (0, 4))
COUNTER_STEP = 960  # x / 60, x / 120 and x / 240 are multiples of 4


# --------------------------------------------------- the constants, as stated
Constants = collections.namedtuple("Constants", (
    "kFoldChunk", "kFoldChunkLarge", "kOrderedFoldChunk", "kChunk",
    "kCombineL1", "kCombineSlices", "kOrderedChunk", "SEL_K", "OTSDB_KT_M",
    "SS_CAP"))


def constants():
    d = os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir,
                     "opentsdb_amd", "csrc")
    text = {n: open(os.path.join(d, n)).read()
            for n in ("foldplan.h", "engine.hip", "kernels.hip", "select.hip")}

    def grab(src, pat):
        m = re.search(pat, text[src])
        assert m, (src, pat)
        return int(m.group(1))

    def const(src, name):
        return grab(src, r"constexpr\s+int(?:64_t)?\s+%s\s*=\s*(\d+)\s*;" % name)

    def define(src, name):
        return grab(src, r"#define\s+%s\s+(\d+)" % name)

    # the two tile sizes are constants initialised from their tuning macros
    assert re.search(r"kFoldChunk = OTSDB_FOLD_CHUNK;", text["foldplan.h"])
    assert re.search(r"kFoldChunkLarge = OTSDB_FOLD_CHUNK_LARGE;",
                     text["foldplan.h"])
    assert re.search(r"KT_M = OTSDB_KT_M;", text["select.hip"])
    return Constants(
        kFoldChunk=define("foldplan.h", "OTSDB_FOLD_CHUNK"),
        kFoldChunkLarge=define("foldplan.h", "OTSDB_FOLD_CHUNK_LARGE"),
        kOrderedFoldChunk=const("foldplan.h", "kOrderedFoldChunk"),
        kChunk=const("foldplan.h", "kChunk"),
        kCombineL1=const("foldplan.h", "kCombineL1"),
        kCombineSlices=const("foldplan.h", "kCombineSlices"),
        kOrderedChunk=const("engine.hip", "kOrderedChunk"),
        SEL_K=const("kernels.hip", "SEL_K"),
        OTSDB_KT_M=define("select.hip", "OTSDB_KT_M"),
        SS_CAP=const("select.hip", "SS_CAP"))


C = constants()
# fold_plan preloads member contexts up to this tile size (foldplan.h:
# `tile_max <= 64`, the one threshold the source writes as a literal)
FOLD_CTX_MAX = int(re.search(
    r"tile_max > 0 && tile_max <= (\d+)",
    open(os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir,
                      "opentsdb_amd", "csrc", "foldplan.h")).read()).group(1))


def ceil_div(a, b):
    return -(-a // b)


# ------------------------------------------------------------------ the sizes
def around(c):
    return [c - 1, c, c + 1]


def fold_ladder():
    """Unordered fold: one tile up to kFoldChunk, tiles of kFoldChunkLarge
    past it; two-level combine past kCombineL1 tiles; all kCombineSlices
    slices used at 3 slices' worth of tiles, the slice one tile longer (and
    the last one short) one member later."""
    L, F = C.kFoldChunkLarge, C.kFoldChunk
    return ([1, 2] + around(L) + around(F) + [F + L, F + L + 1] +
            [C.kCombineL1 * L, C.kCombineL1 * L + 1,
             3 * C.kCombineSlices * L, 3 * C.kCombineSlices * L + 1])


def ordered_ladder():
    """dev: one fold tile up to kOrderedFoldChunk; contexts preloaded up to
    FOLD_CTX_MAX members.  The last size is the first on the row path."""
    F = C.kFoldChunk
    return ([1, 2, F, F + 1, FOLD_CTX_MAX, FOLD_CTX_MAX + 1,
             C.kOrderedFoldChunk - 1, C.kOrderedFoldChunk,
             C.kOrderedFoldChunk + 1])


def row_ladder():
    return around(C.kChunk) + [2 * C.kChunk, 2 * C.kChunk + 1]


def row_two_level():
    return [C.kCombineL1 * C.kChunk, C.kCombineL1 * C.kChunk + 1]


def selection_ladder():
    return around(C.SEL_K) + around(C.OTSDB_KT_M)


def mixed_sizes():
    """Today [1025, 0, 9, 33, 32, 0, 0, 1, 1537, 8, 0]: member-less groups
    first but one, doubled in the middle and last; two-level groups beside
    two-tile and one-tile groups."""
    L, F = C.kFoldChunkLarge, C.kFoldChunk
    return [C.kCombineL1 * L + 1, 0, L + 1, F + 1, F, 0, 0, 1,
            3 * C.kCombineSlices * L + 1, L, 0]


def mixed_large_first():
    L, F = C.kFoldChunkLarge, C.kFoldChunk
    return [3 * C.kCombineSlices * L + 1, L + 1, 1, 0, F, 2 * L, F + 1]


def mixed_large_last():
    return list(reversed(mixed_large_first()))


def tiles_of(n, chunk=None, whole=None):
    """The tiles [m0, m1) of a group of n members (cut_tiles' rule); default:
    the unordered fold's tiling."""
    chunk = C.kFoldChunkLarge if chunk is None else chunk
    whole = C.kFoldChunk if whole is None else whole
    ch = max(n, 1) if n <= whole else chunk
    return [(m, min(n, m + ch)) for m in range(0, n, ch)]


def slice_len(n_tiles):
    return ceil_div(n_tiles, C.kCombineSlices)


# ------------------------------------------------------------ the placements
def placements(n, chunk=None, whole=None):
    """{name: positions of the members that stream nothing}, for every
    placement that exists in a group of n members."""
    L = C.kFoldChunkLarge if chunk is None else chunk
    F = C.kFoldChunk if whole is None else whole
    t = tiles_of(n, L, F)
    out = {}
    if n >= 2:
        out["first"] = {0}
        out["last"] = {n - 1}
    if len(t) >= 2:
        out["tile-edge"] = {L - 1, L}
        if n > F > 0:
            out["whole-edge"] = {F - 1, F}
    if len(t) >= 3:
        out["tile"] = set(range(*t[1]))
        out["last-tile"] = set(range(*t[-1]))
        out["first-tile"] = set(range(*t[0]))
    if len(t) > C.kCombineL1:
        ls = slice_len(len(t))
        out["slice"] = set(range(t[ls][0], t[2 * ls - 1][1]))
        out["first-slice"] = set(range(0, t[ls - 1][1]))
    if n >= 1:
        out["all"] = set(range(n))
    return out


class Group:
    """n members; those at `quiet` stream nothing (QUIET, in rotation)."""

    def __init__(self, n, quiet=()):
        self.n, self.quiet = n, frozenset(quiet)
        assert all(0 <= p < n for p in self.quiet)

    def __repr__(self):
        return "Group(%d, %d quiet)" % (self.n, len(self.quiet))


def groups_of(sizes, quiet_every=0):
    """Plain groups of these sizes; quiet_every = k: every k-th group streams
    nothing at all."""
    return [Group(n, range(n) if quiet_every and g % quiet_every == 1 else ())
            for g, n in enumerate(sizes)]


# ------------------------------------------------------------------ the data
def _present(role, pick, nb):
    """The buckets a member of `role` has a point in."""
    if role == "full":
        return list(range(nb))
    if role == "gappy":
        if nb < NB:
            return [int(pick % nb)]
        return list(GAPPY[pick % len(GAPPY)])
    if role == "late":
        return list(range(1 + pick % max(nb - 2, 1), nb)) if nb > 1 else [0]
    if role == "early":
        return list(range(0, 1 + pick % max(nb - 1, 1)))
    if role == "one":
        return [int(pick % nb)]
    return []


class Built:
    """batch, nb, start, interval, groups (the Group list), roles[g][p],
    form, order."""


def build(groups, form="mixed", nb=NB, order="contig", counter=False,
          raw=False, nan_at=None, only=None):
    """groups: Group list.  order "contig": series numbered group by group;
    "inter": the groups' members dealt round-robin over the series indices
    (group ids through groups_from_ids).  counter: every series is a counter
    that starts at 0 and rises in steps of COUNTER_STEP (rates on the grid
    are multiples of 4), no point outside the window.  raw: one point a
    bucket, on the bucket's start (a raw group-by emits on the grid).
    nan_at(g, p, bucket) -> bool: that member's value there is NaN (double
    points only).  only: the one role of every member that streams."""
    assert form in FORMS and order in ("contig", "inter") and nb in (2, NB)
    assert not (counter and raw)
    S = sum(g.n for g in groups)
    seed = zlib.crc32(repr(([(g.n, sorted(g.quiet)) for g in groups], form, nb,
                            counter, raw)).encode())
    rng = np.random.default_rng(seed)
    mag = rng.integers(1, VMAX // 4 + 1, size=(S, 2 * nb + 2)) * 4
    pick = rng.integers(0, 2**31, size=(S, 4))
    end = START + nb * INTERVAL
    series, roles = [], []
    s = 0
    for gi, g in enumerate(groups):
        roles.append([])
        for p in range(g.n):
            pk = pick[s]
            if p in g.quiet:
                role = QUIET[(p + gi) % len(QUIET)]
            else:
                # mostly full and gappy; every role within any 8 neighbours
                role = ("full", "gappy", "late", "full", "early", "gappy",
                        "one", "straddle")[(p + int(pk[0]) % 2) % 8]
                if counter and role == "straddle":
                    role = "full"
                if only:
                    role = only
            extras = not counter and not raw
            pts = []
            if role in ("before", "straddle") or (
                    role == "full" and pk[1] % 4 == 0 and extras):
                pts.append((START - (1 + pk[1] % 3) * INTERVAL + 1000 *
                            int(pk[2] % 60), int(mag[s, 2 * nb])))
            k = 0
            for b in _present(role, int(pk[3]), nb):
                sign = 1 if b % 2 == 0 else -1
                o = 0 if raw else int(pk[2] + 7 * b) % 29
                two = (not raw) and (int(pk[1]) >> (3 + b)) & 1 and not (
                    counter and k == 0)  # (a counter's first bucket: its 0)
                for j in range(2 if two else 1):
                    if counter:
                        v = 0 if k == 0 else pts[-1][1] + COUNTER_STEP * (
                            1 + int(mag[s, 2 * b + j]) % 997)
                    else:
                        v = sign * int(mag[s, 2 * b + j])
                    pts.append((START + b * INTERVAL + 1000 * (o + 30 * j), v))
                    k += 1
            if role in ("after", "straddle"):
                b1 = nb + int(pk[2] % 3)
            elif role == "early" and pk[1] % 2 == 1 and extras:
                # 1 or 3 empty buckets behind the member's last one, past
                # the window where that reaches it: it interpolates to it
                b0 = (pts[-1][0] - START) // INTERVAL
                b1 = b0 + (2 if b0 + 2 >= nb else 4)
            else:
                b1 = None
            if b1 is not None:
                pts.append((START + b1 * INTERVAL + 1000 * int(1 + pk[2] % 28),
                            (1 if b1 % 2 == 0 else -1) *
                            int(mag[s, 2 * nb + 1])))
            if form == "long":
                fl = [0] * len(pts)
            elif form == "double":
                fl = [1] * len(pts)
            else:
                fl = [(int(pk[0]) >> (i % 16)) & 1 for i in range(len(pts))]
            series.append((gi, p, pts, fl))
            roles[-1].append(role)
            s += 1
    # ---- the preconditions
    for gi, p, pts, fl in series:
        t = [x for x, _ in pts]
        assert all(a < b for a, b in zip(t, t[1:])), "time order"
        assert all(x % 1000 == 0 for x in t), "whole seconds"
        assert all(v % 4 == 0 and abs(v) <= VMAX * (1 if not counter else
                                                    COUNTER_STEP * 4 * nb)
                   for _, v in pts), "values"
        inb = [(x - START) // INTERVAL for x in t if START <= x < end]
        assert all(inb.count(b) <= 2 for b in set(inb)), "2 points a bucket"
        kk = sorted(set((x - START) // INTERVAL for x in t if x >= START))
        assert all(b - a in (1, 2, 4) for a, b in zip(kk, kk[1:])), \
            ("gaps", kk)
    # ---- member order
    G = len(groups)
    if order == "contig":
        seq = list(range(S))
    else:
        per = [[i for i, x in enumerate(series) if x[0] == gi]
               for gi in range(G)]
        seq, r = [], 0
        while len(seq) < S:
            for q in per:
                if r < len(q):
                    seq.append(q[r])
            r += 1
    offs, ts, val, isf, gid = [0], [], [], [], []
    for i in seq:
        gi, p, pts, fl = series[i]
        for (x, v), f in zip(pts, fl):
            nan = nan_at is not None and f and START <= x < end and \
                nan_at(gi, p, (x - START) // INTERVAL)
            ts.append(x)
            isf.append(f)
            val.append(int(np.float64(np.nan if nan else v).view(np.int64))
                       if f else v)
        offs.append(len(ts))
        gid.append(gi)
    if S:
        g_off, members = groups_from_ids(np.array(gid, np.int64), G)
    else:
        g_off, members = np.zeros(G + 1, np.int64), np.zeros(0, np.int64)
    assert [int(b - a) for a, b in zip(g_off, g_off[1:])] == \
        [g.n for g in groups]
    out = Built()
    out.batch = HostBatch(np.array(offs, np.int64), np.array(ts, np.int64),
                          np.array(val, np.int64), np.array(isf, np.uint8),
                          None, g_off, members)
    out.groups, out.roles, out.form, out.order = groups, roles, form, order
    out.nb, out.start, out.interval = nb, START, INTERVAL
    out.counter, out.raw = counter, raw
    return out


def window(built, fill):
    """The grid's nb buckets from start: under NONE the iterator's window
    ends 1 ms before the next bucket's start, a filling grid ends on it."""
    end = built.start + built.nb * built.interval
    return built.start, end - (1 if fill == "none" else 0)


def spec_of(b, agg, ds, fill, rate=False):
    s, e = window(b, fill)
    d = None if b.raw else core.DownsamplingSpecification(
        "1m-%s-%s" % (ds, fill))
    ro = core.RateOptions(True, core.LONG_MAX, 0) if rate else None
    return core.make_spec(s, e, core.Aggregators.get(agg), d, s, e, rate, ro,
                          None)


# ------------------------------------------------------------- the batches
def single(n, placement=None, **kw):
    """One group of n members, the quiet ones at a named placement."""
    q = placements(n)[placement] if placement else ()
    return build([Group(n, q)], **kw)


def mixed(sizes, quiet=None, **kw):
    """quiet: {group index: placement name, or several (their union)}."""
    quiet = quiet or {}

    def at(g, n):
        names = quiet.get(g, ())
        names = (names,) if isinstance(names, str) else names
        return set().union(*[placements(n)[k] for k in names])
    return build([Group(n, at(g, n)) for g, n in enumerate(sizes)], **kw)


def mixed_quiet():
    """The placements the mixed batch of mixed_sizes() carries: a whole
    first-level slice in the first two-level group, a whole tile in the
    second, the tile edge in the two-tile groups, and a one-tile group that
    streams nothing between groups that emit."""
    return {0: "slice", 2: "last", 3: ("tile-edge", "whole-edge"),
            4: "first", 7: "all", 8: "last-tile"}


def singletons(n=300, every=3, **kw):
    return build(groups_of([1] * n, every), **kw)


# ------------------------------------------------- the cases of both suites
FOLD_AGGS = ("sum", "zimsum", "avg", "min", "max", "mimmin", "mimmax",
             "count", "first", "last", "diff")
FILLS = ("none", "zero")
ROW_AGGS = ("sum", "avg", "min", "max", "count", "first", "last")
SEL_AGGS = ("median", "p50", "p99", "p999", "ep95r3")
SEL_FILLS = ("none", "nan")
RAW_AGGS = ("sum", "min", "max", "count")


def fold_batches(n):
    """[(name, Built)] of one ladder size: plain, and every placement."""
    out = [("plain", single(n))]
    out += [(k, single(n, k)) for k in placements(n)]
    # beside members that all have every bucket: under a filling grid a
    # stray 0 shows only where no kept member lacks a value
    out += [(k + "-full", single(n, k, only="full"))
            for k in ("tile", "slice") if k in placements(n)]
    return out


def ordered_batches(n):
    """dev: the group alone and, at the context threshold, beside small
    groups (one group past FOLD_CTX_MAX switches the preload off for all)."""
    pl = placements(n, C.kFoldChunk, C.kOrderedFoldChunk)
    out = [("plain", single(n))]
    out += [(k, build([Group(n, pl[k])])) for k in ("first", "last")
            if k in pl]
    if n in (FOLD_CTX_MAX, FOLD_CTX_MAX + 1):
        out.append(("beside", build(groups_of([3, n, 1, 0, C.kFoldChunk]))))
    return out


def mixed_batches(form="mixed"):
    return [
        ("mixed", mixed(mixed_sizes(), mixed_quiet(), form=form)),
        ("mixed-inter", mixed(mixed_sizes(), mixed_quiet(), order="inter",
                              form=form)),
        ("large-first", mixed(mixed_large_first(), {0: "first-slice",
                                                    6: "tile-edge"},
                              form=form)),
        ("large-last", mixed(mixed_large_last(), {6: "last", 0: "tile"},
                             order="inter", form=form)),
        ("singletons", singletons(form=form)),
    ]


def row_batches(n):
    """[(name, Built)] of one row-path size: plain, the last member quiet
    (a chunk of its own one member past a chunk's end) and, from two full
    chunks on, the whole second chunk quiet (it leaves an identity partial
    from a full chunk)."""
    out = [("plain", single(n)), ("last", build([Group(n, {n - 1})]))]
    t = tiles_of(n, C.kChunk, 0)
    if len(t) >= 2 and t[1][1] - t[1][0] == C.kChunk:
        out.append(("chunk", build([Group(n, range(*t[1]))])))
    return out


def selection_group(n, **kw):
    return build([Group(n)], form="double", **kw)


def ss_cap_batch():
    """SS_CAP + 6 full members over 2 buckets; NaN values leave exactly
    SS_CAP candidates in bucket 0 and SS_CAP + 1 in bucket 1."""
    n = C.SS_CAP + 6
    step = n // 7
    return build([Group(n)], form="double", nb=2, only="full",
                 nan_at=lambda g, p, b: p % step == 1 and
                 p // step < (6 if b == 0 else 5))


def raw_sizes():
    return [1, 0, C.SEL_K, 0, 0, C.SEL_K + 1, C.kChunk + 1, 0]
