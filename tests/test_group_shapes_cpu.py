"""Group-shape edges without a GPU (tests/group_shapes.py):

a. the tile cut (csrc/foldplan.h: cut_tiles, two_level_combine, fold_plan)
   compiled alone for the host with the address and undefined-behaviour
   sanitizers, fed every ladder and every mixed batch, against a restatement
   of the rule in Python; each pair of neighbouring sizes is asserted to
   straddle its predicate;
b. the CPU oracle against a plain model on exact integers (values scaled by
   8: every downsampled value, interpolation and rate of these batches is a
   whole number of eighths, which the model asserts at every step), on every
   batch and aggregator tests/test_gpu_group_shapes.py runs;
c. the same model with the mistakes these boundaries invite switched on, one
   at a time: every one changes at least one emitted point of at least one
   case, so the batches tell a wrong kernel from a right one.
"""
import math
import shutil
import subprocess

import numpy as np
import pytest

from oracle import pyoracle
from tests import group_shapes as GS
from tests.test_fold_plan_cpu import CSRC

C = GS.C
SC = 8  # the model's values are integers: eighths

# ------------------------------------------------------------ a. the tile cut
# stdin, one case a line: "sel_all chunk whole_upto NB ordered n k_1 .. k_n";
# stdout per case: "T MG LG max_chunks two_level fold_ctx", then one line
# each of tg tm0 tm1 single mg mt0 mt1 ag at0 at1 lgg lgo lgk lgc
DRIVER = r"""
#include <cstdio>
#include "foldplan.h"
static void row(const std::vector<int64_t>& v) {
  for (int64_t x : v) printf("%lld ", (long long)x);
  printf("\n");
}
int main() {
  int sel_all, ordered, n;
  long long chunk, whole, NB;
  while (scanf("%d %lld %lld %lld %d %d", &sel_all, &chunk, &whole, &NB,
               &ordered, &n) == 6) {
    std::vector<int64_t> goff{0};
    for (int i = 0; i < n; ++i) {
      long long k;
      if (scanf("%lld", &k) != 1) return 2;
      goff.push_back(goff.back() + k);
    }
    const otsdb::TileCut c =
        otsdb::cut_tiles(goff, sel_all != 0, chunk, whole, SEL_K, SEL_CHUNK);
    const int64_t T = (int64_t)c.tg.size(), MG = (int64_t)c.mg.size();
    const otsdb::FoldPlan p =
        otsdb::fold_plan(goff, T, NB, 2048, ordered != 0, true);
    printf("%lld %lld %lld %lld %d %d\n", (long long)T, (long long)MG,
           (long long)c.lgg.size(), (long long)c.max_chunks,
           (int)otsdb::two_level_combine(c.max_chunks, MG, NB),
           (int)p.fold_ctx);
    row(c.tg); row(c.tm0); row(c.tm1);
    row(std::vector<int64_t>(c.single.begin(), c.single.end()));
    row(c.mg); row(c.mt0); row(c.mt1); row(c.ag); row(c.at0); row(c.at1);
    row(c.lgg); row(c.lgo); row(c.lgk); row(c.lgc);
  }
  return 0;
}
"""
SEL_CHUNK = 1 << 17
FOLD = (C.kFoldChunkLarge, C.kFoldChunk)        # (chunk, whole_upto)
ORDERED = (C.kFoldChunk, C.kOrderedFoldChunk)
ROW = (C.kChunk, 0)
ROW_ORDERED = (C.kChunk, C.kOrderedChunk)


@pytest.fixture(scope="module")
def cut(tmp_path_factory):
    # (no skip: the sanitizer build is part of what this file promises)
    assert shutil.which("g++") is not None, "g++ is needed for the tile cut"
    d = tmp_path_factory.mktemp("tilecut")
    src = d / "cut.cc"
    src.write_text(DRIVER)
    exe = d / "cut"
    subprocess.run(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-Wall", "-Werror",
                    "-DSEL_K=%d" % C.SEL_K, "-DSEL_CHUNK=%d" % SEL_CHUNK,
                    "-I", CSRC, "-o", str(exe), str(src)], check=True)

    def run(cases):
        """cases: (sizes, (chunk, whole), sel_all, ordered, NB) -> dicts."""
        text = "".join("%d %d %d %d %d %d %s\n" % (
            sel_all, tiling[0], tiling[1], NB, ordered, len(sizes),
            " ".join(map(str, sizes)))
            for sizes, tiling, sel_all, ordered, NB in cases)
        r = subprocess.run([str(exe)], input=text, capture_output=True,
                           text=True)
        assert r.returncode == 0, r.stderr
        lines = r.stdout.split("\n")
        assert len(lines) == 15 * len(cases) + 1
        keys = ("tg", "tm0", "tm1", "single", "mg", "mt0", "mt1", "ag", "at0",
                "at1", "lgg", "lgo", "lgk", "lgc")
        out = []
        for i in range(len(cases)):
            h = list(map(int, lines[15 * i].split()))
            o = dict(zip(("T", "MG", "LG", "max_chunks", "two_level",
                          "fold_ctx"), h))
            for j, k in enumerate(keys):
                o[k] = list(map(int, lines[15 * i + 1 + j].split()))
            out.append(o)
        return out
    return run


def cut_restated(sizes, tiling, sel_all, ordered, NB):
    chunk, whole = tiling
    o = {k: [] for k in ("tg", "tm0", "tm1", "single", "mg", "mt0", "mt1",
                         "ag", "at0", "at1", "lgg", "lgo", "lgk")}
    o["lgc"] = [0]
    a = 0
    for g, n in enumerate(sizes):
        t0 = len(o["tg"])
        tiles = GS.tiles_of(n, chunk, whole)
        for m0, m1 in tiles:
            o["tg"].append(g), o["tm0"].append(a + m0), o["tm1"].append(a + m1)
            o["single"].append(int(len(tiles) == 1))
        if len(tiles) > 1:
            o["mg"].append(g), o["mt0"].append(t0)
            o["mt1"].append(t0 + len(tiles))
        o["ag"].append(g), o["at0"].append(t0), o["at1"].append(t0 + len(tiles))
        if n > C.SEL_K or sel_all:
            o["lgg"].append(g), o["lgo"].append(a), o["lgk"].append(n)
            o["lgc"].append(o["lgc"][-1] + GS.ceil_div(n, SEL_CHUNK))
        a += n
    o["T"], o["MG"], o["LG"] = len(o["tg"]), len(o["mg"]), len(o["lgg"])
    o["max_chunks"] = max([e - b for b, e in zip(o["at0"], o["at1"])],
                          default=0)
    o["two_level"] = int(o["max_chunks"] > C.kCombineL1 and
                         o["MG"] * C.kCombineSlices * NB * 33.0 < 2.0e9)
    tile_max = max([min(n, C.kOrderedFoldChunk) if ordered else
                    (n if n <= C.kFoldChunk else min(n, C.kFoldChunkLarge))
                    for n in sizes], default=0)
    o["fold_ctx"] = tile_max if 1 <= tile_max <= GS.FOLD_CTX_MAX else 0
    return o


def all_cut_cases():
    cases = []
    for n in GS.fold_ladder():
        cases.append(([n], FOLD, 0, 0, GS.NB))
    for n in GS.ordered_ladder():
        cases.append(([n], ORDERED, 0, 1, GS.NB))
        cases.append(([3, n, 1, 0, C.kFoldChunk], ORDERED, 0, 1, GS.NB))
    for n in GS.row_ladder() + GS.row_two_level():
        cases.append(([n], ROW, 0, 0, GS.NB))
    for n in (C.kOrderedChunk, C.kOrderedChunk + 1):
        cases.append(([n], ROW_ORDERED, 0, 1, 2))
    for n in GS.selection_ladder() + [C.SS_CAP + 6]:
        cases.append(([n], ROW, 0, 0, GS.NB))
        cases.append(([n], ROW, 1, 0, GS.NB))
    for sizes in (GS.mixed_sizes(), GS.mixed_large_first(),
                  GS.mixed_large_last(), [1] * 300, GS.raw_sizes(),
                  [C.SEL_K, C.SEL_K + 1], [], [0], [0, 0, 0]):
        for tiling in (FOLD, ORDERED, ROW):
            for sel_all in (0, 1):
                cases.append((sizes, tiling, sel_all, int(tiling == ORDERED),
                              GS.NB))
    return cases


def test_cut_matches_the_rule(cut):
    cases = all_cut_cases()
    for case, got in zip(cases, cut(cases)):
        want = cut_restated(*case)
        for k in want:
            assert got[k] == want[k], (case[1:], case[0][:12], k)
        # every member in exactly one tile, in order; no tile is empty
        n = sum(case[0])
        assert got["tm0"][:1] == ([0] if n else [])
        assert got["tm1"][-1:] == ([n] if n else [])
        assert got["tm0"][1:] == got["tm1"][:-1]
        assert all(a < b for a, b in zip(got["tm0"], got["tm1"]))
        # a group without members has no tile at all
        for g, k in enumerate(case[0]):
            assert (got["at0"][g] == got["at1"][g]) == (k == 0)


def one(cut, n, tiling, ordered=0, sizes=None):
    return cut([(sizes or [n], tiling, 0, ordered, GS.NB)])[0]


def test_pairs_straddle_their_predicates(cut):
    L, F = FOLD
    # one tile against several
    assert one(cut, F, FOLD)["T"] == 1 and one(cut, F, FOLD)["single"] == [1]
    r = one(cut, F + 1, FOLD)
    assert r["T"] == GS.ceil_div(F + 1, L) and r["MG"] == 1
    assert set(r["single"]) == {0}
    # tile ends: L | L + 1 inside a large group
    assert r["tm1"][:2] == [L, 2 * L] and r["tm1"][-1] - r["tm0"][-1] == 1
    assert one(cut, F + L, FOLD)["T"] + 1 == one(cut, F + L + 1, FOLD)["T"]
    # ordered: one chain up to kOrderedFoldChunk
    assert one(cut, ORDERED[1], ORDERED, 1)["T"] == 1
    assert one(cut, ORDERED[1] + 1, ORDERED, 1)["T"] > 1
    # fold_ctx nonzero against 0, alone and beside small groups (one large
    # group switches the preload off for every group of the batch)
    m = GS.FOLD_CTX_MAX
    assert one(cut, m, ORDERED, 1)["fold_ctx"] == m
    assert one(cut, m + 1, ORDERED, 1)["fold_ctx"] == 0
    assert one(cut, 0, ORDERED, 1, [3, m, 1, 0, F])["fold_ctx"] == m
    assert one(cut, 0, ORDERED, 1, [3, m + 1, 1, 0, F])["fold_ctx"] == 0
    assert 0 < one(cut, F + 1, FOLD)["fold_ctx"] <= m
    # single-level against two-level
    n1 = C.kCombineL1 * L
    a, b = one(cut, n1, FOLD), one(cut, n1 + 1, FOLD)
    assert (a["max_chunks"], a["two_level"]) == (C.kCombineL1, 0)
    assert (b["max_chunks"], b["two_level"]) == (C.kCombineL1 + 1, 1)
    a, b = [one(cut, n, ROW) for n in GS.row_two_level()]
    assert (a["two_level"], b["two_level"]) == (0, 1)
    # 64 against fewer than 64 used slices, and the last slice short
    S = C.kCombineSlices
    n3 = 3 * S * L
    used = lambda t: GS.ceil_div(t, GS.slice_len(t))
    a, b = one(cut, n3, FOLD), one(cut, n3 + 1, FOLD)
    assert a["two_level"] and b["two_level"]
    assert used(a["T"]) == S and a["T"] % GS.slice_len(a["T"]) == 0
    assert used(b["T"]) < S and b["T"] % GS.slice_len(b["T"]) != 0
    assert GS.slice_len(b["T"]) == GS.slice_len(a["T"]) + 1
    assert used(one(cut, n1 + 1, FOLD)["T"]) < S
    # the row path's chunks and the ordered chain
    assert [one(cut, n, ROW)["T"] for n in GS.row_ladder()] == [1, 1, 2, 2, 3]
    assert one(cut, C.kOrderedChunk, ROW_ORDERED, 1)["T"] == 1
    assert one(cut, C.kOrderedChunk + 1, ROW_ORDERED, 1)["T"] == \
        GS.ceil_div(C.kOrderedChunk + 1, C.kChunk)
    # selections: the LDS sort's groups against the radix select's
    assert one(cut, C.SEL_K, ROW)["LG"] == 0
    assert one(cut, C.SEL_K + 1, ROW)["LG"] == 1
    r = one(cut, 0, ROW, 0, [C.SEL_K, C.SEL_K + 1])
    assert r["lgg"] == [1] and r["lgo"] == [C.SEL_K]


def test_mixed_batch_small_groups_are_in_the_two_level_set(cut):
    for sizes in (GS.mixed_sizes(), GS.mixed_large_first(),
                  GS.mixed_large_last()):
        r = one(cut, 0, FOLD, 0, sizes)
        assert r["two_level"] == 1
        small = [g for g, n in enumerate(sizes) if C.kFoldChunk < n <=
                 C.kCombineL1 * C.kFoldChunkLarge]
        assert small and set(small) <= set(r["mg"])
        # each of them fills fewer first-level slices than there are
        for g in small:
            assert r["at1"][g] - r["at0"][g] < C.kCombineSlices
        # member-less groups: in no list but ag, with an empty tile range
        for g, n in enumerate(sizes):
            if n == 0:
                assert g not in r["mg"] and g not in r["tg"]


def test_constants_are_the_sources():
    assert GS.mixed_sizes() == [1025, 0, 9, 33, 32, 0, 0, 1, 1537, 8, 0] or \
        (C.kFoldChunk, C.kFoldChunkLarge, C.kCombineL1, C.kCombineSlices) != \
        (32, 8, 128, 64)
    assert C.kFoldChunk >= C.SEL_K  # (engine.hip: the multi fold's condition)
    assert C.kFoldChunkLarge < C.kFoldChunk < GS.FOLD_CTX_MAX < \
        C.kOrderedFoldChunk <= C.kChunk < C.kOrderedChunk


# ---------------------------------------------------------------- b. the model
NAN = None          # a NaN value in the model
MUTANTS = ("tile_last_dropped", "tile_first_twice", "identity_zero",
           "identity_real", "slice_floor", "emit_first_tile",
           "empty_inherits", "sel_k_lt", "cand_from_members")
LERP_AGGS = ("sum", "avg", "min", "max", "diff", "dev")
ZIM_AGGS = ("zimsum", "count", "first", "last")


def exact_div(a, b):
    assert a % b == 0, "inexact quotient %d / %d" % (a, b)
    return a // b


def downsample(fn, vals):
    """One bucket's values (scaled integers or NAN, in time order)."""
    v = [x for x in vals if x is not NAN]
    if fn == "count":
        return len(v) * SC
    if fn in ("first", "last"):
        return vals[0] if fn == "first" else vals[-1]
    if not v:
        return NAN
    if fn == "sum":
        return sum(v)
    if fn == "avg":
        return exact_div(sum(v), len(v))
    if fn == "min":
        return min(v)
    if fn in ("max", "p90"):
        # the legacy percentile of one or two values at 90: the larger
        assert len(vals) <= 2
        return max(v)
    raise AssertionError(fn)


class Model:
    """One (batch, fill, downsampling function): the members' streams."""

    def __init__(self, built, fill, ds="sum", rate=False):
        self.b, self.fill, self.nb, self.rate = built, fill, built.nb, rate
        hb = built.batch
        self.start, self.end = GS.window(built, fill)
        iv = built.interval
        isf = hb.is_float
        self.kept = {}      # states(), per group
        self.streams = []   # per series: None (not kept) or {bucket: value}
        for s in range(hb.n_series):
            a, e = int(hb.offsets[s]), int(hb.offsets[s + 1])
            ts = hb.ts[a:e].tolist()
            if not ts or ts[0] > self.end or ts[-1] < self.start:
                self.streams.append(None)
                continue
            buckets = {}
            for i in range(a, e):
                t = int(hb.ts[i])
                if t < self.start:
                    continue
                if isf[i]:
                    f = float(hb.val[i:i + 1].view(np.float64)[0])
                    v = NAN if math.isnan(f) else int(f) * SC
                    assert v is NAN or f == int(f)
                else:
                    v = int(hb.val[i]) * SC
                buckets.setdefault((t - self.start) // iv, []).append(v)
            if built.raw:
                st = {k: downsample("sum", v) for k, v in buckets.items()}
                assert all(len(v) == 1 for v in buckets.values())
            else:
                st = {k: downsample(ds, v) for k, v in buckets.items()}
            if fill == "none":
                st = {k: v for k, v in st.items() if v is not NAN}
            else:
                fv = 0 if fill == "zero" else NAN
                st = {k: st.get(k, fv) for k in range(self.nb)}
            if rate:
                assert fill == "none"
                ks = sorted(st)
                r = {}
                for i, k in enumerate(ks):
                    if i == 0:
                        # the first rate is taken from (0, 0): 0 for a
                        # counter that starts at 0
                        assert st[k] == 0
                        r[k] = 0
                    else:
                        r[k] = exact_div(st[k] - st[ks[i - 1]],
                                         60 * (k - ks[i - 1]))
                st = r
            self.streams.append(st)

    def run_rate(self, agg, g):
        """The aggregation iterator over rates, slot by slot
        (AggregationIterator.java:395-797): a member's first rate, taken from
        the point (0, 0), goes straight to its current slot and is never
        emitted; a member without a rate at an emitted time gives the rate it
        holds (no interpolation of rates); a member whose stream has ended
        is cleared only from the previous emission's first member on."""
        hb = self.b.batch
        mem = hb.group_members[hb.group_offsets[g]:hb.group_offsets[g + 1]]
        its = [sorted(self.streams[s].items()) for s in mem.tolist()
               if self.streams[s] is not None]
        assert all(k < self.nb for it in its for k, _ in it)
        size = len(its)
        END = (1 << 62, None)
        at = [0] * size
        cur = [None] * size
        nxt = [it[0] if it else END for it in its]

        def move(i):
            cur[i] = nxt[i]
            at[i] += 1
            nxt[i] = its[i][at[i]] if at[i] < len(its[i]) else END
        for i in range(size):
            if nxt[i] is not END:
                if len(its[i]) > 1:
                    move(i)
                else:
                    nxt[i] = END
        ts, vals, current = [], [], 0
        while any(n is not END for n in nxt):
            for i in range(current, size):
                if nxt[i] is END:
                    cur[i] = None
            k = min(n[0] for n in nxt)
            current = [n[0] for n in nxt].index(k)
            for i in range(current, size):
                if nxt[i][0] == k:
                    move(i)
            ts.append(self.start + k * self.b.interval)
            vals.append(finish(agg, [c[1] for c in cur if c is not None]))
        return ts, vals

    def states(self, g):
        """Per bucket of the window, per member in order: None (not live),
        ("own", v) or ("lerp", v)."""
        if g in self.kept:
            return self.kept[g]
        hb = self.b.batch
        mem = hb.group_members[hb.group_offsets[g]:hb.group_offsets[g + 1]]
        out = self.kept[g] = [[None] * len(mem) for _ in range(self.nb)]
        for p, s in enumerate(mem.tolist()):
            st = self.streams[s]
            if not st:
                continue
            ks = sorted(st)
            for i, k in enumerate(ks):
                if k < self.nb:
                    out[k][p] = ("own", st[k])
                if i + 1 < len(ks):
                    k1 = ks[i + 1]
                    for x in range(k + 1, min(k1, self.nb)):
                        v0, v1 = st[k], st[k1]
                        if v0 is NAN or v1 is NAN:
                            v = NAN
                        else:
                            v = v0 + exact_div((x - k) * (v1 - v0), k1 - k)
                        out[x][p] = ("lerp", v)
        return out

    def run(self, agg, mutant=None, tiling=None):
        """[(ts list, value list)] per group; a NaN value is math.nan."""
        if self.rate:
            assert mutant is None
            return [self.run_rate(agg, g) for g in range(self.b.batch.n_groups)]
        hb = self.b.batch
        sizes = np.diff(hb.group_offsets).tolist()
        tiling = tiling or FOLD
        tiles = [GS.tiles_of(n, *tiling) for n in sizes]
        two = max([len(t) for t in tiles], default=0) > C.kCombineL1
        res, prev_emit = [], []
        for g, n in enumerate(sizes):
            st = self.states(g)
            ts, vals, emitted = [], [], []
            for b in range(self.nb):
                row = st[b]
                emit_from = row
                if mutant == "emit_first_tile" and tiles[g]:
                    emit_from = row[:tiles[g][0][1]]
                emit = any(x is not None and x[0] == "own" for x in emit_from)
                if mutant == "empty_inherits" and n == 0 and g > 0:
                    if b in prev_emit:
                        ts.append(self.start + b * self.b.interval)
                        vals.append(0.0)
                        emitted.append(b)
                    continue
                if not emit:
                    continue
                if mutant == "sel_k_lt" and agg in GS.SEL_AGGS and \
                        n == C.SEL_K:
                    continue
                v = aggregate(agg, row, mutant, tiles[g], two)
                if v is None:
                    continue
                ts.append(self.start + b * self.b.interval)
                vals.append(v)
                emitted.append(b)
            prev_emit = emitted
            res.append((ts, vals))
        return res


def slices_of(tiles, floor=False):
    """The first-level slices of a multi-tile group: member ranges, the empty
    ones included."""
    T, S = len(tiles), C.kCombineSlices
    ls = T // S if floor else GS.ceil_div(T, S)
    out = []
    for sl in range(S):
        a, e = sl * ls, min((sl + 1) * ls, T)
        out.append((tiles[a][0], tiles[e - 1][1]) if a < e else None)
    return out


def aggregate(agg, row, mutant, tiles, two):
    """One (group, bucket): the aggregator looped over the members in order."""
    multi = len(tiles) > 1
    parts = None  # the member ranges whose partials the combine merges
    if multi:
        parts = slices_of(tiles, mutant == "slice_floor") if two else tiles
    keep = list(range(len(row)))
    if multi and mutant == "tile_last_dropped":
        drop = {m1 - 1 for m0, m1 in tiles[:-1]}
        keep = [p for p in keep if p not in drop]
    if multi and mutant == "tile_first_twice":
        keep = sorted(keep + [m0 for m0, m1 in tiles[1:]])
    if multi and two and mutant == "slice_floor":
        covered = [r for r in parts if r is not None]
        top = covered[-1][1] if covered else 0
        keep = [p for p in keep if p < top]
    live = [(p, row[p]) for p in keep if row[p] is not None]
    if not live:
        return None  # (a mutant that lost every member: nothing emitted)
    if agg in LERP_AGGS or agg in GS.SEL_AGGS:
        vals = [x[1] for _, x in live]
    elif agg in ZIM_AGGS:
        vals = [x[1] if x[0] == "own" else 0 for _, x in live]
    else:  # mimmin / mimmax: a missing value never wins
        assert agg in ("mimmin", "mimmax")
        vals = [x[1] for _, x in live if x[0] == "own"]
    if multi and mutant in ("identity_zero", "identity_real"):
        # the parts with no live member: their identity partial mistaken
        dead = [r is None or not any(row[p] is not None
                                     for p in range(r[0], r[1]))
                for r in parts]
        if mutant == "identity_zero" and any(dead) and \
                agg in ("min", "max", "mimmin", "mimmax"):
            vals = vals + [0]
        if mutant == "identity_real" and agg == "first" and dead[0]:
            vals = [0] + vals
        if mutant == "identity_real" and agg == "last" and dead[-1]:
            vals = vals + [0]
    return finish(agg, vals, mutant)


def percentile(a, n, percent):
    """commons-math3 Percentile.evaluate, LEGACY estimation, on the sorted
    doubles a with n taken as the count."""
    if n == 1:
        return a[0]
    p = percent / 100.0
    pos = 0 if p == 0.0 else (float(n) if p == 1.0 else p * float(n + 1))
    fpos = math.floor(pos)
    if pos < 1:
        return a[0]
    if pos >= n:
        return a[min(n, len(a)) - 1]
    top = len(a) - 1
    lower, upper = a[min(int(fpos) - 1, top)], a[min(int(fpos), top)]
    return lower + (pos - fpos) * (upper - lower)


PCT = {"p50": 50.0, "p99": 99.0, "p999": 99.9, "ep95r3": 95.0}


def finish(agg, vals, mutant=None):
    v = [x for x in vals if x is not NAN]
    n_all = len(vals)
    if agg == "count":
        return float(len(v))
    if agg in ("first", "last"):
        x = vals[0] if agg == "first" else vals[-1]
        return math.nan if x is NAN else x / SC
    if not v:
        return math.nan
    if agg in ("sum", "zimsum"):
        return sum(v) / SC
    if agg == "avg":
        s = sum(v) / SC
        assert s == sum(v) / SC and abs(sum(v)) < 2**53
        return s / float(len(v))
    if agg in ("min", "mimmin"):
        return min(v) / SC
    if agg in ("max", "mimmax"):
        return max(v) / SC
    if agg == "diff":
        return 0.0 if len(v) == 1 else v[-1] / SC - v[0] / SC
    if agg == "dev":
        if len(v) == 1:
            return 0.0
        old, m2, n = v[0] / SC, 0.0, 2
        for x in v[1:]:
            x = x / SC
            new = old + (x - old) / float(n)
            m2 += (x - old) * (x - new)
            old = new
            n += 1
        return math.sqrt(m2 / float(n - 1))
    a = sorted(x / SC for x in v)
    n = n_all if mutant == "cand_from_members" else len(a)
    if agg == "median":
        return a[min(n // 2, len(a) - 1)]
    return percentile(a, n, PCT[agg])


def as_model(ref):
    """The oracle's groups as the model writes them."""
    from tests.test_gpu_parity import _vals
    return [(r["ts"].tolist(), _vals(r["bits"], r["is_int"]).tolist())
            for r in ref]


def differs(a, b):
    """None, or where two results differ: emission, then value bits (a ±0.0
    by value, the percentiles' rule of test_gpu_value_domain.py)."""
    for g, ((ta, va), (tb, vb)) in enumerate(zip(a, b)):
        if ta != tb:
            return "g%d: emission %s vs %s" % (g, ta[:8], tb[:8])
        for t, x, y in zip(ta, va, vb):
            if math.isnan(x) != math.isnan(y) or (
                    not math.isnan(x) and x != y):
                return "g%d @%d: %r vs %r" % (g, t, x, y)
    return None


def pinned(b, aggs, fills, ds="sum", rate=False, where=""):
    for fill in fills:
        m = Model(b, fill, ds, rate)
        for agg in aggs:
            ref = pyoracle.group_by(GS.spec_of(b, agg, ds, fill, rate), b.batch)
            d = differs(m.run(agg), as_model(ref))
            assert d is None, "%s/%s:%s-%s: %s" % (where, agg, ds, fill, d)


@pytest.mark.parametrize("n", GS.fold_ladder())
def test_oracle_is_the_model_fold_ladder(n):
    for name, b in GS.fold_batches(n):
        pinned(b, GS.FOLD_AGGS, GS.FILLS, where="%d/%s" % (n, name))


@pytest.mark.parametrize("n", GS.ordered_ladder())
def test_oracle_is_the_model_ordered(n):
    for name, b in GS.ordered_batches(n):
        pinned(b, ("dev",), GS.FILLS, where="dev/%d/%s" % (n, name))


def test_oracle_is_the_model_mixed_batches():
    for name, b in GS.mixed_batches():
        pinned(b, GS.FOLD_AGGS + ("dev",), GS.FILLS, where=name)
        pinned(b, ("sum", "max"), GS.FILLS, ds="avg", where=name)
    # all doubles: the form the device encoder takes
    for name, b in GS.mixed_batches("double"):
        pinned(b, GS.FOLD_AGGS + ("dev",), GS.FILLS, where=name + "/double")


@pytest.mark.parametrize("n", GS.row_ladder())
def test_oracle_is_the_model_row_path(n):
    pinned(GS.single(n, counter=True), GS.ROW_AGGS, ("none",), ds="max",
           rate=True, where="rate/%d" % n)
    for name, b in GS.row_batches(n):
        pinned(b, GS.ROW_AGGS, GS.FILLS, ds="p90",
               where="p90/%d/%s" % (n, name))


@pytest.mark.parametrize("n", GS.row_two_level())
def test_oracle_is_the_model_row_two_level(n):
    pinned(GS.single(n, nb=2), ("sum", "min", "first", "last"), ("none",),
           ds="p90", where="p90/%d" % n)


@pytest.mark.parametrize("n", [C.kOrderedChunk, C.kOrderedChunk + 1])
def test_oracle_is_the_model_long_chain(n):
    pinned(GS.single(n, nb=2), ("dev",), ("none",), where="dev/%d" % n)


def selection_batches():
    out = [(str(n), GS.selection_group(n)) for n in GS.selection_ladder()]
    out.append(("both", GS.build(GS.groups_of([C.SEL_K, C.SEL_K + 1]),
                                 form="double")))
    out.append(("ss_cap", GS.ss_cap_batch()))
    return out


def test_oracle_is_the_model_selections():
    for name, b in selection_batches():
        pinned(b, GS.SEL_AGGS, GS.SEL_FILLS, where="sel/" + name)


def test_ss_cap_batch_sits_on_the_cap():
    b = GS.ss_cap_batch()
    m = Model(b, "none")
    n = [sum(1 for x in row if x is not None and x[1] is not NAN)
         for row in m.states(0)]
    assert n == [C.SS_CAP, C.SS_CAP + 1]


@pytest.mark.parametrize("form", ["long", "double"])
def test_oracle_is_the_model_raw(form):
    b = GS.build(GS.groups_of(GS.raw_sizes()), form=form, raw=True)
    pinned(b, GS.RAW_AGGS, ("none",), where="raw/" + form)


# ------------------------------------------------------------- c. the mutants
def mutant_cases():
    """(where, Built, aggs, fills): the fold ladder's two-level rungs and
    tile edges, the mixed batches and the selections."""
    L, F = FOLD
    out = []
    for n in (F + 1, F + L + 1, C.kCombineL1 * L + 1,
              3 * C.kCombineSlices * L + 1):
        for name, b in GS.fold_batches(n):
            out.append(("%d/%s" % (n, name), b, GS.FOLD_AGGS, GS.FILLS))
    for name, b in GS.mixed_batches():
        out.append((name, b, GS.FOLD_AGGS, GS.FILLS))
    for name, b in selection_batches():
        out.append(("sel/" + name, b, GS.SEL_AGGS, GS.SEL_FILLS))
    return out


@pytest.fixture(scope="module")
def truth():
    out = []
    for w, b, aggs, fills in mutant_cases():
        models = {f: Model(b, f) for f in fills}
        base = {(f, a): models[f].run(a) for f in fills for a in aggs}
        out.append((w, b, aggs, fills, models, base))
    return out


@pytest.mark.parametrize("mutant", MUTANTS)
def test_the_batches_catch(truth, mutant):
    caught = []
    for w, b, aggs, fills, models, base in truth:
        for f in fills:
            for agg in aggs:
                d = differs(models[f].run(agg, mutant), base[f, agg])
                if d is not None:
                    caught.append("%s/%s-%s: %s" % (w, agg, f, d))
    assert caught, mutant + ": no case tells it from the true model"
    if mutant in ("identity_zero",):
        # a minimum and a maximum each, under both fills
        for agg in ("min", "max"):
            for f in GS.FILLS:
                assert any("/%s-%s:" % (agg, f) in c for c in caught), (agg, f)
    if mutant == "identity_real":
        assert any("/first-" in c for c in caught)
        assert any("/last-" in c for c in caught)
    if mutant in ("tile_last_dropped", "tile_first_twice"):
        # seen by a plain batch too: no quiet member is needed
        assert any("/plain/" in c for c in caught)
