"""The ordered fold's launch plan (csrc/foldplan.h: fold_plan, fold_tiling)
compiled alone for the host, with the address and undefined-behaviour
sanitizers, and compared with a restatement of the rule in Python.  The plan
decides how many workgroups a fold gets (window narrowing) and whether a tile
preloads its member contexts; no query's result depends on it, so only this
test sees it drift between the single and the multi-aggregator fold or change
under a later edit.  Default tuning constants: no -D is passed."""
import itertools
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "opentsdb_amd", "csrc")

# stdin: one case a line, "T NB cap may_narrow ordered n k_1 .. k_n" (k: the
# groups' member counts); stdout: "WB NW fold_wb fold_ctx chunk whole_upto"
DRIVER = r"""
#include <cstdio>
#include "foldplan.h"
int main() {
  long long T, NB, cap;
  int narrow, ordered, n;
  while (scanf("%lld %lld %lld %d %d %d", &T, &NB, &cap, &narrow, &ordered,
               &n) == 6) {
    std::vector<int64_t> goff{0};
    for (int i = 0; i < n; ++i) {
      long long k;
      if (scanf("%lld", &k) != 1) return 2;
      goff.push_back(goff.back() + k);
    }
    if (n == 0) goff.clear();  // no groups at all: not even the leading 0
    const otsdb::FoldPlan p =
        otsdb::fold_plan(goff, T, NB, cap, ordered != 0, narrow != 0);
    const otsdb::FoldTiling t = otsdb::fold_tiling(ordered != 0);
    printf("%lld %lld %d %d %lld %lld\n", (long long)p.WB, (long long)p.NW,
           (int)p.fold_wb, (int)p.fold_ctx, (long long)t.chunk,
           (long long)t.whole_upto);
  }
  return 0;
}
"""

MIN_BLOCKS, MIN_WINDOW = 1024, 128
CHUNK, CHUNK_LARGE, ORDERED_CHUNK = 32, 8, 256

TS = (0, 1, 7, 8, 9, 100, 300, 1023, 1024, 1025)
NBS = (1, 127, 128, 129, 1023, 1024, 1025, 2047, 2048, 2049, 10081)
CAPS = (1024, 2048)
GROUPS = ((), (0,), (1,), (10, 10), (32,), (33,), (32, 700), (64, 3), (65,),
          (256,), (257,), (0, 0, 5))


def ceil_div(a, b):
    return -(-a // b)


def plan_windows(T, NB, cap, narrow):
    """(WB, NW, fold_wb): the window rule restated."""
    WB, fold_wb = cap, 0
    NW = ceil_div(NB, WB)
    if narrow and T > 0 and NB > MIN_WINDOW and T * NW < MIN_BLOCKS:
        want = ceil_div(MIN_BLOCKS, T)
        wb = max(ceil_div(ceil_div(NB, want), 64) * 64, MIN_WINDOW)
        if wb < WB:
            WB = fold_wb = wb
    return WB, ceil_div(NB, WB), fold_wb


def plan_ctx(groups, ordered):
    per = [min(k, ORDERED_CHUNK) if ordered
           else (k if k <= CHUNK else min(k, CHUNK_LARGE)) for k in groups]
    m = max(per, default=0)
    return m if 1 <= m <= 64 else 0


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ absent")
    d = tmp_path_factory.mktemp("foldplan")
    src = d / "plan.cc"
    src.write_text(DRIVER)
    exe = d / "plan"
    subprocess.run(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-Wall", "-Werror",
                    "-I", CSRC, "-o", str(exe), str(src)], check=True)

    def run(cases):
        """cases: (T, NB, cap, narrow, ordered, groups) -> 6-tuples."""
        text = "".join("%d %d %d %d %d %d %s\n" % (
            T, NB, cap, narrow, ordered, len(g), " ".join(map(str, g)))
            for T, NB, cap, narrow, ordered, g in cases)
        r = subprocess.run([str(exe)], input=text, capture_output=True,
                           text=True)
        assert r.returncode == 0, r.stderr
        rows = [tuple(map(int, ln.split())) for ln in r.stdout.splitlines()]
        assert len(rows) == len(cases)
        return rows
    return run


def test_windows_match_the_rule(plan):
    cases = [(T, NB, cap, narrow, 0, (10, 10)) for T, NB, cap, narrow in
             itertools.product(TS, NBS, CAPS, (1, 0))]
    for case, got in zip(cases, plan(cases)):
        T, NB, cap, narrow = case[:4]
        WB, NW, fold_wb = got[:3]
        assert (WB, NW, fold_wb) == plan_windows(T, NB, cap, narrow), case
        assert NW == ceil_div(NB, WB) and NW * WB >= NB, case
        assert fold_wb in (0, WB), case
        if fold_wb:
            assert fold_wb % 64 == 0 and 128 <= fold_wb < cap and narrow, case
        else:
            assert WB == cap, case
        assert got[3] == 10, case  # the windows do not touch the contexts


def test_windows_pinned(plan):
    pinned = {
        (100, 1440, 2048, 1): (192, 8, 192),
        (100, 1440, 1024, 1): (192, 8, 192),
        (1, 129, 2048, 1): (128, 2, 128),
        (1, 128, 2048, 1): (2048, 1, 0),
        (1024, 4096, 2048, 1): (2048, 2, 0),
        (300, 2049, 2048, 1): (576, 4, 576),
        (300, 2049, 1024, 1): (576, 4, 576),
        (1, 2049, 1024, 1): (128, 17, 128),
        (8, 1025, 1024, 1): (128, 9, 128),
        (1, 10081, 2048, 1): (128, 79, 128),
        (100, 1440, 2048, 0): (2048, 1, 0),
    }
    cases = [k + (0, (10, 10)) for k in pinned]
    for case, got in zip(cases, plan(cases)):
        assert got[:3] == pinned[case[:4]], case


def test_member_contexts(plan):
    # the windows' inputs vary too: the contexts do not depend on them
    cases = [(T, NB, 2048, narrow, ordered, g)
             for g in GROUPS for ordered in (0, 1)
             for T, NB, narrow in ((len(g), 1440, 1), (0, 1, 0), (1025, 2049, 1))]
    for case, got in zip(cases, plan(cases)):
        ordered, g = case[4], case[5]
        assert got[3] == plan_ctx(g, ordered), case
        assert 0 <= got[3] <= 64, case
        assert got[:3] == plan_windows(*case[:4]), case
        # the tiling the contexts are stated for
        assert got[4:] == ((32, 256) if ordered else (8, 32)), case
    pinned = {(0, (10, 10)): 10, (0, (33,)): 8, (0, (32, 700)): 32,
              (1, (65,)): 0, (1, (64, 3)): 64, (1, (257,)): 0}
    for (ordered, g), want in pinned.items():
        assert plan_ctx(g, ordered) == want
        assert plan([(len(g), 1440, 2048, 1, ordered, g)])[0][3] == want
