"""Builds libotsdb_agg.so (the HIP engine + C-ABI) for gfx950 in-tree.

hipcc cross-compiles without a GPU, so this runs in the CPU container; the
resulting .so travels to the GPU box with the repository snapshot.

The library links 28 translation units compiled in parallel (UNIT_FILES
below names each kind's source and every csrc file it includes; a unit is
rebuilt when one of those, or include/otsdb_agg.h, is newer than its object):

- three engine units with the host code and the C-ABI: csrc/engine.hip (the
  context, planning, the pipeline, multi / panel / cells / selection queries,
  the non-template kernels of kernels.hip and the aggregator-templated ones),
  csrc/engine_rows.hip (storage rows and rollup rows: rows.hip,
  rollup_rows.hip) and csrc/engine_hist.hip (histogram queries: hist.hip,
  hist_rows.hip);
  csrc/engine_int.h is what they share;
- two units per downsampling monoid (csrc/ds_tu.hip with -DOTSDB_DS_MONOID=n:
  the downsample / ordered-fold kernels of that monoid, and with
  -DOTSDB_DS_PART=1 the cells fold of that monoid);
- csrc/rollup.hip (the prep and ring kernels of the two rollup states).

Build times on one 8-core machine, each one run.  Clean (force=True): 320 s,
taken right after the preceding commit's 325 s (that commit, with engine.hip
as the one engine unit, took 293 - 325 s over three runs as the machine
drifted).  After touching one file: engine_hist.hip 3 s, engine_rows.hip
26 s, engine.hip 40 s, against 68 s for the one engine.hip before.
"""
import glob
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
DEPS = sorted(glob.glob(os.path.join(CSRC, "*.hip")) +
              glob.glob(os.path.join(CSRC, "*.h"))) + [
    os.path.join(ROOT, "include", "otsdb_agg.h")]
OUT_DIR = os.path.join(HERE, "_build")
OUT = os.path.join(OUT_DIR, "libotsdb_agg.so")
ARCH = os.environ.get("OTSDB_OFFLOAD_ARCH", "gfx950")
N_DS_MONOIDS = 12  # dispatch.h with_monoid: distinct reduction state types
HIPCC = "/opt/rocm/bin/hipcc"

# Every kind of unit: its source, then every csrc file that source includes,
# directly or through another (tests/test_build_units_cpu.py holds the rows
# to the #include lines).  A unit is rebuilt when one of its own files, or
# include/otsdb_agg.h, is newer than its object.
_SHARED = ("kernels.hip", "kernels.h", "monoids.h", "rollup_monoids.h",
           "launch.h", "dispatch.h")
_DS = ("ds_tu.hip", "decode.hip", "fold.hip", "foldmulti.hip",
       "menv.h") + _SHARED
UNIT_FILES = {
    "engine": ("engine.hip", "engine_int.h", "compact.hip", "select.hip",
               "decode.hip", "raw.hip", "calendar.hip", "multi.hip",
               "panel.hip", "topn.hip", "foldplan.h", "menv.h") + _SHARED,
    "engine_rows": ("engine_rows.hip", "engine_int.h", "decode.hip",
                    "rows.hip", "rollup_rows.hip") + _SHARED,
    "engine_hist": ("engine_hist.hip", "engine_int.h", "compact.hip",
                    "hist.hip", "hist_rows.hip", "histplan.h") + _SHARED,
    "rollup": ("rollup.hip",) + _SHARED,
    "ds": _DS,                          # ds_tu.hip, -DOTSDB_DS_PART=0
    "cells": _DS + ("cellfold.hip",),   # ds_tu.hip, -DOTSDB_DS_PART=1
}
ENGINE_UNITS = ("engine", "engine_rows", "engine_hist")

FLAGS = [
    "--offload-arch=" + ARCH, "-O3", "-std=c++17", "-fPIC",
    # Java rounds every multiply and add separately: no FMA contraction
    "-ffp-contract=off",
    "-Wall", "-Wno-unused-variable", "-Wno-unused-lambda-capture",
    "-Wno-unused-function", "-Wno-unused-value", "-Wno-unused-result",
]


def up_to_date(out=OUT):
    if not os.path.exists(out):
        return False
    t = os.path.getmtime(out)
    return all(os.path.getmtime(d) <= t for d in DEPS)


def _units(out_dir, defines):
    """(source, flags, object, kind) of every unit: the engine units first,
    then the longest (part 1, the cells fold: cellfold.hip)."""
    d = ["-D" + x for x in defines]
    units = [(os.path.join(CSRC, UNIT_FILES[k][0]), d,
              os.path.join(out_dir, k + ".o"), k)
             for k in ENGINE_UNITS + ("rollup",)]
    for part, kind in ((1, "cells"), (0, "ds")):
        for m in range(N_DS_MONOIDS):
            units.append((os.path.join(CSRC, "ds_tu.hip"),
                          d + ["-DOTSDB_DS_MONOID=%d" % m,
                               "-DOTSDB_DS_PART=%d" % part],
                          os.path.join(out_dir, "ds_%d_%d.o" % (part, m)),
                          kind))
    return units


def build(force=False, verbose=False, jobs=None, defines=(), out=None):
    """defines / out: a debug or tuning variant (extra -D flags) built into
    its own directory next to the production library."""
    out_dir = OUT_DIR
    if out:
        out_dir = os.path.dirname(out)
    OUT_ = out or OUT
    if not force and up_to_date(OUT_):
        return OUT_
    os.makedirs(out_dir, exist_ok=True)
    jobs = jobs or min(8, os.cpu_count() or 1)

    def compile_unit(u):
        src, extra, obj, _ = u
        cmd = [HIPCC] + FLAGS + extra + ["-c", "-o", obj + ".tmp", src]
        if verbose:
            print(" ".join(cmd), flush=True)
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           text=True)
        if r.returncode != 0:
            raise RuntimeError("compile failed: %s\n%s" % (" ".join(cmd),
                                                           r.stdout))
        if r.stdout.strip() and verbose:
            print(r.stdout, flush=True)
        os.replace(obj + ".tmp", obj)
        return obj

    units = _units(out_dir, defines)

    def stale(u):
        obj, kind = u[2], u[3]
        if force or not os.path.exists(obj):
            return True
        t = os.path.getmtime(obj)
        deps = [os.path.join(CSRC, f) for f in UNIT_FILES[kind]] + [DEPS[-1]]
        return any(os.path.getmtime(d) > t for d in deps)

    # longest first (a cells unit takes ~2 min of one core, a ds unit ~1 min,
    # engine.hip 40 s, engine_rows.hip 30 s, the rest seconds): the short ones
    # fill the pool's tail
    order = ("cells", "engine", "ds", "engine_rows", "rollup", "engine_hist")
    todo = sorted((u for u in units if stale(u)),
                  key=lambda u: order.index(u[3]))
    with ThreadPoolExecutor(jobs) as ex:
        list(ex.map(compile_unit, todo))
    objs = [u[2] for u in units]
    cmd = [HIPCC, "--offload-arch=" + ARCH, "-shared", "-fPIC", "-o",
           OUT_ + ".tmp"] + objs
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    os.replace(OUT_ + ".tmp", OUT_)
    return OUT_


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
