"""highestMax / highestCurrent (N = 10) over the result of a bench query that
stays in HBM, timed by the engine's own stage events (otsdb_prof_*: [13] the
top-N call from numbering to gather, [4] the producing query's output
compaction).

    python -m scripts.topn_probe [--series 100000] [--named] [--reps 7]
        [--warmup 2] [--topn 10] [--out profiles/topn_probe.json]

The producing query is bench.py's C2 (zimsum:5m-avg{host=*}: series / 10
groups x 2,017 buckets) or, with --named, its named query
(sum:1m-avg{host=*}, 10,081 buckets a group).  Reported per function: the
top-N stage's median and range on the grid path and (--general) on the
general path, the producing query's compaction stage beside it, and the bytes a host
entry copies back before (every group) and after (the picked series, their
numbers and keys).  --series scales the producing query down; the library is
abi.LIB_PATH (OTSDB_LIB points a run at another build for the compaction
stage alone: --compact-only)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--series", type=int, default=100000)
    ap.add_argument("--named", action="store_true")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--topn", type=int, default=10)
    ap.add_argument("--compact-only", action="store_true")
    ap.add_argument("--general", action="store_true",
                    help="time the general path too (no promise): choose "
                         "--series so that it ends in about a second")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import bench
    from opentsdb_amd import core, workload
    from opentsdb_amd.engine import (DeviceResult, DeviceTopN, Engine,
                                     run_device, run_topn_device)
    eng = Engine(0)
    g = workload.gen_spec("C2")
    db = workload.generate_device(eng, g, 0, a.series, config="C2")
    spec = bench.named_spec("C2") if a.named else workload.query_spec("C2")
    ds = "1m-avg" if a.named else workload.CONFIGS["C2"]["ds"]
    sz = eng.plan(spec, db)
    res = DeviceResult(torch, db.n_groups, int(sz.max_out_points), "cuda")
    assert eng.lib.otsdb_prof_enable(eng.ctx, 1) == 0

    def stages():
        ms = (C.c_double * 14)()
        cnt = (C.c_int64 * 14)()
        assert eng.lib.otsdb_prof_read(eng.ctx, ms, cnt, 14, 1) == 0
        return list(ms)

    compact = []
    for i in range(a.warmup + max(a.reps, 3)):
        run_device(eng, spec, db, res)
        st = stages()
        if i >= a.warmup:
            compact.append(st[4])
    points = int(res.offsets[-1].item())
    G = db.n_groups
    med = statistics.median
    line = dict(query=("sum:1m-avg{host=*}" if a.named else
                       "zimsum:5m-avg{host=*}") + " over %d series x 7 d" % a.series,
                groups=G, result_points=points, buckets=int(sz.n_buckets),
                reps=len(compact), warmup=a.warmup,
                compact_stage_ms=dict(median=med(compact), min=min(compact),
                                      max=max(compact)),
                d2h_bytes_every_group=17 * points + 8 * (G + 1))
    if not a.compact_only:
        start, end = spec.query_start_ms, spec.query_end_ms
        grid = core.topn_grid_interval_ms(ds)
        paths = [("grid", grid)] + ([("general", 0)] if a.general else [])
        for fn, (path, promise) in [(f, p) for f in ("highestMax",
                                                     "highestCurrent")
                                    for p in paths]:
            dtop = DeviceTopN(torch, a.topn, points, "cuda")
            t = []
            for i in range(a.warmup + max(a.reps, 3)):
                run_topn_device(eng, fn, a.topn, start, end, [res], dtop,
                                grid_interval_ms=promise)
                st = stages()
                if i >= a.warmup:
                    t.append(st[13])
            picked_points = int(dtop.offsets[dtop.n_picked].item())
            line[fn + "_" + path] = dict(
                path=eng.topn_counters(), topn=a.topn,
                stage_ms=dict(median=med(t), min=min(t), max=max(t)),
                over_compact_stage=med(t) / med(compact),
                picked=dtop.picked[:dtop.n_picked].tolist(),
                picked_points=picked_points,
                d2h_bytes_picked=17 * picked_points + 8 * (dtop.n_picked + 1)
                + 16 * dtop.n_picked)
    print(json.dumps(line), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(json.dumps(line) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
