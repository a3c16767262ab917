"""The multi-aggregator fold (OTSDB_SPEC_MULTI_FOLD) against the row path, on
the BASELINE shapes.

    python -m scripts.multi_fold_probe --parent-lib PATH
        [--cases C2:min,avg,max ...] [--reps 20] [--warmup 3] [--series N]
        [--out profiles/multi_fold_probe.json]

--parent-lib: libotsdb_agg.so built from the parent commit (the row path:
it does not know the flag).  Per case three calls alternate in one process,
each timed synchronously:
  fold     run_multi_device(..., fold=True) on this tree's library;
  rows     the same multi call on the parent library (baseline i);
  singles  the same aggregators as back-to-back single queries on the
           parent library (baseline ii).
Reported: the median of the repetitions with min / max, and DESIGN.md
§4.2's routing rule — the fold "wins" a shape only if its median is below
baseline (i)'s by more than (i)'s own min - max spread.  For C2 the fold
kernel's HIP-event time (stage 0 of otsdb_prof_read) is recorded beside
k_fold's of a single query in the same run.  One JSON line per case.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CASES = ["C2:min,avg,max", "C2:min,avg,max,sum", "C3:min,avg,max",
         "C3:min,avg,max,sum", "C5:min,avg,max", "C5:min,avg,max,sum"]


def with_agg(spec, agg):
    from opentsdb_amd import core
    s = type(spec).from_buffer_copy(spec)
    s.agg_id = core.Aggregators.get(agg).id
    s.interp = -1
    return s


def engine_on(path):
    """An Engine over another build of the library."""
    from opentsdb_amd import abi
    from opentsdb_amd.engine import Engine
    e = Engine.__new__(Engine)
    e.lib = abi.load(path)
    e.ctx = C.c_void_p()
    e._check(e.lib.otsdb_ctx_create(0, C.byref(e.ctx)))
    e.device = 0
    return e


def stage0_ms(eng, fn, reps):
    """Mean HIP-event time of stage 0 (the downsample / fold kernel) over
    `reps` calls of fn."""
    import torch
    eng.lib.otsdb_prof_enable(eng.ctx, 1)
    eng.lib.otsdb_prof_read(eng.ctx, None, None, 0, 1)
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    ms = (C.c_double * 8)()
    nn = (C.c_int64 * 8)()
    eng.lib.otsdb_prof_read(eng.ctx, ms, nn, 8, 1)
    eng.lib.otsdb_prof_enable(eng.ctx, 0)
    return ms[0] / max(int(nn[0]), 1)


def probe(eng, par, config, aggs, db, n_series, warm, reps):
    import torch
    from opentsdb_amd import workload
    from opentsdb_amd.engine import DeviceResult, run_device, run_multi_device
    spec = workload.query_spec(config)
    sz = eng.plan_multi(spec, aggs, db)
    n = len(aggs)

    def results():
        return [DeviceResult(torch, db.n_groups, int(sz.max_out_points), "cuda")
                for _ in aggs]
    r_fold, r_rows, r_one = results(), results(), results()
    specs = [with_agg(spec, a) for a in aggs]

    def fold():
        run_multi_device(eng, spec, aggs, db, r_fold, fold=True)

    def rows():
        run_multi_device(par, spec, aggs, db, r_rows)

    def singles():
        for i in range(n):
            run_device(par, specs[i], db, r_one[i])

    def timed(fn):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3

    for _ in range(warm):
        fold()
        rows()
        singles()
    torch.cuda.synchronize()
    t = dict(fold=[], rows=[], singles=[])
    for _ in range(reps):
        t["fold"].append(timed(fold))
        t["rows"].append(timed(rows))
        t["singles"].append(timed(singles))
    fold()
    launches = eng.multi_fold_counters()["fold_launches"]
    counters = eng.multi_counters()
    # the three must agree before their times are compared: the same points,
    # values within 1e-12 (sum / avg downsampling: another step alignment)
    same = True
    worst = 0.0
    for i in range(n):
        k = int(r_one[i].offsets[-1].item())
        same = same and torch.equal(r_fold[i].offsets, r_one[i].offsets)
        same = same and torch.equal(r_fold[i].ts[:k], r_one[i].ts[:k])
        a = r_fold[i].val[:k].view(torch.float64)
        b = r_one[i].val[:k].view(torch.float64)
        ok = ~(a.isnan() & b.isnan())
        if k and bool(ok.any()):
            rel = ((a[ok] - b[ok]).abs() / b[ok].abs().clamp(min=1e-300)).max()
            worst = max(worst, float(rel))

    def stat(x):
        return dict(median=statistics.median(x), min=min(x), max=max(x))
    s = {k: stat(v) for k, v in t.items()}
    spread = s["rows"]["max"] - s["rows"]["min"]
    line = dict(config=config, aggs=aggs, series=n_series,
                points=int(db.n_points_total), groups=int(db.n_groups),
                buckets=int(sz.n_buckets), reps=reps, fold_ms=s["fold"],
                rows_ms=s["rows"], singles_ms=s["singles"],
                rows_spread_ms=spread,
                fold_wins=bool(s["fold"]["median"] <
                               s["rows"]["median"] - spread),
                fold_launches=launches, counters=counters,
                same_points=bool(same), worst_rel_diff_vs_singles=worst)
    if config == "C2":
        line["k_fold_multi_event_ms"] = stage0_ms(eng, fold, 5)
        line["k_fold_event_ms"] = stage0_ms(
            eng, lambda: run_device(eng, specs[0], db, r_one[0]), 5)
    print(json.dumps(line), flush=True)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--cases", nargs="*", default=CASES)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--series", type=int, default=0,
                    help="series per case (default: the config's per GPU)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from opentsdb_amd import build, workload
    from opentsdb_amd.engine import Engine
    build.build()
    eng = Engine(0)
    par = engine_on(a.parent_lib)
    lines = []
    have, db = None, None
    for case in a.cases:
        config, aggs = case.split(":")
        n = a.series or workload.default_series_per_gpu(config)
        if have != config:  # one generated batch for the cases of a config
            db = None
            torch.cuda.empty_cache()
            db = workload.generate_device(eng, workload.gen_spec(config), 0,
                                          n, config=config)
            have = config
        lines.append(probe(eng, par, config, aggs.split(","), db, n,
                           a.warmup, max(a.reps, 1)))
        torch.cuda.empty_cache()
        if a.out:  # (after every case: a long run leaves what it measured)
            with open(a.out, "w") as f:
                for ln in lines:
                    f.write(json.dumps(ln) + "\n")
    par.close()
    eng.close()


if __name__ == "__main__":
    main()
