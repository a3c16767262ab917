"""The cells multi-aggregator fold (OTSDB_SPEC_CELLS_MULTI_FOLD) against the
cells row path, on the BASELINE shapes from compacted cells.

    python -m scripts.cells_multi_fold_probe --parent-lib PATH
        [--cases C2:min,avg,max ...] [--reps 20] [--warmup 3] [--series N]
        [--days D] [--out profiles/cells_multi_fold_probe.json]

--parent-lib: libotsdb_agg.so built from the parent commit (it does not know
the bit).  Each shape is generated columnar, encoded to cells on the device
and the columnar copy dropped (as scripts/cells_panel_probe.py).  Per case
three calls alternate in one process, each timed synchronously:
  fold     run_cells_multi_device(..., fold=True) on this tree's library;
  rows     the same cells multi call on the parent library (baseline i);
  singles  the same aggregators as back-to-back run_cells_device calls on
           the parent library (baseline ii).
Reported: the median of the repetitions with min / max, and DESIGN.md §4.2's
routing rule — the fold "wins" a shape only if its median is below baseline
(i)'s by more than (i)'s own min - max spread.  For C2 the engine's stages by
HIP events (otsdb_prof_read; stage 0 holds k_fold_multi<cells>) are recorded
for the flagged call, the unflagged one and one single cells query (k_fold<
cells>) in the same run.  One JSON line per case.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from scripts.multi_fold_probe import CASES, engine_on, with_agg  # noqa: E402


def stage_ms(eng, fn, reps):
    """HIP-event time per call of the engine's stages over `reps` calls of
    fn (otsdb_prof_read: 0 the downsample / fold launches, 1 transform, 2
    group stage / combine, 3 prep, 4 compaction, 7 decode / qualifier
    rewrite), and the intervals a call records per stage (a cells pass run
    again after the rewrite records its stages twice)."""
    import ctypes as C
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
    return dict(ms_per_call=[ms[i] / reps for i in range(8)],
                intervals_per_call=[nn[i] / reps for i in range(8)])


def cells_of(eng, config, n_series, days):
    """(spec, the groups' DeviceBatch without its points, DeviceCells, points)."""
    import torch
    from opentsdb_amd import workload
    saved = workload.CONFIGS[config]
    try:  # (--days: the config's data and query over a shorter window)
        if days:
            workload.CONFIGS[config] = dict(saved, days=days)
        g = workload.gen_spec(config)
        spec = workload.query_spec(config)
    finally:
        workload.CONFIGS[config] = saved
    db = workload.generate_device(eng, g, 0, n_series, config=config)
    n_points = int(db.n_points_total)
    dc = workload.encode_cells_device(eng, db)
    db.ts = db.ts[:0]
    db.val = db.val[:0]
    torch.cuda.empty_cache()
    return spec, db, dc, n_points


def probe(eng, par, config, aggs, spec, db, dc, n_points, n_series, warm,
          reps):
    import torch
    from opentsdb_amd import workload
    from opentsdb_amd.engine import DeviceResult
    n = len(aggs)
    n_buckets = int((spec.end_ms - spec.start_ms) // spec.ds_interval_ms) + 2
    cap = n_buckets * db.n_groups + 8

    def results():
        return [DeviceResult(torch, db.n_groups, cap, "cuda") for _ in aggs]
    r_fold, r_rows, r_one = results(), results(), results()
    specs = [with_agg(spec, a) for a in aggs]

    def fold():
        workload.run_cells_multi_device(eng, spec, aggs, dc, db, r_fold,
                                        fold=True)

    def rows():
        workload.run_cells_multi_device(par, spec, aggs, dc, db, r_rows)

    def singles():
        for i in range(n):
            workload.run_cells_device(par, specs[i], dc, db, r_one[i])

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
    cells_counters = eng.counters()
    # the three must agree before their times are compared: the same points,
    # values within 1e-12
    same = True
    worst = 0.0
    for other in (r_one, r_rows):
        for i in range(n):
            k = int(other[i].offsets[-1].item())
            same = same and torch.equal(r_fold[i].offsets, other[i].offsets)
            same = same and torch.equal(r_fold[i].ts[:k], other[i].ts[:k])
            a = r_fold[i].val[:k].view(torch.float64)
            b = other[i].val[:k].view(torch.float64)
            ok = ~(a.isnan() & b.isnan())
            if k and bool(ok.any()):
                rel = ((a[ok] - b[ok]).abs() /
                       b[ok].abs().clamp(min=1e-300)).max()
                worst = max(worst, float(rel))

    def stat(x):
        return dict(median=statistics.median(x), min=min(x), max=max(x))
    s = {k: stat(v) for k, v in t.items()}
    spread = s["rows"]["max"] - s["rows"]["min"]
    line = dict(config=config, aggs=aggs, series=n_series, points=n_points,
                cells_bytes=int(dc.n_bytes), groups=int(db.n_groups),
                buckets=n_buckets, reps=reps, warmup=warm, fold_ms=s["fold"],
                rows_ms=s["rows"], singles_ms=s["singles"],
                rows_spread_ms=spread,
                fold_wins=bool(s["fold"]["median"] <
                               s["rows"]["median"] - spread),
                fold_launches=launches, counters=counters,
                cells_uniform=int(cells_counters["cells_uniform"]),
                cells_general=int(cells_counters["cells_general"]),
                same_points=bool(same),
                worst_rel_diff=worst, within_1e12=bool(worst <= 1e-12))
    if config == "C2":
        # (all three on this tree's library)
        line["stages_fold"] = stage_ms(eng, fold, 5)
        line["stages_rows"] = stage_ms(
            eng, lambda: workload.run_cells_multi_device(eng, spec, aggs, dc,
                                                         db, r_rows), 5)
        line["stages_single"] = stage_ms(
            eng, lambda: workload.run_cells_device(eng, specs[0], dc, db,
                                                   r_one[0]), 5)
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
    ap.add_argument("--days", type=int, default=0,
                    help="window in days (default: the config's)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from opentsdb_amd import build, workload
    from opentsdb_amd.engine import Engine
    build.build()
    eng = Engine(0)
    par = engine_on(a.parent_lib)
    lines = []
    have, data = None, None
    for case in a.cases:
        config, aggs = case.split(":")
        n = a.series or workload.default_series_per_gpu(config)
        if have != config:  # one encoded batch for the cases of a config
            data = None
            torch.cuda.empty_cache()
            data = cells_of(eng, config, n, a.days)
            have = config
        spec, db, dc, n_points = data
        lines.append(probe(eng, par, config, aggs.split(","), spec, db, dc,
                           n_points, n, a.warmup, max(a.reps, 1)))
        torch.cuda.empty_cache()
        if a.out:  # (after every case: a long run leaves what it measured)
            with open(a.out, "w") as f:
                for ln in lines:
                    f.write(json.dumps(ln) + "\n")
    par.close()
    eng.close()


if __name__ == "__main__":
    main()
