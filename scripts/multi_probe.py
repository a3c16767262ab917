"""Multi-aggregator call against the same aggregators as back-to-back single
queries (the unchanged otsdb_agg_run_device, in the same process), on the
BASELINE workloads.

    python -m scripts.multi_probe [--cases C5:p99,p999 ...] [--reps 20]
                                  [--series N] [--out profiles/multi_probe.json]

Per case: after a warm-up the two alternate, each timed synchronously; the
script reports the median of the repetitions, the spread (min / max) and the
ratio singles / multi, one JSON line per case, and writes the lines to --out.
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

CASES = ["C5:p99,p999", "C5:p50,p90,p99,p999", "C3:min,avg,max,p99",
         "C4:sum,dev,max", "C2:zimsum,min,max"]


def with_agg(spec, agg):
    from opentsdb_amd import core
    s = type(spec).from_buffer_copy(spec)
    s.agg_id = core.Aggregators.get(agg).id
    s.interp = -1
    return s


def probe(eng, config, aggs, n_series, warm, reps, prefixes):
    import torch
    from opentsdb_amd import workload
    from opentsdb_amd.engine import DeviceResult, run_device, run_multi_device
    g = workload.gen_spec(config)
    db = workload.generate_device(eng, g, 0, n_series, config=config)
    spec = workload.query_spec(config)
    sz = eng.plan_multi(spec, aggs, db)
    res = [DeviceResult(torch, db.n_groups, int(sz.max_out_points), "cuda")
           for _ in aggs]
    ref = [DeviceResult(torch, db.n_groups, int(sz.max_out_points), "cuda")
           for _ in aggs]
    specs = [with_agg(spec, a) for a in aggs]

    def timed(fn):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3

    lines = []
    sets = [len(aggs)] if not prefixes else range(2, len(aggs) + 1)
    for n in sets:
        def multi():
            run_multi_device(eng, spec, aggs[:n], db, res[:n])

        def singles():
            for i in range(n):
                run_device(eng, specs[i], db, ref[i])
        for _ in range(warm):
            multi()
            singles()
        torch.cuda.synchronize()
        tm, ts = [], []
        for _ in range(reps):
            tm.append(timed(multi))
            ts.append(timed(singles))
        counters = None
        multi()
        counters = eng.multi_counters()
        # the two must agree before their times are compared
        same = all(torch.equal(res[i].offsets, ref[i].offsets) for i in range(n))
        for i in range(n):
            k = int(ref[i].offsets[-1].item())
            same = same and torch.equal(res[i].ts[:k], ref[i].ts[:k])
        med_m, med_s = statistics.median(tm), statistics.median(ts)
        lines.append(dict(
            config=config, aggs=aggs[:n], n_out=n, series=n_series,
            points=int(db.n_points_total), groups=int(db.n_groups),
            buckets=int(sz.n_buckets), reps=reps,
            multi_ms=dict(median=med_m, min=min(tm), max=max(tm)),
            singles_ms=dict(median=med_s, min=min(ts), max=max(ts)),
            singles_over_multi=med_s / med_m, counters=counters,
            same_timestamps=bool(same)))
        print(json.dumps(lines[-1]), flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="*", default=CASES)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--series", type=int, default=0,
                    help="series per case (default: the config's per GPU)")
    ap.add_argument("--prefixes", action="store_true",
                    help="every prefix of each aggregator list from 2 on "
                         "(the n_out at which sharing starts to win)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from opentsdb_amd import build, workload
    from opentsdb_amd.engine import Engine
    build.build()
    eng = Engine(0)
    lines = []
    for case in a.cases:
        config, aggs = case.split(":")
        n = a.series or workload.default_series_per_gpu(config)
        lines += probe(eng, config, aggs.split(","), n, a.warmup,
                       max(a.reps, 1), a.prefixes)
        import torch
        torch.cuda.empty_cache()
    eng.close()
    if a.out:
        with open(a.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
