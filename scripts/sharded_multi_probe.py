"""The series-sharded multi-aggregator paths against the same aggregators as
back-to-back single sessions / single partials + finalize calls (the
unchanged entries of the same library, in the same process), at the per-GPU
series counts of the BASELINE workloads.  One process, a world of one: the
rank-local work of the protocols with no collectives (what every rank of a
node launch repeats per aggregator today).

    python -m scripts.sharded_multi_probe [--cases C5:p99,p999 ...]
        [--reps 20] [--series N] [--out profiles/sharded_multi_probe.json]

Selection sets run one otsdb_sel_* session with otsdb_sel_retarget between
the aggregators; scalar sets otsdb_agg_partials_multi_device +
otsdb_agg_finalize_multi_device.  Per case: after a warm-up the two variants
alternate, each timed synchronously; the script reports the median of the
repetitions, the spread (min / max), the ratio singles / shared and the pass
counters, one JSON line per case, and writes the lines to --out.
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

CASES = ["C5:p99,p999", "C5:p50,p90,p99,p999", "C4:sum,dev,max",
         "C4:min,avg,max"]


def with_agg(spec, agg):
    from opentsdb_amd import core
    s = type(spec).from_buffer_copy(spec)
    s.agg_id = core.Aggregators.get(agg).id
    s.interp = -1
    return s


def resolve(sel):
    """The pass loop, pick and finish of a world of one (the local
    histograms are the global ones)."""
    p = 0
    while sel.hist_pass(p):
        p += 1
    sel.pick()
    return sel.finish()


def same_results(a, b):
    import torch
    for x, y in zip(a, b):
        k = int(y.offsets[-1].item())
        if not (torch.equal(x.offsets, y.offsets) and
                torch.equal(x.ts[:k], y.ts[:k]) and
                torch.equal(x.val[:k], y.val[:k])):
            return False
    return True


def selection_variants(eng, spec, aggs, db, G):
    from opentsdb_amd import dist
    specs = [with_agg(spec, a) for a in aggs]
    sel = dist.ShardedSelect(eng, specs[0], db, G)  # buffers reused
    out = {}

    def shared():
        sel.spec = specs[0]
        sel.prepare()
        res = [resolve(sel)]
        for a in aggs[1:]:
            sel.retarget(a)
            res.append(resolve(sel))
        out["shared"] = res

    def singles():
        res = []
        for s in specs:
            sel.spec = s
            sel.prepare()
            res.append(resolve(sel))
        out["singles"] = res

    def counters(fn):
        n0 = eng.sel_sessions()
        fn()
        return dict(sel_sessions=eng.sel_sessions() - n0)
    return shared, singles, counters, out


def scalar_variants(eng, spec, aggs, db, G):
    import torch
    from opentsdb_amd.engine import (DeviceResult, finalize_multi_device,
                                     partials_multi_device)
    specs = [with_agg(spec, a) for a in aggs]
    nb = int(eng.plan(spec, db).n_buckets)
    GB, n = max(G * nb, 1), len(aggs)
    parts = torch.zeros((n, GB, 4), dtype=torch.int64, device="cuda")
    emit = torch.zeros(GB, dtype=torch.uint8, device="cuda")
    res = [DeviceResult(torch, G, GB, "cuda") for _ in aggs]
    ref = [DeviceResult(torch, G, GB, "cuda") for _ in aggs]
    b = db.as_abi()
    out = {"shared": res, "singles": ref}

    def shared():
        partials_multi_device(eng, spec, aggs, db, parts, emit)
        finalize_multi_device(eng, spec, aggs, G, nb, 1, parts, emit, res)

    def singles():
        for i, s in enumerate(specs):
            r = ref[i].as_abi()
            eng._check(eng.lib.otsdb_agg_partials_device(
                eng.ctx, C.byref(s), C.byref(b), parts[i].data_ptr(),
                emit.data_ptr(), None))
            eng._check(eng.lib.otsdb_agg_finalize_device(
                eng.ctx, C.byref(s), G, nb, 1, parts[i].data_ptr(),
                emit.data_ptr(), C.byref(r), None))

    def counters(fn):
        if fn is shared:
            partials_multi_device(eng, spec, aggs, db, parts, emit)
            return dict(downsample_passes=int(
                eng.multi_counters()["downsample_passes"]))
        return dict(downsample_passes=n)  # one per single partials call
    return shared, singles, counters, out


def probe(eng, config, aggs, n_series, warm, reps):
    import torch
    from opentsdb_amd import dist, workload
    g = workload.gen_spec(config)
    db = workload.generate_device(eng, g, 0, n_series, config=config)
    spec = with_agg(workload.query_spec(config), aggs[0])
    G = db.n_groups
    sel = all(dist._is_selection(with_agg(spec, a).agg_id) for a in aggs)
    shared, singles, counters, out = (
        selection_variants if sel else scalar_variants)(eng, spec, aggs, db, G)

    def timed(fn):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3

    for _ in range(warm):
        shared()
        singles()
    torch.cuda.synchronize()
    tm, ts = [], []
    for _ in range(reps):
        tm.append(timed(shared))
        ts.append(timed(singles))
    c_shared, c_singles = counters(shared), counters(singles)
    torch.cuda.synchronize()
    # the two must agree before their times are compared (timestamps; the
    # values bit for bit where one session / one finalize kernel gives both)
    same = same_results(out["shared"], out["singles"]) if sel else all(
        torch.equal(x.offsets, y.offsets) for x, y in
        zip(out["shared"], out["singles"]))
    med_m, med_s = statistics.median(tm), statistics.median(ts)
    line = dict(
        config=config, aggs=aggs, n_out=len(aggs), series=n_series,
        path="sel_retarget" if sel else "partials_multi",
        points=int(db.n_points_total), groups=int(G), reps=reps,
        shared_ms=dict(median=med_m, min=min(tm), max=max(tm)),
        singles_ms=dict(median=med_s, min=min(ts), max=max(ts)),
        singles_over_shared=med_s / med_m, counters_shared=c_shared,
        counters_singles=c_singles, same_results=bool(same))
    print(json.dumps(line), flush=True)
    return line


def main():
    ap = argparse.ArgumentParser()
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
    lines = []
    for case in a.cases:
        config, aggs = case.split(":")
        n = a.series or workload.default_series_per_gpu(config)
        lines.append(probe(eng, config, aggs.split(","), n, a.warmup,
                           max(a.reps, 1)))
        torch.cuda.empty_cache()
    eng.close()
    if a.out:
        with open(a.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
