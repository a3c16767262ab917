"""Panel call from compacted cells (several downsampling functions over one
decode of the columns) against what a caller does without it: the same
outputs as back-to-back otsdb_agg_run_cells_device single queries on a
library built from the PARENT commit, in the same process, on the BASELINE
shapes.

    python -m scripts.cells_panel_probe --baseline-lib PATH/libotsdb_agg.so
        [--cases C3 C2 C5] [--reps 20] [--series N] [--days D]
        [--out profiles/cells_panel_probe.json]

--baseline-lib: the parent commit's build (check the parent out beside the
tree, build it there, pass its libotsdb_agg.so); without it the singles run
on this tree's library and the line says so.  Shapes: the per-GPU series
counts of C3 (1h buckets, {dc=*}), C2 (5m, {host=*}; --days shortens its
window) and C5's shape (1m buckets, fill nan, one group), each generated
columnar, encoded to cells on the device, the columnar copy dropped.
Panels: [min-min, avg-avg, max-max] and the same plus sum-sum.  After the
warm-up rounds the two alternate, each timed synchronously; per case the
median, min and max of the repetitions, and the routing rule of DESIGN.md
§4.2: the shared pass stays the default for a shape only if its median is
below the baseline's by more than the baseline's own min-max spread.
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

from scripts.panel_probe import PANELS, with_query  # noqa: E402


class BaselineEngine:
    """A context of another build of the library (abi.load(path)): only the
    single cells query is called on it."""

    def __init__(self, path):
        from opentsdb_amd import abi
        self.lib = abi.load(path)
        self.ctx = C.c_void_p()
        st = self.lib.otsdb_ctx_create(0, C.byref(self.ctx))
        assert st == 0, st

    def run_cells_device(self, spec, c, b, r):
        st = self.lib.otsdb_agg_run_cells_device(
            self.ctx, C.byref(spec), C.byref(c), C.byref(b), C.byref(r), None)
        assert st == 0, (st, self.lib.otsdb_last_error())

    def close(self):
        self.lib.otsdb_ctx_destroy(self.ctx)


def probe(eng, base, config, n_series, days, warm, reps):
    import torch
    from opentsdb_amd import abi, workload
    from opentsdb_amd.engine import DeviceResult
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
    # the groups stay; the columnar points go
    db.ts = db.ts[:0]
    db.val = db.val[:0]
    torch.cuda.empty_cache()
    b = abi.Batch()
    b.n_series = dc.n_series
    b.n_points = 0
    b.n_groups = db.n_groups
    b.group_offsets = db.group_offsets.data_ptr()
    b.group_members = db.group_members.data_ptr()
    c_abi = dc.as_abi()
    n_buckets = int((spec.end_ms - spec.start_ms) // spec.ds_interval_ms) + 2
    cap = n_buckets * db.n_groups + 8

    def timed(fn):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3

    lines = []
    for queries in PANELS:
        n = len(queries)
        res = [DeviceResult(torch, db.n_groups, cap, "cuda") for _ in queries]
        ref = [DeviceResult(torch, db.n_groups, cap, "cuda") for _ in queries]
        ref_abi = [r.as_abi() for r in ref]
        specs = [with_query(spec, a, d) for a, d in queries]

        def panel():
            workload.run_cells_panel_device(eng, spec, queries, dc, db, res)

        def singles():
            for i in range(n):
                base.run_cells_device(specs[i], c_abi, b, ref_abi[i])
        for _ in range(warm):
            panel()
            singles()
        torch.cuda.synchronize()
        tp, ts = [], []
        for _ in range(reps):
            tp.append(timed(panel))
            ts.append(timed(singles))
        panel()
        counters = eng.panel_counters()
        # the two must agree before their times are compared
        same = True
        for i in range(n):
            k = int(ref[i].offsets[-1].item())
            same = (same and torch.equal(res[i].offsets, ref[i].offsets) and
                    torch.equal(res[i].ts[:k], ref[i].ts[:k]))
        med_p, med_s = statistics.median(tp), statistics.median(ts)
        spread = max(ts) - min(ts)
        lines.append(dict(
            config=config, panel=["%s-%s" % q for q in queries], n_out=n,
            series=n_series, points=n_points, cells_bytes=int(dc.n_bytes),
            groups=int(db.n_groups), buckets=n_buckets, days=days or None,
            reps=reps, warmup=warm,
            panel_ms=dict(median=med_p, min=min(tp), max=max(tp)),
            singles_ms=dict(median=med_s, min=min(ts), max=max(ts)),
            baseline=base.path, singles_over_panel=med_s / med_p,
            counters=counters, same_timestamps=bool(same),
            shared_pass_stays=bool(med_s - med_p > spread)))
        print(json.dumps(lines[-1]), flush=True)
        del res, ref
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="*", default=["C3", "C2", "C5"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--series", type=int, default=0,
                    help="series per case (default: the config's per GPU)")
    ap.add_argument("--days", type=int, default=0,
                    help="window in days (default: the config's)")
    ap.add_argument("--baseline-lib", default=None,
                    help="libotsdb_agg.so built from the parent commit")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from opentsdb_amd import abi, build, workload
    from opentsdb_amd.engine import Engine
    build.build()
    eng = Engine(0)
    base = BaselineEngine(a.baseline_lib or abi.LIB_PATH)
    base.path = ("parent commit" if a.baseline_lib
                 else "this tree (no --baseline-lib)")
    lines = []
    for config in a.cases:
        n = a.series or workload.default_series_per_gpu(config)
        lines += probe(eng, base, config, n, a.days, a.warmup, max(a.reps, 1))
        import torch
        torch.cuda.empty_cache()
    base.close()
    eng.close()
    if a.out:
        with open(a.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
