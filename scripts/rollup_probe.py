"""The rollup ring kernel against the plain one it was derived from: the C5
batch shape (p99:1m-avg-nan, a row-path query) through

    otsdb_agg_run_device          on a library built from the PARENT commit
    otsdb_agg_run_rollup_device   on this tree, rollup avg, counts of 1

in one process, warmed, alternating, each timed by the engine's own stage
events (otsdb_prof_*; stage 0 is the downsample pass: k_bucketize_k /
k_bucketize_rollup).

    python -m scripts.rollup_probe --baseline-lib PATH/libotsdb_agg.so
        [--config C5] [--series N] [--reps 7] [--out profiles/rollup_probe.json]

--baseline-lib: the parent commit's build (check the parent out beside the
tree, build it there, pass its libotsdb_agg.so); without it the plain query
runs on this tree's library and the line says so.

By bytes the rollup stage reads 24 B a point where the plain one reads 16:
the target is  rollup stage <= 1.5 x parent stage x (1 + spread),  spread
being the parent's own (max - min) / median over the repetitions.
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


class Ctx:
    """A context of one build of the library with stage timing on."""

    def __init__(self, path):
        from opentsdb_amd import abi
        self.lib = abi.load(path)
        self.ctx = C.c_void_p()
        assert self.lib.otsdb_ctx_create(0, C.byref(self.ctx)) == 0
        assert self.lib.otsdb_prof_enable(self.ctx, 1) == 0

    def stages(self):
        """ms per stage since the last read (reset)."""
        ms = (C.c_double * 8)()
        assert self.lib.otsdb_prof_read(self.ctx, ms, None, 8, 1) == 0
        return list(ms)

    def check(self, st):
        assert st == 0, (st, self.lib.otsdb_last_error())

    def close(self):
        self.lib.otsdb_ctx_destroy(self.ctx)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C5")
    ap.add_argument("--series", type=int, default=0,
                    help="series (default: the config's per GPU)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--baseline-lib", default=None,
                    help="libotsdb_agg.so built from the parent commit")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from opentsdb_amd import abi, build, core, workload
    from opentsdb_amd.engine import DeviceResult, Engine
    build.build()
    eng = Engine(0)  # generates the batch
    new = Ctx(abi.LIB_PATH)
    base = Ctx(a.baseline_lib or abi.LIB_PATH)
    n = a.series or workload.default_series_per_gpu(a.config)
    g = workload.gen_spec(a.config)
    db = workload.generate_device(eng, g, 0, n, config=a.config)
    spec = workload.query_spec(a.config)
    assert spec.ds_agg_id == core.Aggregators.AVG.id
    npts = int(db.n_points_total)
    ones = torch.ones(max(npts, 2), dtype=torch.int64, device="cuda")
    sz = eng.plan(spec, db)
    res = DeviceResult(torch, db.n_groups, int(sz.max_out_points), "cuda")
    ref = DeviceResult(torch, db.n_groups, int(sz.max_out_points), "cuda")
    b, r_new, r_ref = db.as_abi(), res.as_abi(), ref.as_abi()
    avg = core.Aggregators.AVG.id

    def plain():
        base.check(base.lib.otsdb_agg_run_device(
            base.ctx, C.byref(spec), C.byref(b), C.byref(r_ref), None))

    def rollup():
        new.check(new.lib.otsdb_agg_run_rollup_device(
            new.ctx, C.byref(spec), C.byref(b), avg, ones.data_ptr(),
            C.byref(r_new), None))

    def timed(fn, ctx):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t) * 1e3
        return wall, ctx.stages()

    for _ in range(a.warmup):
        timed(plain, base)
        timed(rollup, new)
    tp, tr = [], []
    for _ in range(max(a.reps, 5)):
        tp.append(timed(plain, base))
        tr.append(timed(rollup, new))
    # counts of 1: the same query — the outputs must agree before the times
    # are compared (avg buckets: the same sums, the same divisors)
    k = int(ref.offsets[-1].item())
    same = (torch.equal(res.offsets, ref.offsets) and
            torch.equal(res.ts[:k], ref.ts[:k]) and
            torch.equal(res.val[:k], ref.val[:k]))
    sp = [s[0] for _, s in tp]   # downsample stage, plain
    sr = [s[0] for _, s in tr]
    med_p, med_r = statistics.median(sp), statistics.median(sr)
    spread = (max(sp) - min(sp)) / med_p
    target = 1.5 * med_p * (1.0 + spread)
    line = dict(
        config=a.config, query="p99:1m-avg-nan", series=n, points=npts,
        buckets=int(sz.n_buckets), reps=len(tp), warmup=a.warmup,
        baseline=("parent commit" if a.baseline_lib
                  else "this tree (no --baseline-lib)"),
        plain_stage_ms=dict(median=med_p, min=min(sp), max=max(sp)),
        rollup_stage_ms=dict(median=med_r, min=min(sr), max=max(sr)),
        plain_gpts=npts / med_p / 1e6, rollup_gpts=npts / med_r / 1e6,
        plain_bytes_per_point=16, rollup_bytes_per_point=24,
        plain_spread=spread, ratio=med_r / med_p, target_ms=target,
        target_met=bool(med_r <= target),
        plain_wall_ms=statistics.median(w for w, _ in tp),
        rollup_wall_ms=statistics.median(w for w, _ in tr),
        same_output_bits=bool(same))
    print(json.dumps(line), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(line) + "\n")
    base.close()
    new.close()
    eng.close()


if __name__ == "__main__":
    main()
