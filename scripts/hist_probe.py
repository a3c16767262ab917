"""The histogram query at latency-panel scale, timed by the engine's own
stage events (otsdb_prof_*: [8] k_hist_prep + k_hist_fold together, [9]
k_hist_combine, [10] k_hist_percentiles, [11] the compaction).

    python -m scripts.hist_probe [--series 20000] [--points 1440] [--bins 100]
        [--groups 100] [--reps 7] [--warmup 2] [--kfold-tbs X]
        [--out profiles/hist_probe.json]

Shape: `series` series of `points` one-minute histograms of `bins` buckets
(20,000 x 1,440 x 102 x 8 B = 23.5 GB of records), generated on the device,
`groups` groups, 5m-sum, percentiles {50, 99, 99.9}.  Per stage: the median
time and bytes / time (the fold reads every record and timestamp once, the
percentile kernel the dense sums).  --kfold-tbs: the read rate k_fold reaches
on bench.py's C2 in the same session, recorded beside the fold's as the rate
this chip reaches on a per-series stream.  The whole call is timed for one
and for three percentiles: the difference is the percentile kernel's.
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

T0 = 1_600_000_020_000  # a whole minute


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--series", type=int, default=20000)
    ap.add_argument("--points", type=int, default=1440)
    ap.add_argument("--bins", type=int, default=100)
    ap.add_argument("--groups", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kfold-tbs", type=float, default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import ctypes as C

    import numpy as np
    import torch
    from opentsdb_amd import build, core
    from opentsdb_amd.engine import (DeviceBatch, DeviceHist,
                                     DeviceHistResult, Engine,
                                     run_hist_device)
    build.build()
    eng = Engine(0)
    assert eng.lib.otsdb_prof_enable(eng.ctx, 1) == 0
    S, n, K, G = a.series, a.points, a.bins, a.groups
    R, N = K + 2, a.series * a.points
    dev = "cuda"
    offsets = torch.arange(S + 1, dtype=torch.int64, device=dev) * n
    # one histogram a minute, each series on its own phase inside the minute
    phase = torch.randint(0, 60000, (S, 1), dtype=torch.int64, device=dev)
    ts = (T0 + 60000 * torch.arange(n, dtype=torch.int64, device=dev)[None, :]
          + phase).reshape(-1).contiguous()
    counts = torch.empty((N, R), dtype=torch.int64, device=dev)
    step = max(1, (1 << 28) // R)
    for i in range(0, N, step):  # latency-shaped: mass in the low buckets
        j = min(N, i + step)
        x = torch.randint(0, 1000, (j - i, R), dtype=torch.int64, device=dev)
        counts[i:j] = x // (1 + torch.arange(R, device=dev)[None, :])
    goff = torch.tensor([S * g // G for g in range(G + 1)], dtype=torch.int64,
                        device=dev)
    members = torch.arange(S, dtype=torch.int64, device=dev)
    db = DeviceBatch(offsets, ts, None, goff, members)
    lower = np.float32(1.25) ** np.arange(K, dtype=np.float32)
    dh = DeviceHist(lower, lower * np.float32(1.25), counts)
    spec = core.make_spec(T0, T0 + n * 60000 - 1, core.Aggregators.get("sum"),
                          core.DownsamplingSpecification("5m-sum"), T0,
                          T0 + n * 60000 - 1)
    nb = (n * 60000 + 299999) // 300000 + 1
    res = DeviceHistResult(torch, G, G * nb, K, 3, False, dev)

    def stages():
        ms = (C.c_double * 12)()
        cnt = (C.c_int64 * 12)()
        assert eng.lib.otsdb_prof_read(eng.ctx, ms, cnt, 12, 1) == 0
        return list(ms)[8:12]

    def timed(pcts):
        torch.cuda.synchronize()
        t = time.perf_counter()
        run_hist_device(eng, spec, db, dh, pcts, res)
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3, stages()

    p3, p1 = [50.0, 99.0, 99.9], [99.0]
    for _ in range(a.warmup):
        timed(p3)
        timed(p1)
    r3, r1 = [], []
    for _ in range(max(a.reps, 3)):
        r3.append(timed(p3))
        r1.append(timed(p1))
    out_points = int(res.offsets[-1].item())
    med = lambda xs: statistics.median(xs)  # noqa: E731
    st3 = [med([s[k] for _, s in r3]) for k in range(4)]
    st1 = [med([s[k] for _, s in r1]) for k in range(4)]
    rec_bytes = N * R * 8 + N * 8
    dense_bytes = out_points * R * 8
    line = dict(
        series=S, points_per_series=n, bins=K, groups=G, ds="5m-sum",
        record_bytes=rec_bytes, out_points=out_points, reps=len(r3),
        warmup=a.warmup, window_buckets=int(eng.lib.otsdb_hist_window(K)),
        # stage [8]: the k_hist_prep launch (a thread per series) is inside it
        prep_and_fold_ms=st3[0], prep_and_fold_tbs=rec_bytes / st3[0] / 1e9,
        combine_ms=st3[1], percentiles_ms_3=st3[2], percentiles_ms_1=st1[2],
        percentiles_gbs_3=dense_bytes / max(st3[2], 1e-9) / 1e6,
        compact_ms=st3[3],
        call_ms_3=med([w for w, _ in r3]), call_ms_1=med([w for w, _ in r1]),
        call_ms_3_minmax=[min(w for w, _ in r3), max(w for w, _ in r3)],
        kfold_c2_tbs=a.kfold_tbs, counters=eng.hist_counters())
    print(json.dumps(line), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(line) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
