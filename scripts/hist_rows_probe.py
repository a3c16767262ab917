"""The histogram query from storage rows at panel scale: the rows decode
(hist_rows.hip) beside the fold that reads what it writes.

    python -m scripts.hist_rows_probe [--series 2000] [--points 1440]
        [--bins 100] [--reps 7] [--warmup 2] [--out profiles/hist_rows_probe.json]

Shape: `series` series of `points` one-minute blobs of `bins` buckets (a
tenth of hist_probe's series: the rows are built on the host by tiling 256
distinct blobs, about 3 GB), counts of 1- to 3-byte var-longs, one storage row
per (series, hour), groups of 200 series, 5m-sum, percentiles {50, 99, 99.9}.

Timed with the engine's stage events (otsdb_prof_*: [12] the rows decode of
otsdb_hist_run_rows_device — cells, the scan walk, assembly, the write walk
and the two read-backs between them; [8] k_hist_prep + k_hist_fold) and, for
the entries that have no stage, the wall clock around the synchronous call:
the schema call (k_hr_cells + k_hr_walk<0>), the count-only decode (k_hr_cells
+ k_hr_walk<1> + assembly) and the whole decode (the same + k_hr_walk<2>);
their difference is the write walk's.  A per-kernel split needs a kernel
trace (rocprofv3 --kernel-trace --stats) around this script.  The yardstick is
the same session's otsdb_hist_run_device over the decoded columns of the same
batch, stage [8].
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

B0 = 1356998400  # an hour base, seconds
CODEC = 0
DISTINCT = 256


def build_rows(S, n, K, torch, np, dev="cuda"):
    """storage.DeviceRawRows of S series x n one-minute cells, built by
    tiling DISTINCT blobs; the schema; the value bytes."""
    from opentsdb_amd import histogram as H
    from opentsdb_amd.storage import DeviceRawRows
    lower = (np.float32(1.25) ** np.arange(K, dtype=np.float32))
    upper = lower * np.float32(1.25)
    rng = np.random.default_rng(1)
    blobs = []
    for j in range(DISTINCT):  # latency-shaped: mass in the low buckets
        cnt = rng.integers(0, 200000, K) // (1 + np.arange(K)) ** 2
        h = H.Histogram({(lo, up): int(c)
                         for lo, up, c in zip(lower, upper, cnt)},
                        int(rng.integers(0, 100)), int(rng.integers(0, 100)))
        blobs.append(np.frombuffer(H.encode_simple(h, CODEC), np.uint8))
    lens = np.array([len(b) for b in blobs], np.int64)
    L = int(lens.max())
    mat = np.zeros((DISTINCT, L), np.uint8)
    for j, b in enumerate(blobs):
        mat[j, :len(b)] = b
    keep = np.arange(L)[None, :] < lens[:, None]
    C = S * n
    which = ((np.arange(S)[:, None] * 7 + np.arange(n)[None, :] * 13)
             % DISTINCT).reshape(-1)
    voff = np.zeros(C + 1, np.int64)
    np.cumsum(lens[which], out=voff[1:])
    val = torch.zeros(int(voff[-1]) + 16, dtype=torch.uint8, device=dev)
    step = max(1, (64 << 20) // L)
    for i in range(0, C, step):  # tile on the host, 64 MB at a time
        w = which[i:i + step]
        val[int(voff[i]):int(voff[min(C, i + step)])] = torch.from_numpy(
            mat[w][keep[w]]).to(dev)
    # one row per (series, hour); second qualifiers 06 <short offset>
    hours = (n + 59) // 60
    minute = np.arange(n)
    sec = (minute % 60) * 60
    q = np.zeros((S, n, 3), np.uint8)
    q[:, :, 0] = 6
    phase = (np.arange(S) % 60)[:, None]
    q[:, :, 1] = (sec[None, :] + phase) >> 8
    q[:, :, 2] = (sec[None, :] + phase) & 0xFF
    per_row = np.minimum(60, n - 60 * np.arange(hours))
    row_col = np.zeros(S * hours + 1, np.int64)
    np.cumsum(np.tile(per_row, S), out=row_col[1:])
    t = dict(
        row_series=np.repeat(np.arange(S, dtype=np.int64), hours),
        row_base_s=np.tile(B0 + 3600 * np.arange(hours, dtype=np.int64), S),
        row_col_off=row_col, col_qual_off=3 * np.arange(C + 1, dtype=np.int64),
        qual=np.concatenate([q.reshape(-1), np.zeros(16, np.uint8)]),
        col_val_off=voff)
    t = {k: torch.from_numpy(v).to(dev) for k, v in t.items()}
    t["val"] = val
    t["col_ts"] = None
    return (DeviceRawRows(t, S * hours, S, 3 * C, int(voff[-1])),
            (lower, upper), int(voff[-1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--series", type=int, default=2000)
    ap.add_argument("--points", type=int, default=1440)
    ap.add_argument("--bins", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import ctypes as C

    import numpy as np
    import torch
    from opentsdb_amd import build, core
    from opentsdb_amd.engine import (DeviceBatch, DeviceHist,
                                     DeviceHistResult, Engine,
                                     hist_decode_rows_device, run_hist_device,
                                     run_hist_rows_device)
    build.build()
    eng = Engine(0)
    S, n, K = a.series, a.points, a.bins
    G = max(1, S // 200)
    R, N = K + 2, S * n
    draw, schema, value_bytes = build_rows(S, n, K, torch, np)
    dev = "cuda"
    goff = torch.tensor([S * g // G for g in range(G + 1)], dtype=torch.int64,
                        device=dev)
    members = torch.arange(S, dtype=torch.int64, device=dev)
    t0, t1 = B0 * 1000, B0 * 1000 + n * 60000 - 1
    spec = core.make_spec(t0, t1, core.Aggregators.get("sum"),
                          core.DownsamplingSpecification("5m-sum"), t0, t1)
    nb = (n * 60000 + 299999) // 300000 + 1
    pcts = [50.0, 99.0, 99.9]
    med = statistics.median

    def wall(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3, r

    def stages():
        ms = (C.c_double * 13)()
        cnt = (C.c_int64 * 13)()
        assert eng.lib.otsdb_prof_read(eng.ctx, ms, cnt, 13, 1) == 0
        return list(ms)

    # the schema, the decode alone
    lo, up = eng.hist_rows_schema(draw, CODEC)
    assert np.array_equal(lo, schema[0]) and np.array_equal(up, schema[1])
    offsets, ts, counts = hist_decode_rows_device(eng, draw, CODEC, S, schema)
    assert int(offsets[-1].item()) == N
    dec_counters = eng.hist_rows_counters()
    h = DeviceHist(*schema).as_abi()
    raw = draw.as_abi()
    offs2 = torch.zeros(S + 1, dtype=torch.int64, device=dev)

    def count_only():
        assert eng.lib.otsdb_hist_decode_rows_device(
            eng.ctx, C.byref(raw), CODEC, S, C.byref(h), offs2.data_ptr(),
            None, None, 0, None) == 0

    def whole_decode():
        assert eng.lib.otsdb_hist_decode_rows_device(
            eng.ctx, C.byref(raw), CODEC, S, C.byref(h), offs2.data_ptr(),
            ts.data_ptr(), counts.data_ptr(), N, None) == 0

    db_rows = DeviceBatch(torch.zeros(S + 1, dtype=torch.int64, device=dev),
                          torch.zeros(0, dtype=torch.int64, device=dev), None,
                          goff, members)
    db_cols = DeviceBatch(offsets, ts, None, goff, members)
    dh_cols = DeviceHist(schema[0], schema[1], counts)
    res_a = DeviceHistResult(torch, G, G * nb, K, 3, False, dev)
    res_b = DeviceHistResult(torch, G, G * nb, K, 3, False, dev)
    assert eng.lib.otsdb_prof_enable(eng.ctx, 1) == 0
    rounds = []
    for i in range(a.warmup + max(a.reps, 3)):
        stages()
        r = dict(schema_ms=wall(lambda: eng.hist_rows_schema(draw, CODEC))[0],
                 count_ms=wall(count_only)[0], decode_ms=wall(whole_decode)[0])
        stages()
        r["rows_call_ms"] = wall(lambda: run_hist_rows_device(
            eng, spec, draw, CODEC, db_rows, DeviceHist(*schema), pcts,
            res_a))[0]
        st = stages()
        r["rows_decode_stage_ms"], r["rows_fold_stage_ms"] = st[12], st[8]
        r["cols_call_ms"] = wall(lambda: run_hist_device(
            eng, spec, db_cols, dh_cols, pcts, res_b))[0]
        r["cols_fold_stage_ms"] = stages()[8]
        if i >= a.warmup:
            rounds.append(r)
    same = (torch.equal(res_a.offsets, res_b.offsets) and
            torch.equal(res_a.ts, res_b.ts) and
            torch.equal(res_a.pct.view(torch.int64),
                        res_b.pct.view(torch.int64)))
    m = {k: med([r[k] for r in rounds]) for k in rounds[0]}
    rec_bytes = N * R * 8 + N * 8
    write_ms = m["decode_ms"] - m["count_ms"]
    line = dict(
        date=time.strftime("%Y-%m-%d"), series=S, points_per_series=n, bins=K,
        groups=G, ds="5m-sum", cells=N, value_bytes=value_bytes,
        record_bytes=rec_bytes, reps=len(rounds), warmup=a.warmup,
        counters=dec_counters, results_identical=bool(same), **m,
        write_walk_ms=write_ms,
        schema_walk_gbs=value_bytes / m["schema_ms"] / 1e6,
        count_pass_gbs=value_bytes / m["count_ms"] / 1e6,
        write_walk_in_gbs=value_bytes / max(write_ms, 1e-9) / 1e6,
        write_walk_out_gbs=rec_bytes / max(write_ms, 1e-9) / 1e6,
        decode_over_fold=m["rows_decode_stage_ms"] / m["cols_fold_stage_ms"],
        fold_tbs=rec_bytes / m["cols_fold_stage_ms"] / 1e9)
    print(json.dumps(line), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(line) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
