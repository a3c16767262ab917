"""The rollup query from storage rows (otsdb_agg_run_rollup_rows_device)
against the rollup query over already-paired columns it ends in.

Workload: a 10-minute rollup table in day rows — 144 sum cells (4-byte longs)
then 144 count cells (2-byte longs) per row, in qualifier order as the scanner
delivers them — `--series` series of `--days` rows each in ONE group (C5's
grouping), queried avg:1h-avg over the whole range.  Two variants: every cell
paired, and 2 % of the count cells missing.

In one process, after `--warmup` rounds, `--reps` repetitions of

    rows      otsdb_agg_run_rollup_rows_device       this tree
    columns   otsdb_agg_run_rollup_device            --baseline-lib (the parent
              over the columns the decode produced   commit's build)
    own       the same columns call                  this tree (a control: the
                                                     same kernels as columns)

in an order that rotates from repetition to repetition (a call's time depends
on the call before it), each timed by a host clock around a device synchronise, the rows call also by
the engine's stage events (otsdb_prof_*; stage 7 is the decode: count pass,
seek passes, scan, write pass).

    python -m scripts.rollup_rows_probe --baseline-lib PATH/libotsdb_agg.so
        [--series 125000] [--days 7] [--out profiles/rollup_rows_probe.json]

The gate: rows call - its decode stage <= the parent's columns call x (1 + the
parent's own run-to-run spread, (max - min) / median).  The decode figures are
a record: the bytes are what the decode has to move once (row and column
offsets, qualifiers, values in; 25 B a point out), the rate those bytes over
the stage time, the fraction that rate over the 6.3 TB/s an MI355X copy
reaches.  The two passes of the decode read the input twice.  Every call is
also split, by the same events, into its pipeline stages and what is left of
the host clock (`*_split`).
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

from scripts.rollup_probe import Ctx  # noqa: E402

HBM_ACHIEVABLE = 6.3e12  # B/s, a float4 copy on an MI355X
CELLS = 144              # 10-minute cells of a kind in a day row
T0_S = 1356998400


def make_rows(torch, n_series, days, missing, seed, dev="cuda"):
    """DeviceRawRows of the table: per row 144 sum cells then the kept count
    cells; values below 2^20, counts 1..60."""
    from opentsdb_amd.storage import DeviceRawRows
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    R = n_series * days
    keep = torch.ones((R, 2 * CELLS), dtype=torch.bool, device=dev)
    if missing > 0:
        keep[:, CELLS:] = torch.rand((R, CELLS), device=dev,
                                     generator=g) >= missing
    ids = keep.flatten().nonzero().flatten()  # kept cells, in scanner order
    n_col = keep.sum(1)
    del keep
    row_col_off = torch.zeros(R + 1, dtype=torch.int64, device=dev)
    torch.cumsum(n_col, 0, out=row_col_off[1:])
    j = ids % (2 * CELLS)
    kind = (j >= CELLS).to(torch.int64)
    off = j % CELLS
    del ids, j
    n = kind.numel()
    vlen = 4 - 2 * kind
    q16 = (off << 4) | (vlen - 1)
    qual = torch.empty((n, 3), dtype=torch.uint8, device=dev)
    qual[:, 0] = kind.to(torch.uint8)           # RollupConfig ids: sum 0, count 1
    qual[:, 1] = (q16 >> 8).to(torch.uint8)
    qual[:, 2] = (q16 & 0xFF).to(torch.uint8)
    del q16, off
    col_val_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    torch.cumsum(vlen, 0, out=col_val_off[1:])
    vb = int(col_val_off[-1].item())
    v = torch.where(kind == 0,
                    torch.randint(0, 1 << 20, (n,), device=dev, generator=g),
                    torch.randint(1, 61, (n,), device=dev, generator=g))
    val = torch.zeros(vb + 16, dtype=torch.uint8, device=dev)
    for k in range(4):  # big-endian, byte k of the cells that have one
        m = vlen > k
        pos = col_val_off[:-1][m] + k
        sh = (vlen[m] - 1 - k) * 8
        val[pos] = ((v[m] >> sh) & 0xFF).to(torch.uint8)
        del m, pos, sh
    del v, vlen, kind
    rows = torch.arange(R, dtype=torch.int64, device=dev)
    t = dict(row_series=rows // days,
             row_base_s=T0_S + (rows % days) * 86400,
             row_col_off=row_col_off,
             col_qual_off=torch.arange(n + 1, dtype=torch.int64,
                                       device=dev) * 3,
             qual=torch.cat([qual.flatten(),
                             torch.zeros(16, dtype=torch.uint8, device=dev)]),
             col_val_off=col_val_off, val=val, col_ts=None)
    in_bytes = R * 24 + 8 + 2 * 8 * (n + 1) + 3 * n + vb
    return DeviceRawRows(t, R, n_series, 3 * n, vb), n, in_bytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--series", type=int, default=125000)
    ap.add_argument("--days", type=int, default=7)
    ap.add_argument("--missing", type=float, default=0.02)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--baseline-lib", default=None,
                    help="libotsdb_agg.so built from the parent commit")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from opentsdb_amd import abi, build, core
    from opentsdb_amd.engine import (DeviceBatch, DeviceResult, Engine,
                                     rollup_decode_rows_device)
    build.build()
    eng = Engine(0)
    new = Ctx(abi.LIB_PATH)
    base = Ctx(a.baseline_lib or abi.LIB_PATH)
    S, D = a.series, a.days
    start, end = T0_S * 1000, (T0_S + D * 86400) * 1000 - 1
    spec = core.make_spec(start, end, core.Aggregators.AVG,
                          core.DownsamplingSpecification("1h-avg"), start, end)
    table = abi.RollupTable(600, 0, 1, 0)
    avg = core.Aggregators.AVG.id
    g_off = torch.tensor([0, S], dtype=torch.int64, device="cuda")
    members = torch.arange(S, dtype=torch.int64, device="cuda")
    variants = {}
    for name, miss in (("paired", 0.0), ("missing_counts", a.missing)):
        raw, n_cells, in_bytes = make_rows(torch, S, D, miss, 42)
        offs, ts, val, isf, cnt = rollup_decode_rows_device(
            eng, raw, table, "avg", S, start)
        cols = DeviceBatch(offs, ts, val, g_off, members, is_float=isf)
        sz = eng.plan(spec, cols)
        cap = int(sz.max_out_points)
        variants[name] = dict(
            raw=raw, raw_abi=raw.as_abi(), cols=cols, cols_abi=cols.as_abi(),
            cnt=cnt, n_cells=n_cells, in_bytes=in_bytes, points=ts.numel(),
            res=DeviceResult(torch, 1, cap, "cuda"),
            ref=DeviceResult(torch, 1, cap, "cuda"),
            own=DeviceResult(torch, 1, cap, "cuda"), t_rows=[], t_cols=[],
            t_own=[])
    gb = abi.Batch()
    gb.n_series, gb.n_points, gb.n_groups = S, 0, 1
    gb.group_offsets, gb.group_members = g_off.data_ptr(), members.data_ptr()
    hg = (C.c_int64 * 2)(0, S)
    gb.group_offsets_host = C.addressof(hg)

    def rows_call(v):
        r = v["res"].as_abi()
        new.check(new.lib.otsdb_agg_run_rollup_rows_device(
            new.ctx, C.byref(spec), C.byref(v["raw_abi"]), C.byref(table), avg,
            C.byref(gb), C.byref(r), None))

    def cols_call(v):
        r = v["ref"].as_abi()
        base.check(base.lib.otsdb_agg_run_rollup_device(
            base.ctx, C.byref(spec), C.byref(v["cols_abi"]), avg,
            v["cnt"].data_ptr(), C.byref(r), None))

    def own_call(v):  # the columns call on this tree's library
        r = v["own"].as_abi()
        new.check(new.lib.otsdb_agg_run_rollup_device(
            new.ctx, C.byref(spec), C.byref(v["cols_abi"]), avg,
            v["cnt"].data_ptr(), C.byref(r), None))

    def timed(fn, v, ctx):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn(v)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t) * 1e3
        return wall, ctx.stages()

    for _ in range(a.warmup):
        for v in variants.values():
            timed(rows_call, v, new)
            timed(cols_call, v, base)
            timed(own_call, v, new)
    # the order of the three calls rotates from repetition to repetition:
    # a call's time depends on what ran before it (the columns call right
    # after the 16 ms rows call runs its downsample pass up to 8 % faster
    # than after another columns call), so every call gets every predecessor
    calls = [("t_rows", rows_call, new), ("t_cols", cols_call, base),
             ("t_own", own_call, new)]
    for rep in range(max(a.reps, 5)):
        for v in variants.values():
            for i in range(3):
                key, fn, ctx = calls[(i + rep) % 3]
                v[key].append(timed(fn, v, ctx))
    line = dict(
        query="avg:1h-avg", series=S, days=D, rows=S * D, reps=max(a.reps, 5),
        warmup=a.warmup, hbm_achievable_Bps=HBM_ACHIEVABLE,
        baseline=("parent commit" if a.baseline_lib
                  else "this tree (no --baseline-lib)"), variants={})
    ok = True
    for name, v in variants.items():
        res, ref = v["res"], v["ref"]
        k = int(ref.offsets[-1].item())
        same = (torch.equal(res.offsets, ref.offsets) and
                torch.equal(res.ts[:k], ref.ts[:k]) and
                torch.equal(res.val[:k], ref.val[:k]))
        wr = [w for w, _ in v["t_rows"]]
        dec = [s[7] for _, s in v["t_rows"]]
        rest = [w - d for w, d in zip(wr, dec)]
        wc = [w for w, _ in v["t_cols"]]
        wo = [w for w, _ in v["t_own"]]
        med = statistics.median
        # where a call's time goes: the pipeline's stages by their events
        # (0 downsample, 1 transform, 2 group, 3 prep, 4 compaction) and what
        # is left of the host clock (launch latency, host work, gaps)
        def split(ts, skip=()):
            pipe = [sum(x for i, x in enumerate(s_) if i not in skip)
                    for _, s_ in ts]
            return dict(pipeline_stages_ms=med(pipe),
                        outside_stages_ms=med(
                            [w - sum(s_) for w, s_ in ts]),
                        stage_ms=[med([s_[i] for _, s_ in ts])
                                  for i in range(8)])
        spread = (max(wc) - min(wc)) / med(wc)
        limit = med(wc) * (1.0 + spread)
        out_bytes = 25 * v["points"] + 8 * (S + 1)
        moved = v["in_bytes"] + out_bytes
        rate = moved / (med(dec) * 1e-3)
        gate = bool(med(rest) <= limit)
        ok = ok and gate and bool(same)
        line["variants"][name] = dict(
            cells=v["n_cells"], points=v["points"],
            decode_in_bytes=v["in_bytes"], decode_out_bytes=out_bytes,
            decode_stage_ms=dict(median=med(dec), min=min(dec), max=max(dec)),
            decode_Bps=rate, decode_fraction_of_hbm=rate / HBM_ACHIEVABLE,
            decode_gcells_per_s=v["n_cells"] / med(dec) / 1e6,
            rows_call_ms=dict(median=med(wr), min=min(wr), max=max(wr)),
            rows_call_minus_decode_ms=dict(median=med(rest), min=min(rest),
                                           max=max(rest)),
            parent_columns_call_ms=dict(median=med(wc), min=min(wc),
                                        max=max(wc)),
            this_tree_columns_call_ms=dict(median=med(wo), min=min(wo),
                                           max=max(wo)),
            rows_call_split=split(v["t_rows"], skip=(7,)),
            parent_columns_call_split=split(v["t_cols"]),
            this_tree_columns_call_split=split(v["t_own"]),
            parent_spread=spread, gate_limit_ms=limit, gate_met=gate,
            same_output_bits=bool(same))
    line["gate_met"] = ok
    print(json.dumps(line), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(line, indent=1) + "\n")
    base.close()
    new.close()
    eng.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
