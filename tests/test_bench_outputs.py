"""bench.py --dump-outputs: the files hold the timed path's result, whole or
as a fixed sample, and a plain run leaves the secondary figures to --full."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    import bench
    return bench


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def _result(n, n_groups=7):
    rng = np.random.default_rng(3)
    offsets = np.zeros(n_groups + 1, np.int64)
    offsets[1:] = np.sort(rng.integers(0, n + 1, n_groups))
    offsets[-1] = n
    ts = np.arange(n, dtype=np.int64) * 1000 + 1356998400000
    is_int = (np.arange(n) % 3 == 0).astype(np.uint8)
    dbl = rng.standard_normal(n)
    dbl[::11] = np.nan
    val = np.where(is_int.astype(bool), np.arange(n) - 5, dbl.view(np.int64))
    want = np.where(is_int.astype(bool), (np.arange(n) - 5).astype(np.float64),
                    dbl)
    return offsets, ts, val, is_int, want


def test_dump_outputs_whole(tmp_path):
    """A result under the budget is written whole, beyond-size capacity
    dropped: float64 offsets / timestamps / values (longs converted, NaNs
    kept), float32 is_int."""
    offsets, ts, val, is_int, want = _result(1000)
    pad = np.full(24, -1, np.int64)  # result capacity past offsets[-1]
    _bench().dump_outputs(str(tmp_path), offsets, np.append(ts, pad),
                          np.append(val, pad),
                          np.append(is_int, pad.astype(np.uint8)))
    got = _load(str(tmp_path))
    assert sorted(got) == ["group_offsets", "is_int", "timestamps", "values"]
    assert got["values"].dtype == np.float64
    assert got["timestamps"].dtype == got["group_offsets"].dtype == np.float64
    assert got["is_int"].dtype == np.float32
    assert np.array_equal(got["group_offsets"], offsets)
    assert np.array_equal(got["timestamps"], ts)
    assert np.array_equal(got["is_int"], is_int)
    assert np.array_equal(got["values"], want, equal_nan=True)


def test_dump_outputs_sample_is_fixed(tmp_path, monkeypatch):
    """Over the budget: the same seeded positions on every call, the files
    within the budget, every sampled point the result's own."""
    bench = _bench()
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4096)
    offsets, ts, val, is_int, want = _result(1000)
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    bench.dump_outputs(a, offsets, ts, val, is_int)
    bench.dump_outputs(b, offsets, ts, val, is_int)
    ga, gb = _load(a), _load(b)
    assert sorted(ga) == ["group_offsets", "is_int", "sample_index",
                          "timestamps", "values"]
    for k in ga:
        assert np.array_equal(ga[k], gb[k], equal_nan=True)
    assert sum(v.nbytes for v in ga.values()) <= 4096
    idx = ga["sample_index"].astype(np.int64)
    assert 0 < len(idx) < 1000 and (np.diff(idx) > 0).all()
    assert np.array_equal(ga["group_offsets"], offsets)  # never sampled
    assert np.array_equal(ga["timestamps"], ts[idx])
    assert np.array_equal(ga["is_int"], is_int[idx])
    assert np.array_equal(ga["values"], want[idx], equal_nan=True)


def _run_bench(*argv):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"),
                        "--gpus", "1", "--config", "C1"] + list(argv),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_bench_full_keeps_the_stage_figures():
    """--full (here with every secondary figure switched off) still runs
    the profiled pass: per-stage times and the kernel's own roofline."""
    d = _run_bench("--steps", "2", "--warmup", "1", "--full",
                   "--no-cpu-baseline", "--no-extra", "--no-decode")
    assert d["steps"] == 2 and d["ms_per_step"] > 0
    assert sorted(d["config"]["stage_ms"]) == [
        "compact", "downsample", "group", "prep", "transform"]
    assert d["config"]["stage_ms"]["downsample"] > 0
    assert d["roofline"]["kernel_ms"] > 0 and d["roofline"]["kernel_frac"] > 0


@pytest.mark.gpu
def test_bench_plain_run_dumps_the_query_result(tmp_path):
    """A plain C1 run: --steps sets the timed steps, the line carries the
    headline fields and none of --full's figures, and the dumped arrays are
    the C1 query's result (the oracle's, over the same generated series)."""
    from opentsdb_amd import workload
    from oracle import pyoracle
    out = str(tmp_path / "dump")
    d = _run_bench("--steps", "4", "--warmup", "1", "--dump-outputs", out)
    assert d["steps"] == 4 and d["warmup"] == 1
    assert d["ms_per_step"] > 0 and d["value"] > 0
    assert d["unit"] == "data points/s" and d["dtype"] == "f64"
    assert d["higher_is_better"] is True
    assert d["config"]["stage_ms"] is None and d["cpu_baseline"] is None
    for k in ("named_query", "p999", "pcie_inclusive", "decode"):
        assert k not in d

    got = _load(out)
    assert "sample_index" not in got
    n_series = workload.default_series_per_gpu("C1")
    hb = pyoracle.gen_batch(workload.gen_spec("C1"), 0, n_series,
                            lambda s: workload.group_of("C1", s))
    ref = pyoracle.group_by(workload.query_spec("C1"), hb)
    offs = got["group_offsets"].astype(np.int64)
    assert len(offs) == len(ref) + 1
    assert d["config"]["output_points_per_gpu"] == offs[-1]
    for g, want in enumerate(ref):
        a, b = offs[g], offs[g + 1]
        assert np.array_equal(got["timestamps"][a:b], want["ts"])
        assert not got["is_int"][a:b].any()
        assert np.allclose(got["values"][a:b],
                           want["bits"].view(np.float64), rtol=1e-12, atol=0,
                           equal_nan=True)
