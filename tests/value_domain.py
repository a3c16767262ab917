"""Shared by tests/test_gpu_value_domain.py and tests/test_value_domain_cpu.py:
the query matrix, windows and batches of the value-domain edge tests (the
values come from tests/datasets.py's edge generators).  Imports nothing
that needs a GPU."""
import functools

import numpy as np

from opentsdb_amd import core
from tests import datasets

T0 = datasets.T0
SPAN = 600_000
# the 10-minute window, and one cut inside buckets at both ends
WINDOWS = ((T0, T0 + SPAN), (T0 + 37_000, T0 + 511_000))

AGGS = ["sum", "avg", "min", "max", "mimmin", "mimmax", "dev", "count",
        "first", "last", "diff", "squareSum", "zimsum"]
DS = ["min", "max", "first", "last", "sum", "avg", "dev", "count", "diff"]
FILLS = ["none", "nan", "zero"]
SEL = ["median", "p50", "p99", "p999", "ep95r3", "ep50r7"]
RATE_DS = ["max", "sum", "first", "p90"]
RATE_AGGS = ["sum", "max", "dev", "count", "avg", "p99"]
COUNTER_TOPS = {"l63": (2**63 - 1, False), "l62": (2**62, False),
                "d53": (2**53, True)}


def rate_options(top):
    return [core.RateOptions(),
            core.RateOptions(True, core.LONG_MAX, 0),
            core.RateOptions(True, top, 0),
            core.RateOptions(True, top, 10**6),
            core.RateOptions(True, top, 0, True)]


def matrix():
    """(aggregator, downsampler, fill) of the downsampled fold tests: the
    whole product."""
    return [(a, d, f) for a in AGGS for d in DS for f in FILLS]


def base_batch(grouping, seed=301):
    """a: 40 series in 3 groups (each at most SEL_K = 32 members: LDS-sort
    select, one fold chunk); b: one group of 300 (k_seg_select's direct
    gather, chunk merges); c: one group of 1,100, all of them in the window
    (more than SS_CAP = 1,024 candidates a bucket: the digit passes; 138
    fold tiles of 8 members, past the 128 of the two-level combine, or 5
    row-path chunks of 256); f: 300 series in 2 groups, both large (the FILL transpose)."""
    kw = dict(span_ms=SPAN, cadence_ms=20_000)
    if grouping == "a":
        return datasets.random_batch(seed, n_series=40, n_groups=3, **kw)
    if grouping == "b":
        return datasets.random_batch(seed + 1, n_series=300, big_group=True,
                                     **kw)
    if grouping == "c":
        return datasets.random_batch(seed + 2, n_series=1100, big_group=True,
                                     empty_frac=0.0, outside=False, **kw)
    if grouping == "f":
        return datasets.random_batch(seed + 3, n_series=300, n_groups=2, **kw)
    raise ValueError(grouping)


@functools.lru_cache(maxsize=None)
def edge_batch(kind, grouping):
    hb = base_batch(grouping)
    rng = np.random.default_rng(977 + 31 * datasets.EDGE_KINDS.index(kind)
                                + ord(grouping))
    return datasets.with_values(hb, *datasets.edge_values(kind, rng,
                                                          len(hb.ts)))


@functools.lru_cache(maxsize=None)
def counter_batch(top_name, grouping="a"):
    top, as_float = COUNTER_TOPS[top_name]
    rng = np.random.default_rng(1201 + top.bit_length())
    return datasets.edge_counters(base_batch(grouping), rng, top, as_float)


# every percentile aggregator of the registry (Aggregators.java:130-172):
# PercentileAgg sorts a double[] with `<`; Median is not one of them
PERCENTILES = frozenset(
    [p for p in ("p999", "p99", "p95", "p90", "p75", "p50")] +
    ["e%sr%d" % (p, k) for p in ("p999", "p99", "p95", "p90", "p75", "p50")
     for k in (3, 7)])
assert all(core.Aggregators.get(p) for p in PERCENTILES)
assert "median" not in PERCENTILES and "pfsum" not in PERCENTILES
