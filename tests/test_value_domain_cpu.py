"""The CPU oracle on the edges of the value domain (CPU only), against
references that share no code with it: a Python big-integer model of Java
`long`, math.fsum, direct loops written from Aggregators.java's rules, and
numpy sorts.  tests/test_gpu_value_domain.py compares the HIP engine with
the oracle on these values; the transcribed known answers pin the oracle on
small, friendly literals only.

Also the conditions on tests/datasets.py's edge generators that keep the
GPU tests from turning into error-parity tests: which queries the reference
accepts on each kind of values.
"""
import math
import struct

import numpy as np
import pytest

from opentsdb_amd import core
from oracle import pyoracle
from tests import datasets
from tests.test_gpu_parity import _raw, _spec, _vals
from tests.value_domain import (AGGS, COUNTER_TOPS, DS, RATE_AGGS, RATE_DS,
                                WINDOWS, base_batch, counter_batch,
                                edge_batch, matrix, rate_options)

A = core.Aggregators
LENGTHS = [1, 2, 3, 50, 257]
MASK = (1 << 64) - 1


# ---------------------------------------------------- Java long in Python
def wrap(x):
    """The low 64 bits of x as a signed long (Java's overflow rule)."""
    x &= MASK
    return x - (1 << 64) if x >> 63 else x


def jdiv(a, b):
    """Java long division: truncates toward zero; MIN / -1 wraps to MIN."""
    q = abs(a) // abs(b)
    return wrap(q if (a < 0) == (b < 0) else -q)


def d2l(d):
    """Java's (long) cast of a double: NaN -> 0, saturating."""
    if d != d:
        return 0
    if d >= 2.0 ** 63:
        return 2**63 - 1
    if d <= -2.0 ** 63:
        return -2**63
    return int(d)


def welford(xs):
    """StdDev.runLong / runDouble's loop (Aggregators.java:504-523) in
    Python floats; the variance M2 / (n - 1) with n one past the count."""
    old = xs[0]
    if len(xs) == 1:
        return None
    n, m2 = 2, 0.0
    for x in xs[1:]:
        new = old + (x - old) / n
        m2 += (x - old) * (x - new)
        old = new
        n += 1
    return m2 / (n - 1)


def long_model(agg, v):
    v = [int(x) for x in v]
    if agg in ("sum", "zimsum"):
        return wrap(sum(v))
    if agg == "avg":  # Aggregators.java:371-379: long sum / int n
        return jdiv(wrap(sum(v)), len(v))
    if agg == "squareSum":  # :269-277
        return wrap(sum(wrap(x * x) for x in v))
    if agg == "mult":
        r = 1
        for x in v:
            r = wrap(r * x)
        return r
    if agg == "min":
        return min(v)
    if agg == "max":
        return max(v)
    if agg == "first":
        return v[0]
    if agg == "last":
        return v[-1]
    if agg == "diff":  # :582-595
        return 0 if len(v) == 1 else wrap(v[-1] - v[0])
    if agg == "count":
        return len(v)
    if agg == "median":  # :403-413
        return sorted(v)[len(v) // 2]
    raise ValueError(agg)


def _bigints(n, seed):
    return datasets.edge_values("bigint", np.random.default_rng(seed), n)[0]


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("agg", ["sum", "zimsum", "avg", "squareSum", "mult",
                                 "min", "max", "first", "last", "diff",
                                 "count", "median"])
def test_run_long_is_java_long_arithmetic(agg, n):
    for seed in range(8):
        v = _bigints(n, 100 * n + seed)
        assert pyoracle.run_long(A.get(agg).id, v) == long_model(agg, v), (
            agg, n, seed)


def test_run_long_wrap_cases():
    """Hand-picked: MIN / -1, sums that wrap twice, a truncating average of
    a negative sum, MIN * MIN."""
    lo, hi = datasets.LONG_MIN, datasets.LONG_MAX
    for agg, v, exp in (("avg", [lo], lo), ("avg", [-7, 0], -3),
                        ("avg", [hi, hi, 2], wrap(2 * hi + 2) // 3),
                        ("sum", [hi, 1], lo), ("sum", [lo, lo], 0),
                        ("diff", [hi, lo], 1), ("mult", [lo, -1], lo),
                        ("squareSum", [lo], 0), ("squareSum", [hi], 1),
                        ("squareSum", [2**32, 3], 9)):
        assert long_model(agg, v) == exp
        assert pyoracle.run_long(A.get(agg).id, np.array(v, np.int64)) == exp


def test_model_division_is_javas():
    assert jdiv(-7, 2) == -3 and jdiv(7, -2) == -3 and jdiv(-7, -2) == 3
    assert jdiv(datasets.LONG_MIN, -1) == datasets.LONG_MIN
    assert wrap(2**63) == -2**63 and wrap(-2**63 - 1) == 2**63 - 1


@pytest.mark.parametrize("n", LENGTHS)
def test_run_long_dev(n):
    """StdDev.runLong: the same Welford loop in Python floats, bit for bit
    ((long) of the root), and the two-pass variance through math.fsum to
    1e-9 relative: Welford's error is about n * eps * (1 + mean^2 / var),
    and the mean of whole-range longs is below their deviation, so 257
    values keep it under 1e-13; the (long) cast adds at most 1."""
    for seed in range(8):
        v = _bigints(n, 900 + 10 * n + seed)
        got = pyoracle.run_long(A.DEV.id, v)
        var = welford([float(int(x)) for x in v])
        assert got == (0 if var is None else d2l(math.sqrt(var)))
        if n > 1:
            mean = math.fsum(float(int(x)) for x in v) / n
            two_pass = math.sqrt(math.fsum((float(int(x)) - mean) ** 2
                                           for x in v) / n)
            assert abs(got - two_pass) <= 1e-9 * two_pass + 1


# ----------------------------------------------------------- run_double
def _signed(n, seed):
    bits, _ = datasets.edge_values("signed", np.random.default_rng(seed), n)
    return bits.view(np.float64)


def _bits(x):
    return struct.pack(">d", x)


@pytest.mark.parametrize("n", LENGTHS)
def test_run_double_sum_avg(n):
    """Sequential double sums against math.fsum: within n * 2^-53 * sum|x|
    (the forward error bound of n - 1 rounded adds)."""
    for seed in range(8):
        v = _signed(n, 40 * n + seed)
        bound = n * 2.0 ** -53 * math.fsum(abs(x) for x in v)
        s = math.fsum(v)
        assert abs(pyoracle.run_double(A.SUM.id, v) - s) <= bound
        assert abs(pyoracle.run_double(A.ZIMSUM.id, v) - s) <= bound
        assert abs(pyoracle.run_double(A.AVG.id, v) - s / n) <= \
            bound / n + 2.0 ** -53 * abs(s / n)


def _min(v):  # Aggregators.java:315-327: strict <, so the earliest stays
    m = v[0]
    for x in v[1:]:
        if x < m:
            m = x
    return m


def _max(v):  # :349-361
    m = v[0]
    for x in v[1:]:
        if x > m:
            m = x
    return m


@pytest.mark.parametrize("n", LENGTHS)
def test_run_double_order_rules(n):
    """min / max / first / last / diff bit for bit, which of -0.0 and 0.0
    survives included: strict comparisons keep the earliest of equal
    values."""
    for seed in range(12):
        v = list(_signed(n, 70 * n + seed))
        if seed % 3 == 0:  # nothing but zeros of both signs
            v = [(-0.0 if (i * 7 + seed) % 3 else 0.0) for i in range(n)]
        a = np.array(v)
        for agg, exp in (("min", _min(v)), ("max", _max(v)),
                         ("mimmin", _min(v)), ("mimmax", _max(v)),
                         ("first", v[0]), ("last", v[-1]),
                         ("diff", 0.0 if n == 1 else v[-1] - v[0])):
            got = pyoracle.run_double(A.get(agg).id, a)
            assert _bits(got) == _bits(exp), (agg, n, seed, got, exp)
    assert _bits(pyoracle.run_double(A.MIN.id, np.array([0.0, -0.0]))) == \
        _bits(0.0)
    assert _bits(pyoracle.run_double(A.MAX.id, np.array([-0.0, 0.0]))) == \
        _bits(-0.0)


def compare_to_key(x):
    """Double.compareTo's total order on non-NaN doubles: by value, -0.0
    before 0.0."""
    return (x, 0 if math.copysign(1.0, x) < 0 else 1)


@pytest.mark.parametrize("n", LENGTHS)
def test_run_double_median(n):
    """Median.runDouble (Aggregators.java:416-430): Collections.sort of a
    List<Double>, element n / 2 — bit for bit, zeros of both signs
    included."""
    for seed in range(12):
        v = list(_signed(n, 130 * n + seed))
        if seed % 3 == 0:
            v = [(-0.0 if (i * 5 + seed) % 2 else 0.0) for i in range(n)]
        exp = sorted(v, key=compare_to_key)[n // 2]
        got = pyoracle.run_double(A.MEDIAN.id, np.array(v))
        assert _bits(got) == _bits(exp), (n, seed)


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("name,p", [("p50", 50.0), ("p75", 75.0),
                                    ("p99", 99.0), ("p999", 99.9),
                                    ("ep95r3", 95.0), ("ep50r7", 50.0)])
def test_run_double_percentiles(name, p, n):
    """PercentileAgg.runDouble (Aggregators.java:689-706) never sets the
    estimation type: LEGACY, pos = p (n + 1) / 100 over the sorted values,
    lower + (pos - floor(pos)) * (upper - lower)."""
    for seed in range(6):
        v = _signed(n, 170 * n + seed)
        a = np.sort(v)
        pos = (p / 100.0) * (n + 1)
        if n == 1 or pos < 1:
            exp = a[0]
        elif pos >= n:
            exp = a[-1]
        else:
            k = int(math.floor(pos))
            exp = a[k - 1] + (pos - k) * (a[k] - a[k - 1])
        got = pyoracle.run_double(A.get(name).id, v)
        assert got == exp, (name, n, seed, got, exp)


# ------------------------------------------------- generator conditions
def _accepted(spec, b):
    try:
        return pyoracle.group_by(spec, b)
    except pyoracle.OracleError:
        return None


def _queries():
    s, e = WINDOWS[0]
    for agg, ds, fill in matrix():
        yield "%s:1m-%s-%s" % (agg, ds, fill), _spec(agg, ds, fill, s, e)
    for agg in AGGS:
        yield "raw:" + agg, _raw(agg, s, e)


@pytest.mark.parametrize("grouping", ["a", "b"])
@pytest.mark.parametrize("kind", ["signed", "bigint", "bigmixed",
                                  "nanpayload"])
def test_generators_overflow_only_through_mult(kind, grouping):
    """On these kinds the reference accepts every query of the GPU matrix
    (no aggregator or downsampler of it is `mult`): the GPU tests compare
    values, not statuses."""
    assert "mult" not in AGGS and "mult" not in DS
    b = edge_batch(kind, grouping)
    for where, spec in _queries():
        ref = _accepted(spec, b)
        assert ref is not None, (kind, where)
        assert sum(len(r) for r in ref) > 0, (kind, where)


@pytest.mark.parametrize("top_name", list(COUNTER_TOPS))
def test_counter_generator(top_name):
    top, as_float = COUNTER_TOPS[top_name]
    b = counter_batch(top_name)
    assert (b.is_float == (1 if as_float else 0)).all()
    v = b.val.view(np.float64).astype(np.int64) if as_float else b.val
    assert v.min() >= 0 and v.max() <= top
    assert v.max() > top - 2**44
    wraps = sum(int((np.diff(v[b.offsets[s]:b.offsets[s + 1]]) < 0).sum())
                for s in range(b.n_series))
    assert wraps >= 5, wraps  # counters do pass `top`
    if not as_float:  # differencing the doubles is not the long difference
        d = np.diff(v)
        assert (np.diff(v.astype(np.float64)) != d.astype(np.float64)).any()
    s, e = WINDOWS[0]
    for ri, ro in enumerate(rate_options(top)):
        for agg in RATE_AGGS:
            assert _accepted(_raw(agg, s, e, rate=True, ro=ro), b) \
                is not None, (top_name, ri, agg)
            for ds in RATE_DS:
                spec = _spec(agg, ds, "none", s, e, rate=True, ro=ro)
                assert _accepted(spec, b) is not None, (top_name, ri, agg, ds)


@pytest.mark.parametrize("grouping", ["a", "b"])
def test_wide_generator_overflows_some(grouping):
    """`wide` is the "Got Infinity" kind: the reference rejects some of the
    matrix and accepts some."""
    b = edge_batch("wide", grouping)
    res = [_accepted(spec, b) is not None for _, spec in _queries()]
    assert any(res) and not all(res), (sum(res), len(res))


def test_grouping_regimes():
    """Group sizes that put each grouping in its selection regime: at most
    SEL_K = 32 members (a); above it and, per bucket, at most SS_CAP = 1,024
    non-NaN values (b); more than SS_CAP values in some bucket (c)."""
    assert np.diff(base_batch("a").group_offsets).max() <= 32
    assert np.diff(base_batch("b").group_offsets).tolist() == [300]
    assert np.diff(base_batch("f").group_offsets).min() > 32
    s, e = WINDOWS[0]
    ref = pyoracle.group_by(_spec("count", "max", "none", s, e),
                            edge_batch("signed", "c"))
    n = _vals(ref[0]["bits"], ref[0]["is_int"])
    assert n.max() > 1024, n.max()


def test_edge_values_hold_their_edges():
    rng = np.random.default_rng(1)
    m = 4000
    bits, f = datasets.edge_values("signed", rng, m)
    v = bits.view(np.float64)
    assert f.all() and np.isfinite(v).all() and (v < 0).any()
    assert (bits == 0).any() and (bits == np.int64(-2**63)).any()  # +-0.0
    assert (v == 5e-324).any() and (v == -5e-324).any()
    assert (v == datasets.DBL_MIN_NORMAL).any() and np.abs(v).max() < 1e152
    bits, f = datasets.edge_values("wide", rng, m)
    v = bits.view(np.float64)
    assert np.isfinite(v).all() and (v == datasets.DBL_MAX).any() and \
        (v == -datasets.DBL_MAX).any()
    bits, f = datasets.edge_values("bigint", rng, m)
    assert not f.any()
    for x in (datasets.LONG_MIN, datasets.LONG_MAX, -1, 0, 2**53 - 3,
              2**53 + 3):
        assert (bits == x).any(), x
    assert (np.abs(bits.astype(np.float64)) > 2.0 ** 62).mean() > 0.3
    bits, f = datasets.edge_values("bigmixed", rng, m)
    assert 0.4 < f.mean() < 0.6
    bits, f = datasets.edge_values("nanpayload", rng, m)
    nan = np.isnan(bits.view(np.float64))
    assert 0.05 < nan.mean() < 0.15
    assert set(bits[nan].view(np.uint64).tolist()) == \
        set(datasets.NAN_PATTERNS)
    bits, f = datasets.edge_values("f4edge", rng, m)
    v = bits.view(np.float64)
    ok = ~np.isnan(v)
    assert (v[ok].astype(np.float32).astype(np.float64) == v[ok]).all()
    for x in (1.401298464324817e-45, -1.401298464324817e-45,
              3.4028234663852886e38, -3.4028234663852886e38):
        assert (v == x).any(), x
    assert (bits == 0).any() and (bits == np.int64(-2**63)).any()
    assert (~ok).any()
    for x in v[ok][:200]:
        struct.pack(">f", x)  # cells.encode_point packs with '>f'
