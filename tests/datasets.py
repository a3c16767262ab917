"""Seeded synthetic query batches for parity tests (small enough for the
oracle to finish in seconds).  Shapes follow BaseTsdbTest's datasets
(BaseTsdbTest.java:612-791) in spirit: regular cadences with missing points,
offsets, late/early series, long and double values, plus the edge cases the
reference tests cover (empty spans, points outside the window, NaNs)."""
import numpy as np

from opentsdb_amd.batch import HostBatch, groups_from_ids

T0 = 1356998400000  # BaseTsdbTest base time, ms


def random_batch(seed, n_series=40, n_groups=5, span_ms=3 * 3600 * 1000,
                 cadence_ms=10000, value_kind="float", nan_frac=0.0,
                 empty_frac=0.05, outside=True, counter=False,
                 big_group=False, t0=T0):
    rng = np.random.default_rng(seed)
    offs = [0]
    tss, vals, isf = [], [], []
    for s in range(n_series):
        if rng.random() < empty_frac:
            offs.append(offs[-1])
            continue
        n = span_ms // cadence_ms
        phase = int(rng.integers(0, cadence_ms))
        t = t0 + phase + cadence_ms * np.arange(n, dtype=np.int64)
        keep = rng.random(n) > 0.05
        # an outage
        if rng.random() < 0.4:
            a = int(rng.integers(0, n))
            keep[a:a + int(rng.integers(1, n // 3 + 2))] = False
        # late start / early end
        if rng.random() < 0.2:
            keep[:int(rng.integers(0, n // 2))] = False
        if rng.random() < 0.2:
            keep[n - int(rng.integers(0, n // 2)):] = False
        if outside and rng.random() < 0.3:
            # points before the window start and after the end
            t = t - int(rng.integers(0, 2 * 3600 * 1000))
        t = t[keep]
        m = len(t)
        if counter:
            inc = rng.integers(0, 1000, m)
            v = np.cumsum(inc) + int(rng.integers(0, 2**32))
            rs = rng.random(m) < 0.02
            for i in np.nonzero(rs)[0]:
                v[i:] -= v[i]
            f = np.zeros(m, np.uint8)
            bits = v.astype(np.int64)
        elif value_kind == "float":
            v = rng.random(m) * 100.0
            if nan_frac:
                v[rng.random(m) < nan_frac] = np.nan
            bits = v.view(np.int64)
            f = np.ones(m, np.uint8)
        elif value_kind == "offset":
            # large values with a small spread (a gauge of ~3e9 moving by
            # < 1e4): Welford's result depends on its order at ~1e-11
            v = 3.0e9 + rng.random(m) * 1.0e4
            bits = v.view(np.int64)
            f = np.ones(m, np.uint8)
        elif value_kind == "int":
            bits = rng.integers(-50, 100, m).astype(np.int64)
            f = np.zeros(m, np.uint8)
        else:  # mixed
            f = (rng.random(m) < 0.5).astype(np.uint8)
            fv = (rng.random(m) * 100.0).view(np.int64)
            iv = rng.integers(0, 100, m).astype(np.int64)
            bits = np.where(f == 1, fv, iv)
        tss.append(t)
        vals.append(bits)
        isf.append(f)
        offs.append(offs[-1] + m)
    ts = np.concatenate(tss) if tss else np.zeros(0, np.int64)
    val = np.concatenate(vals) if vals else np.zeros(0, np.int64)
    isf = np.concatenate(isf) if isf else np.zeros(0, np.uint8)
    if big_group:
        gid = np.zeros(n_series, np.int64)
    else:
        gid = rng.integers(0, n_groups, n_series)
        gid[:n_groups] = np.arange(n_groups)  # every group non-empty
    g_off, members = groups_from_ids(gid, n_groups if not big_group else 1)
    return HostBatch(np.array(offs, np.int64), ts, val, isf, None, g_off,
                     members)


# ------------------------------------------------------- value-domain edges
LONG_MIN, LONG_MAX = -2**63, 2**63 - 1
DBL_MAX = 1.7976931348623157e308
DBL_MIN_NORMAL = 2.2250738585072014e-308
NAN_PATTERNS = (0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001,
                0x7FFFFFFFFFFFFFFF,
                0x7FF4DEAD0BADF00D)  # the engine's absent-bucket sentinel
EDGE_KINDS = ("signed", "wide", "bigint", "bigmixed", "nanpayload", "f4edge")


def _signed(rng, m, lo=-150, hi=150):
    v = rng.standard_normal(m) * 10.0 ** rng.integers(lo, hi, m)
    z = rng.random(m)
    v[z < 0.05] = 0.0
    v[(z >= 0.05) & (z < 0.10)] = -0.0
    v[(z >= 0.10) & (z < 0.12)] = 5e-324
    v[(z >= 0.12) & (z < 0.14)] = -5e-324
    v[(z >= 0.14) & (z < 0.16)] = DBL_MIN_NORMAL
    return v


def _bigint(rng, m):
    v = rng.integers(LONG_MIN, LONG_MAX, m, dtype=np.int64, endpoint=True)
    z = rng.random(m)
    v[z < 0.03] = LONG_MIN
    v[(z >= 0.03) & (z < 0.06)] = LONG_MAX
    v[(z >= 0.06) & (z < 0.10)] = -1
    v[(z >= 0.10) & (z < 0.14)] = 0
    near = (z >= 0.14) & (z < 0.21)
    v[near] = 2**53 + rng.integers(-3, 4, int(near.sum()))
    return v


def edge_values(kind, rng, m):
    """(bits int64[m], is_float uint8[m]) of m values from the edges of the
    value domain (the values random_batch never draws):

    signed      both signs over 10^+-150 (no sum, square or difference of
                them overflows; only `mult` can), +-0.0, the smallest
                subnormals, the smallest normal
    wide        10^+-300 and +-Double.MAX_VALUE: sums, squares, LERPs and
                rates overflow ("Got Infinity")
    bigint      longs over the whole range, LONG_MIN / LONG_MAX, -1, 0 and
                2^53 +- 3 (long arithmetic wraps; long -> double rounds)
    bigmixed    per point bigint or signed
    nanpayload  signed with ~10 % NaNs of several bit patterns, the
                absent-bucket sentinel's included
    f4edge      doubles that are exactly float32 values, from float32 bit
                patterns (normals of both signs, subnormals, +-0.0,
                +-FLT_MAX, NaNs): every value packs with '>f'"""
    if kind == "signed":
        return _signed(rng, m).view(np.int64), np.ones(m, np.uint8)
    if kind == "wide":
        v = rng.standard_normal(m) * 10.0 ** rng.integers(-300, 301, m)
        z = rng.random(m)
        v[z < 0.02] = DBL_MAX
        v[(z >= 0.02) & (z < 0.04)] = -DBL_MAX
        v[~np.isfinite(v)] = DBL_MAX
        return v.view(np.int64), np.ones(m, np.uint8)
    if kind == "bigint":
        return _bigint(rng, m), np.zeros(m, np.uint8)
    if kind == "bigmixed":
        f = (rng.random(m) < 0.5).astype(np.uint8)
        bits = np.where(f == 1, _signed(rng, m).view(np.int64),
                        _bigint(rng, m))
        return bits, f
    if kind == "nanpayload":
        bits = _signed(rng, m).view(np.int64).copy()
        nan = rng.random(m) < 0.10
        pat = np.array(NAN_PATTERNS, np.uint64).view(np.int64)
        bits[nan] = pat[rng.integers(0, len(pat), int(nan.sum()))]
        return bits, np.ones(m, np.uint8)
    if kind == "f4edge":
        b32 = rng.integers(0, 2**32, m, dtype=np.uint64).astype(np.uint32)
        # random patterns are normals of both signs but for exponents 0 / 255
        exp = (b32 >> np.uint32(23)) & np.uint32(0xFF)
        b32[(exp == 0) | (exp == 255)] = np.uint32(0x3F800000)
        special = np.array([0x00000001, 0x007FFFFF, 0x80000001, 0x807FFFFF,
                            0x00000000, 0x80000000, 0x7F7FFFFF, 0xFF7FFFFF,
                            0x00800000, 0x7FC00000, 0xFFC00000, 0x7F800001,
                            0x7FFFFFFF], np.uint32)
        z = rng.random(m) < 0.35
        b32[z] = special[rng.integers(0, len(special), int(z.sum()))]
        with np.errstate(invalid="ignore"):  # widening a signalling NaN
            v = b32.view(np.float32).astype(np.float64)
        return v.view(np.int64), np.ones(m, np.uint8)
    raise ValueError(kind)


def with_values(hb, bits, is_float):
    """A copy of a batch (same timestamps, offsets and groups) holding the
    given values."""
    assert len(bits) == len(hb.ts) == len(is_float)
    return HostBatch(np.array(hb.offsets, np.int64), np.array(hb.ts, np.int64),
                     np.ascontiguousarray(bits, np.int64).copy(),
                     np.ascontiguousarray(is_float, np.uint8).copy(), None,
                     np.array(hb.group_offsets, np.int64),
                     np.array(hb.group_members, np.int64))


def edge_counters(hb, rng, top, as_float):
    """A copy of a batch whose every series is a running counter near `top`:
    it starts within 2^44 below `top`, takes increments below 2^40 and, when
    it passes `top`, restarts from the remainder (a counter wrap at `top`).
    Longs, or doubles (as_float: `top` <= 2^53 keeps them exact).  The
    running sum is done in Python integers (past int64 at top = 2^63 - 1)."""
    top = int(top)
    bits = np.zeros(len(hb.ts), np.int64)
    for s in range(hb.n_series):
        a, b = int(hb.offsets[s]), int(hb.offsets[s + 1])
        v = top - int(rng.integers(0, 2**44))
        for i in range(a, b):
            v += int(rng.integers(0, 2**40))
            if v > top:
                v -= top
            bits[i] = (np.float64(v).view(np.int64) if as_float else v)
    f = np.full(len(hb.ts), 1 if as_float else 0, np.uint8)
    return with_values(hb, bits, f)
