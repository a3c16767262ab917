"""Host mirror of the histogram query's inputs (otsdb_hist_columns).

The engine takes decoded histograms as one dense count matrix over the
query's bucket schema; this module builds both from the sparse
{(lower, upper): count} maps the Java side holds
(SimpleHistogram.getHistogram(), HistogramDataPoint.getHistogramBucketsIfHas):

  HistogramBucket     a (lower, upper) key in TreeMap order
                      (HistogramDataPoint.java:147-165: Float.compare on the
                      lower bound, then on the upper)
  union_schema        the sorted union of the keys of every histogram
  densify             the [N][K + 2] int64 matrix, underflow and overflow in
                      the last two columns, 0 where a histogram lacks a key
  percentile_spec     the percentiles as the reference holds them: floats
                      (HistogramDataPointsToDataPointsAdaptor.percentile)
  encode_simple, hist_qualifier, hist_rows
                      the stored form: a histogram's value bytes, its
                      qualifier, and the storage rows of a set of series
                      (what otsdb_hist_run_rows decodes on the device)

A key a histogram lacks is padded with 0: a zero-count key never qualifies
for a percentile (its area is its predecessor's, or +-0.0 / NaN at the start),
so the padding changes no percentile.
"""
import functools

import numpy as np

from . import abi
from .core import IllegalArgumentException, UnsupportedOperationException


def float_to_int_bits(f):
    """Float.floatToIntBits: the IEEE bits, every NaN the canonical one."""
    f = np.float32(f)
    if np.isnan(f):
        return 0x7fc00000
    return int(f.view(np.int32))


def float_compare(a, b):
    """Float.compare: numeric order, -0.0 below 0.0, NaN above everything."""
    a, b = np.float32(a), np.float32(b)
    if a < b:
        return -1
    if a > b:
        return 1
    ia, ib = float_to_int_bits(a), float_to_int_bits(b)
    return 0 if ia == ib else (-1 if ia < ib else 1)


@functools.total_ordering
class HistogramBucket:
    """A regular bucket key (HistogramDataPoint.HistogramBucket): float
    bounds, compareTo's order."""
    __slots__ = ("lower", "upper")

    def __init__(self, lower, upper):
        self.lower, self.upper = np.float32(lower), np.float32(upper)

    def compare_to(self, that):
        c = float_compare(self.lower, that.lower)
        return c if c else float_compare(self.upper, that.upper)

    def __eq__(self, that):
        return self.compare_to(that) == 0

    def __lt__(self, that):
        return self.compare_to(that) < 0

    def __hash__(self):
        return hash((float_to_int_bits(self.lower),
                     float_to_int_bits(self.upper)))

    def __repr__(self):
        return "HistogramBucket(%r, %r)" % (float(self.lower),
                                            float(self.upper))


class Histogram:
    """One decoded histogram point: {(lower, upper): count} plus the
    underflow and overflow counts (SimpleHistogram)."""

    def __init__(self, buckets, underflow=0, overflow=0):
        self.buckets = {}
        for k, v in dict(buckets).items():
            if not isinstance(k, HistogramBucket):
                k = HistogramBucket(*k)
            self.buckets[k] = int(v)
        self.underflow, self.overflow = int(underflow), int(overflow)


def union_schema(histograms):
    """The query's bucket schema: the keys of every histogram, sorted.
    Returns (lower, upper) float32 arrays of K entries."""
    keys = set()
    for h in histograms:
        keys.update(h.buckets.keys())
    keys = sorted(keys)
    return (np.array([k.lower for k in keys], np.float32),
            np.array([k.upper for k in keys], np.float32))


def _wrap_long(v):
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >> 63 else v


def densify(series_of_histograms, schema):
    """The [N][K + 2] count matrix of the series' histograms in series order
    (the batch's point order) over `schema` = (lower, upper); columns K and
    K + 1 are underflow and overflow.  A key outside the schema is an
    error."""
    lower, upper = schema
    col = {HistogramBucket(lo, up): i
           for i, (lo, up) in enumerate(zip(lower, upper))}
    K = len(lower)
    rows = [h for s in series_of_histograms for h in s]
    out = np.zeros((len(rows), K + 2), np.int64)
    for i, h in enumerate(rows):
        for k, v in h.buckets.items():
            if k not in col:
                raise IllegalArgumentException("%r is not in the schema" % k)
            out[i, col[k]] = _wrap_long(v)
        out[i, K] = _wrap_long(h.underflow)
        out[i, K + 1] = _wrap_long(h.overflow)
    return out


def percentile_spec(percentiles):
    """The percentiles of a call as float32 (the reference parses and holds
    them as floats: 99.9 is 99.90000152587890625 there)."""
    p = np.ascontiguousarray(
        [np.float32(x) for x in percentiles], dtype=np.float32).reshape(-1)
    if len(p) > abi.HIST_MAX_PCT:
        raise UnsupportedOperationException(
            "%d percentiles: a histogram call takes up to %d"
            % (len(p), abi.HIST_MAX_PCT))
    return p


class HistColumns:
    """otsdb_hist_columns on the host: the schema and the count matrix."""

    def __init__(self, lower, upper, counts):
        self.lower = np.ascontiguousarray(lower, dtype=np.float32)
        self.upper = np.ascontiguousarray(upper, dtype=np.float32)
        self.counts = np.ascontiguousarray(counts, dtype=np.int64)
        K = len(self.lower)
        if len(self.upper) != K:
            raise IllegalArgumentException("lower and upper differ in length")
        if self.counts.ndim != 2 or self.counts.shape[1] != K + 2:
            raise IllegalArgumentException(
                "counts is %r for %d buckets" % (self.counts.shape, K))

    @property
    def n_bins(self):
        return len(self.lower)

    def as_abi(self):
        return abi.HistColumns(self.n_bins, self.lower.ctypes.data,
                               self.upper.ctypes.data,
                               self.counts.ctypes.data
                               if self.counts.size else None)


# ------------------------------------------------- stored form (storage rows)
# What TSDB.addHistogramPoint writes and otsdb_hist_run_rows reads: the
# qualifier of Internal.getQualifier with HistogramDataPoint.PREFIX and the
# value of SimpleHistogram.histogram(true) through Kryo 3.0.0's Output.
HIST_PREFIX = 0x06
MAX_TIMESPAN = 3600
SECOND_MASK = 0xFFFFFFFF00000000


def write_var_long(v):
    """Output.writeLong(v, true): 7 value bits a byte from the least
    significant group, bit 7 set while more follow, the ninth byte whole."""
    v &= (1 << 64) - 1
    out = bytearray()
    for _ in range(8):
        if v >> 7 == 0:
            out.append(v)
            return bytes(out)
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def encode_simple(hist, codec_id):
    """The value bytes of `hist` (a Histogram) as
    SimpleHistogram.histogram(true) writes them: the codec id, the short
    bucket count, each key in TreeMap order as two big-endian floats and the
    var-long count, then the var-long underflow and overflow.  (A histogram
    without buckets whose underflow and overflow take one byte each is 5
    bytes: fromHistogram refuses anything under 6, so it is never read
    back.)"""
    keys = sorted(hist.buckets)
    out = bytearray([codec_id & 0xFF])
    out += (len(keys) & 0xFFFF).to_bytes(2, "big")
    for k in keys:
        out += np.array([k.lower, k.upper], ">f4").tobytes()
        out += write_var_long(hist.buckets[k])
    out += write_var_long(hist.underflow)
    out += write_var_long(hist.overflow)
    return bytes(out)


def hist_qualifier(ts, ms=None):
    """Internal.getQualifier(ts, 0x06) -> (base_s, qualifier): `ts` in
    seconds or, past 32 bits, in milliseconds as the reference tells them
    apart (ms: say so instead).  A second timestamp gives the 3-byte form
    (a short offset), a millisecond one the 5-byte form (an int offset)."""
    ts = int(ts)
    if ts < 1:
        raise IllegalArgumentException("The start timestamp has not been set")
    if ms is None:
        ms = (ts & SECOND_MASK) != 0
    if ms:
        base = ts // 1000 - (ts // 1000) % MAX_TIMESPAN
        return base, bytes([HIST_PREFIX]) + (ts - base * 1000).to_bytes(4, "big")
    base = ts - ts % MAX_TIMESPAN
    return base, bytes([HIST_PREFIX]) + (ts - base).to_bytes(2, "big")


def hist_rows(series_points, codec_id):
    """storage.HostRawRows of the series' histograms: series_points[s] is
    [(ts_ms, Histogram)] in time order, one row per (series, base hour), one
    cell per point — a whole-second timestamp with the 3-byte qualifier, any
    other with the 5-byte one."""
    from .storage import HostRawRows
    rows = []
    for s, pts in enumerate(series_points):
        for ts, h in pts:
            ts = int(ts)
            base, q = (hist_qualifier(ts // 1000, ms=False) if ts % 1000 == 0
                       else hist_qualifier(ts, ms=True))
            if not rows or rows[-1][0] != s or rows[-1][1] != base:
                rows.append((s, base, []))
            rows[-1][2].append((q, encode_simple(h, codec_id)))
    rr = HostRawRows(rows, with_ts=False)
    rr.n_series = len(series_points)
    return rr
