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
