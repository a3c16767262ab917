"""Plain-Python model of the reference's histogram query path, restated at
the iterator level (not a vectorised twin of the kernels):

  Hist                     SimpleHistogram: a TreeMap of (lower, upper) keys
                           (Float.compare on lower, then upper) to Java longs,
                           underflow, overflow; aggregate and percentile
                           (SimpleHistogram.java:124-164, :246-261)
  SpanView                 a span's seekable iterator
  Downsampler              HistogramDownsampler with its ValuesInInterval
                           (HistogramDownsampler.java:129-149, :195-377),
                           fixed intervals only
  AggregationIterator      HistogramAggregationIterator's constructor,
                           hasNext and next (:115-160, :229-301)
  group_query              HistogramSpanGroup.add + iterator() for each group

Java longs are Python integers reduced mod 2^64, intValue() mod 2^32 with
sign, the midpoint numpy.float32.
"""
import json
import os

import numpy as np

SUM = "SUM"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "kat_histogram.json")


def wrap_long(v):
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >> 63 else v


def int_value(v):
    """Long.intValue(): the low 32 bits, signed."""
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v >> 31 else v


def _float_bits(f):
    f = np.float32(f)
    return 0x7fc00000 if np.isnan(f) else int(f.view(np.int32))


def _float_order(f):
    """A sort key with Float.compare's order."""
    b = _float_bits(f)
    return b if b >= 0 else -(b & 0x7FFFFFFF) - 1


def key_order(k):
    return (_float_order(k[0]), _float_order(k[1]))


def make_key(lower, upper):
    """Keys are compared through floatToIntBits: every NaN is one key."""
    return (_float_bits(lower), _float_bits(upper))


def key_bounds(k):
    return (np.array(k[0], np.int32).view(np.float32),
            np.array(k[1], np.int32).view(np.float32))


_ORDER = {}


def _key_order_cached(k):
    o = _ORDER.get(k)
    if o is None:
        o = _ORDER[k] = key_order(key_bounds(k))
    return o


class Hist:
    """SimpleHistogram.  buckets: {make_key(lower, upper): long}."""

    def __init__(self, buckets=None, underflow=0, overflow=0):
        self.buckets = dict(buckets or {})
        self.underflow, self.overflow = underflow, overflow

    @staticmethod
    def of(triples, underflow=0, overflow=0):
        return Hist({make_key(lo, up): wrap_long(int(c))
                     for lo, up, c in triples}, wrap_long(int(underflow)),
                    wrap_long(int(overflow)))

    def clone(self):
        return Hist(self.buckets, self.underflow, self.overflow)

    def entries(self):
        """The TreeMap's entrySet(): keys in compareTo order."""
        for k in sorted(self.buckets, key=_key_order_cached):
            yield k, self.buckets[k]

    def aggregate(self, other, func):
        if func == SUM:
            for k, v in other.entries():
                self.buckets[k] = wrap_long(self.buckets.get(k, 0) + v)
            self.overflow = wrap_long(other.overflow + self.overflow)
            self.underflow = wrap_long(other.underflow + self.underflow)
        # else: LOG.debug("Unsupported histogram aggregation used")

    def percentile(self, perc):
        """perc: a Python float (the double the float percentile widens to)."""
        perc = np.float64(perc)
        if perc < 1.0 or perc > 100.0:
            return -1.0
        bucket_sum = 0
        for _, v in self.entries():
            bucket_sum = int_value(bucket_sum + int_value(v))
        running = 0
        value = 0.0
        with np.errstate(all="ignore"):
            for k, v in self.entries():
                running = wrap_long(running + int_value(v))
                area = (np.float64(running) * np.float64(100.0)
                        / np.float64(bucket_sum))
                if area >= perc:
                    lo, up = key_bounds(k)
                    value = float(np.float64((np.float32(lo) + np.float32(up))
                                             / np.float32(2)))
                    break
        return value


class SpanView:
    """A span's points [(ts, Hist)] as a HistogramSeekableView."""

    def __init__(self, points):
        self.points, self.i = points, 0

    def hasNext(self):
        return self.i < len(self.points)

    def next(self):
        p = self.points[self.i]
        self.i += 1
        return p

    def seek(self, ts):
        self.i = 0
        while self.i < len(self.points) and self.points[self.i][0] < ts:
            self.i += 1


class Downsampler:
    """HistogramDownsampler over a fixed interval; hist_agg: SUM or None
    (DownsamplingSpecification.getHistogramAggregation)."""

    def __init__(self, source, interval, hist_agg):
        self.source, self.interval, self.hist_agg = source, interval, hist_agg
        # ValuesInInterval
        self.end_interval = interval
        self.has_next_value = False
        self.next_dp = None
        self.initialized = False

    def _align(self, t):
        r = abs(t) % self.interval  # Java's %: the sign of the dividend
        return t - (r if t >= 0 else -r)

    def _move_to_next_value(self):
        if self.source.hasNext():
            self.has_next_value = True
            self.next_dp = self.source.next()
        else:
            self.has_next_value = False

    def _initialize_if_not_done(self):
        if not self.initialized:
            self.initialized = True
            if self.source.hasNext():
                self._move_to_next_value()
                self.end_interval = (self._align(self.next_dp[0])
                                     + self.interval)

    def _reset_end_of_interval(self):
        if self.has_next_value:
            self.end_interval = self._align(self.next_dp[0]) + self.interval

    def _move_to_next_interval(self):
        self._initialize_if_not_done()
        self._reset_end_of_interval()

    def _interval_timestamp(self):
        return self._align(self.end_interval - self.interval)

    def _has_next_value(self):
        self._initialize_if_not_done()
        return self.has_next_value and self.next_dp[0] < self.end_interval

    def _next_value(self):
        assert self._has_next_value()
        v = self.next_dp[1].clone()
        self._move_to_next_value()
        return v

    def seek(self, ts):
        self.source.seek(self._align(ts + self.interval - 1))
        self.initialized = False

    def hasNext(self):
        return self._has_next_value()

    def next(self):
        assert self.hasNext()
        value = self._next_value()
        while self._has_next_value():
            value.aggregate(self._next_value(), self.hist_agg)
        ts = self._interval_timestamp()
        self._move_to_next_interval()
        return ts, value


class AggregationIterator:
    def __init__(self, iterators, start, end):
        self.iterators = list(iterators)
        self.start, self.end = start, end
        n = len(self.iterators)
        self.timestamps = [0] * n
        self.values = [None] * n
        for i, it in enumerate(self.iterators):
            it.seek(start)
            if not it.hasNext():
                self._end_reached(i)
                continue
            ts, v = it.next()
            if ts >= start:
                self._put(i, ts, v)
            else:
                self._end_reached(i)

    def _end_reached(self, i):
        self.timestamps[i] = 0
        self.iterators[i] = None

    def _put(self, i, ts, v):
        self.timestamps[i] = ts
        self.values[i] = v.clone()

    def _move_to_next(self, i):
        it = self.iterators[i]
        if it.hasNext():
            self._put(i, *it.next())
        else:
            self._end_reached(i)

    def hasNext(self):
        return any(t != 0 and t <= self.end for t in self.timestamps)

    def next(self):
        min_ts, first, multiple = None, -1, False
        for i, t in enumerate(self.timestamps):
            if t == 0 or t > self.end:
                continue
            if min_ts is None or t < min_ts:
                min_ts, first, multiple = t, i, False
            elif t == min_ts:
                multiple = True
        assert first >= 0
        value = self.values[first]
        if multiple:
            for i in range(first + 1, len(self.iterators)):
                if self.timestamps[i] == min_ts:
                    value.aggregate(self.values[i], SUM)
                    self._move_to_next(i)
        self._move_to_next(first)
        return min_ts, value


def group_query(start_ms, end_ms, interval, hist_agg, series, groups):
    """series: per series a list of (ts, Hist) in time order; groups: lists of
    series indices.  Returns per group [(ts, Hist)]: HistogramSpanGroup.add's
    filter, then iterator() drained."""
    out = []
    for members in groups:
        spans = []
        for s in members:
            pts = series[s]
            if not pts:
                continue
            if pts[0][0] <= end_ms and pts[-1][0] >= start_ms:
                spans.append(pts)
        it = AggregationIterator(
            [Downsampler(SpanView(p), interval, hist_agg) for p in spans],
            start_ms, end_ms)
        res = []
        while it.hasNext():
            res.append(it.next())
        out.append(res)
    return out


def load_kats():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


def hist_of_case(h):
    return Hist.of(h["buckets"], h["underflow"], h["overflow"])


def kat_query_points(c):
    """A query KAT's spans as the model takes them: the one-long test
    histogram is one bucket (0, 1) holding the value."""
    return [[(ts, Hist.of([(0.0, 1.0, v)])) for ts, v in s]
            for s in c["series"]]
