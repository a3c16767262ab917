"""Plain-Python restatement of the gexp top-N functions highestMax and
highestCurrent (src/query/expression/HighestMax.java:40-148,
HighestCurrent.java:40-152) and of the iterator they run:
AggregationIterator(views, start, end, agg, LERP, rate = false) over
PostAggregatedDataPoints (AggregationIterator.java:395-797).

A series is a list of points (ts, value, is_int): value a Python int (a Java
long) when is_int, else a float.  Nothing here is vectorised or clever: it is
the yardstick the engine is compared with bit for bit.

`mut` names ONE deliberate mistake (MUTATIONS) for the tests that show the
GPU batches can tell the model from it; None is the reference."""
import math
import struct

LONG_MIN, LONG_MAX = -2 ** 63, 2 ** 63 - 1
DOUBLE_MIN_VALUE = 4.9e-324          # Double.MIN_VALUE: smallest POSITIVE
MS_MASK = 0xFFFFF00000000000         # Const.java:92
CANON_NAN = 0x7FF8000000000000

HIGHEST_MAX, HIGHEST_CURRENT = "highestMax", "highestCurrent"

OK, ILLEGAL_STATE, ILLEGAL_ARGUMENT, UNSUPPORTED = 0, 2, 3, 5

MUTATIONS = (
    "own_slot",        # values credited to the series' own slot
    "neg_inf_start",   # max_doubles started at -Infinity
    "no_interp",       # interpolated values left out
    "tie_high",        # ties broken by the higher index
    "current_own_last",  # highestCurrent from each series' own last point
    "no_long_pad",     # the zero padding of integer emissions dropped
    "no_lerp_past_end",  # points past `end` not used as LERP ends
)


# ------------------------------------------------------------ Java numbers
def jlong(v):
    """Wraps to a Java long."""
    v &= 0xFFFFFFFFFFFFFFFF
    return v - (1 << 64) if v >> 63 else v


def jdiv(a, b):
    """Java long division: truncating; MIN / -1 wraps."""
    q = abs(a) // abs(b)
    return jlong(q if (a < 0) == (b < 0) else -q)


def bits_of(d):
    return struct.unpack("<q", struct.pack("<d", d))[0]


def double_of(bits):
    return struct.unpack("<d", struct.pack("<q", bits))[0]


def canon_bits(d):
    """Double.doubleToLongBits: every NaN is the canonical one."""
    return CANON_NAN if d != d else bits_of(d)


def jmax(a, b):
    """Math.max(double, double): NaN if either is, +0.0 over -0.0."""
    if a != a:
        return a
    if b != b:
        return b
    if a == 0.0 and b == 0.0:
        return b if math.copysign(1.0, a) < 0 else a
    return a if a >= b else b


def compare_key(d):
    """An integer that orders doubles as Double.compare does: -0.0 < 0.0,
    NaN (any) above +Infinity."""
    b = canon_bits(d) & 0xFFFFFFFFFFFFFFFF
    return (b ^ 0xFFFFFFFFFFFFFFFF) if b >> 63 else (b | (1 << 63))


# ------------------------------------------------------------ the iterator
class X1MaskError(Exception):
    """AggregationIterator.java:706-708 / :776-778 (an AssertionError)."""


def _lerp_long(x, x0, y0, x1, y1):
    if x1 & MS_MASK:
        raise X1MaskError()
    return jlong(y0 + jdiv(jlong(jlong(x - x0) * jlong(y1 - y0)),
                           jlong(x1 - x0)))


def _lerp_double(x, x0, y0, x1, y1):
    if x1 & MS_MASK:
        raise X1MaskError()
    return y0 + float(x - x0) * (y1 - y0) / float(x1 - x0)


def iterate(series, start, end, mut=None):
    """The emissions of the iterator over `series`: a list of (x, is_int,
    values) with `values` the list of (series index, value) of the series
    that contribute at x, in series order — what nextLongValue /
    nextDoubleValue hand out one after another."""
    views = []
    for pts in series:
        a = 0
        while a < len(pts) and pts[a][0] < start:   # seek(start)
            a += 1
        pts = pts[a:]
        if mut == "no_lerp_past_end":
            pts = [p for p in pts if p[0] <= end]
        views.append(pts)
    xs = sorted({p[0] for pts in views for p in pts if p[0] <= end})
    out = []
    for x in xs:
        is_int = True
        slots = []
        for pts in views:
            if not pts or x > pts[-1][0]:
                slots.append(None)                  # ended / empty
                continue
            if pts[0][0] > x:                       # not started: next slot
                is_int = is_int and pts[0][2]
                slots.append(None)
                continue
            c = 0
            while c + 1 < len(pts) and pts[c + 1][0] <= x:
                c += 1
            cur = pts[c]
            nxt = pts[c + 1] if c + 1 < len(pts) else None
            is_int = is_int and cur[2] and (nxt is None or nxt[2])
            slots.append((cur, nxt))
        values = []
        for i, sl in enumerate(slots):
            if sl is None:
                continue
            cur, nxt = sl
            if mut == "no_interp" and cur[0] != x:
                continue
            if is_int:
                v = cur[1] if cur[0] == x else _lerp_long(
                    x, cur[0], cur[1], nxt[0], nxt[1])
            else:
                y0 = cur[1] if not cur[2] else float(cur[1])
                if cur[0] == x:
                    v = y0
                else:
                    y1 = nxt[1] if not nxt[2] else float(nxt[1])
                    v = _lerp_double(x, cur[0], y0, nxt[0], y1)
            values.append((i, v))
        out.append((x, is_int, values))
    return out


# ------------------------------------------------------------ the functions
def _vector(n, values, zero, mut):
    """The aggregator's n-vector of one emission: the k-th contributing
    series' value in slot k, the rest `zero`."""
    vec = [zero] * n
    if mut == "own_slot":
        for i, v in values:
            vec[i] = v
    else:
        for k, (_, v) in enumerate(values):
            vec[k] = v
    return vec


def evaluate(function, topn, start, end, results, mut=None):
    """highestMax / highestCurrent over `results`, a list of sub-query
    results, each a list of series.  Returns (status, picked, keys, series):
    picked = the picked series' numbers in the flat numbering of the inputs
    (empty series counted), keys = their keys as canonical double bits,
    series = their whole point lists, in rank order."""
    if function not in (HIGHEST_MAX, HIGHEST_CURRENT) or topn < 1:
        return ILLEGAL_ARGUMENT, [], [], []
    flat = [pts for res in results for pts in res]
    numbering = [i for i, pts in enumerate(flat)
                 if function == HIGHEST_MAX or len(pts) > 0]
    series = [flat[i] for i in numbering]
    n = len(series)
    if n == 0:
        return OK, [], [], []
    for pts in series:
        if any(b[0] <= a[0] for a, b in zip(pts, pts[1:])):
            return UNSUPPORTED, [], [], []
    try:
        emissions = iterate(series, start, end, mut)
    except X1MaskError:
        return ILLEGAL_STATE, [], [], []
    if not emissions:
        return ILLEGAL_STATE, [], [], []   # the reference: NullPointerException
    d0 = -math.inf if mut == "neg_inf_start" else DOUBLE_MIN_VALUE
    max_longs, max_doubles = [LONG_MIN] * n, [d0] * n
    has_longs = has_doubles = False
    for x, is_int, values in emissions:
        if is_int:
            vec = _vector(n, values, 0, mut)
            if function == HIGHEST_MAX:
                m = len(values) if mut == "no_long_pad" else n
                for k in range(m):
                    max_longs[k] = max(max_longs[k], vec[k])
            else:
                max_longs = vec
            has_longs = True
        else:
            vec = _vector(n, values, 0.0, mut)
            if function == HIGHEST_MAX:
                for k in range(n):
                    max_doubles[k] = jmax(max_doubles[k], vec[k])
            else:
                max_doubles = vec
            has_doubles = True
    if has_longs and has_doubles:
        keys = [jmax(float(max_longs[k]), max_doubles[k]) for k in range(n)]
    elif has_longs:
        keys = [float(max_longs[k]) for k in range(n)]
    else:
        keys = list(max_doubles)
    if mut == "current_own_last" and function == HIGHEST_CURRENT:
        keys = []
        for pts in series:
            own = [p for p in pts if start <= p[0] <= end]
            keys.append(float(own[-1][1]) if own else 0.0)
    if mut == "tie_high":
        order = sorted(range(n), key=lambda k: (-compare_key(keys[k]), -k))
    else:   # Arrays.sort: stable, descending by Double.compare
        order = sorted(range(n), key=lambda k: -compare_key(keys[k]))
    order = order[:min(topn, n)]
    return (OK, [numbering[k] for k in order],
            [canon_bits(keys[k]) for k in order],
            [series[k] for k in order])
