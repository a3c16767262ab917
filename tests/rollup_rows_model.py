"""Iterator-faithful Python restatement of the reference's rollup row path:
RollupSpan.addRow (RollupSpan.java:55-72), RollupSeq.setRow / addRow / append
(RollupSeq.java:126-322), RollupSeq.size / timestamp (:417-462),
RollupIterator's sync / hasNext / next / seek / valueCount (:515-745) and
Span.seekRow / Span.Iterator over them (Span.java:360-471).  It follows the
source line by line — cursors into byte arrays, not sets of offsets — so the
set-level rules the kernels use (rollup_rows.hip) are checked against it.

Where this model leaves the source (the engine's documented deviations):
  * a first qualifier byte 0xF0..0xFF (the millisecond form, which
    RollupUtils.getOffsetFromRollupQualifier reads past the 2 bytes) raises
    UnsupportedOperationException;
  * value bytes whose length is not the qualifier's, or not one of 1/2/4/8
    (4/8 for a float), raise IllegalDataException at append — for every cell
    that passes the order check, a skipped older duplicate included (the
    reference appends them unchecked and reads misaligned);
  * a row's base time below the series' last raises
    UnsupportedOperationException (the reference sorts the rows later);
  * seek timestamps are always milliseconds (RollupIterator.seek multiplies
    a timestamp below 2^32 by 1000).

Also here: a builder of otsdb_raw_rows arrays from per-series (offset, value,
count) lists, the KAT loader, and the decode / whole-query expectations.
"""
import json
import os
import struct

import numpy as np

from opentsdb_amd import core
from opentsdb_amd.batch import HostBatch
from opentsdb_amd.core import (IllegalArgumentException, IllegalDataException,
                               UnsupportedOperationException)

FLAG_FLOAT, LENGTH_MASK, FLAG_BITS = 0x8, 0x7, 4
AGGREGATOR_MASK = 0x7F
SUM, COUNT = b"sum", b"count"
NO_SEEK = -2 ** 63


class Table:
    """The rollup table as a query sees it (otsdb_rollup_table + R)."""

    def __init__(self, rollup_agg, interval_s, value_id, count_id=1,
                 fix_duplicates=False):
        self.rollup_agg = rollup_agg
        self.interval_s = int(interval_s)
        self.value_id, self.count_id = int(value_id), int(count_id)
        self.fix_duplicates = bool(fix_duplicates)
        # RollupQuery: the prefix of the old string qualifiers
        name = "sum" if rollup_agg == "avg" else rollup_agg
        self.agg_prefix = name.lower().encode() + b":"

    @property
    def need_count(self):
        return self.rollup_agg in ("avg", "dev")

    def as_abi(self):
        from opentsdb_amd import abi
        return abi.RollupTable(self.interval_s, self.value_id, self.count_id,
                               1 if self.fix_duplicates else 0)


def java_long(d):
    """(long) d."""
    if d != d:
        return 0
    if d >= 9223372036854775808.0:
        return 2 ** 63 - 1
    if d <= -9223372036854775808.0:
        return -2 ** 63
    return int(d)


def offset_from_qualifier(q, i):
    """Internal.getOffsetFromQualifier (second qualifiers): ms."""
    return ((q[i] << 8 | q[i + 1]) >> FLAG_BITS) * 1000


def value_length(q, i):
    return (q[i + 1] & LENGTH_MASK) + 1


def extract_integer(values, idx, flags):
    n = (flags & LENGTH_MASK) + 1
    if n not in (1, 2, 4, 8):
        raise IllegalDataException("Integer value not on 8/4/2/1 bytes")
    return int.from_bytes(values[idx:idx + n], "big", signed=True)


def extract_float(values, idx, flags):
    n = (flags & LENGTH_MASK) + 1
    if n == 8:
        return struct.unpack(">d", bytes(values[idx:idx + 8]))[0]
    if n == 4:
        return float(np.frombuffer(bytes(values[idx:idx + 4]), ">f4")[0])
    raise IllegalDataException("Floating point value not on 8 or 4 bytes")


class RollupSeq:
    def __init__(self, table, base_s):
        self.t = table
        self.base_s = int(base_s)
        self.qualifiers, self.values = bytearray(), bytearray()
        self.count_qualifiers, self.count_values = bytearray(), bytearray()
        self.indices = [0, 0, 0, 0]  # q, v, cq, cv
        self.last_offset = self.last_count_offset = -1
        self.last_value_ts = self.last_count_ts = 0
        self.n_arrived = 0  # cells handed to add_cell without a timestamp

    # -- setRow / addRow: the same tests (RollupSeq.java:136-161, :182-207)
    def add_cell(self, qual, value, ts):
        t = self.t
        if len(qual) < 1:
            raise IllegalDataException("empty qualifier")
        if t.need_count:
            if qual[0] & AGGREGATOR_MASK == t.value_id:
                self.append(qual, value, ts, False, False)
            elif qual[0] & AGGREGATOR_MASK == t.count_id:
                self.append(qual, value, ts, True, False)
            elif qual[:len(SUM)] == SUM:
                self.append(qual, value, ts, False, True)
            elif qual[:len(COUNT)] == COUNT:
                self.append(qual, value, ts, True, True)
            else:
                raise IllegalDataException(
                    "Attempt to add a different aggrregate cell")
        else:
            if qual[0] & AGGREGATOR_MASK == t.value_id:
                self.append(qual, value, ts, False, False)
            elif qual[:len(t.agg_prefix)] == t.agg_prefix:
                self.append(qual, value, ts, False, True)
            else:
                raise IllegalDataException(
                    "Attempt to add a different aggrregate cell")

    def _checked(self, qual, strip, value):
        if len(qual) < strip + 2:
            raise IllegalDataException("qualifier too short")
        if qual[strip] & 0xF0 == 0xF0:
            raise UnsupportedOperationException("millisecond rollup qualifier")
        return offset_from_qualifier(qual, strip)

    def _check_value(self, qual, strip, value):
        fl, n = qual[strip + 1] & FLAG_FLOAT, value_length(qual, strip)
        if len(value) != n or n not in ((4, 8) if fl else (1, 2, 4, 8)):
            raise IllegalDataException("value bytes do not match the qualifier")

    def append(self, qual, value, ts, is_count, strip_string):
        t, ix = self.t, self.indices
        if is_count:
            strip = len(COUNT) + 1 if strip_string else 1
            offset = self._checked(qual, strip, value)
            if self.last_count_offset > -1 and \
                    offset <= self.last_count_offset:
                if offset == self.last_count_offset and t.fix_duplicates:
                    if ts < self.last_count_ts:
                        self._check_value(qual, strip, value)
                        return
                    ix[2] -= 2
                    ix[3] -= value_length(self.count_qualifiers, ix[2])
                else:
                    raise IllegalArgumentException(
                        "The count offset is <= the last offset")
            self._check_value(qual, strip, value)
            self.last_count_offset = offset
            self.last_count_ts = ts
            self.count_qualifiers[ix[2]:] = qual[strip:strip + 2]
            ix[2] += 2
            self.count_values[ix[3]:] = value
            ix[3] += len(value)
        else:
            strip = len(t.agg_prefix) if strip_string else 1
            offset = self._checked(qual, strip, value)
            if self.last_offset > -1 and offset <= self.last_offset:
                if offset == self.last_offset and t.fix_duplicates:
                    if ts < self.last_value_ts:
                        self._check_value(qual, strip, value)
                        return
                    ix[0] -= 2
                    ix[1] -= value_length(self.qualifiers, ix[0])
                else:
                    raise IllegalDataException(
                        "The offset is <= the last offset")
            self._check_value(qual, strip, value)
            self.last_offset = offset
            self.last_value_ts = ts
            self.qualifiers[ix[0]:] = qual[strip:strip + 2]
            ix[0] += 2
            self.values[ix[1]:] = value
            ix[1] += len(value)

    def next_arrival(self):
        """The HBase timestamp of a cell given without one: its arrival rank
        (col_ts == NULL: ascending column order)."""
        self.n_arrived += 1
        return self.n_arrived - 1

    def ts_at(self, quals, i):
        """RollupUtils.getTimestampFromRollupQualifier."""
        off = (quals[i] << 8 | quals[i + 1]) >> FLAG_BITS
        return self.base_s * 1000 + off * self.t.interval_s * 1000

    def iterator(self):
        return RollupIterator(self)

    def size(self):
        if self.t.need_count:
            n, it = 0, self.iterator()
            while it.hasNext():
                it.next()
                n += 1
            return n
        return self.indices[0] // 2

    def timestamp(self, i):
        if i < 0:
            raise IndexError(i)
        if self.t.need_count:
            it, n = self.iterator(), 0
            while it.hasNext():
                it.next()
                if n == i:
                    return it.timestamp()
                n += 1
            raise IndexError(i)
        if i * 2 >= self.indices[0]:
            raise IndexError(i)
        return self.ts_at(self.qualifiers, i * 2)


class RollupIterator:
    def __init__(self, seq):
        self.s = seq
        self.qualifier = self.count_qualifier = 0
        self.qual_index = self.value_index = 0
        self.count_qual_index = self.count_value_index = 0
        if seq.t.need_count:
            self.sync()

    def hasNext(self):
        s = self.s
        if s.t.need_count:
            self.sync()
            return self.qual_index < s.indices[0] and \
                self.count_qual_index < s.indices[2]
        return self.qual_index < s.indices[0]

    def sync(self):
        s = self.s
        while True:  # (the source recurses)
            if self.qual_index >= s.indices[0] or \
                    self.count_qual_index >= s.indices[2]:
                return
            q_ts = offset_from_qualifier(s.qualifiers, self.qual_index)
            c_ts = offset_from_qualifier(s.count_qualifiers,
                                         self.count_qual_index)
            if q_ts == c_ts:
                return
            if q_ts > c_ts:
                self.count_value_index += value_length(
                    s.count_qualifiers, self.count_qual_index)
                self.count_qual_index += 2
            else:
                self.value_index += value_length(s.qualifiers, self.qual_index)
                self.qual_index += 2

    def next(self):
        s = self.s
        if not self.hasNext():
            raise core.NoSuchElementException("no more elements")
        self.value_index += value_length(s.qualifiers, self.qual_index)
        self.qualifier = s.qualifiers[self.qual_index] << 8 | \
            s.qualifiers[self.qual_index + 1]
        self.qual_index += 2
        if s.t.need_count:
            self.count_value_index += value_length(s.count_qualifiers,
                                                   self.count_qual_index)
            self.count_qualifier = \
                s.count_qualifiers[self.count_qual_index] << 8 | \
                s.count_qualifiers[self.count_qual_index + 1]
            self.count_qual_index += 2
        return self

    def seek(self, ts):
        s = self.s
        self.qual_index = self.value_index = 0
        self.count_qual_index = self.count_value_index = 0
        if not self.hasNext():
            return
        while self.qual_index < s.indices[0] and \
                s.ts_at(s.qualifiers, self.qual_index) < ts:
            self.value_index += value_length(s.qualifiers, self.qual_index)
            self.qual_index += 2
            if s.t.need_count:
                # (the source reads the qualifier array's spare capacity past
                # indices[2]; the cursor only has to end up past the end)
                if self.count_qual_index < s.indices[2]:
                    self.count_value_index += value_length(
                        s.count_qualifiers, self.count_qual_index)
                self.count_qual_index += 2

    def timestamp(self):
        off = self.qualifier >> FLAG_BITS
        return self.s.base_s * 1000 + off * self.s.t.interval_s * 1000

    def isInteger(self):
        return self.qualifier & FLAG_FLOAT == 0

    def longValue(self):
        flags = self.qualifier & 0xFF
        n = (flags & LENGTH_MASK) + 1
        return extract_integer(self.s.values, self.value_index - n, flags)

    def doubleValue(self):
        flags = self.qualifier & 0xFF
        n = (flags & LENGTH_MASK) + 1
        return extract_float(self.s.values, self.value_index - n, flags)

    def bits(self):
        """The point's value as the engine's int64 column holds it."""
        if self.isInteger():
            return self.longValue()
        return int(np.float64(self.doubleValue()).view(np.int64))

    def valueCount(self):
        s = self.s
        if not s.t.need_count and s.t.rollup_agg != "count":
            return 1
        if s.t.rollup_agg == "count":
            return self.longValue() if self.isInteger() \
                else java_long(self.doubleValue())
        flags = self.count_qualifier & 0xFF
        n = (flags & LENGTH_MASK) + 1
        if self.count_qualifier & FLAG_FLOAT == 0:
            return extract_integer(s.count_values, self.count_value_index - n,
                                   flags)
        return java_long(extract_float(s.count_values,
                                       self.count_value_index - n, flags))


class RollupSpan:
    """One series' rows (RollupSpan.addRow) and Span's seekRow / Iterator."""

    def __init__(self, table):
        self.t = table
        self.rows = []

    def add_row(self, base_s, cells):
        """cells: [(qualifier, value[, hbase_ts])] in arrival order; without
        timestamps a cell's is its arrival index in the row."""
        if not cells:
            return
        if self.rows and self.rows[-1].base_s == base_s:
            seq = self.rows[-1]
        else:
            if self.rows and base_s < self.rows[-1].base_s:
                raise UnsupportedOperationException("rows out of order")
            seq = RollupSeq(self.t, base_s)
            self.rows.append(seq)
        for c in cells:
            seq.add_cell(bytes(c[0]), bytes(c[1]),
                         c[2] if len(c) > 2 else seq.next_arrival())

    def seek_row(self, timestamp):
        row_index = 0
        for row in self.rows:
            sz = row.size()
            if sz < 1:
                row_index += 1
            elif row.timestamp(sz - 1) < timestamp:
                row_index += 1
            else:
                break
        if row_index == len(self.rows):
            row_index -= 1
        return row_index

    def iterate(self, seek=None):
        """Span.Iterator: every point [(ts, bits, is_float, value_count)],
        after seek(seek) when given."""
        out = []
        if not self.rows:
            return out
        row_index, cur = 0, self.rows[0].iterator()
        if seek is not None:
            r = self.seek_row(seek)
            if r != row_index:
                row_index, cur = r, self.rows[r].iterator()
            cur.seek(seek)
        while True:
            if not cur.hasNext():
                found = False
                while row_index < len(self.rows) - 1:
                    row_index += 1
                    cur = self.rows[row_index].iterator()
                    if cur.hasNext():
                        found = True
                        break
                if not found:
                    return out
            dp = cur.next()
            out.append((dp.timestamp(), dp.bits(), 0 if dp.isInteger() else 1,
                        dp.valueCount()))


def decode_series(table, rows, seek_ms=NO_SEEK):
    """What otsdb_rollup_decode_rows_device emits for one series' rows
    [(base_s, cells)]: the plain iteration's points before seek_ms, then what
    Span.Iterator yields after seek(seek_ms).  Only a rollup avg table's
    iterator depends on the seek."""
    span = RollupSpan(table)
    for base_s, cells in rows:
        span.add_row(base_s, cells)
    plain = span.iterate()
    if seek_ms == NO_SEEK or not table.need_count:
        return plain
    return [p for p in plain if p[0] < seek_ms] + span.iterate(seek_ms)


def decode_rows(table, rows, n_series, seek_ms=NO_SEEK):
    """rows: [(series, base_s, cells)] with nondecreasing series.  Returns
    (offsets, ts, bits, is_float, value_count) numpy arrays; the first failing
    row raises."""
    per = [[] for _ in range(n_series)]
    for s, base_s, cells in rows:
        per[s].append((base_s, cells))
    pts, offs = [], [0]
    # (rows are processed in row order so the first failing row decides)
    for s in range(n_series):
        pts += decode_series(table, per[s], seek_ms)
        offs.append(len(pts))
    col = lambda k, dt: np.array([p[k] for p in pts], dt)  # noqa: E731
    return (np.array(offs, np.int64), col(0, np.int64), col(1, np.int64),
            col(2, np.uint8), col(3, np.int64))


# ------------------------------------------------------------------ builder
def qualifier(offset, flags, agg_id=None, prefix=None):
    """A rollup cell's qualifier: the numeric id byte, or the old string
    prefix, then offset << 4 | flags."""
    head = bytes([agg_id]) if prefix is None else prefix
    return head + struct.pack(">H", (offset << FLAG_BITS | flags) & 0xFFFF)


def encode_value(v, width=None):
    """(value bytes, flags): a Python int in the smallest of 1/2/4/8 bytes
    (or `width`), a float in 8 bytes (a np.float32 in 4)."""
    if isinstance(v, np.float32):
        return struct.pack(">f", float(v)), FLAG_FLOAT | 3
    if isinstance(v, float):
        return struct.pack(">d", v), FLAG_FLOAT | 7
    v = int(v)
    if width is None:
        width = next(w for w in (1, 2, 4, 8)
                     if -(1 << (8 * w - 1)) <= v < (1 << (8 * w - 1)))
    return v.to_bytes(width, "big", signed=True), width - 1


def build_rows(table, series, cells_per_row=None, old_style=lambda s, o: False,
               width=None, split=1, dup=None, with_ts=False):
    """series: per series a list of (abs_offset, value, count) — value / count
    None drops that cell; abs_offset counts intervals from base 0, rows hold
    `cells_per_row` offsets each (default: one row).  old_style(series,
    offset): write the string-prefixed qualifiers.  split: the cells of every
    row dealt over this many consecutive input rows of the same base time.
    dup: {(series, abs_offset): [(value, count, hbase_ts), ...]} extra cells
    after the first of that offset.  Returns [(series, base_s, cells)]."""
    span = cells_per_row or 3840
    out = []
    for s, pts in enumerate(series):
        by_row = {}
        for (o, v, c) in pts:
            by_row.setdefault(o // span, []).append((o, v, c))
        for r in sorted(by_row):
            cells, n = [], 0

            def emit(o, v, c, ts):
                old = old_style(s, o)
                for kind, x in ((0, v), (1, c)):
                    if x is None or (kind and not table.need_count):
                        continue
                    vb, fl = encode_value(x, None if kind else width)
                    aid = table.count_id if kind else table.value_id
                    pre = ((COUNT + b":") if kind else table.agg_prefix) \
                        if old else None
                    q = qualifier(o % span, fl, aid, pre)
                    cells.append((q, vb, ts) if with_ts else (q, vb))
            for (o, v, c) in by_row[r]:
                emit(o, v, c, n)
                n += 1
                for (dv, dc, dts) in (dup or {}).get((s, o), []):
                    emit(o, dv, dc, dts)
            base_s = r * span * table.interval_s
            k = max(1, (len(cells) + split - 1) // split)
            for i in range(0, len(cells), k):
                out.append((s, base_s, cells[i:i + k]))
    return out


def host_rows(rows, with_ts=None):
    from opentsdb_amd.storage import HostRawRows
    return HostRawRows([(s, b, [tuple(c) for c in cells])
                        for s, b, cells in rows], with_ts)


# ------------------------------------------------------- whole-query expectation
def points_batch(offsets, ts, bits, isf, group_offsets=None,
                 group_members=None):
    return HostBatch(offsets, ts, bits, isf, None, group_offsets,
                     group_members)


def query_seek_ms(spec):
    """Downsampler.seekInterval (Downsampler.java:412-434)."""
    if spec.run_all:
        return int(spec.start_ms)
    if spec.use_calendar:
        from tests import rollup_model as RM
        e = RM._spec_edges(spec)
        k = int(np.searchsorted(e, spec.start_ms, side="left"))
        return int(e[k]) if k < len(e) else int(spec.start_ms)
    iv = int(spec.ds_interval_ms)
    return (int(spec.start_ms) + iv - 1) // iv * iv


# --------------------------------------------------------------------- KATs
def load_kats():
    """tests/golden/kat_rollup_rows.json (make_rollup_rows_kats.py)."""
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, "golden", "kat_rollup_rows.json")) as f:
        return json.load(f)


def kat_table(c):
    t = c["table"]
    return Table(t["rollup_agg"], t["interval_s"], t["value_id"],
                 t.get("count_id", 1), t.get("fix_duplicates", False))


def kat_rows(c):
    """[(series, base_s, cells)] of a case: every stored cell is its own
    scanner row of one column unless the case groups them."""
    return [(r[0], r[1], [(bytes.fromhex(x[0]), bytes.fromhex(x[1])) +
                          tuple(x[2:]) for x in r[2]]) for r in c["rows"]]


ERRORS = {"IllegalDataException": IllegalDataException,
          "IllegalArgumentException": IllegalArgumentException,
          "UnsupportedOperationException": UnsupportedOperationException}
