"""Plain-Python model of the reference's path from the scanner's rows to a
histogram span's points, restated at the iterator level (not a twin of the
kernels), and of the engine's refusal rules over the same rows:

  Output / Input        Kryo 3.0.0's writeShort / writeFloat /
                        writeLong(v, true) and their reads, with the buffer
                        underflow exception (KryoException)
  from_histogram        SimpleHistogram.fromHistogram (SimpleHistogram.java:
                        97-122)
  timestamp_from_non_dp Internal.getTimeStampFromNonDP (Internal.java:
                        1059-1074)
  decode_point          Internal.decodeHistogramDataPoint (:1095-1104) behind
                        the codec lookup of HistogramCodecManager.getCodec
  row_points            the scanner's loop over a row's histogram cells with
                        its catch (Throwable): a cell that throws is skipped
                        (SaltScanner.java:788-795)
  RowSeq / Span         HistogramRowSeq.setRow / addRow (:56-105) and
                        HistogramSpan.addRow (:280-328) with checkRowOrder,
                        including the out-of-order replay the engine refuses
  decode_rows           rows -> (offsets, ts, counts) over a schema
  union_keys            the schema of the rows
  refusal               the engine's refusal rules (include/otsdb_agg.h),
                        separate from what the reference does

The Kryo jar is not available: the byte format is restated from Kryo 3.0.0's
documented variable-length encoding and pinned by the hand-derived vectors of
tests/golden/kat_hist_rows.json, not by a run of the reference.
"""
import json
import os
import struct

import numpy as np

from tests import hist_model as HM

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "kat_hist_rows.json")
PREFIX = 0x06
MAX_KEYS = 254       # OTSDB_HIST_MAX_ROW - 2
MAX_RUN_ROWS = 64


class KryoException(Exception):
    """Buffer underflow."""


class Output:
    def __init__(self):
        self.buf = bytearray()

    def writeByte(self, v):
        self.buf.append(v & 0xFF)

    def writeShort(self, v):
        self.buf += struct.pack(">H", v & 0xFFFF)

    def writeInt(self, v):
        self.buf += struct.pack(">I", v & 0xFFFFFFFF)

    def writeFloat(self, f):
        self.buf += struct.pack(">f", f)

    def writeFloatBits(self, bits):
        self.buf += struct.pack(">I", bits & 0xFFFFFFFF)

    def writeLong(self, v, optimize_positive=True):
        assert optimize_positive
        v &= (1 << 64) - 1
        for _ in range(8):
            if v >> 7 == 0:
                self.buf.append(v)
                return
            self.buf.append((v & 0x7F) | 0x80)
            v >>= 7
        self.buf.append(v)

    def toBytes(self):
        return bytes(self.buf)


class Input:
    def __init__(self, raw):
        self.raw, self.pos = bytes(raw), 0

    def _require(self, n):
        if self.pos + n > len(self.raw):
            raise KryoException("Buffer underflow.")

    def readByte(self):
        self._require(1)
        b = self.raw[self.pos]
        self.pos += 1
        return b

    def readShort(self):
        self._require(2)
        v = struct.unpack_from(">h", self.raw, self.pos)[0]
        self.pos += 2
        return v

    def readFloatBits(self):
        """readFloat as Float.floatToRawIntBits of what it returns."""
        self._require(4)
        v = struct.unpack_from(">i", self.raw, self.pos)[0]
        self.pos += 4
        return v

    def readLong(self, optimize_positive=True):
        assert optimize_positive
        v = 0
        for i in range(8):
            b = self.readByte()
            v |= (b & 0x7F) << (7 * i)
            if not b & 0x80:
                return HM.wrap_long(v)
        return HM.wrap_long(v | (self.readByte() << 56))


def canon(bits):
    """floatToIntBits of raw bits: every NaN the canonical one."""
    bits &= 0xFFFFFFFF
    if (bits & 0x7FFFFFFF) > 0x7F800000:
        bits = 0x7FC00000
    return bits - (1 << 32) if bits >> 31 else bits


def from_histogram(raw, include_id=True):
    """-> HM.Hist.  A repeated key keeps the later count (TreeMap.put)."""
    if len(raw) < 6:
        raise ValueError("Byte array shorter than 6 bytes detected")
    inp = Input(raw)
    if include_id:
        inp.readByte()
    n = inp.readShort()
    buckets = {}
    for _ in range(max(n, 0)):
        lo = canon(inp.readFloatBits())
        up = canon(inp.readFloatBits())
        buckets[(lo, up)] = inp.readLong(True)
    under = inp.readLong(True)
    over = inp.readLong(True)
    return HM.Hist(buckets, under, over)


def _sbyte(b):
    return b - 256 if b >= 128 else b


def _int32(v):
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v >> 31 else v


def timestamp_from_non_dp(base_s, q):
    if len(q) == 3:
        return (base_s + _int32((_sbyte(q[1]) << 8) | q[2])) * 1000
    if len(q) == 5:
        return base_s * 1000 + _int32(q[1] << 24 | q[2] << 16 | q[3] << 8 | q[4])
    raise ValueError("Quantifier is not valid")


def is_hist_cell(q):
    return len(q) % 2 == 1 and q[0] == PREFIX


def decode_point(base_s, q, v, codec_id):
    """(ts, Hist), or raises what the scanner catches.  Only the simple
    codec is configured: any other id has no codec (IllegalArgument)."""
    cid = v[0]  # IndexError on an empty value
    if cid != codec_id:
        raise LookupError("No codec found mapped to ID %d" % cid)
    ts = timestamp_from_non_dp(base_s, q)
    return ts, from_histogram(v, True)


def row_points(base_s, cols, codec_id):
    """The row's histogram points in column order and the cells skipped."""
    pts, skipped = [], 0
    for c in cols:
        q, v = bytes(c[0]), bytes(c[1])
        if not q or not is_hist_cell(q):
            continue
        try:
            pts.append(decode_point(base_s, q, v, codec_id))
        except Exception:
            skipped += 1
    return pts, skipped


class RowSeq:
    def __init__(self):
        self.key, self.seq = None, None

    def setRow(self, key, row):
        if self.key is not None:
            raise RuntimeError("setRow was already called")
        self.key, self.seq = key, list(row)

    def addRow(self, row):
        if self.key is None:
            raise RuntimeError("setRow was never called")
        il = ir = 0
        out = []
        while il < len(self.seq) and ir < len(row):
            sort = row[ir][0] - self.seq[il][0]
            if sort == 0:
                out.append(self.seq[il])
                il += 1
                ir += 1
            elif sort > 0:
                out.append(self.seq[il])
                il += 1
            else:
                out.append(row[ir])
                ir += 1
        if il < len(self.seq):
            out += self.seq[il:]
        elif ir < len(row):
            out += row[ir:]
        self.seq = out


class Span:
    """HistogramSpan over keys (series, base_s)."""

    def __init__(self):
        self.rows, self.sorted = [], False

    def addRow(self, key, points):
        last_ts = 0
        if self.rows:
            last = self.rows[-1]
            if last.key[0] != key[0]:
                raise ValueError("tags mismatch")
            last_ts = last.seq[-1][0]
        rs = RowSeq()
        rs.setRow(key, points)
        self.sorted = False
        if last_ts >= rs.seq[0][0]:
            for r in self.rows:
                if r.key == key:
                    r.addRow(points)
                    return
        self.rows.append(rs)

    def points(self):
        if not self.sorted:
            self.rows.sort(key=lambda r: r.key[1])  # (a stable sort, as Java's)
            self.sorted = True
        return [p for r in self.rows for p in r.seq]


def unpack_rows(rows):
    """storage.HostRawRows -> [(series, base_s, [(qualifier, value)])]."""
    out = []
    for r in range(rows.n_rows):
        cols = []
        for c in range(int(rows.row_col_off[r]), int(rows.row_col_off[r + 1])):
            q = bytes(rows.qual[rows.col_qual_off[c]:rows.col_qual_off[c + 1]])
            v = bytes(rows.val[rows.col_val_off[c]:rows.col_val_off[c + 1]])
            cols.append((q, v))
        out.append((int(rows.row_series[r]), int(rows.row_base_s[r]), cols))
    return out


def series_points(rows, n_series, codec_id):
    """Per series the span's points [(ts, Hist)], and the counters (cells
    decoded, cells skipped, points dropped by a merge)."""
    spans = [Span() for _ in range(n_series)]
    decoded = skipped = 0
    for s, base, cols in unpack_rows(rows):
        pts, sk = row_points(base, cols, codec_id)
        skipped += sk
        decoded += len(pts)
        if pts:  # hists.size() > 0
            spans[s].addRow((s, base), pts)
    out = [sp.points() for sp in spans]
    kept = sum(len(p) for p in out)
    return out, dict(decoded=decoded, skipped=skipped,
                     merged_away=decoded - kept)


def union_keys(series):
    """The sorted union of the keys of the series' points."""
    keys = set()
    for pts in series:
        for _, h in pts:
            keys.update(h.buckets)
    return sorted(keys, key=lambda k: HM.key_order(HM.key_bounds(k)))


def schema_of(keys):
    lo = np.array([k[0] for k in keys], np.int32).view(np.float32)
    up = np.array([k[1] for k in keys], np.int32).view(np.float32)
    return lo, up


def keys_of(schema):
    return [HM.make_key(a, b) for a, b in zip(*schema)]


def decode_rows(rows, n_series, codec_id, schema):
    """-> (offsets [S + 1], ts [N], counts [N][K + 2]) over `schema` =
    (lower, upper); a key outside the schema is a KeyError."""
    series, _ = series_points(rows, n_series, codec_id)
    col = {k: i for i, k in enumerate(keys_of(schema))}
    K = len(col)
    offs, ts, cnt = [0], [], []
    for pts in series:
        for t, h in pts:
            row = [0] * (K + 2)
            for k, v in h.buckets.items():
                row[col[k]] = v
            row[K], row[K + 1] = h.underflow, h.overflow
            ts.append(t)
            cnt.append(row)
        offs.append(len(ts))
    return (np.array(offs, np.int64), np.array(ts, np.int64),
            np.array(cnt, np.int64).reshape(len(ts), K + 2))


# ------------------------------------------------------------ the engine's rules
OK, E_ILLEGAL_ARGUMENT, E_UNSUPPORTED = 0, 3, 5


def refusal(rows, n_series, codec_id, schema=None):
    """The status the engine returns for the rows (OK, E_ILLEGAL_ARGUMENT,
    E_UNSUPPORTED) and where: (status, position).  The first failing row in
    row order, then the first failing column in it; a failure of the row as a
    whole (a base time going back, the 65th row of a key) counts before its
    columns.  Cell c sits at 2 c + 1, row r at twice its first column.  The
    cross-row timestamp check is made when nothing else failed."""
    cols_in = set(keys_of(schema)) if schema is not None else None
    fails = []
    c = 0
    prev = None   # (series, base) of the row before
    run = 0
    seqs = {}     # (series, base, run start row) -> list of row point lists
    order = []
    for r, (s, base, cols) in enumerate(unpack_rows(rows)):
        row_pos = 2 * c
        if s < 0 or s >= n_series or (prev is not None and prev[0] > s):
            fails.append((row_pos, E_ILLEGAL_ARGUMENT))
        if prev is not None and prev[0] == s and base < prev[1]:
            fails.append((row_pos, E_UNSUPPORTED))
        run = run + 1 if prev == (s, base) else 1
        if run > MAX_RUN_ROWS:
            fails.append((row_pos, E_UNSUPPORTED))
        if run == 1:
            order.append([])
        prev = (s, base)
        last = None
        pts = []
        for q, v in cols:
            pos = 2 * c + 1
            c += 1
            if not q or not is_hist_cell(q):
                continue
            if len(v) < 1 or len(q) not in (3, 5):
                continue  # skipped
            if v[0] != codec_id:
                fails.append((pos, E_UNSUPPORTED))
                continue
            if len(v) < 6:
                continue
            if struct.unpack_from(">h", v, 1)[0] > MAX_KEYS:
                fails.append((pos, E_UNSUPPORTED))
                continue
            try:
                ts, h = decode_point(base, q, v, codec_id)
            except Exception:
                continue
            if cols_in is not None and not set(h.buckets) <= cols_in:
                fails.append((pos, E_ILLEGAL_ARGUMENT))
            if last is not None and ts <= last:
                fails.append((pos, E_UNSUPPORTED))
            last = ts
            pts.append(ts)
        order[-1].append((s, row_pos, pts))
    if fails:
        pos, st = min(fails)
        return st, pos
    last_of = {}
    for seq in order:
        s, pos = seq[0][0], seq[0][1]
        ts = sorted(set(t for _, _, p in seq for t in p))
        if not ts:
            continue
        if s in last_of and ts[0] <= last_of[s]:
            return E_UNSUPPORTED, pos
        last_of[s] = ts[-1]
    return OK, -1


def load_kats():
    with open(GOLDEN) as f:
        return json.load(f)
