"""Row-by-row reference for the window functions (gpuq_window_* and
GpuWindowExec), after WindowExec.scala / WindowFunctionFrame.scala.

The rows are already sorted by (partition keys, order keys). `boundaries`
marks where a partition and where a peer group starts; `scan` then walks the
rows of each partition once with one running accumulator, the way
UnboundedPrecedingWindowFunctionFrame does: for output row i it first feeds
the accumulator every input row up to the upper bound of i's frame (the row
itself for ROWS, the last peer for RANGE, the partition's last row for
PARTITION) and then reads it. `shift` is lag / lead
(FrameLessOffsetWindowFunctionFrame, ignoreNulls = false).

Values are Python ints / floats with None for NULL. Semantics restated:
 - key equality is the sort's: NULL == NULL, NULL != value, -0.0 == 0.0 and
   every NaN equals every NaN;
 - SUM / MIN / MAX skip NULLs and are NULL until the frame holds a non-NULL
   value; COUNT counts non-NULL rows (COUNT(*): rows) and is never NULL;
 - int64 SUM wraps modulo 2^64 (non-ANSI); float64 SUM starts from 0.0 and
   adds in row order;
 - MIN / MAX order float64 with NaN greatest and -0.0 == 0.0, return the
   canonical NaN for a NaN and +0.0 for a zero.
tests/test_window_ref.py pins all of this to hand-written tables.

The np_* functions are vectorised numpy forms of the same functions for
inputs too long for one Python call per row. They take the value column as a
numpy array plus a bool `ok` array (None: no NULLs) and return (out, ok);
test_window_ref.py checks them against the row-by-row ones.
"""
import math

import numpy as np

RANK_OPS = ("row_number", "rank", "dense_rank")
FRAMES = ("rows", "range", "partition")
_M64 = (1 << 64) - 1
_SIGN = 1 << 63


# ---------------- row by row ----------------

def key_eq(a, b):
    """the sort's equality on one key value (None is NULL)."""
    if a is None or b is None:
        return a is None and b is None
    if isinstance(a, float) and isinstance(b, float):
        if math.isnan(a) or math.isnan(b):
            return math.isnan(a) and math.isnan(b)
    return a == b          # -0.0 == 0.0 in Python too


def boundaries(keys, npart, n):
    """keys: list of columns (lists with None for NULL), the first npart of
    them partition keys. Returns (part, peer): lists of n bools."""
    part, peer = [], []
    for i in range(n):
        p = i == 0 or any(not key_eq(k[i - 1], k[i]) for k in keys[:npart])
        q = p or any(not key_eq(k[i - 1], k[i]) for k in keys[npart:])
        part.append(p)
        peer.append(q)
    return part, peer


def wrap_i64(v):
    return ((v + _SIGN) & _M64) - _SIGN


def _f64_key(v):
    """total-order key: NaN greatest, -0.0 == 0.0."""
    return (1, 0.0) if math.isnan(v) else (0, v + 0.0)


def _f64_canon(v):
    if math.isnan(v):
        return float("nan")
    return 0.0 if v == 0.0 else v


class _Acc:
    """one running aggregate; value() is None while it has seen no input."""

    def __init__(self, op, dtype):
        self.op, self.dtype = op, dtype
        self.count = 0            # rows fed (COUNT(*)) / non-NULL rows fed
        self.nonnull = 0
        self.v = None

    def feed(self, x):
        self.count += 1
        if x is None:
            return
        self.nonnull += 1
        if self.op == "sum":
            if self.dtype == "i64":
                self.v = wrap_i64((self.v or 0) + x)
            else:
                self.v = (0.0 if self.v is None else self.v) + x
        elif self.op in ("min", "max"):
            if self.v is None:
                self.v = x
                return
            f64 = self.dtype == "f64"
            kx, kv = (_f64_key(x), _f64_key(self.v)) if f64 else (x, self.v)
            if (kx < kv) if self.op == "min" else (kx > kv):
                self.v = x

    def value(self, star):
        if self.op == "count":
            return self.count if star else self.nonnull
        if self.v is None:
            return None
        if self.op in ("min", "max") and self.dtype == "f64":
            return _f64_canon(self.v)
        return self.v


def _partitions(part):
    """[(begin, end)] with end exclusive."""
    starts = [i for i, p in enumerate(part) if p]
    return list(zip(starts, starts[1:] + [len(part)]))


def scan(op, frame, part, peer, vals=None, dtype="i64"):
    """op: row_number / rank / dense_rank / count / sum / min / max. vals:
    list with None for NULL, or None for the rank ops and COUNT(*). Returns
    the list of results (None for NULL)."""
    assert frame in FRAMES
    n = len(part)
    out = [None] * n
    for b, e in _partitions(part):
        if op in RANK_OPS:
            assert frame == "rows"
            rank = dense = 0
            for i in range(b, e):
                if peer[i]:
                    rank = i - b + 1
                    dense += 1
                out[i] = {"row_number": i - b + 1, "rank": rank,
                          "dense_rank": dense}[op]
            continue
        acc = _Acc(op, dtype)
        fed = b                      # next input row to feed
        for i in range(b, e):
            if frame == "rows":
                upper = i
            elif frame == "partition":
                upper = e - 1
            else:
                upper = i
                while upper + 1 < e and not peer[upper + 1]:
                    upper += 1
            while fed <= upper:
                acc.feed(vals[fed] if vals is not None else 0)
                fed += 1
            out[i] = acc.value(star=vals is None)
    return out


def avg(frame, part, peer, vals):
    """windowed SUM / windowed COUNT over a float64 column; NULL where the
    count is 0."""
    s = scan("sum", frame, part, peer, vals, "f64")
    c = scan("count", frame, part, peer, vals, "f64")
    return [None if ci == 0 else si / ci for si, ci in zip(s, c)]


def shift(vals, offset, part, default=None):
    """lag (offset < 0) / lead (offset > 0): the source row's own value (None
    if it is NULL) inside the partition, the default (None: NULL) outside."""
    n = len(part)
    out = [None] * n
    for b, e in _partitions(part):
        for i in range(b, e):
            j = i + offset
            out[i] = vals[j] if b <= j < e else default
    return out


# ---------------- vectorised numpy forms ----------------

def np_enc_f64(v):
    """the sort-key encoding of float64 (monotone u64; -0.0 -> +0.0, one NaN)."""
    v = np.where(v == 0.0, 0.0, v)
    bits = np.where(np.isnan(v), np.uint64(0x7FF8000000000000),
                    v.view(np.uint64))
    neg = (bits >> np.uint64(63)).astype(bool)
    return np.where(neg, ~bits, bits ^ np.uint64(_SIGN))


def np_dec_f64(e):
    pos = (e >> np.uint64(63)).astype(bool)
    return np.where(pos, e ^ np.uint64(_SIGN), ~e).view(np.float64)


def np_boundaries(keys, npart):
    """keys: list of (values ndarray, ok bool ndarray or None). Returns bool
    arrays (part, peer)."""
    def differs(v, ok):
        w = np_enc_f64(v) if v.dtype == np.float64 else v.view(np.uint64)
        d = w[1:] != w[:-1]
        if ok is not None:
            d = np.where(ok[1:] & ok[:-1], d, ok[1:] != ok[:-1])
        return d
    n = len(keys[0][0])
    part = np.zeros(n, dtype=bool)
    peer = np.zeros(n, dtype=bool)
    part[0] = True
    for c, (v, ok) in enumerate(keys):
        d = differs(v, ok)
        if c < npart:
            part[1:] |= d
        else:
            peer[1:] |= d
    return part, peer | part


def np_begin(bits):
    """position of the last set bit at or before each row."""
    idx = np.where(bits, np.arange(len(bits)), 0)
    return np.maximum.accumulate(idx)


def np_end(bits):
    """last row of each row's group: the next set bit after it, minus one."""
    n = len(bits)
    nxt = np.where(bits, np.arange(n), n)
    nxt = np.minimum.accumulate(nxt[::-1])[::-1]      # first set bit at or after
    return np.append(nxt[1:], n) - 1


def _seg_accumulate(ufunc, arr, part):
    """ufunc.accumulate restarted at every partition start (in row order,
    like the running accumulator of the row-by-row form)."""
    out = np.empty_like(arr)
    starts = np.flatnonzero(part)
    for b, e in zip(starts, np.append(starts[1:], len(arr))):
        out[b:e] = ufunc.accumulate(arr[b:e])
    return out


def np_scan(op, frame, part, peer, vals=None, ok=None):
    """Returns (out ndarray, ok bool ndarray or None). NULL rows hold 0."""
    n = len(part)
    i = np.arange(n)
    pbeg = np_begin(part)
    if op in RANK_OPS:
        assert frame == "rows"
        if op == "row_number":
            return (i - pbeg + 1).astype(np.int64), None
        if op == "rank":
            return (np_begin(peer) - pbeg + 1).astype(np.int64), None
        c = np.cumsum(peer)
        return (c - c[pbeg] + 1).astype(np.int64), None
    if vals is None:
        assert op == "count"
        okk = np.ones(n, dtype=bool)
    else:
        okk = np.ones(n, dtype=bool) if ok is None else ok
    cnt = _seg_accumulate(np.add, okk.astype(np.int64), part)
    if op == "count":
        r, rok = cnt, None
    else:
        f64 = vals.dtype == np.float64
        if op == "sum":
            if f64:
                r = _seg_accumulate(np.add, np.where(okk, vals + 0.0, 0.0), part)
            else:
                with np.errstate(over="ignore"):
                    r = _seg_accumulate(
                        np.add, np.where(okk, vals, 0).view(np.uint64), part
                    ).view(np.int64)
        else:
            enc = np_enc_f64(vals) if f64 else vals.view(np.uint64) ^ np.uint64(_SIGN)
            ident = np.uint64(_M64 if op == "min" else 0)
            enc = np.where(okk, enc, ident)
            acc = _seg_accumulate(np.minimum if op == "min" else np.maximum,
                                  enc, part)
            r = np_dec_f64(acc) if f64 else (acc ^ np.uint64(_SIGN)).view(np.int64)
        rok = cnt > 0
        r = np.where(rok, r, np.zeros(1, dtype=r.dtype))
        if ok is None:
            rok = None
    if frame != "rows":
        end = np_end(peer if frame == "range" else part)
        r = r[end]
        rok = rok[end] if rok is not None else None
    return r, rok


def np_shift(vals, ok, offset, part, default=None):
    """Returns (out, ok): NULL rows hold 0."""
    n = len(part)
    i = np.arange(n)
    j = i + offset
    inside = (j >= np_begin(part)) & (j <= np_end(part))
    jj = np.clip(j, 0, n - 1)
    src_ok = np.ones(n, dtype=bool) if ok is None else ok
    out_ok = np.where(inside, src_ok[jj], default is not None)
    dflt = vals.dtype.type(0 if default is None else default)
    out = np.where(inside, vals[jj], dflt)
    return np.where(out_ok, out, vals.dtype.type(0)), out_ok


# ---------------- conversions between the two forms ----------------

def to_list(vals, ok=None):
    """numpy column (+ ok) -> list with None for NULL."""
    vals = vals.tolist()
    if ok is None:
        return vals
    return [v if o else None for v, o in zip(vals, ok.tolist())]


def from_list(lst, dtype):
    """list with None -> (ndarray with 0 at NULL rows, ok bool ndarray)."""
    ok = np.array([v is not None for v in lst], dtype=bool)
    return np.array([0 if v is None else v for v in lst], dtype=dtype), ok


def bits_of(flags):
    """bool array -> the uint64 bitmap words, LSB-first, zero padded."""
    n = len(flags)
    padded = np.zeros((n + 63) // 64 * 64, dtype=bool)
    padded[:n] = flags
    return np.packbits(padded, bitorder="little").view(np.uint64)
