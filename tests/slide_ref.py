"""Row-by-row reference for sliding ROWS BETWEEN frames and first_value /
last_value (gpuq_window_slide and GpuWindowExec), after
WindowFunctionFrame.scala's SlidingWindowFunctionFrame.

The rows are already sorted; `part` marks where a partition starts (as in
tests/window_ref.py). Row i of the partition [pb, pe] (inclusive positions)
has the frame first..last with

    first = max(pb, i + lo)        (lo None: UNBOUNDED PRECEDING, first = pb)
    last  = min(pe, i + hi)        (hi None: UNBOUNDED FOLLOWING, last = pe)

and the frame is EMPTY when first > last. lo / hi are signed row counts:
negative PRECEDING, 0 CURRENT ROW, positive FOLLOWING.

`slide` evaluates every row on its own, re-adding the frame's rows in row
order the way Spark does, so a float64 SUM is acc = +0.0 followed by acc += v
for the non-NULL rows first..last ascending. NULL and NaN rules are
window_ref's: SUM / MIN / MAX skip NULLs and are NULL when the frame holds no
non-NULL value (an empty frame included); COUNT is never NULL and 0 for an
empty frame; int64 SUM wraps; float64 MIN / MAX order NaN greatest and -0.0 ==
0.0 and return the canonical NaN and +0.0. first_value / last_value
(ignoreNulls = false) copy the value and NULL-ness of row first / last and are
NULL for an empty frame.

`np_slide` is the vectorised numpy twin for long inputs. For two finite
bounds its float SUM adds offset by offset,
    for j in range(lo, hi + 1): acc += where(in_frame & ok, v[i + j], 0.0)
which keeps the left-to-right order (acc starts at +0.0 and can never become
-0.0, so adding +0.0 for a skipped row changes no bit). With lo None it picks
from window_ref.np_scan's running ROWS result, which accumulates in row order
too. tests/test_slide_ref.py pins both to hand-written tables and to each
other.
"""
import numpy as np

import window_ref as R

OPS = ("count", "sum", "min", "max", "first_value", "last_value")


# ---------------- row by row ----------------

def frame_of(i, lo, hi, pb, pe):
    """(first, last) of row i in the partition [pb, pe]; first > last: empty."""
    first = pb if lo is None else max(pb, i + lo)
    last = pe if hi is None else min(pe, i + hi)
    return first, last


def _fold(op, dtype, xs):
    """op over the non-NULL values xs, in order; None when there are none."""
    if not xs:
        return None
    if op == "sum":
        if dtype == "i64":
            acc = 0
            for x in xs:
                acc = R.wrap_i64(acc + x)
            return acc
        acc = 0.0
        for x in xs:
            acc = acc + x
        return acc
    acc = xs[0]
    for x in xs[1:]:
        if dtype == "f64":
            kx, ka = R._f64_key(x), R._f64_key(acc)
        else:
            kx, ka = x, acc
        if (kx < ka) if op == "min" else (kx > ka):
            acc = x
    return R._f64_canon(acc) if dtype == "f64" else acc


def slide(op, lo, hi, part, vals=None, dtype="i64"):
    """op: count / sum / min / max / first_value / last_value. part: list of
    bools. vals: list with None for NULL, or None for COUNT(*). Returns the
    list of results (None for NULL)."""
    assert op in OPS
    n = len(part)
    out = [None] * n
    for b, e in R._partitions(part):
        pb, pe = b, e - 1
        for i in range(b, e):
            first, last = frame_of(i, lo, hi, pb, pe)
            empty = first > last
            if op == "count":
                if empty:
                    out[i] = 0
                elif vals is None:
                    out[i] = last - first + 1
                else:
                    out[i] = sum(v is not None for v in vals[first:last + 1])
            elif empty:
                out[i] = None
            elif op == "first_value":
                out[i] = vals[first]
            elif op == "last_value":
                out[i] = vals[last]
            else:
                out[i] = _fold(op, dtype,
                               [v for v in vals[first:last + 1] if v is not None])
    return out


def avg(lo, hi, part, vals):
    """sliding SUM / sliding COUNT over a float64 column; NULL where the
    count is 0."""
    s = slide("sum", lo, hi, part, vals, "f64")
    c = slide("count", lo, hi, part, vals, "f64")
    return [None if ci == 0 else si / ci for si, ci in zip(s, c)]


# ---------------- vectorised numpy twin ----------------

def np_slide(op, lo, hi, part, vals=None, ok=None):
    """part: bool array; vals: int64 / float64 array or None (COUNT(*)); ok:
    bool array or None (no NULLs). Returns (out, out_ok): out_ok is None for
    count, else a bool array; NULL rows hold 0."""
    assert op in OPS
    n = len(part)
    i = np.arange(n)
    pb, pe = R.np_begin(part), R.np_end(part)
    first = pb if lo is None else np.maximum(pb, i + lo)
    last = pe if hi is None else np.minimum(pe, i + hi)
    nonempty = first <= last
    okk = np.ones(n, dtype=bool) if (vals is None or ok is None) else ok

    if op in ("first_value", "last_value"):
        at = np.clip(first if op == "first_value" else last, 0, n - 1)
        rok = nonempty & okk[at]
        return np.where(rok, vals[at], vals.dtype.type(0)), rok

    if lo is None:
        # UNBOUNDED PRECEDING .. hi: the running ROWS result at row `last`
        with np.errstate(over="ignore", invalid="ignore"):
            r, rok = R.np_scan(op, "rows", part, part, vals,
                               okk if vals is not None else None)
        at = np.clip(last, 0, n - 1)
        if op == "count":
            return np.where(nonempty, r[at], 0).astype(np.int64), None
        rok = nonempty & rok[at]
        return np.where(rok, r[at], r.dtype.type(0)), rok

    f64 = vals is not None and vals.dtype == np.float64
    cnt = np.zeros(n, dtype=np.int64)
    if op == "sum":
        acc = np.zeros(n, dtype=np.float64 if f64 else np.uint64)
    elif op in ("min", "max"):
        enc = R.np_enc_f64(vals) if f64 else vals.view(np.uint64) ^ np.uint64(R._SIGN)
        acc = np.full(n, R._M64 if op == "min" else 0, dtype=np.uint64)
    for j in range(lo, hi + 1):
        idx = i + j
        src = np.clip(idx, 0, n - 1)
        use = (idx >= first) & (idx <= last) & okk[src]
        cnt += use
        if op == "sum":
            if f64:
                with np.errstate(over="ignore", invalid="ignore"):
                    acc = acc + np.where(use, vals[src], 0.0)
            else:
                acc = acc + np.where(use, vals[src].view(np.uint64), np.uint64(0))
        elif op == "min":
            acc = np.where(use, np.minimum(acc, enc[src]), acc)
        elif op == "max":
            acc = np.where(use, np.maximum(acc, enc[src]), acc)
    if op == "count":
        return cnt, None
    rok = cnt > 0
    if op == "sum":
        r = acc if f64 else acc.view(np.int64)
    else:
        r = R.np_dec_f64(acc) if f64 else (acc ^ np.uint64(R._SIGN)).view(np.int64)
    return np.where(rok, r, r.dtype.type(0)), rok
