"""Row-by-row reference for the hash aggregates (gpuq_hash_agg_i64_f64,
gpuq_hash_agg_partitioned, gpuq_hash_agg_multi, gpuq_hash_agg_keys), after
HashAggregateExec.scala and Sum / Count / Min / Max.scala. Pure Python and
numpy; it uses neither `oracle` nor `spark_amd`.

`aggregate(key_cols, key_valids, specs)` groups the rows by the tuple of their
key values (None for a NULL key; NULL == NULL, so NULL keys form groups) and
returns {key tuple: [one result per spec]}.

  key_cols    list of int64 columns (numpy arrays or lists), one per key
  key_valids  list of bool columns or None per key column (None: no NULLs);
              None for the whole list means no key is NULL
  specs       list of (kind, values, valid): kind in KINDS, values an int64
              or float64 numpy array (None for "count*"), valid a bool array
              or None. ("count*",) alone is accepted too.

Semantics restated:
 - count* counts rows, count the non-NULL rows; both are Python ints and are
   never NULL;
 - sum / min / max skip NULL rows and are None (SQL NULL) for a group with no
   non-NULL input. The kernels leave such a group's accumulator at the op's
   init word and callers tell it by a paired COUNT of 0, so the tests compare
   that COUNT and not the word;
 - sum over int64 is the Python int sum reduced to two's-complement int64
   (non-ANSI wrap);
 - sum over float64 starts from +0.0 and is math.fsum of the non-NULL values,
   the correctly rounded sum, so any summation order is within
   sum_error_bound() of it and equal to it whenever every partial sum is
   exactly representable. Non-finite inputs are settled first, where the
   result is the same in every order: any NaN gives NaN, both infinities give
   NaN, one infinity gives that infinity. A group of only -0.0 gives +0.0;
 - min / max over int64 are Python ints;
 - min / max over float64 order NaN greatest with all NaNs equal and
   -0.0 == 0.0; a zero result is +0.0 and a NaN result the canonical quiet
   NaN. This is the order of the sort and of the window functions
   (tests/window_ref.py), and what the kernels' monotone encoding does. It
   DEVIATES from Spark, whose Double.compare puts -0.0 below 0.0: Spark
   returns -0.0 for min([-0.0]) and for min([-0.0, 0.0]), this returns +0.0.
tests/test_agg_ref.py pins all of this to hand-written tables.

`merge(kinds, a, b)` combines two results of the same spec list (sum of sums,
min of mins, ...); `np_aggregate` is a vectorised single-key form for inputs
too long for one Python call per row.
"""
import math

import numpy as np

KINDS = ("count*", "count", "sum", "min", "max")
_M64 = (1 << 64) - 1
_SIGN = 1 << 63


def wrap_i64(v):
    return ((v + _SIGN) & _M64) - _SIGN


def _f64_key(v):
    """total-order key: NaN greatest, all NaNs equal, -0.0 == 0.0."""
    return (1, 0.0) if math.isnan(v) else (0, v + 0.0)


def _f64_canon(v):
    if math.isnan(v):
        return float("nan")
    return v + 0.0          # -0.0 + 0.0 == +0.0, every other value unchanged


def sum_f64(values):
    """the float64 SUM of a non-empty list of non-NULL values."""
    if any(math.isnan(v) for v in values):
        return float("nan")
    pos = any(v == math.inf for v in values)
    neg = any(v == -math.inf for v in values)
    if pos and neg:
        return float("nan")
    if pos or neg:
        return math.inf if pos else -math.inf
    return math.fsum(values) + 0.0


def sum_error_bound(values):
    """|s - fsum(values)| for recursive summation s of the values in ANY
    order and any grouping: each of the len - 1 additions rounds by at most
    2^-53 of its result, and no partial result exceeds sum(|v|) to first
    order (Higham, Accuracy and Stability of Numerical Algorithms, 4.2)."""
    values = [float(v) for v in values]
    return (len(values) - 1) * 2.0 ** -53 * math.fsum(abs(v) for v in values)


def _is_float(values):
    return np.asarray(values).dtype.kind == "f"


def _reduce(kind, is_float, xs):
    """one spec over the non-NULL values xs of one group."""
    if kind == "count":
        return len(xs)
    if not xs:
        return None
    if kind == "sum":
        return sum_f64(xs) if is_float else wrap_i64(sum(xs))
    pick = min if kind == "min" else max
    if is_float:
        return _f64_canon(pick(xs, key=_f64_key))
    return pick(xs)


def _key_tuples(key_cols, key_valids, n):
    if key_valids is None:
        key_valids = [None] * len(key_cols)
    cols = []
    for k, kv in zip(key_cols, key_valids):
        k = [int(x) for x in k]
        if kv is not None:
            k = [x if ok else None for x, ok in zip(k, kv)]
        cols.append(k)
    return list(zip(*cols)) if cols else [()] * n


def aggregate(key_cols, key_valids, specs):
    n = len(key_cols[0])
    tuples = _key_tuples(key_cols, key_valids, n)
    rows = {}
    for i, kt in enumerate(tuples):
        rows.setdefault(kt, []).append(i)
    prepared = []
    for s in specs:
        kind = s[0]
        if kind not in KINDS:
            raise ValueError(f"bad spec kind {kind}")
        if kind == "count*":
            prepared.append((kind, False, None, None))
            continue
        values = s[1]
        valid = s[2] if len(s) > 2 else None
        prepared.append((kind, _is_float(values), np.asarray(values).tolist(),
                         None if valid is None else [bool(b) for b in valid]))
    out = {}
    for kt, idx in rows.items():
        res = []
        for kind, is_float, values, valid in prepared:
            if kind == "count*":
                res.append(len(idx))
                continue
            xs = [values[i] for i in idx if valid is None or valid[i]]
            res.append(_reduce(kind, is_float, xs))
        out[kt] = res
    return out


def _merge_one(kind, x, y):
    if kind in ("count", "count*"):
        return x + y
    if x is None or y is None:
        return y if x is None else x
    is_float = isinstance(x, float)
    if kind == "sum":
        return sum_f64([x, y]) if is_float else wrap_i64(x + y)
    return _reduce(kind, is_float, [x, y])


def merge(kinds, a, b):
    """results a and b of the same spec list (kinds[j] = its j-th kind) over
    two row sets -> the result over their union, when float sums are exact."""
    out = {kt: list(r) for kt, r in a.items()}
    for kt, r in b.items():
        if kt not in out:
            out[kt] = list(r)
        else:
            out[kt] = [_merge_one(k, x, y) for k, x, y in zip(kinds, out[kt], r)]
    return out


# ---------------- vectorised, single key ----------------

def np_aggregate(keys, key_valid, specs):
    """aggregate([keys], [key_valid], specs) for long inputs. Supported:
    count*, count, sum over int64, sum over INTEGER-VALUED finite float64
    whose group sums stay below 2^53 in magnitude (summed as int64, so
    exact; asserted), min / max over int64."""
    keys = np.asarray(keys, dtype=np.int64)
    n = len(keys)
    kv = np.ones(n, dtype=bool) if key_valid is None else np.asarray(key_valid, bool)
    uniq, inv = np.unique(keys[kv], return_inverse=True)
    gid = np.full(n, len(uniq), dtype=np.int64)     # last id: the NULL group
    gid[kv] = inv
    ng = len(uniq) + 1
    names = [(int(k),) for k in uniq] + [(None,)]
    present = np.bincount(gid, minlength=ng) > 0
    cols = []
    for s in specs:
        kind = s[0]
        if kind == "count*":
            cols.append(np.bincount(gid, minlength=ng).tolist())
            continue
        values = np.asarray(s[1])
        ok = np.ones(n, dtype=bool) if len(s) < 3 or s[2] is None \
            else np.asarray(s[2], bool)
        cnt = np.bincount(gid[ok], minlength=ng)
        if kind == "count":
            cols.append(cnt.tolist())
            continue
        g, v = gid[ok], values[ok]
        if kind == "sum" and values.dtype.kind == "f":
            vi = v.astype(np.int64)
            assert (vi.astype(np.float64) == v).all()
            absum = np.zeros(ng, dtype=np.int64)
            np.add.at(absum, g, np.abs(vi))
            assert (absum < (1 << 53)).all()
            acc = np.zeros(ng, dtype=np.int64)
            np.add.at(acc, g, vi)
            res = [float(x) for x in acc.tolist()]
        elif kind == "sum":
            acc = np.zeros(ng, dtype=np.uint64)
            np.add.at(acc, g, v.astype(np.int64).view(np.uint64))   # wraps
            res = acc.view(np.int64).tolist()
        elif kind in ("min", "max"):
            if values.dtype.kind == "f":
                raise ValueError("np_aggregate: min/max over int64 only")
            info = np.iinfo(np.int64)
            acc = np.full(ng, info.max if kind == "min" else info.min, np.int64)
            (np.minimum if kind == "min" else np.maximum).at(acc, g, v)
            res = acc.tolist()
        else:
            raise ValueError(f"bad spec kind {kind}")
        cols.append([r if c else None for r, c in zip(res, cnt.tolist())])
    return {names[i]: [c[i] for c in cols] for i in range(ng) if present[i]}
