"""Row-by-row reference for compound WHERE predicates (spark_amd.predicate).

One row at a time, in plain Python, over the same predicate classes the
engine lowers: each node evaluates to True, False or None (SQL NULL) by
Kleene logic, with the leaf comparisons taken from expr_ref (cmp3_i64 /
cmp3_f64: -0.0 == 0.0, NaN == NaN and greatest; an int64 column against a
float literal compares as doubles). It knows nothing about the lowering: IN
and BETWEEN are evaluated from their SQL definitions, not as OR / AND chains.
tests/test_pred_ref.py pins it to hand-written tables.

`columns` maps a name to (values, valid, dtype): values a list / numpy array,
valid None or one bool per row, dtype "i64" or "f64".
"""
import numpy as np

from expr_ref import _DECIDE, cmp3_f64, cmp3_i64
from spark_amd import predicate as P


def _cmp(x, y, op, dtype):
    """three-valued x OP y; None operands give None."""
    if x is None or y is None:
        return None
    if dtype == "f64" or isinstance(y, float) or isinstance(x, float):
        # float64 column, or the bigint side cast to double (Spark)
        return _DECIDE[op](cmp3_f64(float(x), float(y)))
    return _DECIDE[op](cmp3_i64(int(x), int(y)))


def and3(a, b):
    if a is False or b is False:
        return False
    if a is None or b is None:
        return None
    return True


def or3(a, b):
    if a is True or b is True:
        return True
    if a is None or b is None:
        return None
    return False


def not3(a):
    return None if a is None else (not a)


def eval_row(pred, row, dtypes):
    """row: name -> Python value or None (NULL); dtypes: name -> "i64"/"f64"."""
    if isinstance(pred, P.Cmp):
        rhs = row[pred.rhs.name] if isinstance(pred.rhs, P.Col) else pred.rhs
        return _cmp(row[pred.col], rhs, pred.op, dtypes[pred.col])
    if isinstance(pred, P.IsNull):
        return row[pred.col] is None
    if isinstance(pred, P.IsNotNull):
        return row[pred.col] is not None
    if isinstance(pred, P.Between):
        dt = dtypes[pred.col]
        return and3(_cmp(row[pred.col], pred.lo, ">=", dt),
                    _cmp(row[pred.col], pred.hi, "<=", dt))
    if isinstance(pred, P.In):
        # Spark In.eval: an empty list is FALSE even for a NULL input; else
        # NULL input -> NULL; a hit -> TRUE; no hit -> NULL if the list holds
        # a NULL, else FALSE
        if not pred.values:
            return False
        x = row[pred.col]
        if x is None:
            return None
        dt = dtypes[pred.col]
        if any(v is not None and _cmp(x, v, "==", dt) for v in pred.values):
            return True
        return None if any(v is None for v in pred.values) else False
    if isinstance(pred, P.And):
        out = True
        for q in pred.ps:
            out = and3(out, eval_row(q, row, dtypes))
        return out
    if isinstance(pred, P.Or):
        out = False
        for q in pred.ps:
            out = or3(out, eval_row(q, row, dtypes))
        return out
    if isinstance(pred, P.Not):
        return not3(eval_row(pred.p, row, dtypes))
    raise ValueError(pred)


def _pyrows(vals, valid, dtype):
    rows = vals.tolist() if isinstance(vals, np.ndarray) else list(vals)
    conv = float if dtype == "f64" else int
    if valid is None:
        return [conv(x) for x in rows]
    ok = valid.tolist() if isinstance(valid, np.ndarray) else list(valid)
    assert len(ok) == len(rows)
    return [conv(x) if v else None for x, v in zip(rows, ok)]


def ref_eval(columns, pred):
    """-> list of True / False / None, one per row."""
    names = list(columns)
    dtypes = {k: columns[k][2] for k in names}
    data = [_pyrows(*columns[k]) for k in names]
    n = len(data[0]) if data else 0
    return [eval_row(pred, {k: d[i] for k, d in zip(names, data)}, dtypes)
            for i in range(n)]


def ref_filter_expr(columns, pred):
    """-> passing row ids (predicate TRUE), in input order (uint32)."""
    return np.array([i for i, t in enumerate(ref_eval(columns, pred))
                     if t is True], dtype=np.uint32)
