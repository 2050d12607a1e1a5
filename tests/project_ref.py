"""Row-by-row reference for SELECT-list expressions (spark_amd.expression).

One row at a time over Python ints (int64), floats (float64), bools and None
(SQL NULL), written from the SQL definitions: it walks the expression tree
itself and knows nothing about postfix programs, REF reuse or else-first
lowering. The arithmetic and comparison helpers come from expr_ref, the
Kleene connectives and the predicate leaves from pred_ref; only the tree
classes are imported from the engine. tests/test_project_ref.py pins it to a
hand-written table.

Semantics (Spark, non-ANSI):
  arithmetic  NULL if an operand is NULL or on `/` by zero (-0.0 is zero);
              int64 wraps, `/` truncates toward zero; float64 is IEEE
  neg / abs   int64 wraps (INT64_MIN stays); float64 flips / clears the sign
  cast        i64 -> f64 rounds to nearest even; f64 -> i64 is Java's (long):
              truncation, NaN -> 0, saturation at the int64 ends
  comparison  NULL if an operand is NULL; float64 in Spark's total order; an
              int64 operand against a float literal compares as doubles
  If / CaseWhen  a NULL condition is not TRUE; no arm and no ELSE gives NULL
  Coalesce    the first non-NULL operand

`columns` maps a name to (values, valid, dtype) as in pred_ref.
"""
import math

from expr_ref import (_DECIDE, I64_MAX, I64_MIN, binop_f64, binop_i64,
                      cmp3_f64, cmp3_i64, wrap_i64)
from pred_ref import _pyrows, and3, eval_row, not3, or3
from spark_amd import expression as E
from spark_amd import predicate as P


def cast_f64_to_i64(x: float) -> int:
    """Java's (long) d"""
    if math.isnan(x):
        return 0
    if x >= 2.0 ** 63:
        return I64_MAX
    if x <= -(2.0 ** 63):
        return I64_MIN
    return int(x)       # truncates toward zero


def type_of(e, dtypes):
    """"i64" / "f64" / "bool", or None for an untyped literal"""
    if isinstance(e, P.Pred):
        return "bool"
    if isinstance(e, P.Col):
        return dtypes[e.name]
    if isinstance(e, E.Lit):
        return e.dtype
    if isinstance(e, E.Cast):
        return e.to
    if isinstance(e, (E.Neg, E.Abs)):
        return type_of(e.e, dtypes)
    return _shared(_siblings(e), dtypes)


def _siblings(e):
    if isinstance(e, E.BinOp):
        return [e.a, e.b]
    if isinstance(e, E.If):
        return [e.then, e.else_]
    if isinstance(e, E.CaseWhen):
        return [v for _, v in e.branches] + \
            ([] if e.else_ is None else [e.else_])
    if isinstance(e, E.Coalesce):
        return list(e.es)
    raise ValueError(e)


def _shared(es, dtypes):
    types = {t for t in (type_of(x, dtypes) for x in es) if t is not None}
    assert len(types) <= 1, (es, types)
    return types.pop() if types else None


def _natural(es):
    vals = [x.value for x in es if isinstance(x, E.Lit) and x.value is not None]
    return "f64" if any(isinstance(v, float) for v in vals) else "i64"


def _as(value, dt):
    """a literal's Python value in type dt"""
    if value is None:
        return None
    return float(value) if dt == "f64" else int(value)


def ev(e, row, dtypes, want=None):
    """-> int / float / None. want types an untyped literal."""
    if isinstance(e, P.Pred):
        t = ev_pred(e, row, dtypes)
        return t
    if isinstance(e, P.Col):
        return row[e.name]
    if isinstance(e, E.Lit):
        return _as(e.value, e.dtype or want or _natural([e]))
    if isinstance(e, E.BinOp):
        dt = _shared([e.a, e.b], dtypes) or want or _natural([e.a, e.b])
        x, y = ev(e.a, row, dtypes, dt), ev(e.b, row, dtypes, dt)
        if x is None or y is None or (e.op == "/" and y == 0):
            return None
        return binop_i64(x, e.op, y) if dt == "i64" else binop_f64(x, e.op, y)
    if isinstance(e, E.Neg):
        x = ev(e.e, row, dtypes, want)
        if x is None:
            return None
        return wrap_i64(-x) if isinstance(x, int) else -x
    if isinstance(e, E.Abs):
        x = ev(e.e, row, dtypes, want)
        if x is None:
            return None
        return wrap_i64(abs(x)) if isinstance(x, int) else abs(x)
    if isinstance(e, E.Cast):
        x = ev(e.e, row, dtypes)
        if x is None:
            return None
        if isinstance(x, bool):
            return int(x)
        if e.to == "f64":
            return float(x)
        return cast_f64_to_i64(x) if isinstance(x, float) else x
    if isinstance(e, E.If):
        dt = _shared([e.then, e.else_], dtypes) or want or \
            _natural([e.then, e.else_])
        taken = e.then if ev_pred(e.cond, row, dtypes) is True else e.else_
        return ev(taken, row, dtypes, dt)
    if isinstance(e, E.CaseWhen):
        sib = _siblings(e)
        dt = _shared(sib, dtypes) or want or _natural(sib)
        for cond, val in e.branches:
            if ev_pred(cond, row, dtypes) is True:
                return ev(val, row, dtypes, dt)
        return None if e.else_ is None else ev(e.else_, row, dtypes, dt)
    if isinstance(e, E.Coalesce):
        dt = _shared(e.es, dtypes) or want or _natural(e.es)
        for x in e.es:
            v = ev(x, row, dtypes, dt)
            if v is not None:
                return v
        return None
    raise ValueError(e)


def ev_pred(p, row, dtypes):
    """-> True / False / None"""
    if isinstance(p, E.Compare):
        ta, tb = type_of(p.a, dtypes), type_of(p.b, dtypes)
        dt = ta or tb or _natural([p.a, p.b])

        def side(e):
            # an untyped float literal beside an int64 operand keeps its
            # value: Spark casts the bigint side to double
            if isinstance(e, E.Lit) and e.dtype is None \
                    and isinstance(e.value, float):
                return e.value
            return ev(e, row, dtypes, dt)

        x, y = side(p.a), side(p.b)
        if x is None or y is None:
            return None
        if isinstance(x, float) or isinstance(y, float):
            return _DECIDE[p.op](cmp3_f64(float(x), float(y)))
        return _DECIDE[p.op](cmp3_i64(x, y))
    if isinstance(p, (P.And, P.Or)):
        out = isinstance(p, P.And)
        for q in p.ps:
            out = (and3 if isinstance(p, P.And) else or3)(
                out, ev_pred(q, row, dtypes))
        return out
    if isinstance(p, P.Not):
        return not3(ev_pred(p.p, row, dtypes))
    return eval_row(p, row, dtypes)     # Cmp / In / Between / IsNull / IsNotNull


def out_type(e, dtypes):
    t = type_of(e, dtypes)
    if t is not None:
        return t
    while isinstance(e, (E.Neg, E.Abs)):       # -(2.5) is as untyped as 2.5
        e = e.e
    return _natural([e] if isinstance(e, E.Lit) else _siblings(e))


def ref_project(columns, outputs):
    """-> {name: (list of int / float / None per row, "i64" / "f64")}"""
    names = list(columns)
    dtypes = {k: columns[k][2] for k in names}
    data = [_pyrows(*columns[k]) for k in names]
    n = len(data[0]) if data else 0
    out = {}
    for name, e in outputs:
        e = E._operand(e)
        dt = out_type(e, dtypes)
        out[name] = ([ev(e, {k: d[i] for k, d in zip(names, data)}, dtypes)
                      for i in range(n)], dt)
    return out
