"""Pins tests/project_ref.py to a hand-written known-answer table. Every
expected value below was worked out by hand from the SQL / Java rules, not
produced by the code under test. No GPU needed."""
import math
import struct

import pytest

import project_ref as R
from spark_amd.expression import (Abs, BinOp, CaseWhen, Cast, Coalesce,
                                  Compare, If, Lit, Neg)
from spark_amd.predicate import And, Between, Cmp, Col, In, IsNull, Not, Or

MIN, MAX = -(1 << 63), (1 << 63) - 1
NAN, INF = float("nan"), float("inf")
DT = {"i": "i64", "j": "i64", "x": "f64", "y": "f64"}


def one(e, **row):
    full = {"i": None, "j": None, "x": None, "y": None}
    full.update(row)
    return R.ev(e, full, DT)


def same(got, want):
    """exact, sign of zero included; NaN equals NaN"""
    if want is None or got is None:
        return got is None and want is None
    if isinstance(want, float):
        if math.isnan(want):
            return isinstance(got, float) and math.isnan(got)
        return isinstance(got, float) and \
            struct.pack("<d", got) == struct.pack("<d", want)
    return type(got) is type(want) and got == want


I, J, X, Y = Col("i"), Col("j"), Col("x"), Col("y")

TABLE = [
    # ---- int64 arithmetic wraps ----
    (BinOp("+", I, J), dict(i=MAX, j=1), MIN),
    (BinOp("-", I, J), dict(i=MIN, j=1), MAX),
    (BinOp("*", I, J), dict(i=MAX, j=2), -2),
    (BinOp("*", I, J), dict(i=MIN, j=-1), MIN),
    (BinOp("/", I, J), dict(i=MIN, j=-1), MIN),
    (BinOp("/", I, J), dict(i=-7, j=2), -3),          # toward zero
    (BinOp("/", I, J), dict(i=7, j=-2), -3),
    (BinOp("/", I, J), dict(i=7, j=0), None),
    (BinOp("/", I, 0), dict(i=7), None),
    (BinOp("+", I, J), dict(i=None, j=1), None),
    (BinOp("+", I, J), dict(i=1, j=None), None),
    (BinOp("-", 100, I), dict(i=30), 70),
    # ---- float64 ----
    (BinOp("/", X, Y), dict(x=1.0, y=0.0), None),
    (BinOp("/", X, Y), dict(x=1.0, y=-0.0), None),
    (BinOp("/", X, -0.0), dict(x=1.0), None),
    (BinOp("/", X, Y), dict(x=1.0, y=NAN), NAN),       # a NaN divisor is not zero
    (BinOp("/", X, Y), dict(x=1.0, y=INF), 0.0),
    (BinOp("*", X, Y), dict(x=1e308, y=10.0), INF),
    (BinOp("-", X, Y), dict(x=INF, y=INF), NAN),
    (BinOp("+", X, 1), dict(x=0.5), 1.5),              # int literal beside f64
    (BinOp("*", X, Y), dict(x=-0.0, y=5.0), -0.0),
    # ---- casts ----
    (Cast(X, "i64"), dict(x=NAN), 0),
    (Cast(X, "i64"), dict(x=INF), MAX),
    (Cast(X, "i64"), dict(x=-INF), MIN),
    (Cast(X, "i64"), dict(x=2.0 ** 63), MAX),
    (Cast(X, "i64"), dict(x=-(2.0 ** 63)), MIN),
    (Cast(X, "i64"), dict(x=2.0 ** 63 - 1024), (1 << 63) - 1024),
    (Cast(X, "i64"), dict(x=1e19), MAX),
    (Cast(X, "i64"), dict(x=-1e19), MIN),
    (Cast(X, "i64"), dict(x=-0.9), 0),
    (Cast(X, "i64"), dict(x=-1.9), -1),
    (Cast(X, "i64"), dict(x=2.5), 2),
    (Cast(X, "i64"), dict(x=None), None),
    (Cast(I, "f64"), dict(i=MAX), 2.0 ** 63),          # rounds to nearest even
    (Cast(I, "f64"), dict(i=(1 << 53) + 1), 2.0 ** 53),
    (Cast(I, "f64"), dict(i=(1 << 53) + 3), 2.0 ** 53 + 4),
    (Cast(I, "f64"), dict(i=MIN), -(2.0 ** 63)),
    (Cast(Compare(I, "<", J), "i64"), dict(i=1, j=2), 1),
    (Cast(Compare(I, "<", J), "i64"), dict(i=2, j=2), 0),
    (Cast(Compare(I, "<", J), "i64"), dict(i=None, j=2), None),
    (Cast(IsNull("i"), "i64"), dict(i=None), 1),
    # ---- neg / abs ----
    (Neg(I), dict(i=MIN), MIN),
    (Abs(I), dict(i=MIN), MIN),
    (Neg(I), dict(i=MAX), MIN + 1),
    (Abs(I), dict(i=-5), 5),
    (Neg(X), dict(x=-0.0), 0.0),
    (Neg(X), dict(x=0.0), -0.0),
    (Abs(X), dict(x=-0.0), 0.0),
    (Neg(X), dict(x=NAN), NAN),
    (Abs(X), dict(x=NAN), NAN),
    (Abs(X), dict(x=-INF), INF),
    (Neg(I), dict(i=None), None),
    # ---- If / CaseWhen ----
    (If(Compare(I, ">", 0), Lit(1), Lit(2)), dict(i=None), 2),   # NULL cond -> else
    (If(Compare(I, ">", 0), Lit(1), Lit(2)), dict(i=5), 1),
    (If(Compare(I, ">", 0), J, Lit(None)), dict(i=5, j=None), None),
    (If(Compare(I, ">", 0), BinOp("/", J, 0), Lit(9)), dict(i=-1, j=1), 9),
    (CaseWhen([(Compare(I, "==", 1), Lit(10)), (Compare(I, "==", 2), Lit(20))]),
     dict(i=3), None),
    (CaseWhen([(Compare(I, "==", 1), Lit(10)), (Compare(I, "==", 2), Lit(20))]),
     dict(i=2), 20),
    (CaseWhen([(Compare(I, "==", 1), Lit(10)), (Compare(I, "==", 2), Lit(20))]),
     dict(i=None), None),
    (CaseWhen([(Compare(I, ">", 0), Lit(10)), (Compare(I, ">", 1), Lit(20))],
              else_=Lit(30)), dict(i=5), 10),                    # first arm wins
    (CaseWhen([(Between("i", 1, 3), X), (In("i", [7, None]), Y)], else_=Lit(0.5)),
     dict(i=7, x=1.0, y=2.0), 2.0),
    (CaseWhen([(Between("i", 1, 3), X), (In("i", [7, None]), Y)], else_=Lit(0.5)),
     dict(i=8, x=1.0, y=2.0), 0.5),                              # IN is NULL -> else
    # ---- Coalesce ----
    (Coalesce(I, J, 0), dict(i=None, j=None), 0),
    (Coalesce(I, J, 0), dict(i=None, j=4), 4),
    (Coalesce(I, J), dict(i=None, j=None), None),
    (Coalesce(X, Y), dict(x=NAN, y=1.0), NAN),                   # NaN is not NULL
    (Coalesce(Lit(None, "i64"), Lit(None, "i64")), dict(), None),
    # ---- comparisons as values ----
    (Cast(Compare(X, "==", Y), "i64"), dict(x=NAN, y=NAN), 1),
    (Cast(Compare(X, ">", Y), "i64"), dict(x=NAN, y=INF), 1),
    (Cast(Compare(X, "<", Y), "i64"), dict(x=NAN, y=INF), 0),
    (Cast(Compare(X, "==", Y), "i64"), dict(x=-0.0, y=0.0), 1),
    (Cast(Compare(X, "<", Y), "i64"), dict(x=-0.0, y=0.0), 0),
    (Cast(Compare(X, "!=", Y), "i64"), dict(x=1.0, y=NAN), 1),
    (Cast(Compare(X, "<=", Y), "i64"), dict(x=1.0, y=NAN), 1),
    (Cast(Compare(I, "<", 0.5), "i64"), dict(i=0), 1),           # as doubles
    (Cast(Compare(I, "<", 0.5), "i64"), dict(i=1), 0),
    (Cast(Compare(0.5, "<", I), "i64"), dict(i=1), 1),
    (Cast(Compare(I, "<", NAN), "i64"), dict(i=MAX), 1),
    (Cast(Compare(BinOp("+", I, 1), ">", BinOp("*", J, 2)), "i64"), dict(i=4, j=2), 1),
    # ---- Kleene connectives over Compare ----
    (Cast(And(Compare(I, ">", 0), Compare(J, ">", 0)), "i64"), dict(i=None, j=-1), 0),
    (Cast(And(Compare(I, ">", 0), Compare(J, ">", 0)), "i64"), dict(i=None, j=1), None),
    (Cast(Or(Compare(I, ">", 0), Compare(J, ">", 0)), "i64"), dict(i=None, j=1), 1),
    (Cast(Or(Compare(I, ">", 0), Cmp("j", ">", 0)), "i64"), dict(i=None, j=-1), None),
    (Cast(Not(Compare(I, ">", 0)), "i64"), dict(i=None), None),
    (Cast(Not(Compare(I, ">", 0)), "i64"), dict(i=1), 0),
]


@pytest.mark.parametrize("k", range(len(TABLE)))
def test_known_answers(k):
    e, row, want = TABLE[k]
    got = one(e, **row)
    assert same(got, want), (e, row, got, want)


def test_cast_helper():
    assert R.cast_f64_to_i64(float(1 << 62)) == 1 << 62
    assert R.cast_f64_to_i64(-0.0) == 0
    assert R.cast_f64_to_i64(9.223372036854775e18) == 9223372036854774784


def test_ref_project_columns_and_types():
    cols = {"i": ([1, 2, 3], [True, False, True], "i64"),
            "x": ([0.5, 1.5, NAN], None, "f64")}
    out = R.ref_project(cols, [("a", BinOp("*", Col("i"), 3)),
                               ("b", Neg(Col("x"))),
                               ("c", Lit(7)), ("d", Lit(2.0))])
    assert out["a"] == ([3, None, 9], "i64")
    assert out["b"][1] == "f64" and out["b"][0][:2] == [-0.5, -1.5]
    assert math.isnan(out["b"][0][2])
    assert out["c"] == ([7, 7, 7], "i64")
    assert out["d"] == ([2.0, 2.0, 2.0], "f64")
