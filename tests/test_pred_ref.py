"""Known-answer tables for tests/pred_ref.py (no GPU needed).

The GPU tests trust pred_ref as the reference for compound predicates; these
tables, written out by hand from Spark's rules, pin it. T / F / N are SQL
TRUE / FALSE / NULL.
"""
import pytest

import pred_ref as R
from spark_amd.predicate import (And, Between, Cmp, Col, In, IsNotNull, IsNull,
                                 Not, Or)

T, F, N = True, False, None
NAN, INF = float("nan"), float("inf")


def ev(pred, dtype="i64", **row):
    return R.eval_row(pred, row, {k: dtype for k in row})


# x > 0 over an int64 x is T for 1, F for 0, N for NULL: the three inputs
TV = {T: 1, F: 0, N: None}
AND_TABLE = [(T, T, T), (T, F, F), (T, N, N),
             (F, T, F), (F, F, F), (F, N, F),
             (N, T, N), (N, F, F), (N, N, N)]
OR_TABLE = [(T, T, T), (T, F, T), (T, N, T),
            (F, T, T), (F, F, F), (F, N, N),
            (N, T, T), (N, F, N), (N, N, N)]


@pytest.mark.parametrize("a,b,want", AND_TABLE)
def test_and_truth_table(a, b, want):
    assert R.and3(a, b) is want
    assert ev(And(Cmp("x", ">", 0), Cmp("y", ">", 0)), x=TV[a], y=TV[b]) is want


@pytest.mark.parametrize("a,b,want", OR_TABLE)
def test_or_truth_table(a, b, want):
    assert R.or3(a, b) is want
    assert ev(Or(Cmp("x", ">", 0), Cmp("y", ">", 0)), x=TV[a], y=TV[b]) is want


def test_not():
    assert R.not3(T) is F and R.not3(F) is T and R.not3(N) is N
    assert ev(Not(Cmp("x", ">", 5)), x=6) is F
    assert ev(Not(Cmp("x", ">", 5)), x=5) is T
    assert ev(Not(Cmp("x", ">", 5)), x=None) is N     # NOT NULL is NULL


def test_nary_and_or():
    p = And(Cmp("x", ">", 0), Cmp("x", "<", 10), Cmp("x", "!=", 5))
    assert [ev(p, x=v) for v in (1, 5, 10, None)] == [T, F, F, N]
    q = Or(Cmp("x", "==", 1), Cmp("x", "==", 2), Cmp("x", "==", 3))
    assert [ev(q, x=v) for v in (2, 4, None)] == [T, F, N]


@pytest.mark.parametrize("x,want", [(2, T), (4, F), (None, N)])
def test_in_without_null_literal(x, want):
    assert ev(In("x", [1, 2, 3]), x=x) is want


@pytest.mark.parametrize("x,want", [(2, T), (4, N), (None, N)])
def test_in_with_null_literal(x, want):
    # a miss against a list holding NULL is NULL, not FALSE
    assert ev(In("x", [1, 2, None]), x=x) is want


def test_in_empty_list_is_false_even_for_null():
    assert ev(In("x", []), x=1) is F
    assert ev(In("x", []), x=None) is F


@pytest.mark.parametrize("x", [1, 2, 4, None])
def test_not_in_with_null_is_never_true(x):
    # hit -> NOT TRUE = FALSE; miss or NULL input -> NOT NULL = NULL
    got = ev(Not(In("x", [1, 2, None])), x=x)
    assert got is not T
    assert got is (F if x in (1, 2) else N)


def test_not_in_without_null():
    p = Not(In("x", [1, 2]))
    assert [ev(p, x=v) for v in (1, 3, None)] == [F, T, N]


def test_is_null_or_cmp():
    p = Or(IsNull("x"), Cmp("x", ">", 5))
    assert [ev(p, x=v) for v in (None, 6, 5)] == [T, T, F]
    assert [ev(IsNotNull("x"), x=v) for v in (None, 0)] == [F, T]
    # x > 5 OR y < 3 is TRUE when x is NULL and y = 1
    q = Or(Cmp("x", ">", 5), Cmp("y", "<", 3))
    assert ev(q, x=None, y=1) is T
    assert ev(q, x=None, y=3) is N


def test_between():
    p = Between("x", 2, 4)
    assert [ev(p, x=v) for v in (1, 2, 3, 4, 5, None)] == [F, T, T, T, F, N]


def test_cmp_null_literal():
    assert ev(Cmp("x", "==", None), x=1) is N


F64_COLCOL = [
    # x, y, ==, <, <=, >, >=, !=
    (NAN, NAN, T, F, T, F, T, F),       # NaN == NaN
    (NAN, INF, F, F, F, T, T, T),       # NaN above +inf
    (INF, NAN, F, T, T, F, F, T),
    (-0.0, 0.0, T, F, T, F, T, F),      # -0.0 == 0.0
    (0.0, -0.0, T, F, T, F, T, F),
    (-INF, -0.0, F, T, T, F, F, T),
    (1.5, NAN, F, T, T, F, F, T),
]


@pytest.mark.parametrize("row", F64_COLCOL)
def test_f64_column_vs_column(row):
    x, y = row[0], row[1]
    for op, want in zip(("==", "<", "<=", ">", ">=", "!="), row[2:]):
        assert ev(Cmp("x", op, Col("y")), "f64", x=x, y=y) is want, (x, op, y)
        # a NULL on either side is NULL whatever the other holds
        assert ev(Cmp("x", op, Col("y")), "f64", x=None, y=y) is N
        assert ev(Cmp("x", op, Col("y")), "f64", x=x, y=None) is N


def test_i64_column_vs_column():
    big = (1 << 62) + 1
    assert ev(Cmp("x", "<", Col("y")), x=big, y=big + 1) is T   # exact, no double
    assert ev(Cmp("x", "==", Col("y")), x=-1, y=-1) is T
    assert ev(Cmp("x", "!=", Col("y")), x=-1, y=None) is N


# int64 column against a fractional literal: compared as doubles, never
# truncated (filter_cmp's docstring: k < 0.5 must keep k == 0)
I64_FRACTIONAL = [
    ("<", 0.5, {0: T, 1: F, -1: T}),
    ("<=", 0.5, {0: T, 1: F}),
    (">", 0.5, {0: F, 1: T}),
    (">=", 0.5, {0: F, 1: T}),
    ("==", 0.5, {0: F, 1: F}),
    ("!=", 0.5, {0: T, 1: T}),
    (">", -0.5, {0: T, -1: F}),
    ("<", NAN, {0: T, (1 << 63) - 1: T}),     # NaN above every bigint
    (">=", NAN, {0: F}),
    ("<", INF, {(1 << 63) - 1: T}),
    (">", -INF, {-(1 << 63): T}),
    ("<", -INF, {0: F}),
]


@pytest.mark.parametrize("op,lit,table", I64_FRACTIONAL)
def test_i64_vs_fractional_literal(op, lit, table):
    for x, want in table.items():
        assert ev(Cmp("x", op, lit), x=x) is want, (x, op, lit)
    assert ev(Cmp("x", op, lit), x=None) is N    # NULL row stays NULL


def test_ref_filter_expr_rows():
    import numpy as np
    cols = {"x": (np.array([1, 7, 9, 3], np.int64),
                  np.array([True, True, False, True]), "i64"),
            "y": (np.array([0.5, NAN, 1.0, -0.0]), None, "f64")}
    p = Or(Cmp("x", ">", 5), Cmp("y", "==", 0.0))
    assert R.ref_eval(cols, p) == [F, T, N, T]
    assert R.ref_filter_expr(cols, p).tolist() == [1, 3]
    assert R.ref_filter_expr(cols, p).dtype == np.uint32
