"""Pins tests/join_cond_ref.py (the nested-loop reference the GPU tests of
the residual join condition compare against) to a table small enough to
join by hand. Every expected list below is written out, not computed.

    probe  k     x     f        build  k     y     g
    p0     1     3    -0.0      b0     1     5     0.0
    p1     2     4     2.0      b1     1     1     1.0
    p2     3     1     1.5      b2     1     9     NaN
    p3     NULL  0     0.0      b3     2     0     2.0
    p4     1     NULL  NaN      b4     3     NULL  NULL
    p5     9     0     0.0      b5     NULL  100  -1.0
                                b6     4     7    -0.0

Candidates (keys equal, no NULL key): p0 and p4 -> b0 b1 b2; p1 -> b3;
p2 -> b4; p3 (NULL key) and p5 (no such key) -> none; b5 (NULL key) and b6
are nobody's candidate.

x < y:   p0: b0 TRUE (3 < 5), b1 FALSE, b2 TRUE  — three candidates, the
         1st and 3rd pass;  p1: b3 FALSE — the only candidate fails;
         p2: b4 NULL (y is NULL);  p4: NULL three times (x is NULL).
f != g:  p0: b0 FALSE (-0.0 == 0.0), b1 TRUE, b2 TRUE (NaN differs from
         -0.0);  p1: b3 FALSE;  p2: b4 NULL;  p4: b0 TRUE, b1 TRUE,
         b2 FALSE (NaN == NaN).
"""
import numpy as np
import pytest

import join_cond_ref as R
from spark_amd.predicate import And, Cmp, Col, IsNull, Not

NIL = R.NIL
NAN = float("nan")

PK = [(np.array([1, 2, 3, 0, 1, 9], dtype=np.int64),
       np.array([1, 1, 1, 0, 1, 1], dtype=bool))]
BK = [(np.array([1, 1, 1, 2, 3, 0, 4], dtype=np.int64),
       np.array([1, 1, 1, 1, 1, 0, 1], dtype=bool))]
PCOLS = {
    "x": (np.array([3, 4, 1, 0, 0, 0], dtype=np.int64),
          np.array([1, 1, 1, 1, 0, 1], dtype=bool), "i64"),
    "f": (np.array([-0.0, 2.0, 1.5, 0.0, NAN, 0.0]), None, "f64"),
}
BCOLS = {
    "y": (np.array([5, 1, 9, 0, 0, 100, 7], dtype=np.int64),
          np.array([1, 1, 1, 1, 0, 1, 1], dtype=bool), "i64"),
    "g": (np.array([0.0, 1.0, NAN, 2.0, 0.0, -1.0, -0.0]),
          np.array([1, 1, 1, 1, 0, 1, 1], dtype=bool), "f64"),
}

X_LT_Y = Cmp("x", "<", Col("y"))
F_NE_G = Cmp("f", "!=", Col("g"))

EXPECTED = {
    "x<y": {
        R.INNER: ([(0, 0), (0, 2)], []),
        R.OUTER: ([(0, 0), (0, 2), (1, NIL), (2, NIL), (3, NIL), (4, NIL),
                   (5, NIL)], []),
        R.SEMI: ([(0, NIL)], []),
        R.ANTI: ([(1, NIL), (2, NIL), (3, NIL), (4, NIL), (5, NIL)], []),
        R.FULL: ([(0, 0), (0, 2), (1, NIL), (2, NIL), (3, NIL), (4, NIL),
                  (5, NIL)], [1, 3, 4, 5, 6]),
    },
    "f!=g": {
        R.INNER: ([(0, 1), (0, 2), (4, 0), (4, 1)], []),
        R.OUTER: ([(0, 1), (0, 2), (1, NIL), (2, NIL), (3, NIL), (4, 0),
                   (4, 1), (5, NIL)], []),
        R.SEMI: ([(0, NIL), (4, NIL)], []),
        R.ANTI: ([(1, NIL), (2, NIL), (3, NIL), (5, NIL)], []),
        R.FULL: ([(0, 1), (0, 2), (1, NIL), (2, NIL), (3, NIL), (4, 0),
                  (4, 1), (5, NIL)], [3, 4, 5, 6]),
    },
}
PREDS = {"x<y": X_LT_Y, "f!=g": F_NE_G}


def test_candidates_by_hand():
    assert R.candidate_lists(PK, BK) == [[0, 1, 2], [3], [4], [], [0, 1, 2], []]


def test_verdicts_by_hand():
    cands = R.candidate_lists(PK, BK)
    assert R.verdicts(cands, PCOLS, BCOLS, X_LT_Y) == [
        [(0, True), (1, False), (2, True)], [(3, False)], [(4, None)], [],
        [(0, None), (1, None), (2, None)], []]
    assert R.verdicts(cands, PCOLS, BCOLS, F_NE_G) == [
        [(0, False), (1, True), (2, True)], [(3, False)], [(4, None)], [],
        [(0, True), (1, True), (2, False)], []]


@pytest.mark.parametrize("jt", [R.INNER, R.OUTER, R.SEMI, R.ANTI, R.FULL])
@pytest.mark.parametrize("name", list(PREDS))
def test_known_answers(name, jt):
    pairs, unmatched = R.join_cond_ref(PK, BK, PCOLS, BCOLS, PREDS[name], jt)
    assert (pairs, unmatched) == EXPECTED[name][jt]


def test_null_verdict_is_not_a_false_one():
    # NOT (x < y): the NULL pairs stay NULL and still fail, so p2 and p4
    # match nothing under the predicate and under its negation
    neg = Not(X_LT_Y)
    pairs, _ = R.join_cond_ref(PK, BK, PCOLS, BCOLS, neg, R.INNER)
    assert pairs == [(0, 1), (1, 3)]
    anti, _ = R.join_cond_ref(PK, BK, PCOLS, BCOLS, neg, R.ANTI)
    assert anti == [(2, NIL), (3, NIL), (4, NIL), (5, NIL)]


def test_one_sided_conditions():
    # probe-only: IS NULL(x) holds for p4 alone -> all three candidates pass
    pairs, un = R.join_cond_ref(PK, BK, PCOLS, BCOLS, IsNull("x"), R.FULL)
    assert pairs == [(0, NIL), (1, NIL), (2, NIL), (3, NIL), (4, 0), (4, 1),
                     (4, 2), (5, NIL)]
    assert un == [3, 4, 5, 6]
    # build-only: y >= 5 holds for b0, b2 (and b5, b6: nobody's candidates)
    pairs, un = R.join_cond_ref(PK, BK, PCOLS, BCOLS, Cmp("y", ">=", 5),
                                R.FULL)
    assert pairs == [(0, 0), (0, 2), (1, NIL), (2, NIL), (3, NIL), (4, 0),
                     (4, 2), (5, NIL)]
    assert un == [1, 3, 4, 5, 6]


def test_two_key_columns_null_in_either():
    pk = [(np.array([1, 1, 1], dtype=np.int64), None),
          (np.array([7, 8, 7], dtype=np.int64), np.array([1, 1, 0], bool))]
    bk = [(np.array([1, 1, 1, 2], dtype=np.int64), np.array([1, 0, 1, 1], bool)),
          (np.array([7, 7, 8, 7], dtype=np.int64), None)]
    assert R.candidate_lists(pk, bk) == [[0], [2], []]
    both = And(Cmp("x", ">=", 0), Cmp("y", ">=", 0))
    pairs, un = R.join_cond_ref(
        pk, bk, {"x": (np.array([0, -1, 0]), None, "i64")},
        {"y": (np.array([0, 0, 0, 0]), None, "i64")}, both, R.FULL)
    assert pairs == [(0, 0), (1, NIL), (2, NIL)] and un == [1, 2, 3]
