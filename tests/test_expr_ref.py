"""Known-answer tables for tests/expr_ref.py (no GPU needed).

The GPU parity tests trust expr_ref as the reference for the filter and
project kernels, so the reference itself is pinned here to answers written
out by hand. Every row names the Spark (non-ANSI) rule it encodes; nothing
in the expected columns is computed."""
import math
import struct

import numpy as np
import pytest

import expr_ref as R

MIN, MAX = -(1 << 63), (1 << 63) - 1
INF, NAN = math.inf, math.nan

# ---------------------------------------------------------------- compare
#            -inf  -1.5  -0.0  0.0  1.5  inf  NaN  NULL
F64_VALS = [-INF, -1.5, -0.0, 0.0, 1.5, INF, NAN, 0.0]
F64_VALID = [True, True, True, True, True, True, True, False]

# (literal, op, expected pass string over the 8 rows above, rule)
F64_CMP_TABLE = [
    (0.0, "==", "..TT....", "-0.0 == 0.0; NaN equals only NaN; NULL never passes"),
    (0.0, "<",  "TT......", "-0.0 is not below 0.0; NaN is above everything"),
    (0.0, "<=", "TTTT....", "both zeros tie with the literal"),
    (0.0, ">",  "....TTT.", "NaN is greater than every non-NaN value"),
    (0.0, ">=", "..TTTTT.", "zeros tie; NaN is greatest"),
    (0.0, "!=", "TT..TTT.", "NaN != 0.0 is true; NULL != x is NULL, dropped"),
    (INF, "==", ".....T..", "inf equals inf only"),
    (INF, "<",  "TTTTT...", "NaN is not below +inf"),
    (INF, "<=", "TTTTTT..", "NaN is not <= +inf"),
    (INF, ">",  "......T.", "only NaN is greater than +inf"),
    (INF, ">=", ".....TT.", "inf ties, NaN is greater"),
    (INF, "!=", "TTTTT.T.", "NaN differs from inf"),
    (NAN, "==", "......T.", "NaN = NaN is true in Spark"),
    (NAN, "<",  "TTTTTT..", "every non-NaN value is below NaN"),
    (NAN, "<=", "TTTTTTT.", "NaN ties with NaN"),
    (NAN, ">",  "........", "nothing is greater than NaN"),
    (NAN, ">=", "......T.", "only NaN ties with NaN"),
    (NAN, "!=", "TTTTTT..", "NaN != NaN is false"),
]


@pytest.mark.parametrize("lit,op,expect,rule", F64_CMP_TABLE,
                         ids=[f"{l}{o}" for l, o, _, _ in F64_CMP_TABLE])
def test_f64_compare_table(lit, op, expect, rule):
    got = R.ref_compare(F64_VALS, F64_VALID, op, lit, "f64")
    assert "".join("T" if g else "." for g in got) == expect, rule
    idx = R.ref_filter(F64_VALS, F64_VALID, op, lit, "f64")
    assert idx.dtype == np.uint32
    assert idx.tolist() == [i for i, c in enumerate(expect) if c == "T"]


def test_f64_table_covers_all_ops_and_literals():
    seen = {(repr(l), o) for l, o, _, _ in F64_CMP_TABLE}
    assert len(seen) == 18
    assert {o for _, o in seen} == set(R.CMP_OPS)


def test_f64_negative_zero_literal():
    # -0.0 as the literal behaves exactly like 0.0
    for op in R.CMP_OPS:
        a = R.ref_compare(F64_VALS, F64_VALID, op, -0.0, "f64")
        b = R.ref_compare(F64_VALS, F64_VALID, op, 0.0, "f64")
        assert a.tolist() == b.tolist()


def test_no_validity_means_all_valid():
    got = R.ref_compare([1.0, NAN], None, "!=", 1.0, "f64")
    assert got.tolist() == [False, True]


#            MIN  -7  -1   0   1   7  MAX  NULL
I64_VALS = [MIN, -7, -1, 0, 1, 7, MAX, 0]
I64_VALID = [True] * 7 + [False]

I64_CMP_TABLE = [
    # exact integer literal
    (0, "==",   "...T....", "NULL row holds 0 but never passes"),
    (0, "!=",   "TTT.TTT.", "NULL != 0 is NULL, dropped"),
    (MIN, "<",  "........", "nothing is below INT64_MIN"),
    (MIN, ">=", "TTTTTTT.", "every valid row is >= INT64_MIN"),
    (MAX, ">",  "........", "nothing is above INT64_MAX"),
    (MAX, "<=", "TTTTTTT.", "every valid row is <= INT64_MAX"),
    (MAX, "==", "......T.", "exact at the extreme"),
    # float literal: the column is cast to double
    (0.5, "<",  "TTTT....", "k < 0.5 keeps k == 0 (no truncation of 0.5 to 0)"),
    (0.5, "<=", "TTTT....", "same set as <"),
    (0.5, ">",  "....TTT.", "k > 0.5 starts at 1"),
    (0.5, ">=", "....TTT.", "same set as >"),
    (0.5, "==", "........", "no integer equals 0.5"),
    (0.5, "!=", "TTTTTTT.", "every valid integer differs from 0.5"),
    (-0.5, "<", "TTT.....", "floor toward -inf: k < -0.5 is k <= -1"),
    (1e30, "<", "TTTTTTT.", "literal above the int64 range"),
    (-1e30, "<", "........", "literal below the int64 range"),
    (INF, "<",  "TTTTTTT.", "everything is below +inf"),
    (INF, "<=", "TTTTTTT.", "everything is below +inf"),
    (INF, "!=", "TTTTTTT.", "no integer equals +inf"),
    (INF, "==", "........", "no integer equals +inf"),
    (INF, ">",  "........", "nothing is above +inf"),
    (INF, ">=", "........", "nothing reaches +inf"),
    (-INF, ">",  "TTTTTTT.", "everything is above -inf"),
    (-INF, ">=", "TTTTTTT.", "everything is above -inf"),
    (-INF, "!=", "TTTTTTT.", "no integer equals -inf"),
    (-INF, "==", "........", "no integer equals -inf"),
    (-INF, "<",  "........", "nothing is below -inf"),
    (-INF, "<=", "........", "nothing is below -inf"),
    # NaN literal: NaN is greater than every double a bigint casts to
    (NAN, "<",  "TTTTTTT.", "every valid row is below NaN"),
    (NAN, "<=", "TTTTTTT.", "every valid row is below NaN"),
    (NAN, "!=", "TTTTTTT.", "no integer equals NaN"),
    (NAN, "==", "........", "no integer equals NaN"),
    (NAN, ">",  "........", "nothing is above NaN"),
    (NAN, ">=", "........", "nothing reaches NaN"),
]


@pytest.mark.parametrize("lit,op,expect,rule", I64_CMP_TABLE,
                         ids=[f"{l}{o}" for l, o, _, _ in I64_CMP_TABLE])
def test_i64_compare_table(lit, op, expect, rule):
    got = R.ref_compare(np.array(I64_VALS, dtype=np.int64), I64_VALID, op,
                        lit, "i64")
    assert "".join("T" if g else "." for g in got) == expect, rule


# ------------------------------------------------------------- arithmetic
I64_A = [MIN, -7, -1, 0, 1, 7, MAX]
I64_B = [-1, 0, 2, MAX]
NULL = None   # expected NULL output row

# rows follow I64_A, columns follow I64_B
I64_BINOP_TABLE = {
    # two's-complement wraparound (Add.scala, non-ANSI: Math.addExact is off)
    "+": [
        [MAX,     MIN,     MIN + 2, -1],        # MIN-1 wraps to MAX
        [-8,      -7,      -5,      MAX - 7],
        [-2,      -1,      1,       MAX - 1],
        [-1,      0,       2,       MAX],
        [0,       1,       3,       MIN],       # MAX+1 wraps to MIN
        [6,       7,       9,       MIN + 6],
        [MAX - 1, MAX,     MIN + 1, -2],        # MAX+MAX = 2^64-2 -> -2
    ],
    # a - b, wrapping
    "-": [
        [MIN + 1, MIN,     MAX - 1, 1],         # MIN-2 wraps; MIN-MAX -> 1
        [-6,      -7,      -9,      MAX - 5],
        [0,       -1,      -3,      MIN],       # -1-MAX = MIN exactly
        [1,       0,       -2,      MIN + 1],
        [2,       1,       -1,      MIN + 2],
        [8,       7,       5,       MIN + 8],
        [MIN,     MAX,     MAX - 2, 0],         # MAX+1 wraps to MIN
    ],
    # rsub is b - a (literal - column), wrapping
    "rsub": [
        [MAX,     MIN,     MIN + 2, -1],        # 0-MIN = 2^63 wraps to MIN
        [6,       7,       9,       MIN + 6],
        [0,       1,       3,       MIN],
        [-1,      0,       2,       MAX],
        [-2,      -1,      1,       MAX - 1],
        [-8,      -7,      -5,      MAX - 7],
        [MIN,     MIN + 1, MIN + 3, 0],
    ],
    # low 64 bits of the product
    "*": [
        [MIN,     0,       0,       MIN],       # MIN*-1 = 2^63 -> MIN; MIN*2 -> 0
        [7,       0,       -14,     MIN + 7],
        [1,       0,       -2,      MIN + 1],
        [0,       0,       0,       0],
        [-1,      0,       2,       MAX],
        [-7,      0,       14,      MAX - 6],
        [MIN + 1, 0,       -2,      1],         # MAX*MAX = 2^126-2^64+1 -> 1
    ],
    # Java long division: truncates toward zero; x / 0 is NULL (non-ANSI
    # Divide/IntegralDivide); MIN / -1 overflows back to MIN
    "/": [
        [MIN,     NULL,    -(1 << 62),    -1],
        [7,       NULL,    -3,            0],   # -7/2 = -3, not floor's -4
        [1,       NULL,    0,             0],   # -1/2 = 0, not floor's -1
        [0,       NULL,    0,             0],
        [-1,      NULL,    0,             0],
        [-7,      NULL,    3,             0],
        [MIN + 1, NULL,    (1 << 62) - 1, 1],
    ],
}


@pytest.mark.parametrize("op", list(I64_BINOP_TABLE))
@pytest.mark.parametrize("form", ["literal", "column"])
def test_i64_binop_table(op, form):
    assert set(I64_BINOP_TABLE) == set(R.BIN_OPS)
    table = I64_BINOP_TABLE[op]
    a = np.array(I64_A, dtype=np.int64)
    for j, b in enumerate(I64_B):
        rhs = b if form == "literal" else np.full(len(a), b, dtype=np.int64)
        vals, valid = R.ref_binop(a, None, op, rhs, None, "i64")
        assert vals.dtype == np.int64 and valid.dtype == bool
        for i in range(len(a)):
            exp = table[i][j]
            assert bool(valid[i]) == (exp is not NULL), (op, I64_A[i], b)
            if exp is not NULL:
                assert int(vals[i]) == exp, (op, I64_A[i], b)


def test_binop_null_propagation():
    a = np.array([10, 10, 10, 10], dtype=np.int64)
    b = np.array([2, 2, 0, 0], dtype=np.int64)
    av = [True, False, True, False]
    bv = [True, True, True, False]
    for op in R.BIN_OPS:
        vals, valid = R.ref_binop(a, av, op, b, bv, "i64")
        # valid iff both inputs valid and not a division by zero
        assert valid.tolist() == [True, False, op != "/", False]
    # NULLs on the b side only
    _, valid = R.ref_binop(a, None, "+", b, [False, True, True, False], "i64")
    assert valid.tolist() == [False, True, True, False]
    # a zero divisor hidden under a NULL row is simply NULL
    _, valid = R.ref_binop(a, None, "/", b, [True, True, False, True], "i64")
    assert valid.tolist() == [True, True, False, False]


def _bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


# (a, op, b, expected value or NULL, rule)
F64_BINOP_TABLE = [
    (1.0, "/", 0.0, NULL, "x / 0.0 is NULL, not inf"),
    (1.0, "/", -0.0, NULL, "-0.0 counts as a zero divisor"),
    (0.0, "/", 0.0, NULL, "0/0 is NULL, not NaN"),
    (NAN, "/", 0.0, NULL, "the divisor decides"),
    (1.0, "/", NAN, NAN, "NaN divisor is not zero: IEEE result"),
    (1.0, "/", INF, 0.0, "IEEE"),
    (-1.0, "/", INF, -0.0, "sign of zero is kept"),
    (7.0, "/", 2.0, 3.5, "no truncation for doubles"),
    (INF, "-", INF, NAN, "inf - inf is NaN and stays valid"),
    (INF, "*", 0.0, NAN, "inf * 0 is NaN and stays valid"),
    (1e308, "*", 10.0, INF, "overflow to inf, valid"),
    (5e-324, "*", 0.5, 0.0, "subnormal underflow, ties to even"),
    (5e-324, "+", 5e-324, 1e-323, "subnormal add is exact"),
    (-0.0, "+", 0.0, 0.0, "-0.0 + 0.0 = +0.0"),
    (-0.0, "+", -0.0, -0.0, "-0.0 + -0.0 = -0.0"),
    (1.5, "rsub", 4.0, 2.5, "rsub is b - a"),
    (1.5, "-", 4.0, -2.5, "a - b"),
    (0.1, "+", 0.2, 0.30000000000000004, "one rounding of the single op"),
]


@pytest.mark.parametrize("a,op,b,exp,rule", F64_BINOP_TABLE,
                         ids=[f"{a}{o}{b}" for a, o, b, _, _ in F64_BINOP_TABLE])
def test_f64_binop_table(a, op, b, exp, rule):
    for rhs in (b, np.array([b])):
        vals, valid = R.ref_binop(np.array([a]), None, op, rhs, None, "f64")
        assert vals.dtype == np.float64
        assert bool(valid[0]) == (exp is not NULL), rule
        if exp is NULL:
            continue
        if math.isnan(exp):
            assert math.isnan(vals[0]), rule
        else:
            assert _bits(float(vals[0])) == _bits(exp), rule


def test_div_trunc_differs_from_floor():
    assert R.binop_i64(-7, "/", 2) == -3 and -7 // 2 == -4
    assert R.binop_i64(7, "/", -2) == -3
    assert R.binop_i64(-7, "/", -2) == 3


def test_wrap_i64():
    assert R.wrap_i64(1 << 63) == MIN
    assert R.wrap_i64(-(1 << 63) - 1) == MAX
    assert R.wrap_i64((1 << 64) + 5) == 5
    assert R.wrap_i64(-1) == -1


# ------------------------------------------------------------ cast / range
def test_cast_round_to_nearest_even():
    cases = [
        (0, 0.0),
        (-1, -1.0),
        ((1 << 53) + 1, float(1 << 53)),        # tie -> even mantissa (down)
        (-((1 << 53) + 1), -float(1 << 53)),
        ((1 << 53) + 3, float((1 << 53) + 4)),  # tie -> even mantissa (up)
        (MAX, 9223372036854775808.0),           # 2^63-1 rounds up to 2^63
        (MIN, -9223372036854775808.0),          # exact
        ((1 << 63) - 513, 9223372036854774784.0),   # below the midpoint: 2^63-1024
        ((1 << 63) - 512, 9223372036854775808.0),   # the tie goes to even: 2^63
    ]
    got = R.ref_cast_i64_f64(np.array([c for c, _ in cases], dtype=np.int64))
    assert got.dtype == np.float64
    for g, (_, e) in zip(got, cases):
        assert _bits(float(g)) == _bits(e)


def test_range():
    assert R.ref_range_i64(0, 5, 3).tolist() == []
    assert R.ref_range_i64(4, 5, 3).tolist() == [5, 8, 11, 14]
    assert R.ref_range_i64(4, 5, -3).tolist() == [5, 2, -1, -4]
    # start + i*step wraps past INT64_MAX like Java long arithmetic
    assert R.ref_range_i64(3, MAX - 1, 1).tolist() == [MAX - 1, MAX, MIN]
    assert R.ref_range_i64(3, 1, MAX).tolist() == [1, MIN, -1]
    assert R.ref_range_i64(2, 0, 0).tolist() == [0, 0]
