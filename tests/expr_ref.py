"""Plain row-by-row reference for the filter / project operators.

Everything here is written with Python ints and floats, one row at a time,
so that each rule can be read off the code. It imports nothing from the
engine under test. tests/test_expr_ref.py pins it to a hand-written
known-answer table on a machine without a GPU; the GPU parity tests and
tools/fuzz_parity.py then compare the HIP kernels against it bit for bit.

Semantics (Spark, non-ANSI):
  comparison  - a NULL row never passes, `!=` included (WHERE keeps TRUE only)
              - float64 uses SQLOrderingUtil.compareDoubles: -0.0 == 0.0,
                NaN == NaN, NaN greater than every other value (+inf too)
              - int64 column vs float literal: the column is cast to double
                and compared as doubles; vs int literal: exact
  arithmetic  - output row valid iff both inputs valid and not (`/` by zero;
                for float64 -0.0 is zero too)
              - int64 `+ - *` wrap modulo 2^64; `/` truncates toward zero and
                INT64_MIN / -1 == INT64_MIN (Java long division)
              - float64: the IEEE result of the single operation
              - `rsub` is b - a
dtype is "i64" or "f64". `valid` arguments are None (no NULLs) or one bool
per row.
"""
import math

import numpy as np

I64_MIN = -(1 << 63)
I64_MAX = (1 << 63) - 1

CMP_OPS = ("==", "<", "<=", ">", ">=", "!=")
BIN_OPS = ("+", "-", "*", "/", "rsub")


def wrap_i64(x: int) -> int:
    """Python int -> two's-complement int64 (modulo 2^64)."""
    x &= (1 << 64) - 1
    return x - (1 << 64) if x >= (1 << 63) else x


def cmp3_f64(x: float, y: float) -> int:
    """SQLOrderingUtil.compareDoubles: -1 / 0 / +1."""
    xn, yn = math.isnan(x), math.isnan(y)
    if xn or yn:
        if xn and yn:
            return 0            # NaN == NaN
        return 1 if xn else -1  # NaN is the greatest value
    if x == y:                  # -0.0 == 0.0 under IEEE ==
        return 0
    return -1 if x < y else 1


def cmp3_i64(x: int, y: int) -> int:
    return 0 if x == y else (-1 if x < y else 1)


_DECIDE = {
    "==": lambda c: c == 0,
    "<": lambda c: c < 0,
    "<=": lambda c: c <= 0,
    ">": lambda c: c > 0,
    ">=": lambda c: c >= 0,
    "!=": lambda c: c != 0,
}


def _rows(vals):
    return vals.tolist() if isinstance(vals, np.ndarray) else list(vals)


def _valid_rows(valid, n):
    if valid is None:
        return [True] * n
    v = _rows(valid)
    assert len(v) == n
    return [bool(x) for x in v]


def ref_compare(vals, valid, op, literal, dtype):
    """-> bool mask (numpy): row passes `col OP literal`."""
    decide = _DECIDE[op]
    rows = _rows(vals)
    ok = _valid_rows(valid, len(rows))
    out = []
    if dtype == "f64":
        lit = float(literal)
        for x, v in zip(rows, ok):
            out.append(v and decide(cmp3_f64(float(x), lit)))
    elif dtype == "i64":
        if isinstance(literal, float):
            # Spark casts the bigint column to double for the comparison
            for x, v in zip(rows, ok):
                out.append(v and decide(cmp3_f64(float(int(x)), literal)))
        else:
            lit = int(literal)
            for x, v in zip(rows, ok):
                out.append(v and decide(cmp3_i64(int(x), lit)))
    else:
        raise ValueError(dtype)
    return np.array(out, dtype=bool)


def ref_filter(vals, valid, op, literal, dtype):
    """-> passing row indices, in input order (uint32)."""
    mask = ref_compare(vals, valid, op, literal, dtype)
    return np.array([i for i, m in enumerate(mask.tolist()) if m],
                    dtype=np.uint32)


def _div_trunc(x: int, y: int) -> int:
    q = abs(x) // abs(y)
    return q if (x < 0) == (y < 0) else -q


def binop_i64(x: int, op: str, y: int) -> int:
    """one int64 operation (divisor non-zero), wrapped to int64."""
    if op == "+":
        r = x + y
    elif op == "-":
        r = x - y
    elif op == "rsub":
        r = y - x
    elif op == "*":
        r = x * y
    elif op == "/":
        r = _div_trunc(x, y)    # INT64_MIN / -1 = 2^63, wraps to INT64_MIN
    else:
        raise ValueError(op)
    return wrap_i64(r)


def binop_f64(x: float, op: str, y: float) -> float:
    """one IEEE double operation (divisor non-zero)."""
    if op == "+":
        return x + y
    if op == "-":
        return x - y
    if op == "rsub":
        return y - x
    if op == "*":
        return x * y
    if op == "/":
        return x / y
    raise ValueError(op)


def ref_binop(a, a_valid, op, b_or_literal, b_valid, dtype):
    """-> (values, valid). b_or_literal: a column (array/list) or a scalar
    literal (then b_valid must be None). Values of NULL output rows are 0;
    callers compare values only where `valid` is set."""
    ar = _rows(a)
    n = len(ar)
    if isinstance(b_or_literal, (np.ndarray, list, tuple)):
        br = _rows(b_or_literal)
        assert len(br) == n
    else:
        assert b_valid is None
        br = [b_or_literal] * n
    av = _valid_rows(a_valid, n)
    bv = _valid_rows(b_valid, n)
    vals, valid = [], []
    for x, y, vx, vy in zip(ar, br, av, bv):
        if dtype == "i64":
            x, y = int(x), int(y)
        else:
            x, y = float(x), float(y)
        ok = vx and vy and not (op == "/" and y == 0)   # -0.0 == 0 is True
        valid.append(ok)
        if not ok:
            vals.append(0)
        elif dtype == "i64":
            vals.append(binop_i64(x, op, y))
        else:
            vals.append(binop_f64(x, op, y))
    np_dt = np.int64 if dtype == "i64" else np.float64
    return np.array(vals, dtype=np_dt), np.array(valid, dtype=bool)


def ref_cast_i64_f64(vals):
    """int64 -> float64, round-to-nearest-even (Python's int -> float
    conversion is correctly rounded)."""
    return np.array([float(int(x)) for x in _rows(vals)], dtype=np.float64)


def ref_range_i64(n, start, step):
    """out[i] = start + i*step, wrapped to int64."""
    return np.array([wrap_i64(start + i * step) for i in range(n)],
                    dtype=np.int64)
