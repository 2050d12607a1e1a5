"""Pins tests/slide_ref.py (the reference the GPU sliding-frame tests compare
against) to hand-written tables, and its vectorised numpy twin to the
row-by-row form. No GPU."""
import math
import struct

import numpy as np
import pytest

import slide_ref as S
import window_ref as R

N = None                      # NULL
NAN, INF = float("nan"), float("inf")
ONE = [True, False, False, False]
V = [1, N, 3, 4]

# frame -> {op: expected} over one partition [1, NULL, 3, 4]
TABLE = {
    (-1, 1): {"sum": [1, 4, 7, 7], "count": [1, 2, 2, 2], "min": [1, 1, 3, 3],
              "max": [1, 3, 4, 4], "first_value": [1, 1, N, 3],
              "last_value": [N, 3, 4, 4]},
    (2, 3): {"sum": [7, 4, N, N], "count": [2, 1, 0, 0]},
    (-2, -1): {"sum": [N, 1, 1, 3], "first_value": [N, 1, 1, N],
               "last_value": [N, 1, N, 3]},
    (None, 1): {"sum": [1, 4, 8, 8], "last_value": [N, 3, 4, 4]},
    (None, -1): {"sum": [N, 1, 1, 4], "count": [0, 1, 1, 2]},
}
CASES = [(f, op) for f, ops in TABLE.items() for op in ops]


def bits(x):
    return struct.pack("<d", x)


def same(a, b):
    """lists equal, floats by bits (any NaN equals any NaN)."""
    if len(a) != len(b):
        return False
    for x, y in zip(a, b):
        if isinstance(x, float) and isinstance(y, float):
            if math.isnan(x) or math.isnan(y):
                if not (math.isnan(x) and math.isnan(y)):
                    return False
            elif bits(x) != bits(y):
                return False
        elif x != y or type(x) is not type(y):
            return False
    return True


def twin(op, lo, hi, part, vals, dtype):
    """np_slide's result as a list with None for NULL."""
    npdt = np.float64 if dtype == "f64" else np.int64
    if vals is None:
        out, ok = S.np_slide(op, lo, hi, np.array(part))
    else:
        v, vok = R.from_list(vals, npdt)
        out, ok = S.np_slide(op, lo, hi, np.array(part), v, vok)
    return R.to_list(out, ok)


@pytest.mark.parametrize("frame,op", CASES)
def test_one_partition(frame, op):
    want = TABLE[frame][op]
    assert S.slide(op, *frame, ONE, V) == want
    assert twin(op, *frame, ONE, V, "i64") == want
    # the same column as float64
    fv = [None if v is None else float(v) for v in V]
    fwant = [float(w) if (w is not None and op != "count") else w for w in want]
    assert same(S.slide(op, *frame, ONE, fv, "f64"), fwant)
    assert same(twin(op, *frame, ONE, fv, "f64"), fwant)


@pytest.mark.parametrize("frame,op", CASES)
def test_two_partitions_clip(frame, op):
    """the table's partition twice: no frame reaches across the boundary."""
    want = TABLE[frame][op] * 2
    assert S.slide(op, *frame, ONE * 2, V * 2) == want
    assert twin(op, *frame, ONE * 2, V * 2, "i64") == want


def test_split_partition_by_hand():
    # [1, NULL | 3, 4]: (-1, 1) inside two partitions of two rows
    part = [True, False, True, False]
    assert S.slide("sum", -1, 1, part, V) == [1, 1, 7, 7]
    assert S.slide("count", -1, 1, part, V) == [1, 1, 2, 2]
    assert S.slide("first_value", -1, 1, part, V) == [1, 1, 3, 3]
    assert S.slide("last_value", -1, 1, part, V) == [N, N, 4, 4]
    assert S.slide("sum", 1, 1, part, V) == [N, N, 4, N]
    assert S.slide("count", 1, 1, part, V) == [0, 0, 1, 0]
    assert S.slide("sum", None, None, part, V) == [1, 1, 7, 7]
    assert S.slide("max", None, -1, part, V) == [N, 1, N, 3]
    for op, lo, hi in (("sum", -1, 1), ("count", -1, 1), ("first_value", -1, 1),
                       ("last_value", -1, 1), ("sum", 1, 1), ("count", 1, 1),
                       ("sum", None, None), ("max", None, -1)):
        assert twin(op, lo, hi, part, V, "i64") == S.slide(op, lo, hi, part, V)


def test_count_star():
    assert S.slide("count", -1, 1, ONE) == [2, 3, 3, 2]
    assert S.slide("count", 2, 3, ONE) == [2, 1, 0, 0]
    assert S.slide("count", None, -2, ONE) == [0, 0, 1, 2]
    assert twin("count", -1, 1, ONE, None, "i64") == [2, 3, 3, 2]
    assert twin("count", None, -2, ONE, None, "i64") == [0, 0, 1, 2]


@pytest.mark.parametrize("vals,frame,want", [
    ([INF, -INF, 1.0], (-1, 0), [INF, NAN, -INF]),
    ([1e308, 1e308, -1e308], (-2, 0), [1e308, INF, INF]),
    ([-0.0], (0, 0), [0.0]),
])
def test_float_sum_is_re_added_per_row(vals, frame, want):
    """no prefix differences: inf - inf never arises from a frame that does
    not hold both, an overflow stays in the frames that hold it, and the sum
    of a lone -0.0 is +0.0."""
    part = [True] + [False] * (len(vals) - 1)
    assert same(S.slide("sum", *frame, part, vals, "f64"), want)
    assert same(twin("sum", *frame, part, vals, "f64"), want)


def test_float_sum_order_is_left_to_right():
    vals = [1.0, 1e100, -1e100, 1.0]
    part = [True, False, False, False]
    # ((1 + 1e100) - 1e100) + 1 = 1, not 2
    assert S.slide("sum", -3, 0, part, vals, "f64")[3] == 1.0
    assert twin("sum", -3, 0, part, vals, "f64")[3] == 1.0
    # a NaN reaches only the frames that hold it
    vals = [1.0, NAN, 2.0, 3.0]
    assert same(S.slide("sum", -1, 0, part, vals, "f64"), [1.0, NAN, NAN, 5.0])


def test_float_min_max_canonical():
    vals = [-0.0, 0.0, NAN, -INF, N]
    part = [True] + [False] * 4
    assert same(S.slide("min", 0, 0, part, vals, "f64"), [0.0, 0.0, NAN, -INF, N])
    assert same(S.slide("max", -1, 0, part, vals, "f64"), [0.0, 0.0, NAN, NAN, -INF])
    assert same(twin("max", -1, 0, part, vals, "f64"), [0.0, 0.0, NAN, NAN, -INF])
    # first / last copy the value as it is
    assert same(S.slide("first_value", 0, 0, part, vals, "f64"), vals)


def test_int_sum_wraps():
    big = (1 << 62) + 5
    part = [True, False, False]
    want = [big, R.wrap_i64(2 * big), R.wrap_i64(3 * big)]
    assert want[1] < 0
    assert S.slide("sum", -2, 0, part, [big] * 3) == want
    assert twin("sum", -2, 0, part, [big] * 3, "i64") == want


FRAMES = [(0, 0), (-1, 0), (0, 1), (-2, 2), (-3, -1), (2, 5), (-64, 63),
          (300, 302), (-301, -299), (None, -1), (None, 0), (None, 2), (None, None)]


@pytest.mark.parametrize("n", [1, 2, 7, 64, 65, 257])
def test_numpy_twin_matches_row_by_row(n):
    rng = np.random.RandomState(1000 + n)
    part = rng.rand(n) < 0.08
    part[0] = True
    ok = rng.rand(n) > 0.3
    special = np.array([NAN, INF, -INF, -0.0, 0.0, 1.5, -3.0, 7.0])
    cols = {"i64": rng.randint(-(1 << 62), 1 << 62, size=n).astype(np.int64),
            "f64": np.where(rng.rand(n) < 0.3, special[rng.randint(0, 8, size=n)],
                            rng.rand(n) * 1e3 - 500)}
    for lo, hi in FRAMES:
        for use_ok in (ok, None):
            for dt, v in cols.items():
                lst = R.to_list(v, use_ok)
                for op in S.OPS:
                    want = S.slide(op, lo, hi, part.tolist(), lst, dt)
                    out, rok = S.np_slide(op, lo, hi, part, v, use_ok)
                    assert same(R.to_list(out, rok), want), (op, lo, hi, dt)
        want = S.slide("count", lo, hi, part.tolist())
        assert S.np_slide("count", lo, hi, part)[0].tolist() == want
