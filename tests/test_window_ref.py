"""Pins tests/window_ref.py, the reference the GPU window tests compare
with, to hand-written known answers (CPU only), and checks its vectorised
numpy forms against the row-by-row ones.
"""
import math
import struct

import numpy as np
import pytest

import window_ref as R

NAN = float("nan")


def row(text, conv=int):
    """'· 3 4 · | 1 ·' -> [None, 3, 4, None, 1, None]"""
    return [None if t == "·" else conv(t)
            for t in text.replace("|", " ").split()]


P = row("1 1 1 1 | 2 2 | · ·")
O = row("10 20 20 30 | 5 5 | 7 8")
X = row("· 3 4 · | 1 · | · ·")
PART, PEER = R.boundaries([P, O], 1, 8)


def test_table_boundaries():
    assert PART == [bool(b) for b in row("1 0 0 0 | 1 0 | 1 0")]
    assert PEER == [bool(b) for b in row("1 1 0 1 | 1 0 | 1 1")]


@pytest.mark.parametrize("op,expected", [
    ("row_number", "1 2 3 4|1 2|1 2"),
    ("rank", "1 2 2 4|1 1|1 2"),
    ("dense_rank", "1 2 2 3|1 1|1 2"),
])
def test_table_rank_ops(op, expected):
    assert R.scan(op, "rows", PART, PEER) == row(expected)


@pytest.mark.parametrize("op,frame,star,expected", [
    ("sum", "rows", False, "· 3 7 7|1 1|· ·"),
    ("sum", "range", False, "· 7 7 7|1 1|· ·"),
    ("sum", "partition", False, "7 7 7 7|1 1|· ·"),
    ("count", "rows", False, "0 1 2 2|1 1|0 0"),
    ("count", "range", False, "0 2 2 2|1 1|0 0"),
    ("count", "range", True, "1 3 3 4|2 2|1 2"),
    ("min", "range", False, "· 3 3 3|1 1|· ·"),
    ("max", "rows", False, "· 3 4 4|1 1|· ·"),
])
def test_table_aggregates(op, frame, star, expected):
    got = R.scan(op, frame, PART, PEER, None if star else X, "i64")
    assert got == row(expected)


@pytest.mark.parametrize("offset,default,expected", [
    (-1, None, "· · 3 4|· 1|· ·"),
    (-1, -1, "-1 · 3 4|-1 1|-1 ·"),
    (1, None, "3 4 · ·|· ·|· ·"),
    (1, -1, "3 4 · -1|· -1|· -1"),
    (0, None, "· 3 4 · | 1 · | · ·"),
    (-2, 9, "9 9 · 3|9 9|9 9"),
    (5, None, "· · · ·|· ·|· ·"),
])
def test_table_shift(offset, default, expected):
    assert R.shift(X, offset, PART, default) == row(expected)


def test_avg_is_sum_over_count():
    xs = [None, 3.0, 4.0, None, 1.0, None, None, None]
    assert R.avg("rows", PART, PEER, xs) == \
        [None, 3.0, 3.5, 3.5, 1.0, 1.0, None, None]
    assert R.avg("partition", PART, PEER, xs) == \
        [3.5, 3.5, 3.5, 3.5, 1.0, 1.0, None, None]


def test_float_partition_keys_zero_and_nan_payloads():
    """-0.0 / 0.0 fall in one partition, and so do two NaNs with different
    payloads; NaN and a number do not."""
    nan2 = struct.unpack("<d", struct.pack("<Q", 0x7FF8000000000123))[0]
    assert math.isnan(nan2)
    k = [-0.0, 0.0, 1.0, NAN, nan2, None, None]
    part, peer = R.boundaries([k], 1, len(k))
    assert part == [True, False, True, True, False, True, False]
    assert peer == part
    assert R.scan("row_number", "rows", part, part) == [1, 2, 1, 1, 2, 1, 2]
    # the same keys as order keys: one partition, peer groups instead
    part, peer = R.boundaries([k], 0, len(k))
    assert part == [True] + [False] * 6
    assert R.scan("rank", "rows", part, peer) == [1, 1, 3, 4, 4, 6, 6]
    assert R.scan("dense_rank", "rows", part, peer) == [1, 1, 2, 3, 3, 4, 4]
    # numpy form: the same bitmaps
    v, ok = R.from_list(k, np.float64)
    v[4] = nan2
    npart, npeer = R.np_boundaries([(v, ok)], 0)
    assert npart.tolist() == part and npeer.tolist() == peer


def test_min_max_nan_greatest_and_zero_sign():
    part = [True] + [False] * 4
    xs = [1.0, NAN, -2.0, None, 5.0]
    mx = R.scan("max", "rows", part, part, xs, "f64")
    assert mx[0] == 1.0 and all(math.isnan(v) for v in mx[1:])
    assert R.scan("min", "rows", part, part, xs, "f64") == \
        [1.0, 1.0, -2.0, -2.0, -2.0]
    allnan = R.scan("min", "partition", part, part, [NAN, None, NAN, NAN, NAN], "f64")
    assert all(math.isnan(v) for v in allnan)
    z = R.scan("min", "rows", [True, False], [True, False], [-0.0, 0.0], "f64")
    assert [math.copysign(1.0, v) for v in z] == [1.0, 1.0]   # +0.0 emitted
    z = R.scan("max", "rows", [True, False], [True, False], [0.0, -0.0], "f64")
    assert [math.copysign(1.0, v) for v in z] == [1.0, 1.0]


def test_int64_sum_wraps():
    big = (1 << 63) - 1
    part = [True, False, False, True]
    got = R.scan("sum", "rows", part, part, [big, 1, 1, -5], "i64")
    assert got == [big, -(1 << 63), -(1 << 63) + 1, -5]
    v = np.array([big, 1, 1, -5], dtype=np.int64)
    out, _ = R.np_scan("sum", "rows", np.array(part), np.array(part), v)
    assert out.tolist() == got


def test_float_sum_of_zeros_is_positive_zero():
    got = R.scan("sum", "rows", [True, False], [True, False], [-0.0, -0.0], "f64")
    assert [math.copysign(1.0, v) for v in got] == [1.0, 1.0]


def test_bits_of_layout():
    flags = np.zeros(70, dtype=bool)
    flags[[0, 63, 64, 69]] = True
    w = R.bits_of(flags)
    assert w.dtype == np.uint64 and w.tolist() == [1 | (1 << 63), 1 | (1 << 5)]


# ---------------- vectorised forms == row by row ----------------

def _same(a, b):
    """equal lists: None only equals None, any NaN equals any NaN, and other
    floats compare by their bits (so +0.0 != -0.0)."""
    def key(x):
        if isinstance(x, float):
            return "nan" if math.isnan(x) else struct.pack("<d", x)
        return x
    return [key(x) for x in a] == [key(y) for y in b]


def _random_case(seed, n, null_density):
    rng = np.random.RandomState(seed)
    sizes = []
    while sum(sizes) < n:
        sizes.append(int(rng.choice([1, 2, 3, 17, 200])))
    p = np.repeat(np.arange(len(sizes)), sizes)[:n].astype(np.int64)
    p_ok = p % 7 != 3                       # one NULL partition-key group
    o = np.zeros(n, dtype=np.float64)
    for b in np.flatnonzero(np.r_[True, p[1:] != p[:-1]]):
        e = b + int((p[b:] == p[b]).sum())
        o[b:e] = np.sort(rng.randint(0, 6, size=e - b)).astype(np.float64)
    xi = rng.randint(-50, 50, size=n).astype(np.int64)
    xf = rng.choice([NAN, -0.0, 0.0, 1.5, -3.0, 7.0], size=n)
    ok = rng.rand(n) >= null_density
    return p, p_ok, o, xi, xf, ok


@pytest.mark.parametrize("null_density", [0.0, 0.3, 1.0])
def test_numpy_forms_equal_row_by_row(null_density):
    n = 3000
    p, p_ok, o, xi, xf, ok = _random_case(17, n, null_density)
    part, peer = R.boundaries([R.to_list(p, p_ok), R.to_list(o)], 1, n)
    npart, npeer = R.np_boundaries([(p, p_ok), (o, None)], 1)
    assert npart.tolist() == part and npeer.tolist() == peer
    for op in R.RANK_OPS:
        out, _ = R.np_scan(op, "rows", npart, npeer)
        assert out.tolist() == R.scan(op, "rows", part, peer)
    for frame in R.FRAMES:
        out, _ = R.np_scan("count", frame, npart, npeer)
        assert out.tolist() == R.scan("count", frame, part, peer)
        for vals, dt in ((xi, "i64"), (xf, "f64")):
            lst = R.to_list(vals, ok)
            for op in ("count", "sum", "min", "max"):
                out, rok = R.np_scan(op, frame, npart, npeer, vals, ok)
                got = R.to_list(out, rok if op != "count" else None)
                assert _same(got, R.scan(op, frame, part, peer, lst, dt)), \
                    (op, frame, dt)
    for offset in (-2, -1, 0, 1, 2, 250):
        for default in (None, 7):
            out, ook = R.np_shift(xi, ok, offset, npart, default)
            assert R.to_list(out, ook) == \
                R.shift(R.to_list(xi, ok), offset, part, default)
