"""Pins tests/agg_ref.py, the reference the GPU aggregate tests compare with,
to hand-written tables. No GPU, no kernels."""
import math
import struct

import numpy as np
import pytest

import agg_ref

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
NAN = float("nan")
INF = math.inf


def f64_from_bits(bits):
    return struct.unpack("<d", struct.pack("<Q", bits))[0]


NEG_NAN = f64_from_bits(0xFFF8000000000000)
PAYLOAD_NAN = f64_from_bits(0x7FF8000000ABCDEF)
SIGNALLING_NAN = f64_from_bits(0x7FF0000000000123)


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def i64a(xs):
    return np.array(xs, dtype=np.int64)


def f64a(xs):
    return np.array([bits(x) for x in xs], dtype=np.uint64).view(np.float64)


def one_group(kind, values, valid=None):
    """the spec's result over a single group."""
    keys = i64a([7] * len(values))
    out = agg_ref.aggregate([keys], None, [(kind, values, valid)])
    assert list(out) == [(7,)]
    return out[(7,)][0]


# ---------- counts ----------

def test_counts_are_python_ints_and_never_null():
    keys = i64a([1, 1, 2, 2, 2, 3])
    v = i64a([5, 6, 7, 8, 9, 10])
    valid = np.array([True, False, False, False, False, True])
    out = agg_ref.aggregate([keys], None, [("count*",), ("count", v, valid)])
    assert out == {(1,): [2, 1], (2,): [3, 0], (3,): [1, 1]}
    assert all(type(x) is int for r in out.values() for x in r)


# ---------- int64 ----------

def test_sum_i64_wraps_to_twos_complement():
    assert one_group("sum", i64a([I64_MAX, 1])) == I64_MIN
    assert one_group("sum", i64a([I64_MIN, -1])) == I64_MAX
    assert one_group("sum", i64a([I64_MIN, I64_MIN])) == 0
    assert one_group("sum", i64a([I64_MAX, I64_MAX, 2])) == 0
    assert one_group("sum", i64a([3, -5])) == -2


def test_min_max_i64_extremes():
    assert one_group("min", i64a([I64_MAX])) == I64_MAX
    assert one_group("max", i64a([I64_MIN])) == I64_MIN
    v = i64a([I64_MAX, 0, I64_MIN, -1])
    assert one_group("min", v) == I64_MIN
    assert one_group("max", v) == I64_MAX
    valid = np.array([True, True, False, True])
    assert one_group("min", v, valid) == -1
    assert type(one_group("min", v)) is int


# ---------- float64 SUM ----------

def test_sum_f64_non_finite():
    assert one_group("sum", f64a([1.0, INF, 2.0])) == INF
    assert one_group("sum", f64a([1.0, -INF, -INF])) == -INF
    assert math.isnan(one_group("sum", f64a([INF, 1.0, -INF])))
    assert math.isnan(one_group("sum", f64a([1.0, NAN, 2.0])))
    assert math.isnan(one_group("sum", f64a([INF, NEG_NAN])))
    assert math.isnan(one_group("sum", f64a([SIGNALLING_NAN])))


def test_sum_f64_zero_signs_and_cancellation():
    s = one_group("sum", f64a([-0.0, -0.0]))
    assert s == 0.0 and not math.copysign(1.0, s) < 0     # starts from +0.0
    s = one_group("sum", f64a([1.5, -1.5]))
    assert s == 0.0 and not math.copysign(1.0, s) < 0
    # correctly rounded where a running sum is not
    assert one_group("sum", f64a([1e16, 1.0, -1e16])) == 1.0
    assert one_group("sum", f64a([0.1] * 10)) == 1.0
    assert sum([0.1] * 10) != 1.0


def test_sum_error_bound():
    vals = [1e16, 1.0, -1e16] * 4
    assert agg_ref.sum_error_bound(vals) == 11 * 2.0 ** -53 * (8e16 + 4.0)
    assert agg_ref.sum_error_bound([3.0]) == 0.0
    # every order of a small cancelling set stays inside it
    rng = np.random.default_rng(5)
    exact = math.fsum(vals)
    for _ in range(50):
        s = 0.0
        for i in rng.permutation(len(vals)):
            s += vals[i]
        assert abs(s - exact) <= agg_ref.sum_error_bound(vals)


# ---------- float64 MIN / MAX ----------

def test_min_max_f64_nan_is_greatest_and_canonical():
    v = f64a([1.0, NEG_NAN, INF, -INF])
    assert one_group("min", v) == -INF
    m = one_group("max", v)
    assert math.isnan(m) and bits(m) == 0x7FF8000000000000
    for nan in (NEG_NAN, PAYLOAD_NAN, SIGNALLING_NAN):
        for kind in ("min", "max"):
            r = one_group(kind, f64a([nan, nan]))
            assert bits(r) == 0x7FF8000000000000, (kind, hex(bits(nan)))
    # NaN loses MIN against anything else, +inf included
    assert one_group("min", f64a([PAYLOAD_NAN, INF])) == INF
    assert one_group("max", f64a([1.0, INF])) == INF


def test_min_max_f64_zeros_compare_equal_and_emit_plus_zero():
    """the deviation from Spark: min([-0.0]) is +0.0 here, -0.0 there."""
    for kind in ("min", "max"):
        for vals in ([-0.0], [-0.0, 0.0], [0.0, -0.0], [0.0]):
            r = one_group(kind, f64a(vals))
            assert bits(r) == 0, (kind, vals)
    assert bits(one_group("min", f64a([-0.0, 3.0]))) == 0
    assert bits(one_group("max", f64a([-0.0, -3.0]))) == 0
    assert one_group("min", f64a([-0.0, -3.0])) == -3.0


# ---------- NULLs and keys ----------

def test_all_null_group_is_none_with_count_zero():
    keys = i64a([1, 1, 2])
    vi, vf = i64a([4, 5, 6]), f64a([4.0, 5.0, 6.0])
    valid = np.array([False, False, True])
    specs = [("sum", vi, valid), ("min", vi, valid), ("max", vi, valid),
             ("sum", vf, valid), ("min", vf, valid), ("max", vf, valid),
             ("count", vi, valid), ("count*",)]
    out = agg_ref.aggregate([keys], None, specs)
    assert out[(1,)] == [None] * 6 + [0, 2]
    assert out[(2,)] == [6, 6, 6, 6.0, 6.0, 6.0, 1, 1]


def test_null_keys_group_together_and_apart_from_values():
    k1 = i64a([0, 0, -1, -1, I64_MIN, 0])
    v1 = np.array([True, False, True, False, True, False])
    out = agg_ref.aggregate([k1], [v1], [("count*",)])
    assert out == {(0,): [1], (None,): [3], (-1,): [1], (I64_MIN,): [1]}
    # composite: NULL in one column only, in both, and a stored value under
    # a NULL bit that must not matter
    k2 = i64a([9, 9, 9, 8, 9, 7])
    v2 = np.array([True, True, True, False, True, False])
    out = agg_ref.aggregate([k1, k2], [v1, v2], [("count*",)])
    assert out == {(0, 9): [1], (None, 9): [1], (-1, 9): [1],
                   (None, None): [2], (I64_MIN, 9): [1]}
    assert agg_ref.aggregate([k1, k2], None, [("count*",)])[(0, 9)] == [2]


def test_bad_kind_is_rejected():
    with pytest.raises(ValueError):
        agg_ref.aggregate([i64a([1])], None, [("avg", i64a([1]))])


# ---------- merge property ----------

SPECIALS = [NAN, NEG_NAN, PAYLOAD_NAN, INF, -INF, -0.0, 0.0]


def random_table(seed, n):
    rng = np.random.default_rng(seed)
    k1 = rng.integers(-1, 5, size=n, endpoint=True).astype(np.int64)
    k2 = rng.choice(i64a([I64_MIN, I64_MAX, 0]), size=n)
    kv1, kv2 = rng.random(n) >= 0.15, rng.random(n) >= 0.15
    vi = rng.integers(I64_MIN, I64_MAX, size=n, dtype=np.int64, endpoint=True)
    vs = rng.integers(-(1 << 20), 1 << 20, size=n, endpoint=True).astype(np.float64)
    vm = rng.standard_normal(n)
    pick = rng.random(n) < 0.3
    vm[pick] = f64a(SPECIALS)[rng.integers(0, len(SPECIALS), size=int(pick.sum()))]
    valid = [rng.random(n) >= 0.4 for _ in range(3)]
    valid[0][kv1 & (k1 == 2)] = False          # all-NULL groups
    return [k1, k2], [kv1, kv2], vi, vs, vm, valid


def canon(res):
    """results with NaN made comparable and the zero's sign visible."""
    def c(x):
        if isinstance(x, float):
            return "nan" if math.isnan(x) else (x, math.copysign(1.0, x))
        return x
    return {kt: [c(x) for x in r] for kt, r in res.items()}


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("nkeys", [1, 2])
def test_concatenation_equals_merge_of_halves(seed, nkeys):
    n = 600
    keys, kvs, vi, vs, vm, valid = random_table(seed, n)
    keys, kvs = keys[:nkeys], kvs[:nkeys]

    def run(lo, hi):
        specs = [("sum", vi[lo:hi], valid[0][lo:hi]),
                 ("min", vi[lo:hi], valid[0][lo:hi]),
                 ("max", vi[lo:hi], valid[0][lo:hi]),
                 ("count", vi[lo:hi], valid[0][lo:hi]),
                 ("sum", vs[lo:hi], valid[1][lo:hi]),    # integer-valued: exact
                 ("min", vm[lo:hi], valid[2][lo:hi]),
                 ("max", vm[lo:hi], valid[2][lo:hi]),
                 ("sum", np.where(np.isfinite(vm[lo:hi]), 1.0, vm[lo:hi]),
                  valid[2][lo:hi]),                      # ones, +-inf and NaNs
                 ("count*",)]
        return agg_ref.aggregate([k[lo:hi] for k in keys],
                                 [v[lo:hi] for v in kvs], specs)

    kinds = ["sum", "min", "max", "count", "sum", "min", "max", "sum", "count*"]
    cut = 251
    whole = run(0, n)
    merged = agg_ref.merge(kinds, run(0, cut), run(cut, n))
    assert canon(merged) == canon(whole)
    assert any(r[0] is None and r[3] == 0 for r in whole.values())
    assert any(isinstance(r[7], float) and math.isnan(r[7]) for r in whole.values())


# ---------- the vectorised form ----------

@pytest.mark.parametrize("seed", [1, 2])
def test_np_aggregate_matches_row_by_row(seed):
    n = 3000
    keys, kvs, vi, vs, _, valid = random_table(seed, n)
    vi[:50] = I64_MAX
    vi[50:100] = I64_MIN
    specs = [("sum", vs, valid[1]), ("count", vs, valid[1]),
             ("sum", vi, valid[0]), ("min", vi, valid[0]), ("max", vi, valid[0]),
             ("count", vi, valid[0]), ("count*",), ("sum", vs)]
    want = agg_ref.aggregate([keys[0]], [kvs[0]], specs)
    assert canon(agg_ref.np_aggregate(keys[0], kvs[0], specs)) == canon(want)
    assert (None,) in want and (-1,) in want
    # no key bitmap, and no NULL-key group in the output then
    got = agg_ref.np_aggregate(keys[0], None, specs)
    assert canon(got) == canon(agg_ref.aggregate([keys[0]], None, specs))
    assert (None,) not in got
    with pytest.raises(ValueError):
        agg_ref.np_aggregate(keys[0], None, [("min", vs)])
