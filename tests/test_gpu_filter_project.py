"""GPU parity for the filter / project family against tests/expr_ref.py:
gpuq_filter_cmp, gpuq_project_binop(_nullable), gpuq_cast_i64_f64,
gpuq_range_i64, gpuq_gather as the filter uses it, and GpuFilterExec /
GpuProjectExec on top. The reference is pinned on the CPU by
tests/test_expr_ref.py.

Every comparison is exact: permutation as uint32, count, int64 values,
float64 bit patterns (two NaNs match whatever their payload), validity after
unpacking to n bits, data only where the reference row is valid.

SIZES are the smallest shapes that cross each boundary: bitmap bytes (7/8/9),
one 256-thread block (255/256/257), the 5632-row compaction tile
(5631/5632/5633, two tiles + 1 = 11265) and the 2048x256-thread grid cap
(BIG = 524288 + 257, the only size that enters the grid-stride loops: every
elementwise kernel here, the NULL-aware projection included, runs one thread
per row).
The row-by-row reference costs about a microsecond per row, so at BIG the
parameter cross product is thinned (NULLs in `a` only, one literal per op);
every smaller size runs the full product. References are computed once per
case and shared between the wrapper tests and the exec-node tests."""
import functools
import math

import numpy as np
import pytest

import expr_ref as R
import oracle

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

MIN, MAX = R.I64_MIN, R.I64_MAX
INF, NAN = math.inf, math.nan
BIG = 524288 + 257
SIZES = [0, 1, 7, 8, 9, 255, 256, 257, 5631, 5632, 5633, 11265, BIG]
SMALL_SIZES = SIZES[:-1]
NULL_PATTERNS = ["neither", "a", "b", "both"]


@pytest.fixture(scope="module")
def gq():
    from spark_amd import gpuq
    assert torch.cuda.is_available()
    return gpuq


@pytest.fixture(scope="module")
def gx():
    from spark_amd import exec as gx_
    return gx_


@pytest.fixture(scope="module", autouse=True)
def _drop_cached_cases():
    yield
    for f in (filter_i64_case, filter_f64_case, project_inputs, project_ref):
        f.cache_clear()


def to_dev(a: np.ndarray):
    # copies: the cached case arrays are read-only and shared between tests
    return torch.from_numpy(np.array(a, order="C")).cuda()


def pack_validity(valid_bool: np.ndarray):
    return torch.from_numpy(np.packbits(valid_bool, bitorder="little")).cuda()


def unpack_validity(bits, n):
    assert bits.dtype == torch.uint8 and bits.numel() == (n + 7) // 8
    return np.unpackbits(bits.cpu().numpy(), bitorder="little")[:n].astype(bool)


def gen_i64(seed, n, range_=0):
    return oracle.gen_i64(seed, n, range_=range_) if n else np.empty(0, np.int64)


def gen_f64(seed, n):
    return oracle.gen_f64_unit(seed, n) if n else np.empty(0, np.float64)


def gen_valid(seed, n):
    """about 1 row in 5 NULL"""
    return gen_i64(seed, n, range_=5) != 0


def assert_values_equal(got, exp, valid, what=""):
    """exact on the rows the reference calls valid"""
    assert got.shape == exp.shape and got.dtype == exp.dtype, what
    g, e = got[valid], exp[valid]
    if got.dtype == np.float64:
        both_nan = np.isnan(g) & np.isnan(e)
        same = (g.view(np.uint64) == e.view(np.uint64)) | both_nan
    else:
        same = g == e
    if not same.all():
        i = int(np.flatnonzero(~same)[0])
        raise AssertionError(f"{what}: {int((~same).sum())} rows differ, first "
                             f"valid-row #{i}: got {g[i]!r} expected {e[i]!r}")


def check_filter(gq, vals, valid, op, lit, dtype, what=""):
    perm, cnt = gq.filter_cmp(to_dev(vals), op, lit,
                              validity=None if valid is None
                              else pack_validity(valid))
    exp = R.ref_filter(vals, valid, op, lit, dtype)
    what = f"{what} n={len(vals)} {op} {lit!r}"
    assert cnt == len(exp), f"{what}: count {cnt} != {len(exp)}"
    got = perm.cpu().numpy().view(np.uint32)
    assert got.shape == exp.shape and (got == exp).all(), what
    return cnt


# ------------------------------------------------------------ filter, int64

I64_LIT = 1


@functools.lru_cache(maxsize=None)
def filter_i64_case(n, with_valid):
    vals = gen_i64(101, n, range_=7) - 3          # -3..3: passes, fails, ties
    valid = None
    if with_valid:
        valid = gen_valid(102, n)
        vals[~valid] = I64_LIT    # a kernel that ignored validity fails ==
    return vals, valid


@pytest.mark.parametrize("with_valid", [False, True], ids=["nonull", "nulls"])
@pytest.mark.parametrize("n", SIZES)
def test_filter_i64(gq, n, with_valid):
    vals, valid = filter_i64_case(n, with_valid)
    for op in R.CMP_OPS:
        check_filter(gq, vals, valid, op, I64_LIT, "i64")


@pytest.mark.parametrize("case", ["all_pass", "none_pass", "all_null"])
def test_filter_i64_degenerate(gq, case):
    n = 5633
    vals = gen_i64(103, n, range_=7) - 3
    if case == "all_null":
        valid = np.zeros(n, dtype=bool)
        for op in R.CMP_OPS:
            check_filter(gq, vals, valid, op, 0, "i64", case)
    elif case == "all_pass":
        for op, lit in [(">=", -3), ("<", 4), ("!=", 9), ("<=", MAX)]:
            assert check_filter(gq, vals, None, op, lit, "i64", case) == n
    else:
        for op, lit in [("<", -3), (">", 3), ("==", 9), ("<", MIN)]:
            assert check_filter(gq, vals, None, op, lit, "i64", case) == 0


@pytest.mark.parametrize("with_valid", [False, True], ids=["nonull", "nulls"])
def test_filter_i64_extreme_literals(gq, with_valid):
    n = 5633
    vals = gen_i64(104, n)                         # full 64-bit range
    vals[::5] = MIN
    vals[1::5] = MAX
    vals[2::7] = 0
    valid = gen_valid(105, n) if with_valid else None
    for lit in (MIN, MAX):
        for op in R.CMP_OPS:
            check_filter(gq, vals, valid, op, lit, "i64")


@pytest.mark.parametrize("lit", [INF, -INF, NAN], ids=["inf", "-inf", "nan"])
@pytest.mark.parametrize("n", [9, 5633])
def test_filter_i64_nonfinite_literal(gq, n, lit):
    """constant predicates: cast-to-double never reaches +/-inf, and NaN is
    greater than everything"""
    vals = gen_i64(106, n, range_=7) - 3
    vals[::4] = MAX
    vals[1::4] = MIN
    valid = gen_valid(107, n)
    for v in (None, valid):
        for op in R.CMP_OPS:
            check_filter(gq, vals, v, op, lit, "i64")


def test_filter_i64_float_literal_beyond_2_53_is_exact(gq):
    """Where an int64 no longer fits a double the engine's rewrite compares
    the integer with the literal EXACTLY; Spark's cast-to-double rounds the
    column first (2^53 + 1 == 9007199254740992.0 there). DESIGN.md states
    the difference; this pins the exact behaviour. Python compares an int
    with a float exactly, which is the reference here."""
    P = 1 << 53
    vals = np.array([P - 1, P, P + 1, P + 2, P + 3, -P - 1, -P, -P + 1,
                     MAX, MAX - 511, MAX - 512, MAX - 513, MIN, MIN + 1, 0],
                    dtype=np.int64)
    valid = np.ones(len(vals), bool)
    valid[3] = False
    cmp_ = {"==": lambda k, l: k == l, "<": lambda k, l: k < l,
            "<=": lambda k, l: k <= l, ">": lambda k, l: k > l,
            ">=": lambda k, l: k >= l, "!=": lambda k, l: k != l}
    for lit in (float(P), float(P + 2), -float(P), 2.0 ** 63, -(2.0 ** 63),
                2.0 ** 63 - 1024.0, 1e19, -1e19, 4503599627370496.5):
        for op in R.CMP_OPS:
            exp = np.array([i for i, k in enumerate(vals.tolist())
                            if valid[i] and cmp_[op](k, lit)], dtype=np.uint32)
            perm, cnt = gq.filter_cmp(to_dev(vals), op, lit,
                                      validity=pack_validity(valid))
            assert cnt == len(exp), (op, lit)
            assert (perm.cpu().numpy().view(np.uint32) == exp).all(), (op, lit)
    # the disagreement with cast-to-double, spelled out
    perm, cnt = gq.filter_cmp(to_dev(vals), "==", float(P))
    assert perm.cpu().tolist() == [1]            # not row 2 (2^53 + 1)
    assert R.ref_compare(vals, None, "==", float(P), "i64")[2]


# ---------------------------------------------------------- filter, float64

F64_LITERALS = [0.5, 0.0, -0.0, INF, -INF, NAN]


@functools.lru_cache(maxsize=None)
def filter_f64_case(n, with_valid):
    vals = gen_f64(111, n) * 2 - 1
    vals[0::11] = 0.0
    vals[1::13] = -0.0
    vals[2::7] = NAN
    vals[3::17] = INF
    vals[4::19] = -INF
    vals[5::23] = 0.5
    valid = gen_valid(112, n) if with_valid else None
    return vals, valid


@pytest.mark.parametrize("with_valid", [False, True], ids=["nonull", "nulls"])
@pytest.mark.parametrize("n", SMALL_SIZES)
def test_filter_f64(gq, n, with_valid):
    vals, valid = filter_f64_case(n, with_valid)
    for lit in F64_LITERALS:
        for op in R.CMP_OPS:
            check_filter(gq, vals, valid, op, lit, "f64")


@pytest.mark.parametrize("lit,with_valid", [(0.5, True), (NAN, False)],
                         ids=["0.5-nulls", "nan-nonull"])
def test_filter_f64_grid_stride(gq, lit, with_valid):
    vals, valid = filter_f64_case(BIG, with_valid)
    for op in R.CMP_OPS:
        check_filter(gq, vals, valid, op, lit, "f64")


def test_filter_f64_nan_under_null_rows(gq):
    """NaN hidden under a NULL row must not pass > / >= / == NaN"""
    n = 5633
    vals, _ = filter_f64_case(n, False)
    vals = vals.copy()
    valid = gen_valid(113, n)
    vals[~valid] = NAN
    for lit in (0.5, NAN):
        for op in R.CMP_OPS:
            check_filter(gq, vals, valid, op, lit, "f64")


# ------------------------------------------------------------ GpuFilterExec

@pytest.mark.parametrize("pred", ["some", "nothing", "everything"])
@pytest.mark.parametrize("n", [9, 5633])
def test_filter_exec_batch(gq, gx, n, pred):
    k = gen_i64(121, n, range_=7) - 3
    kv = gen_valid(122, n)
    k[~kv] = I64_LIT
    p = gen_f64(123, n)
    p[2::7] = NAN
    pv = gen_i64(124, n, range_=3) != 0
    q = gen_i64(125, n)
    col, op, lit = {"some": ("k", "<=", I64_LIT), "nothing": ("k", ">", 3),
                    "everything": ("q", ">=", MIN)}[pred]
    batch = gx.ColumnarBatch(
        {"k": to_dev(k), "p": to_dev(p), "q": to_dev(q)},
        validity={"k": pack_validity(kv), "p": pack_validity(pv)})
    plan = gx.GpuColumnarRule().pre_columnar_transitions(
        gx.FilterExec(col, op, lit, gx.InputBatches([batch])))
    out = list(plan.execute_columnar())
    assert len(out) == 1
    out = out[0]
    src = {"k": (k, kv), "p": (p, pv), "q": (q, None)}
    rows = R.ref_filter(src[col][0], src[col][1], op, lit, "i64").astype(np.int64)
    if pred == "nothing":
        assert len(rows) == 0
    if pred == "everything":
        assert len(rows) == n
    assert out.num_rows() == len(rows)
    assert list(out.columns()) == ["k", "p", "q"]
    for name, (data, valid) in src.items():
        m = len(rows)
        exp_valid = valid[rows] if valid is not None else np.ones(m, bool)
        bits = out.validity(name)
        if bits is None:
            # a bitmap may be dropped only when it would say "all valid"
            assert exp_valid.all(), name
        else:
            assert (unpack_validity(bits, m) == exp_valid).all(), name
        assert_values_equal(out.column(name).cpu().numpy(), data[rows],
                            exp_valid, name)


# ------------------------------------------------------------------ project

I64_LITERALS = [-1, 0, 3, MAX]
F64_PROJECT_LITERALS = [2.5, -0.0, NAN, INF]


@functools.lru_cache(maxsize=None)
def project_inputs(dtype, n, nulls):
    """-> (a, a_valid, b, b_valid); NULL rows hide INT64_MIN / a zero divisor"""
    if dtype == "i64":
        a = gen_i64(201, n, range_=201) - 100
        b = gen_i64(202, n, range_=21) - 10
        a[3::11] = MIN
        a[5::13] = MAX
        a[1::17] = -1
        a[2::19] = 0
        a[6::23] = -7
        b[0::5] = 0           # zero divisors
        b[3::11] = -1         # lines up with a == INT64_MIN
        b[1::7] = -1
        b[4::23] = MAX
        b[6::29] = MIN
        b[2::31] = 2
        hide_a, hide_b = MIN, 0
    else:
        a = gen_f64(203, n) * 200 - 100
        b = gen_f64(204, n) * 20 - 10
        a[0::11] = 0.0
        a[1::13] = -0.0
        a[2::17] = INF
        a[3::19] = -INF
        a[4::23] = NAN
        a[5::29] = 5e-324      # subnormal
        b[0::5] = 0.0          # zero divisors, both signs
        b[1::5] = -0.0
        b[2::17] = INF         # inf - inf, inf / inf
        b[0::11] = 0.0         # 0 * ..., 0 / 0
        b[3::31] = NAN
        b[7::37] = 5e-324
        b[4::41] = -INF
        hide_a, hide_b = NAN, 0.0
    av = bv = None
    if nulls in ("a", "both"):
        av = gen_valid(205, n)
        a[~av] = hide_a
    if nulls in ("b", "both"):
        bv = gen_valid(206, n)
        b[~bv] = hide_b
    for arr in (a, b, av, bv):
        if arr is not None:
            arr.setflags(write=False)
    return a, av, b, bv


@functools.lru_cache(maxsize=None)
def project_ref(dtype, n, nulls, op, lit):
    """lit None: column-column form (b and its validity take part);
    otherwise column-literal (b is not an input)."""
    a, av, b, bv = project_inputs(dtype, n, nulls)
    if lit is None:
        return R.ref_binop(a, av, op, b, bv, dtype)
    return R.ref_binop(a, av, op, lit, None, dtype)


def project_literals(dtype, n):
    """literals to run at size n: all of them, but only the first at BIG
    (for int64 that is -1, which keeps INT64_MIN / -1 in the `/` case)"""
    lits = I64_LITERALS if dtype == "i64" else F64_PROJECT_LITERALS
    return lits[:1] if n == BIG else lits


def project_forms(dtype, n, nulls, op):
    """right-hand sides to run: None = column b, otherwise a literal"""
    forms = [None]
    if nulls in ("neither", "a"):    # a literal has no validity of its own
        forms += project_literals(dtype, n)
    return forms


def check_nullable(gq, dtype, n, nulls, op, lit):
    a, av, b, bv = project_inputs(dtype, n, nulls)
    exp_vals, exp_valid = project_ref(dtype, n, nulls, op, lit)
    what = f"{dtype} n={n} nulls={nulls} a {op} {'b' if lit is None else lit!r}"
    dav = pack_validity(av) if av is not None else None
    if lit is None:
        dbv = pack_validity(bv) if bv is not None else None
        out, bits = gq.project_binop_nullable(
            to_dev(a), op, b=to_dev(b), a_validity=dav, b_validity=dbv)
        any_validity = av is not None or bv is not None
    else:
        out, bits = gq.project_binop_nullable(
            to_dev(a), op, literal=lit, a_validity=dav)
        any_validity = av is not None
    if bits is None:
        # only when nothing can be NULL
        assert not any_validity and op != "/", what
        assert exp_valid.all(), what
    else:
        got_valid = unpack_validity(bits, n)
        assert (got_valid == exp_valid).all(), \
            f"{what}: validity differs on {int((got_valid != exp_valid).sum())} rows"
    assert_values_equal(out.cpu().numpy(), exp_vals, exp_valid, what)


@pytest.mark.parametrize("nulls", NULL_PATTERNS)
@pytest.mark.parametrize("n", SMALL_SIZES)
@pytest.mark.parametrize("dtype", ["i64", "f64"])
def test_project_binop_nullable(gq, dtype, n, nulls):
    assert set(gq.BINOP) == set(R.BIN_OPS)
    for op in gq.BINOP:
        for lit in project_forms(dtype, n, nulls, op):
            check_nullable(gq, dtype, n, nulls, op, lit)


@pytest.mark.parametrize("op", list(R.BIN_OPS))
@pytest.mark.parametrize("dtype", ["i64", "f64"])
def test_project_binop_nullable_grid_stride(gq, dtype, op):
    check_nullable(gq, dtype, BIG, "a", op, None)
    lit = project_literals(dtype, BIG)[0]
    check_nullable(gq, dtype, BIG, "a", op, lit)


def check_plain(gq, dtype, n, op, lit):
    """gpuq.project_binop: tensor only; rows the reference calls NULL (a zero
    divisor) are the caller's business and are not compared"""
    a, _, b, _ = project_inputs(dtype, n, "neither")
    exp_vals, exp_valid = project_ref(dtype, n, "neither", op, lit)
    if lit is None:
        out = gq.project_binop(to_dev(a), op, b=to_dev(b))
    else:
        out = gq.project_binop(to_dev(a), op, literal=lit)
    assert isinstance(out, torch.Tensor)
    assert_values_equal(out.cpu().numpy(), exp_vals, exp_valid,
                        f"plain {dtype} n={n} a {op} {'b' if lit is None else lit!r}")


@pytest.mark.parametrize("n", SMALL_SIZES)
@pytest.mark.parametrize("dtype", ["i64", "f64"])
def test_project_binop_plain(gq, dtype, n):
    """wraparound, negative truncation and INT64_MIN / -1 in the entry point
    the AVG evaluation and non-nullable projections use"""
    for op in gq.BINOP:
        for lit in project_forms(dtype, n, "neither", op):
            check_plain(gq, dtype, n, op, lit)


@pytest.mark.parametrize("op", list(R.BIN_OPS))
@pytest.mark.parametrize("dtype", ["i64", "f64"])
def test_project_binop_plain_grid_stride(gq, dtype, op):
    check_plain(gq, dtype, BIG, op, None)
    check_plain(gq, dtype, BIG, op, project_literals(dtype, BIG)[0])


def run_project(gx, batch, projections):
    plan = gx.GpuColumnarRule().pre_columnar_transitions(
        gx.ProjectExec(projections, gx.InputBatches([batch])))
    out = list(plan.execute_columnar())
    assert len(out) == 1
    return out[0]


def check_project_exec(gq, gx, dtype, n, nulls, ops):
    a, av, b, bv = project_inputs(dtype, n, nulls)
    p = gen_i64(207, n)
    pv = gen_i64(208, n, range_=3) != 0
    validity = {"p": pack_validity(pv)}
    if av is not None:
        validity["a"] = pack_validity(av)
    if bv is not None:
        validity["b"] = pack_validity(bv)
    p_bits = validity["p"].clone()
    batch = gx.ColumnarBatch({"a": to_dev(a), "b": to_dev(b), "p": to_dev(p)},
                             validity=validity)
    lit = project_literals(dtype, n)[0]
    projections, expect = ["p", "a"], {}
    for op in ops:
        projections.append((f"cc{op}", "a", op, "b", None))
        expect[f"cc{op}"] = (op, None, av is not None or bv is not None)
        if nulls in ("neither", "a"):
            projections.append((f"cl{op}", "a", op, None, lit))
            expect[f"cl{op}"] = (op, lit, av is not None)
    out = run_project(gx, batch, projections)
    assert out.num_rows() == n
    assert list(out.columns()) == [q if isinstance(q, str) else q[0]
                                   for q in projections]
    # pass-through columns keep data and bitmap bit for bit
    assert torch.equal(out.column("p"), to_dev(p))
    assert out.validity("p") is not None
    assert torch.equal(out.validity("p"), p_bits)
    assert torch.equal(out.column("a").view(torch.int64),
                       to_dev(a).view(torch.int64))
    if av is None:
        assert out.validity("a") is None
    else:
        assert torch.equal(out.validity("a"), pack_validity(av))
    for name, (op, l, any_validity) in expect.items():
        exp_vals, exp_valid = project_ref(dtype, n, nulls, op, l)
        what = f"exec {dtype} n={n} nulls={nulls} {name}"
        bits = out.validity(name)
        if bits is None:
            assert not any_validity and op != "/", what
            assert exp_valid.all(), what
        else:
            assert (unpack_validity(bits, n) == exp_valid).all(), what
        assert_values_equal(out.column(name).cpu().numpy(), exp_vals,
                            exp_valid, what)


@pytest.mark.parametrize("nulls", NULL_PATTERNS)
@pytest.mark.parametrize("n", SMALL_SIZES)
@pytest.mark.parametrize("dtype", ["i64", "f64"])
def test_project_exec(gq, gx, dtype, n, nulls):
    check_project_exec(gq, gx, dtype, n, nulls, list(R.BIN_OPS))


@pytest.mark.parametrize("dtype", ["i64", "f64"])
def test_project_exec_grid_stride(gq, gx, dtype):
    check_project_exec(gq, gx, dtype, BIG, "a", list(R.BIN_OPS))


@pytest.mark.parametrize("dtype", ["i64", "f64"])
def test_project_exec_divide_by_zero_is_null(gq, gx, dtype):
    """non-ANSI Spark: x / 0 is NULL, not 0 / inf / NaN — with no NULL in any
    input, through the exec node, column and literal divisors"""
    n = 257
    a, _, b, _ = project_inputs(dtype, n, "neither")
    zero = 0 if dtype == "i64" else -0.0
    batch = gx.ColumnarBatch({"a": to_dev(a), "b": to_dev(b)})
    out = run_project(gx, batch, [("q", "a", "/", "b", None),
                                  ("z", "a", "/", None, zero)])
    exp_vals, exp_valid = project_ref(dtype, n, "neither", "/", None)
    assert 0 < int((~exp_valid).sum()) < n
    assert out.validity("q") is not None
    assert (unpack_validity(out.validity("q"), n) == exp_valid).all()
    assert_values_equal(out.column("q").cpu().numpy(), exp_vals, exp_valid)
    assert out.validity("z") is not None
    assert not unpack_validity(out.validity("z"), n).any()


def test_project_then_aggregate_skips_nulls(gq, gx):
    """scan -> project -> SUM / COUNT(col) / COUNT(*) over a nullable column,
    as one plan through the rule: NULL rows must not count as values"""
    n = 5633
    k = gen_i64(211, n, range_=50)
    a = gen_i64(212, n, range_=2001) - 1000
    b = gen_i64(213, n, range_=2001) - 1000
    av = gen_valid(214, n)
    a[~av] = MIN                   # would wreck the sums if it leaked
    batch = gx.ColumnarBatch({"k": to_dev(k), "a": to_dev(a), "b": to_dev(b)},
                             validity={"a": pack_validity(av)})
    plan = gx.HashAggregateExec(
        "k", [("sum", "a"), ("count", "a"), ("sum", "r"), ("count", "r"),
              ("sum", "s"), ("count", "s"), ("count*", None)], "complete",
        gx.ProjectExec(["k", "a", ("r", "a", "+", None, 1),
                        ("s", "a", "*", "b", None)],
                       gx.InputBatches([batch])))
    plan = gx.GpuColumnarRule().pre_columnar_transitions(plan)
    out = list(plan.execute_columnar())
    assert len(out) == 1
    out = out[0]
    got = {c: t.cpu().numpy() for c, t in out.columns().items()}
    r_vals, r_valid = R.ref_binop(a, av, "+", 1, None, "i64")
    s_vals, s_valid = R.ref_binop(a, av, "*", b, None, "i64")
    assert (r_valid == av).all() and (s_valid == av).all()
    ref = {}
    for i in range(n):
        g = ref.setdefault(int(k[i]), dict(sa=0, ca=0, sr=0, cr=0, ss=0, cs=0, rows=0))
        g["rows"] += 1
        if av[i]:
            g["sa"] += int(a[i]); g["ca"] += 1
        if r_valid[i]:
            g["sr"] += int(r_vals[i]); g["cr"] += 1
        if s_valid[i]:
            g["ss"] += int(s_vals[i]); g["cs"] += 1
    assert sorted(got["k"].tolist()) == sorted(ref)
    assert out.num_rows() == len(ref)
    for j, key in enumerate(got["k"].tolist()):
        g = ref[key]
        assert got["count(1)"][j] == g["rows"]
        for col, s, c in (("a", "sa", "ca"), ("r", "sr", "cr"), ("s", "ss", "cs")):
            assert got[f"count({col})"][j] == g[c], (col, key)
            bits = out.validity(f"sum({col})")
            valid = True if bits is None else \
                bool(unpack_validity(bits, out.num_rows())[j])
            assert valid == (g[c] > 0), (col, key)
            if g[c]:
                assert int(got[f"sum({col})"][j]) == R.wrap_i64(g[s]), (col, key)
    assert sum(g["ca"] for g in ref.values()) == int(av.sum()) < n


# ----------------------------------------------------------- mixed operands

@pytest.mark.parametrize("entry", ["project_binop", "project_binop_nullable"])
def test_mixed_operands_are_rejected(gq, entry):
    n = 9
    ai = to_dev(gen_i64(221, n, range_=10))
    af = to_dev(gen_f64(222, n))
    errors = (ValueError, gq.GpuqError)
    fn = getattr(gq, entry)
    with pytest.raises(errors):
        fn(ai, "+", literal=0.5)          # would truncate to 0
    with pytest.raises(errors):
        fn(ai, "*", literal=NAN)
    with pytest.raises(errors):
        fn(ai, "-", literal=INF)
    with pytest.raises(errors):
        fn(af, "+", b=ai)                 # would read int bits as doubles
    with pytest.raises(errors):
        fn(ai, "+", b=af)
    # the same values in matching types are fine
    out = gq.project_binop(ai, "+", literal=2.0)      # integral float literal
    assert (out.cpu().numpy() == ai.cpu().numpy() + 2).all()
    out = gq.project_binop(af, "+", literal=2)        # int literal on doubles
    assert (out.cpu().numpy() == af.cpu().numpy() + 2.0).all()


# -------------------------------------------------------------- cast, range

@pytest.mark.parametrize("n", SIZES)
def test_cast_i64_f64(gq, n):
    vals = gen_i64(231, n)                    # full 64-bit range: most round
    planted = [(1 << 53) + 1, -((1 << 53) + 1), MIN, MAX, (1 << 63) - 513,
               (1 << 53) + 3, (1 << 63) - 512, 0, -1]
    for j, v in enumerate(planted):
        vals[j::37] = v
    got = gq.cast_i64_f64(to_dev(vals)).cpu().numpy()
    exp = R.ref_cast_i64_f64(vals)
    assert_values_equal(got, exp, np.ones(n, bool), f"cast n={n}")


@pytest.mark.parametrize("n", SMALL_SIZES)
@pytest.mark.parametrize("start,step", [(5, 3), (100, -7), (MAX - 5, 3),
                                        (1, MAX), (MIN, -1), (7, 0)])
def test_range_i64(gq, n, start, step):
    got = gq.range_i64(n, start, step).cpu().numpy()
    exp = R.ref_range_i64(n, start, step)
    assert got.dtype == np.int64 and got.shape == exp.shape
    assert (got == exp).all()


@pytest.mark.parametrize("start,step", [(100, -7), (MAX - 1000, 1 << 40)])
def test_range_i64_grid_stride(gq, start, step):
    got = gq.range_i64(BIG, start, step).cpu().numpy()
    assert (got == R.ref_range_i64(BIG, start, step)).all()


# --------------------------------------------------------------------- n = 0

def test_empty_inputs_return_cleanly(gq, gx):
    ei = to_dev(np.empty(0, np.int64))
    ef = to_dev(np.empty(0, np.float64))
    eb = torch.empty(0, dtype=torch.uint8, device="cuda")
    for col, lit in ((ei, 1), (ef, 0.5), (ef, NAN), (ei, INF)):
        for v in (None, eb):
            perm, cnt = gq.filter_cmp(col, "<=", lit, validity=v)
            assert cnt == 0 and perm.numel() == 0
    perm = torch.empty(0, dtype=torch.int32, device="cuda")
    for col in (ei, ef):
        out = gq.gather(col, perm)
        assert out.numel() == 0 and out.dtype == col.dtype
        for op in gq.BINOP:
            out = gq.project_binop(col, op, b=col)
            assert out.numel() == 0 and out.dtype == col.dtype
            out = gq.project_binop(col, op, literal=2)
            assert out.numel() == 0
            out, bits = gq.project_binop_nullable(col, op, b=col, a_validity=eb,
                                                  b_validity=eb)
            assert out.numel() == 0 and bits is not None and bits.numel() == 0
            out, bits = gq.project_binop_nullable(col, op, literal=2)
            assert out.numel() == 0
            assert (bits is None) == (op != "/")
    out = gq.cast_i64_f64(ei)
    assert out.numel() == 0 and out.dtype == torch.float64
    out = gq.range_i64(0, 5, -3)
    assert out.numel() == 0 and out.dtype == torch.int64
    torch.cuda.synchronize()
    # and the exec nodes on an empty batch
    rule = gx.GpuColumnarRule()
    batch = gx.ColumnarBatch({"k": ei, "v": ef}, validity={"k": eb})
    plan = rule.pre_columnar_transitions(gx.ProjectExec(
        ["k", ("w", "v", "/", None, 2.0)],
        gx.FilterExec("k", "!=", 3, gx.InputBatches([batch]))))
    out = list(plan.execute_columnar())
    assert len(out) == 1 and out[0].num_rows() == 0
    assert list(out[0].columns()) == ["k", "w"]
    torch.cuda.synchronize()
