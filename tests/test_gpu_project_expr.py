"""GPU parity for compound SELECT-list expressions (gpuq_project_expr,
gpuq.project_expr and the expression form of ProjectExec / GpuProjectExec)
against the row-by-row evaluator of tests/project_ref.py.

Every comparison is exact: the bitmap bytes, and the 64-bit value patterns
wherever the row is valid (NULL rows must hold 0), with the one exception
that any NaN equals any NaN.

Sizes: 0 and 1; 7 / 8 / 9 (one bitmap byte); 63 / 64 / 65 (one ballot word);
255 / 256 / 257 (one round of a block); T-1 / T / T+1 around the T = 1024-row
tile of one block (the full-tile and the tail code path) and 3T + 17 (three
full blocks and a tail). The full expression list runs up to 257 rows, a
thinned list at the tile sizes.
"""
import ctypes
import functools
import struct

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import project_ref as R  # noqa: E402
from expr_gen import random_expr  # noqa: E402
from spark_amd import expression as E  # noqa: E402
from spark_amd.expression import (Abs, BinOp, CaseWhen, Cast, Coalesce,  # noqa: E402
                                  Compare, If, Insn, Lit, Neg)
from spark_amd.predicate import (And, Between, Cmp, Col, In, IsNotNull,  # noqa: E402
                                 IsNull, Not, Or)

T = 1024
SMALL = [0, 1, 7, 8, 9, 63, 64, 65, 255, 256, 257]
TILES = [T - 1, T, T + 1, 3 * T + 17]
NAN, INF = float("nan"), float("inf")
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
ISPECIAL = np.array([I64_MIN, I64_MAX, 0, -1, 1, 2, -7, 100, 1 << 53, -(1 << 40)],
                    dtype=np.int64)
FSPECIAL = np.array([NAN, INF, -INF, 0.0, -0.0, 2.5, -0.9, 1e19, -1e19, 3.0])
DTYPES = {"a": "i64", "b": "i64", "d": "i64", "ep": "i64", "t": "i64",
          "z": "i64", "k": "i64", "m": "i64", "x": "f64", "y": "f64", "w": "f64"}
ICOLS = [c for c, dt in DTYPES.items() if dt == "i64"]
FCOLS = [c for c, dt in DTYPES.items() if dt == "f64"]


@pytest.fixture(scope="module")
def gq():
    from spark_amd import gpuq
    assert torch.cuda.is_available()
    assert gpuq.EXPR_TILE == T
    return gpuq


# ---------------- data ----------------

@functools.lru_cache(maxsize=None)
def host_cols(n):
    """name -> (values, valid or None, dtype). NULL rows hold live-looking
    values drawn like the valid ones; z is NULL in every row; k only in its
    last row; d, ep, m and w carry no bitmap."""
    rng = np.random.RandomState(7000 + n % 9973)
    last_clear = np.ones(n, bool)
    if n:
        last_clear[-1] = False
    cols = {
        "a": (ISPECIAL[rng.randint(0, len(ISPECIAL), size=n)], rng.rand(n) > 0.25),
        "b": (ISPECIAL[rng.randint(0, len(ISPECIAL), size=n)], rng.rand(n) > 0.3),
        "d": (rng.randint(0, 11, size=n).astype(np.int64), None),
        "ep": (rng.randint(90000, 10500000, size=n).astype(np.int64), None),
        "t": (rng.randint(0, 9, size=n).astype(np.int64), rng.rand(n) > 0.2),
        "z": (rng.randint(-3, 4, size=n).astype(np.int64), np.zeros(n, bool)),
        "k": (rng.randint(-3, 4, size=n).astype(np.int64), last_clear),
        "m": (rng.randint(-3, 4, size=n).astype(np.int64), None),
        "x": (FSPECIAL[rng.randint(0, len(FSPECIAL), size=n)], rng.rand(n) > 0.2),
        "y": (FSPECIAL[rng.randint(0, len(FSPECIAL), size=n)], rng.rand(n) > 0.2),
        "w": (FSPECIAL[rng.randint(0, len(FSPECIAL), size=n)], None),
    }
    for v, ok in cols.values():
        v.setflags(write=False)
        if ok is not None:
            ok.setflags(write=False)
    return {c: (v, ok, DTYPES[c]) for c, (v, ok) in cols.items()}


@functools.lru_cache(maxsize=None)
def dev_cols(n):
    h = host_cols(n)
    cols = {c: torch.from_numpy(np.array(v)).cuda() for c, (v, _, _) in h.items()}
    valid = {c: torch.from_numpy(np.packbits(ok, bitorder="little")).cuda()
             for c, (_, ok, _) in h.items() if ok is not None}
    return cols, valid


# ---------------- comparison ----------------

def expected_arrays(vals, dt):
    """reference rows -> (raw 64-bit patterns with 0 under NULL, valid mask,
    NaN mask)"""
    n = len(vals)
    valid = np.array([v is not None for v in vals], dtype=bool)
    raw = np.zeros(n, dtype=np.int64)
    nan = np.zeros(n, dtype=bool)
    for i, v in enumerate(vals):
        if v is None:
            continue
        if dt == "f64":
            if v != v:
                nan[i] = True
            else:
                raw[i] = struct.unpack("<q", struct.pack("<d", v))[0]
        else:
            raw[i] = v
    return raw, valid, nan


def assert_output(name, got, bits, vals, dt, n, nullable):
    raw, valid, nan = expected_arrays(vals, dt)
    assert got.dtype == (torch.float64 if dt == "f64" else torch.int64), name
    assert got.numel() == n, name
    g = got.cpu().numpy()
    if dt == "f64":
        assert np.isnan(g[nan]).all(), name
    graw = g.view(np.int64).copy()
    graw[nan] = 0
    bad = np.flatnonzero(graw != raw)
    assert bad.size == 0, (name, n, bad[:5], graw[bad[:5]], raw[bad[:5]])
    if nullable:
        assert bits is not None, name
        want = np.packbits(valid, bitorder="little")
        assert bits.numel() == (n + 7) // 8, name
        assert (bits.cpu().numpy() == want).all(), (name, n)
    else:
        assert bits is None, name        # nothing in it can be NULL
        assert valid.all(), name


@functools.lru_cache(maxsize=None)
def reference(n, case_id):
    return R.ref_project(host_cols(n), CASES[case_id])


def run_case(gq, n, case_id):
    outputs = CASES[case_id]
    cols, valid = dev_cols(n)
    got = gq.project_expr(cols, outputs, validities=valid)
    ref = reference(n, case_id)
    _, _, dts, nls = E.lower(outputs, {c: dt for c, dt in DTYPES.items()},
                             nullable=list(valid))
    assert list(got) == [name for name, _ in outputs]
    for (name, _), dt, nl in zip(outputs, dts, nls):
        vals, rdt = ref[name]
        assert rdt == dt
        assert_output(f"{case_id}:{name}", got[name][0], got[name][1], vals, dt, n, nl)


# ---------------- expressions ----------------

A, B, D, EP, TX, Z, K, M = (Col(c) for c in ICOLS)
X, Y, W = (Col(c) for c in FCOLS)


def q1():
    disc_price = BinOp("*", Col("ep"), BinOp("-", Lit(100), Col("d")))
    charge = BinOp("*", BinOp("*", Col("ep"), BinOp("-", Lit(100), Col("d"))),
                   BinOp("+", Lit(100), Col("t")))
    return [("disc_price", disc_price), ("charge", charge)]


def deep(nlits, leaf):
    e = leaf
    for _ in range(nlits):
        e = BinOp("+", Lit(1), e)
    return e


def flag(p):
    return Cast(p, "i64")


CASES = {}
for _op, _nm in (("+", "add"), ("-", "sub"), ("*", "mul"), ("/", "div")):
    CASES[f"{_nm}_i64"] = [("o", BinOp(_op, A, B))]
    CASES[f"{_nm}_f64"] = [("o", BinOp(_op, X, Y))]
    CASES[f"{_nm}_i64_lit"] = [("o", BinOp(_op, A, 3))]
    CASES[f"{_nm}_f64_lit"] = [("o", BinOp(_op, W, 2.5))]
for _op, _nm in (("==", "eq"), ("<", "lt"), ("<=", "le"), (">", "gt"), (">=", "ge"),
                 ("!=", "ne")):
    CASES[f"cmp_{_nm}_i64"] = [("o", flag(Compare(A, _op, B)))]
    CASES[f"cmp_{_nm}_f64"] = [("o", flag(Compare(X, _op, Y)))]
CASES.update({
    "div_i64_by_minus1": [("o", BinOp("/", A, -1))],
    "div_i64_by_0": [("o", BinOp("/", A, 0))],
    "div_f64_by_neg0": [("o", BinOp("/", W, -0.0))],
    "div_i64_nonnull": [("o", BinOp("/", EP, D))],            # zeros in d
    "neg_i64": [("o", Neg(A))], "neg_f64": [("o", Neg(X))],
    "abs_i64": [("o", Abs(A))], "abs_f64": [("o", Abs(X))],
    "neg_nonnull": [("o", Neg(M)), ("p", Abs(W))],
    "cast_f64_i64": [("o", Cast(X, "i64")), ("p", Cast(W, "i64"))],
    "cast_i64_f64": [("o", Cast(A, "f64")), ("p", Cast(EP, "f64"))],
    "cast_scaled": [("o", Cast(BinOp("*", W, 1.5), "i64"))],
    "cmp_lit_f64_nan": [("o", flag(Compare(X, "==", NAN))), ("p", flag(Cmp("y", "<", NAN)))],
    "cmp_i64_frac": [("o", flag(Compare(A, "<", 0.5))), ("p", flag(Compare(-0.5, "<=", B)))],
    "cmp_nonnull": [("o", flag(Compare(D, "<", 5)))],
    "cmp_as_value": [("o", flag(Compare(X, "<", Y)))],
    "is_null": [("o", flag(IsNull("a"))), ("p", flag(IsNotNull("x"))),
                ("q", flag(IsNull("z"))), ("r", flag(IsNotNull("k")))],
    "and_or_not": [("o", flag(And(Cmp("a", ">", 0), Cmp("b", ">", 0)))),
                   ("p", flag(Or(Cmp("a", ">", 0), Cmp("b", ">", 0)))),
                   ("q", flag(Not(Cmp("x", ">", 0.0))))],
    "select_i64": [("o", If(Compare(A, ">", B), A, B))],
    "select_f64": [("o", If(Cmp("x", "<", Col("y")), X, Y))],
    "select_null_cond": [("o", If(Cmp("z", ">", 0), Lit(1), Lit(2)))],
    "select_div_untaken": [("o", If(Compare(D, "!=", 0), BinOp("/", EP, D), Lit(-1)))],
    "coalesce_i64": [("o", Coalesce(A, B))], "coalesce_f64": [("o", Coalesce(X, Y))],
    "coalesce_ab0": [("o", Coalesce(A, B, 0))],
    "coalesce_all_null": [("o", Coalesce(Z, Lit(None, "i64")))],
    "lit_only": [("o", Lit(42)), ("p", Lit(-0.0)), ("q", Lit(None, "f64"))],
    "col_copy": [("o", A), ("p", W), ("q", Z), ("r", K)],
    "q1": q1(),
    "case_between_in": [("o", CaseWhen(
        [(Between("d", 0, 2), BinOp("*", EP, 2)), (In("d", [3, 5, None]), A),
         (Cmp("t", ">=", 6), Neg(EP))], else_=Lit(0)))],
    "case_no_else": [("o", CaseWhen([(Cmp("x", ">", 1.0), Y), (IsNull("x"), W)]))],
    "case_five_arms": [("o", CaseWhen(
        [(Cmp("d", "==", k), deep(2, Col("a"))) for k in range(5)], else_=B))],
    "three_outputs": [("s", BinOp("+", A, B)), ("n", Neg(BinOp("+", A, B))),
                      ("f", BinOp("*", Cast(BinOp("+", A, B), "f64"), W))],
    "four_outputs": [("disc_price", q1()[0][1]), ("charge", q1()[1][1]),
                     ("flag", flag(Compare(q1()[1][1], ">", 50000000000))),
                     ("ratio", BinOp("/", Cast(q1()[0][1], "f64"), Cast(EP, "f64")))],
    "last_bit_clear": [("o", BinOp("+", K, M))],
    "all_null_in": [("o", BinOp("*", Z, EP)), ("p", Coalesce(Z, M))],
    # one program at each cap exactly
    "cap_insns_48": [("o", Coalesce(*([A, B] * 12)))],
    "cap_depth_8": [("o", deep(7, Col("d")))],
    "cap_cols_8": [("o", BinOp("+", BinOp("+", BinOp("+", A, B), BinOp("+", D, EP)),
                               BinOp("+", BinOp("+", TX, Z), BinOp("+", K, M))))],
    "cap_outs_4": [("o", Neg(A)), ("p", Abs(B)), ("q", Neg(X)), ("r", Abs(Y))],
})
THIN = ["add_i64", "div_i64", "div_f64", "cmp_lt_f64", "cast_f64_i64", "is_null",
        "select_i64", "coalesce_ab0", "q1", "case_between_in", "four_outputs",
        "last_bit_clear", "all_null_in", "cap_insns_48", "cap_depth_8",
        "cap_cols_8", "cap_outs_4", "lit_only"]


def test_cases_are_what_they_claim():
    schema = dict(DTYPES)
    cols, prog, _, _ = E.lower(CASES["cap_insns_48"], schema)
    assert len(prog) == E.MAX_INSNS
    cols, prog, _, _ = E.lower(CASES["cap_depth_8"], schema)
    assert E.stack_depth(prog) == E.MAX_DEPTH
    cols, prog, _, _ = E.lower(CASES["cap_cols_8"], schema)
    assert len(cols) == E.MAX_COLS
    assert len(CASES["cap_outs_4"]) == E.MAX_OUTS
    _, prog, _, _ = E.lower(CASES["q1"], schema)
    assert sum(i.opcode == E.REF for i in prog) == 1
    # both kernel variants are exercised: stacks within and beyond 4 slots
    depths = {c: E.stack_depth(E.lower(CASES[c], schema)[1]) for c in CASES}
    assert min(depths.values()) <= 4 < max(depths.values())
    assert {c for c in THIN if depths[c] > 4} and {c for c in THIN if depths[c] <= 4}
    used = set()
    for c in CASES:
        used |= {i.opcode for i in E.lower(CASES[c], schema)[1]}
    assert used == set(range(16))


def test_data_holds_the_edges():
    h = host_cols(257)
    a, ok, _ = h["a"]
    for v in (I64_MIN, I64_MAX, 0, -1):
        assert (a[ok] == v).any()
    assert (~ok).any() and (a[~ok] != 0).any()       # live values under NULLs
    x, okx, _ = h["x"]
    assert np.isnan(x[okx]).any() and np.isinf(x[okx]).any()
    assert (np.signbit(x[okx]) & (x[okx] == 0)).any()
    assert not h["z"][1].any()
    assert h["k"][1][:-1].all() and not h["k"][1][-1]
    assert (h["d"][0] == 0).any() and h["d"][1] is None


@pytest.mark.parametrize("case_id", list(CASES))
def test_parity_small(gq, case_id):
    for n in SMALL:
        run_case(gq, n, case_id)


@pytest.mark.parametrize("n", TILES)
@pytest.mark.parametrize("case_id", THIN)
def test_parity_tiles(gq, n, case_id):
    run_case(gq, n, case_id)


def test_reference_sees_every_outcome():
    """non-vacuity at 257 rows: NULLs from inputs, from x / 0 and from a CASE
    without ELSE all occur, next to valid rows"""
    for case_id in ("div_i64_nonnull", "case_no_else", "q1", "select_i64",
                    "cast_f64_i64", "cmp_lt_f64"):
        for name, (vals, _) in reference(257, case_id).items():
            if (case_id, name) in (("q1", "disc_price"), ("cast_f64_i64", "p")):
                assert all(v is not None for v in vals)
                continue
            assert any(v is None for v in vals), (case_id, name)
            assert any(v is not None for v in vals), (case_id, name)
    vals = reference(257, "cast_f64_i64")["p"][0]
    assert {I64_MIN, I64_MAX, 0, 2} <= set(vals)
    assert set(reference(257, "cmp_lt_f64")["o"][0]) == {0, 1, None}


# ---------------- raw programs ----------------

def test_is_null_of_a_bool(gq):
    """IS_NULL takes any stack type: (a < b) IS NULL"""
    n = 257
    cols, valid = dev_cols(n)
    prog = [Insn(E.COL, 0, E.I64), Insn(E.COL, 1, E.I64), Insn(E.CMP_OP, 1, E.I64),
            Insn(E.IS_NULL, 0, E.BOOL), Insn(E.CAST, E.I64, E.BOOL),
            Insn(E.OUT, 0, E.I64)]
    out = gq.project_expr_program(cols, ["a", "b"], prog, ["o"], ["i64"], [False],
                                  validities=valid)
    h = host_cols(n)
    want = (~(h["a"][1] & h["b"][1])).astype(np.int64)
    assert out["o"][1] is None
    assert (out["o"][0].cpu().numpy() == want).all()


def test_guard_bytes_and_unaligned_bitmaps(gq):
    """64 guard bytes of 0xA5 after every output and bitmap stay untouched,
    the spare bits of the last bitmap byte are zero, and a bitmap needs no
    alignment beyond one byte (it starts at an odd address here)."""
    L = gq.lib()
    schema = dict(DTYPES)
    for case_id in ("q1", "cast_f64_i64", "four_outputs"):
        for n in [1, 7, 9, 65, 257, T - 1, T + 1, 3 * T + 17]:
            cols, valid = dev_cols(n)
            names, prog, dts, nls = E.lower(CASES[case_id], schema, nullable=list(valid))
            nb = (n + 7) // 8
            outs = [torch.full((n * 8 + 64,), 0xA5, dtype=torch.uint8, device="cuda")
                    for _ in dts]
            bits = [torch.full((1 + nb + 64,), 0xA5, dtype=torch.uint8, device="cuda")
                    for _ in dts]
            vp = ctypes.c_void_p
            rc = L.gpuq_project_expr(
                gq._stream(), n,
                (gq._Col * len(names))(*[gq._col(cols[c], valid.get(c)) for c in names]),
                len(names),
                (gq._ExprInsn * len(prog))(*[gq._ExprInsn(*i) for i in prog]), len(prog),
                (vp * len(dts))(*[o.data_ptr() for o in outs]),
                (vp * len(dts))(*[b.data_ptr() + 1 for b in bits]),   # always given
                (ctypes.c_int32 * len(dts))(*[E.TYPE_CODE[dt] for dt in dts]), len(dts))
            assert rc == 0, L.gpuq_last_error()
            ref = reference(n, case_id)
            for (name, _), o, b, dt in zip(CASES[case_id], outs, bits, dts):
                oh, bh = o.cpu().numpy(), b.cpu().numpy()
                assert (oh[n * 8:] == 0xA5).all(), (case_id, n, name)
                assert bh[0] == 0xA5 and (bh[1 + nb:] == 0xA5).all(), (case_id, n, name)
                vals = ref[name][0]
                raw, ok, nan = expected_arrays(vals, dt)
                got = oh[:n * 8].view(np.int64).copy()
                if dt == "f64":
                    assert np.isnan(oh[:n * 8].view(np.float64)[nan]).all()
                got[nan] = 0
                assert (got == raw).all(), (case_id, n, name)
                want_bits = np.packbits(ok, bitorder="little")
                assert (bh[1:1 + nb] == want_bits).all(), (case_id, n, name)
                if n % 8:
                    assert bh[nb] >> (n % 8) == 0        # spare bits zero


def test_inputs_not_written(gq):
    n = 3 * T + 17
    cols, valid = dev_cols(n)
    before = {c: t.clone() for c, t in cols.items()}
    vbefore = {c: t.clone() for c, t in valid.items()}
    for case_id in ("q1", "cap_cols_8", "four_outputs"):
        gq.project_expr(cols, CASES[case_id], validities=valid)
    torch.cuda.synchronize()
    for c, t in cols.items():
        assert torch.equal(t.view(torch.int64), before[c].view(torch.int64))
    for c, t in valid.items():
        assert torch.equal(t, vbefore[c])


# ---------------- seeded random trees ----------------

@pytest.mark.parametrize("seed", range(40))
def test_random_tree(gq, seed):
    rng = np.random.RandomState(90000 + seed)
    schema = dict(DTYPES)
    while True:
        outs = [(f"o{k}", random_expr(rng, rng.randint(1, 5),
                                      "i64" if rng.rand() < 0.5 else "f64",
                                      ICOLS, FCOLS))
                for k in range(rng.randint(1, 5))]
        try:
            E.lower(outs, schema)
            break
        except ValueError:      # over a cap, or an untyped NULL: draw again
            continue
    n = (SMALL + TILES)[seed % len(SMALL + TILES)] or 257
    cols, valid = dev_cols(n)
    got = gq.project_expr(cols, outs, validities=valid)
    ref = R.ref_project(host_cols(n), outs)
    _, _, dts, nls = E.lower(outs, schema, nullable=list(valid))
    for (name, _), dt, nl in zip(outs, dts, nls):
        assert_output(f"seed{seed}:{name}", got[name][0], got[name][1],
                      ref[name][0], dt, n, nl)


# ---------------- exec nodes ----------------

def lineitem_batch(gx, n, seed):
    rng = np.random.RandomState(seed)
    cols = {"l_extendedprice": rng.randint(90000, 10500000, size=n).astype(np.int64),
            "l_discount": rng.randint(0, 11, size=n).astype(np.int64),
            "l_tax": rng.randint(0, 9, size=n).astype(np.int64),
            "l_quantity": rng.randint(1, 51, size=n).astype(np.int64)}
    tax_ok = rng.rand(n) > 0.2
    return gx.ColumnarBatch(
        {c: torch.from_numpy(v).cuda() for c, v in cols.items()},
        validity={"l_tax": torch.from_numpy(
            np.packbits(tax_ok, bitorder="little")).cuda()})


def stacked_q1(gx, child):
    passthru = ["l_quantity", "l_extendedprice"]
    return gx.ProjectExec(
        passthru + ["disc_price",
                    ("charge", "disc_price", "*", "__one_plus_tax", None)],
        gx.ProjectExec(
            passthru + ["__one_plus_tax",
                        ("disc_price", "l_extendedprice", "*", "__one_minus_disc", None)],
            gx.ProjectExec(
                passthru + [("__one_minus_disc", "l_discount", "rsub", None, 100),
                            ("__one_plus_tax", "l_tax", "+", None, 100)], child)))


def fused_q1(gx, child):
    ep, d, t = Col("l_extendedprice"), Col("l_discount"), Col("l_tax")
    disc_price = BinOp("*", ep, BinOp("-", Lit(100), d))
    return gx.ProjectExec(
        ["l_quantity", "l_extendedprice", ("disc_price", disc_price),
         ("charge", BinOp("*", BinOp("*", ep, BinOp("-", Lit(100), d)),
                          BinOp("+", Lit(100), t)))], child)


def batch_bits(batch, name):
    v = batch.validity(name)
    return None if v is None else v.cpu().numpy()


def test_fused_node_equals_stacked_nodes(gq):
    """one node with both Q1 expressions == the three stacked 5-tuple nodes,
    values and bitmaps, bit for bit; a second batch through the same node
    gives the same result; the old form stays on its old kernel."""
    from spark_amd import exec as gx
    n = 3 * T + 17
    rule = gx.GpuColumnarRule()
    names = ["l_quantity", "l_extendedprice", "disc_price", "charge"]

    def run(make, nbatches):
        plan = rule.pre_columnar_transitions(
            make(gx, gx.InputBatches([lineitem_batch(gx, n, 11) for _ in range(nbatches)])))
        assert plan.output == names
        gq.kernel_stats_reset()
        gq.profiling(True)
        try:
            out = list(plan.execute_columnar())
            torch.cuda.synchronize()
            calls = gq.kernel_stats("project_expr")[1]
        finally:
            gq.profiling(False)
            gq.kernel_stats_reset()
        return out, calls

    old, old_calls = run(stacked_q1, 1)
    new, new_calls = run(fused_q1, 2)
    assert old_calls == 0            # 5-tuples: call for call on the old kernel
    assert new_calls == 2            # one fused call per batch
    for batch in new:
        assert list(batch.columns()) == names and batch.num_rows() == n
        for c in names:
            assert torch.equal(batch.column(c), old[0].column(c)), c
            ob, nb = batch_bits(old[0], c), batch_bits(batch, c)
            assert (ob is None) == (nb is None), c
            if ob is not None:
                assert (ob == nb).all(), c
    assert batch_bits(new[0], "charge") is not None
    assert batch_bits(new[0], "disc_price") is None     # nothing in it can be NULL
    ok = np.unpackbits(batch_bits(new[0], "charge"), count=n, bitorder="little")
    assert 0 < ok.sum() < n


def test_node_chunks_past_the_output_cap(gq):
    """six expression entries: more than one call, same answers"""
    from spark_amd import exec as gx
    n = 257
    cols, valid = dev_cols(n)
    names = ["a", "b", "x"]
    batch = gx.ColumnarBatch({c: cols[c].clone() for c in names},
                             validity={c: valid[c].clone() for c in names})
    entries = [("o0", BinOp("+", A, B)), ("o1", Neg(A)), ("o2", Abs(X)),
               ("o3", Coalesce(A, B, 0)), ("o4", flag(Compare(A, "<", B))),
               ("o5", BinOp("*", BinOp("+", A, B), 2))]
    plan = gx.GpuColumnarRule().pre_columnar_transitions(
        gx.ProjectExec(["a"] + entries, gx.InputBatches([batch])))
    (out,) = plan.execute_columnar()
    assert list(out.columns()) == ["a"] + [name for name, _ in entries]
    ref = R.ref_project({c: host_cols(n)[c] for c in names}, entries)
    for name, _ in entries:
        vals, dt = ref[name]
        nullable = any(v is None for v in vals)
        assert_output(name, out.column(name), out.validity(name), vals, dt, n,
                      nullable or out.validity(name) is not None)
    assert out.validity("o3") is None
