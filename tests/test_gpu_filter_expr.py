"""GPU parity for compound WHERE predicates (gpuq_filter_expr, gpuq.filter_expr
and the condition form of FilterExec / GpuFilterExec) against the row-by-row
Kleene evaluator of tests/pred_ref.py. Every comparison is exact: the count,
and the permutation as uint32.

Sizes: 0 and 1; 63 / 64 / 65 (one mask word is 64 rows); 255 / 256 / 257 (one
round of a block); 2047 / 2048 / 2049 (the 2048-row tile of one block); 4097
(three blocks); and BIG = 4096 * 2048 + 1 = 8388609. The emit phase scans one
count per 2048-row tile with exclusive_scan_u32, whose first level scans
SCAN_TILE = 256 * 16 = 4096 counts per block and whose second level (the scan
of the block sums, added back by k_scan_add) only carries a non-zero value
into a second block: that takes 4097 counts, so 4096 * 2048 + 1 rows.

pred_ref is one Python call per row and node, too slow for BIG, so BIG uses
the numpy evaluator np_eval below on a thinned predicate list; np_eval itself
is checked against pred_ref on every predicate at every smaller size, and on
every fuzz tree.
"""
import ctypes
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import pred_ref as R  # noqa: E402
from spark_amd import predicate as P  # noqa: E402
from spark_amd.predicate import (And, Between, Cmp, Col, In, Insn,  # noqa: E402
                                 IsNotNull, IsNull, Not, Or)

SMALL = [0, 1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4097]
BIG = 4096 * 2048 + 1
NAN, INF = float("nan"), float("inf")
DTYPES = {"d": "i64", "a": "i64", "b": "i64", "q": "f64", "disc": "f64",
          "x": "f64", "y": "f64"}
FSPECIAL = np.array([NAN, INF, -INF, -0.0, 0.0, 1.0, -1.0, 2.5])


@pytest.fixture(scope="module")
def gq():
    from spark_amd import gpuq
    assert torch.cuda.is_available()
    return gpuq


# ---------------- data ----------------

@functools.lru_cache(maxsize=None)
def host_cols(n):
    """name -> (values, valid or None, dtype). NULL rows hold values drawn
    like the valid ones (for `a`, always 7, which passes every `a` leaf
    below), so a kernel that ignored validity would let them through."""
    rng = np.random.RandomState(1000 + n % 9973)
    a_valid = rng.rand(n) > 0.25
    a = rng.randint(-3, 9, size=n).astype(np.int64)
    a[~a_valid] = 7
    cols = {
        "d": (rng.randint(200, 900, size=n).astype(np.int64), None),
        "a": (a, a_valid),
        "b": (rng.randint(-3, 9, size=n).astype(np.int64), rng.rand(n) > 0.3),
        "q": (rng.randint(1, 51, size=n).astype(np.float64), rng.rand(n) > 0.25),
        "disc": (rng.randint(0, 11, size=n) / 100.0, None),
        "x": (FSPECIAL[rng.randint(0, len(FSPECIAL), size=n)], rng.rand(n) > 0.2),
        "y": (FSPECIAL[rng.randint(0, len(FSPECIAL), size=n)], rng.rand(n) > 0.2),
    }
    for v, ok in cols.values():
        v.setflags(write=False)
        if ok is not None:
            ok.setflags(write=False)
    return {k: (v, ok, DTYPES[k]) for k, (v, ok) in cols.items()}


def to_dev(a):
    return torch.from_numpy(np.array(a)).cuda()   # a writable copy


def pack_validity(valid_bool):
    return torch.from_numpy(np.packbits(valid_bool, bitorder="little")).cuda()


@functools.lru_cache(maxsize=4)
def dev_cols(n):
    h = host_cols(n)
    return ({k: to_dev(v) for k, (v, _, _) in h.items()},
            {k: pack_validity(ok) for k, (_, ok, _) in h.items() if ok is not None})


# ---------------- numpy evaluator (for BIG) ----------------

def _np_cmp(x, y, op, as_f64):
    """x OP y elementwise under the engine's ordering -> bool array."""
    if as_f64:
        x = np.asarray(x, dtype=np.float64)
        y = np.asarray(y, dtype=np.float64)
        xn, yn = np.isnan(x), np.isnan(y)
        with np.errstate(invalid="ignore"):
            lt = (~xn & yn) | (~xn & ~yn & (x < y))
            eq = (xn & yn) | (x == y)
    else:
        lt, eq = x < y, x == y
    gt = ~(lt | eq)
    return {"==": eq, "<": lt, "<=": lt | eq, ">": gt, ">=": gt | eq,
            "!=": ~eq}[op]


def np_eval(cols, pred, n):
    """-> (is_true, is_null) bool arrays of n rows."""
    def valid(name):
        ok = cols[name][1]
        return np.ones(n, bool) if ok is None else np.asarray(ok)

    def leaf(name, op, rhs):
        vals, _, dt = cols[name]
        if rhs is None:
            return np.zeros(n, bool), np.ones(n, bool)
        ok = valid(name)
        if isinstance(rhs, Col):
            ok = ok & valid(rhs.name)
            t = _np_cmp(vals, cols[rhs.name][0], op, dt == "f64")
        elif dt == "f64" or isinstance(rhs, float):
            t = _np_cmp(vals, np.float64(rhs), op, True)
        else:
            t = _np_cmp(vals, np.int64(rhs), op, False)
        return t & ok, ~ok

    def and_(l, r):
        (lt, ln), (rt, rn) = l, r
        lf, rf = ~lt & ~ln, ~rt & ~rn
        return lt & rt, (ln | rn) & ~(lf | rf)

    def or_(l, r):
        (lt, ln), (rt, rn) = l, r
        t = lt | rt
        return t, (ln | rn) & ~t

    def go(p):
        if isinstance(p, Cmp):
            return leaf(p.col, p.op, p.rhs)
        if isinstance(p, IsNull):
            return ~valid(p.col), np.zeros(n, bool)
        if isinstance(p, IsNotNull):
            return valid(p.col).copy(), np.zeros(n, bool)
        if isinstance(p, Between):
            return and_(leaf(p.col, ">=", p.lo), leaf(p.col, "<=", p.hi))
        if isinstance(p, In):
            out = np.zeros(n, bool), np.zeros(n, bool)
            for v in p.values:
                out = or_(out, leaf(p.col, "==", v))
            return out
        if isinstance(p, (And, Or)):
            out = go(p.ps[0])
            for q in p.ps[1:]:
                out = (and_ if isinstance(p, And) else or_)(out, go(q))
            return out
        if isinstance(p, Not):
            t, nl = go(p.p)
            return ~t & ~nl, nl
        raise ValueError(p)

    return go(pred)


@functools.lru_cache(maxsize=None)
def reference(n, case_id):
    """-> (list of True/False/None per row, passing rows uint32), computed
    once per (size, predicate) and shared."""
    pred = CASES[case_id][0]
    if n == BIG:
        t, nl = np_eval(host_cols(n), pred, n)
        tv = None
    else:
        tv = R.ref_eval(host_cols(n), pred)
        t = np.array([v is True for v in tv], dtype=bool)
        nl = np.array([v is None for v in tv], dtype=bool)
    rows = np.flatnonzero(t).astype(np.uint32)
    rows.setflags(write=False)
    return t, nl, rows


# ---------------- predicates ----------------

def right_nested(nleaves):
    """l1 AND (l2 AND (... AND l_n)): evaluation depth n."""
    leaves = [Cmp("a", "!=", -3), Cmp("b", "!=", -3), Cmp("x", "!=", -1.0),
              Cmp("y", "!=", 2.5), Cmp("d", "!=", 5), Cmp("q", "!=", 3.0)]
    p = leaves[(nleaves - 1) % len(leaves)]
    for k in range(nleaves - 2, -1, -1):
        p = And(leaves[k % len(leaves)], p)
    return p


# id -> (predicate, the outcomes it can produce among T / F / N, runs at BIG);
# in_null is never FALSE (a miss against a list with a NULL is NULL) and
# not_in_null never TRUE
CASES = {
    "leaf_i64": (Cmp("a", ">", 5), "TFN", True),
    "leaf_i64_frac": (Cmp("b", "<", 0.5), "TFN", False),
    "leaf_f64": (Cmp("x", ">=", 1.0), "TFN", True),
    "leaf_f64_nan": (Cmp("y", "==", NAN), "TFN", False),
    "leaf_nonnull": (Cmp("d", "<", 400), "TF", False),
    "q6": (And(Cmp("d", ">=", 365), Cmp("d", "<", 730),
               Between("disc", 0.05, 0.07), Cmp("q", "<", 24.0)), "TFN", True),
    "or_two_nullable": (Or(Cmp("a", ">", 5), Cmp("b", "<", 3)), "TFN", True),
    "not_cmp": (Not(Cmp("b", ">", 5)), "TFN", False),
    "in_null": (In("a", [1, 7, None]), "TN", False),
    "in_plain": (In("x", [0.0, NAN, 2.5]), "TFN", False),
    "not_in": (Not(In("b", [0, 1, 2, 3])), "TFN", False),
    "not_in_null": (Not(In("b", [0, 1, 2, 3, 4, 5, 6, None])), "FN", False),
    "isnull_or_cmp": (Or(IsNull("a"), Cmp("a", ">", 5)), "TF", True),
    "isnotnull_and": (And(IsNotNull("x"), Cmp("y", "<", 0.0)), "TFN", False),
    "colcol_i64": (Cmp("a", "<=", Col("b")), "TFN", True),
    "colcol_f64_eq": (Cmp("x", "==", Col("y")), "TFN", True),
    "colcol_f64_lt": (Cmp("x", "<", Col("y")), "TFN", False),
    "colcol_f64_ne": (Not(Cmp("y", "!=", Col("x"))), "TFN", False),
    "depth16": (right_nested(16), "TFN", True),
    "insns32": (Not(And(*[Cmp("a" if k % 2 else "b", "!=", k - 4)
                          for k in range(16)])), "TFN", False),
    "mixed": (Or(And(Cmp("a", "<", Col("b")), Not(IsNull("x"))),
                 And(Between("q", 10.0, 20.0), In("d", [201, 202, 203, 500, None])),
                 Cmp("y", ">", INF)), "TFN", False),
}
# CONST-only programs, given pre-lowered: all rows, none, NULL
CONST_PROGS = {"const_true": ([], [Insn(P.CONST, P.TRUE)], "all"),
               "const_false": ([], [Insn(P.CONST, P.FALSE)], "none"),
               "const_null": ([], [Insn(P.CONST, P.NULL)], "none"),
               "in_empty": (None, In("a", []), "none"),
               "not_in_empty": (None, Not(In("a", [])), "all"),
               "in_only_null": (None, In("a", [None]), "none"),
               "const_and_leaf": (["a"], [Insn(P.CONST, P.NULL),
                                         Insn(P.CMP_LIT, P.CMP[">"], 0, 0, 5, 5.0),
                                         Insn(P.OR)], "a>5")}


def seen(t, nl):
    """which of TRUE / FALSE / NULL occur, as a string like 'TFN'"""
    return ("T" if t.any() else "") + ("F" if (~t & ~nl).any() else "") \
        + ("N" if nl.any() else "")


def perm_u32(perm):
    return perm.cpu().numpy().view(np.uint32)


def run(gq, n, pred):
    cols, valid = dev_cols(n)
    perm, cnt = gq.filter_expr(cols, pred, validities=valid)
    assert perm.numel() == cnt
    return perm_u32(perm), cnt


def test_program_shapes():
    """the two cap cases are what they claim to be"""
    schema = {k: ("int64" if v == "i64" else "float64") for k, v in DTYPES.items()}
    _, prog = P.lower(CASES["depth16"][0], schema)
    assert P.stack_depth(prog) == 16
    _, prog = P.lower(CASES["insns32"][0], schema)
    assert len(prog) == 32


@pytest.mark.parametrize("case_id", list(CASES))
@pytest.mark.parametrize("n", SMALL)
def test_parity_small(gq, n, case_id):
    pred, outcomes, _ = CASES[case_id]
    t, nl, want = reference(n, case_id)
    # the numpy evaluator BIG relies on agrees with pred_ref here
    nt, nn = np_eval(host_cols(n), pred, n)
    assert (nt == t).all() and (nn == nl).all()
    if n >= 64:   # non-vacuity: every outcome the predicate can produce
        assert seen(t, nl) == outcomes, case_id
    got, cnt = run(gq, n, pred)
    assert cnt == len(want)
    assert (got == want).all()


@pytest.mark.parametrize("case_id", [c for c in CASES if "N" in CASES[c][1]
                                     and "T" in CASES[c][1]])
@pytest.mark.parametrize("n", [256, 2049])
def test_data_punishes_ignoring_validity(n, case_id):
    """dropping the bitmaps changes the answer: the NULL rows matter"""
    t, _, _ = reference(n, case_id)
    bare = {k: (v, None, dt) for k, (v, _, dt) in host_cols(n).items()}
    bt, _ = np_eval(bare, CASES[case_id][0], n)
    assert (bt != t).any()


@pytest.mark.parametrize("case_id", [c for c in CASES if CASES[c][2]])
def test_parity_big(gq, case_id):
    t, nl, want = reference(BIG, case_id)
    assert seen(t, nl) == CASES[case_id][1]
    got, cnt = run(gq, BIG, CASES[case_id][0])
    assert cnt == len(want)
    assert (got == want).all()


@pytest.mark.parametrize("n", [0, 1, 65, 2049])
@pytest.mark.parametrize("name", list(CONST_PROGS))
def test_const_programs(gq, n, name):
    names, prog, want = CONST_PROGS[name]
    pred = prog if names is None else (names, prog)
    got, cnt = run(gq, n, pred)
    if want == "all":
        exp = np.arange(n, dtype=np.uint32)
    elif want == "none":
        exp = np.zeros(0, dtype=np.uint32)
    else:   # NULL OR a > 5: TRUE where a > 5, NULL elsewhere
        exp = reference(n, "leaf_i64")[2]
    assert cnt == len(exp) and (got == exp).all()


@pytest.mark.parametrize("n", [1, 65, 2049, 4097])
@pytest.mark.parametrize("case_id,col,op,lit", [
    ("leaf_i64", "a", ">", 5), ("leaf_i64_frac", "b", "<", 0.5),
    ("leaf_f64", "x", ">=", 1.0), ("leaf_f64_nan", "y", "==", NAN),
    ("leaf_nonnull", "d", "<", 400)])
def test_single_leaf_equals_filter_cmp(gq, n, case_id, col, op, lit):
    cols, valid = dev_cols(n)
    old, old_cnt = gq.filter_cmp(cols[col], op, lit, validity=valid.get(col))
    got, cnt = run(gq, n, CASES[case_id][0])
    assert cnt == old_cnt == len(reference(n, case_id)[2])
    assert (got == perm_u32(old)).all()


def test_inputs_not_written_and_workspace_reuse(gq):
    n = 4097
    cols, valid = dev_cols(n)
    before = {k: t.clone() for k, t in cols.items()}
    ws = gq.filter_expr_workspace(n)
    for case_id in ("q6", "colcol_f64_eq", "q6"):
        perm, cnt = gq.filter_expr(cols, CASES[case_id][0], validities=valid,
                                   workspace=ws)
        assert (perm_u32(perm) == reference(n, case_id)[2]).all()
    for k, t in cols.items():
        assert torch.equal(t.view(torch.int64), before[k].view(torch.int64))


# ---------------- seeded fuzz ----------------

ICOLS, FCOLS = ["d", "a", "b"], ["q", "disc", "x", "y"]


def leaf_kinds(p, out):
    """collect the kinds of leaves in a tree"""
    if isinstance(p, (And, Or)):
        for q in p.ps:
            leaf_kinds(q, out)
    elif isinstance(p, Not):
        leaf_kinds(p.p, out)
    elif isinstance(p, Cmp):
        out.add("CmpCol" if isinstance(p.rhs, Col) else "CmpLit")
    else:
        out.add(type(p).__name__)
    return out


def random_tree(rng, depth, names):
    def leaf():
        c = names[rng.randint(len(names))]
        isf = c in FCOLS
        kind = rng.randint(6)
        same = [o for o in names if o != c and (o in FCOLS) == isf]
        if isf:
            lit = [float(FSPECIAL[rng.randint(len(FSPECIAL))]),
                   float(rng.randint(0, 50)), rng.randint(0, 11) / 100.0][rng.randint(3)]
        else:
            lit = [int(rng.randint(-3, 9)), int(rng.randint(200, 900)),
                   float(rng.randint(-6, 18)) / 2][rng.randint(3)]
        op = list(P.CMP)[rng.randint(6)]
        if kind == 0:
            return IsNull(c)
        if kind == 1:
            return IsNotNull(c)
        if kind == 2 and same:
            return Cmp(c, op, Col(same[rng.randint(len(same))]))
        if kind == 3:
            vals = [float(v) if isf else int(v)
                    for v in rng.randint(-3, 9, size=rng.randint(0, 4))]
            if rng.rand() < 0.3:
                vals.append(None)
            return In(c, vals)
        if kind == 4:
            lo = float(rng.randint(-3, 5)) if isf else int(rng.randint(-3, 5))
            return Between(c, lo, lo + int(rng.randint(0, 400)))
        return Cmp(c, op, lit)

    def node(d):
        if d == 0 or rng.rand() < 0.25:
            return leaf()
        k = rng.randint(4)
        if k == 0:
            return Not(node(d - 1))
        parts = [node(d - 1) for _ in range(rng.randint(2, 4))]
        return (And if k % 2 else Or)(*parts)

    return node(depth)


@pytest.mark.parametrize("chunk", range(8))
def test_fuzz(gq, chunk):
    """200 random trees in 8 chunks of 25: depth up to 6 over 1-4 columns of
    mixed dtype and NULL density, at sizes from the small list."""
    rng = np.random.RandomState(4242 + chunk)
    schema = {k: ("int64" if v == "i64" else "float64") for k, v in DTYPES.items()}
    done, kinds = 0, set()
    while done < 25:
        names = [str(c) for c in rng.choice(list(DTYPES), size=rng.randint(1, 5),
                                            replace=False)]
        pred = random_tree(rng, rng.randint(1, 7), names)
        try:
            P.lower(pred, schema)
        except ValueError:      # over a cap: draw again
            continue
        n = SMALL[rng.randint(len(SMALL))]
        tv = R.ref_eval(host_cols(n), pred)
        want = np.array([i for i, v in enumerate(tv) if v is True], dtype=np.uint32)
        nt, nn = np_eval(host_cols(n), pred, n)
        assert nt.tolist() == [v is True for v in tv], pred
        assert nn.tolist() == [v is None for v in tv], pred
        got, cnt = run(gq, n, pred)
        assert cnt == len(want), pred
        assert (got == want).all(), pred
        leaf_kinds(pred, kinds)
        done += 1
    assert kinds == {"CmpLit", "CmpCol", "IsNull", "IsNotNull", "In", "Between"}


# ---------------- ABI errors ----------------

def _insns(gq, items):
    return (gq._PredInsn * len(items))(*[gq._PredInsn(*i) for i in items])


LEAF = Insn(P.CMP_LIT, 0, 0, 0, 1, 1.0)
K = Insn(P.CONST, P.TRUE)
BAD_PROGRAMS = {
    "no_insns": [],
    "too_many_insns": [K] + [K, Insn(P.AND)] * 16,                  # 33
    "opcode_high": [Insn(8)],
    "opcode_negative": [Insn(-1)],
    "cmp_code": [Insn(P.CMP_LIT, 6, 0)],
    "cmp_code_col": [Insn(P.CMP_COL, -1, 0, 1)],
    "const_value": [Insn(P.CONST, 3)],
    "col_a_range": [Insn(P.CMP_LIT, 0, 3)],
    "col_a_negative": [Insn(P.IS_NULL, 0, -1)],
    "col_b_range": [Insn(P.CMP_COL, 0, 0, 3)],
    "cmp_col_dtypes": [Insn(P.CMP_COL, 0, 0, 2)],                   # i64 vs f64
    "underflow_and": [LEAF, Insn(P.AND)],
    "underflow_not": [Insn(P.NOT)],
    "depth_17": [K] * 17 + [Insn(P.AND)] * 15,                      # 32 insns
    "ends_at_2": [LEAF, LEAF],
}


def test_abi_errors(gq):
    n = 100
    L = gq.lib()
    a = torch.arange(n, dtype=torch.int64, device="cuda")
    f = torch.zeros(n, dtype=torch.float64, device="cuda")
    i32 = torch.zeros(n, dtype=torch.int32, device="cuda")
    cols3 = (gq._Col * 3)(gq._col(a), gq._col(a), gq._col(f))
    ws = gq.filter_expr_workspace(n)
    perm = torch.empty(n, dtype=torch.int32, device="cuda")
    cnt = torch.full((1,), -5, dtype=torch.int64, device="cuda")

    def call(nrows, cols, ncols, items, ws_bytes=ws.numel()):
        prog = _insns(gq, items or [K])
        return L.gpuq_filter_expr(gq._stream(), nrows, cols, ncols, prog,
                                  len(items), perm.data_ptr(), cnt.data_ptr(),
                                  ws.data_ptr(), ws_bytes)

    def rejected(rc, what):
        assert rc == 2, what
        assert L.gpuq_last_error().decode().startswith("filter_expr:"), what

    for name, items in BAD_PROGRAMS.items():
        rejected(call(n, cols3, 3, items), name)
    rejected(call(0x100000000, cols3, 3, [LEAF]), "nrows over 2^32 - 1")
    rejected(call(n, cols3, 9, [LEAF]), "nine columns")
    rejected(call(n, cols3, -1, [LEAF]), "negative column count")
    bad = (gq._Col * 1)(gq._col(i32))
    rejected(call(n, bad, 1, [LEAF]), "int32 column")
    rejected(call(n, cols3, 3, [LEAF], ws_bytes=ws.numel() - 1), "short workspace")
    assert L.gpuq_filter_expr_workspace_bytes(n) == ws.numel() > 0
    torch.cuda.synchronize()
    assert int(cnt.item()) == -5          # nothing was launched or written

    # a valid call right after: a == 1 on a = 0..99
    assert call(n, cols3, 3, [LEAF]) == 0
    assert int(cnt.item()) == 1 and perm_u32(perm)[0] == 1
    # largest legal programs at the ABI: 32 instructions, depth 16
    assert call(n, cols3, 3, [K] * 16 + [Insn(P.AND)] * 15 + [Insn(P.NOT)]) == 0
    assert int(cnt.item()) == 0
    assert call(0, cols3, 3, [LEAF]) == 0
    assert int(cnt.item()) == 0


# ---------------- exec nodes ----------------

def batch_of(gx, n, names):
    cols, valid = dev_cols(n)
    return gx.ColumnarBatch({k: cols[k].clone() for k in names},
                            validity={k: valid[k].clone() for k in names
                                      if k in valid})


def batch_to_rows(batch, names):
    """device batch -> one list per column, None where the bitmap says NULL"""
    n = batch.num_rows()
    out = []
    for name in names:
        data = batch.column(name).cpu().numpy()
        v = batch.validity(name)
        ok = (np.unpackbits(v.cpu().numpy(), count=n, bitorder="little")
              .astype(bool) if v is not None else np.ones(n, bool))
        out.append([x if o else None for x, o in zip(data.view(np.int64).tolist(), ok)])
    return out


def ref_rows(n, names, rows):
    h = host_cols(n)
    out = []
    for name in names:
        v, ok, _ = h[name]
        bits = v.view(np.int64)
        out.append([int(bits[i]) if ok is None or ok[i] else None for i in rows])
    return out


@pytest.mark.parametrize("sizes", [(2049,), (257, 4097)])
def test_filter_exec_condition(gq, sizes):
    from spark_amd import exec as gx
    names = ["d", "a", "q", "x", "y"]     # a, q, x, y carry bitmaps
    pred = Or(And(Cmp("d", ">=", 365), Cmp("q", "<", 24.0)),
              Cmp("x", "==", Col("y")), IsNull("a"))
    plan = gx.FilterExec(pred, gx.InputBatches([batch_of(gx, n, names) for n in sizes]))
    assert plan.col is None and plan.condition is pred
    gpu = gx.GpuColumnarRule().pre_columnar_transitions(plan)
    assert isinstance(gpu, gx.GpuFilterExec) and gpu.condition is pred
    assert gpu.output == names
    out = list(gpu.execute_columnar())
    assert len(out) == len(sizes)
    for n, batch in zip(sizes, out):
        rows = R.ref_filter_expr({k: host_cols(n)[k] for k in names}, pred)
        assert 0 < len(rows) < n
        assert batch.num_rows() == len(rows)
        # values compare as raw 64-bit patterns (NaN and -0.0 included)
        assert batch_to_rows(batch, names) == ref_rows(n, names, rows)


def test_filter_exec_nothing_passes(gq):
    from spark_amd import exec as gx
    names = ["a", "x"]
    plan = gx.FilterExec(In("a", [None]), gx.InputBatches([batch_of(gx, 257, names)]))
    (batch,) = gx.GpuColumnarRule().pre_columnar_transitions(plan).execute_columnar()
    assert batch.num_rows() == 0 and list(batch.columns()) == names


def test_rule_keeps_the_old_form_on_the_old_path(gq):
    from spark_amd import exec as gx
    names = ["d", "a"]

    def tags(plan):
        gpu = gx.GpuColumnarRule().pre_columnar_transitions(plan)
        gq.kernel_stats_reset()
        gq.profiling(True)
        try:
            list(gpu.execute_columnar())
            torch.cuda.synchronize()
            return {t: gq.kernel_stats(t)[1]
                    for t in ("filter_pred", "filter_scatter",
                              "filter_expr_mask", "filter_expr_emit")}
        finally:
            gq.profiling(False)
            gq.kernel_stats_reset()

    old = gx.FilterExec("d", "<", 400, gx.InputBatches([batch_of(gx, 2049, names)]))
    assert (old.col, old.op, old.literal, old.condition) == ("d", "<", 400, None)
    assert tags(old) == {"filter_pred": 1, "filter_scatter": 1,
                         "filter_expr_mask": 0, "filter_expr_emit": 0}
    new = gx.FilterExec(Cmp("d", "<", 400),
                        gx.InputBatches([batch_of(gx, 2049, names)]))
    assert tags(new) == {"filter_pred": 0, "filter_scatter": 0,
                         "filter_expr_mask": 1, "filter_expr_emit": 1}


def test_and_equals_stacked_filters(gq):
    """o_orderdate >= d0 AND o_orderdate < d1, as the Q5 test stacks it"""
    from spark_amd import exec as gx
    names = ["d", "a", "x"]
    d0, d1 = 365, 730
    rule = gx.GpuColumnarRule()
    stacked = rule.pre_columnar_transitions(gx.FilterExec(
        "d", "<", d1, gx.FilterExec("d", ">=", d0,
                                    gx.InputBatches([batch_of(gx, 4097, names)]))))
    fused = rule.pre_columnar_transitions(gx.FilterExec(
        And(Cmp("d", ">=", d0), Cmp("d", "<", d1)),
        gx.InputBatches([batch_of(gx, 4097, names)])))
    assert isinstance(stacked.children[0], gx.GpuFilterExec)   # not merged
    assert isinstance(fused.children[0], gx.InputBatches)
    (sb,), (fb,) = stacked.execute_columnar(), fused.execute_columnar()
    assert 0 < fb.num_rows() < 4097
    assert batch_to_rows(sb, names) == batch_to_rows(fb, names)


def test_output_ordering_passes_through(gq):
    from spark_amd import exec as gx
    order = gx.SortOrder("d")
    plan = gx.FilterExec(Cmp("a", ">", 5), gx.SortExec(
        order, False, gx.InputBatches([batch_of(gx, 65, ["d", "a"])])))
    gpu = gx.GpuColumnarRule().pre_columnar_transitions(plan)
    assert gpu.output_ordering == gpu.children[0].output_ordering
    assert [o.key for o in gpu.output_ordering] == ["d"]
    assert gpu.output == ["d", "a"]
