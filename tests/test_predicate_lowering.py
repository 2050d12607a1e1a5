"""spark_amd.predicate.lower: predicate trees -> the postfix program of
gpuq_filter_expr. No GPU needed (the module imports no torch).

Besides the instruction sequences themselves, every lowered program is run
through a tiny stack interpreter here and compared with tests/pred_ref.py on
a grid of rows, so a lowering that is well-formed but means something else
fails too.
"""
import itertools
import math

import pytest

import pred_ref as R
from spark_amd import predicate as P
from spark_amd.predicate import (AND, CMP, CMP_COL, CMP_LIT, CONST, FALSE,
                                 IS_NOT_NULL, IS_NULL, NOT, NULL, OR, And,
                                 Between, Cmp, Col, In, Insn, IsNotNull,
                                 IsNull, Not, Or, lower)

SCHEMA = {"a": "int64", "b": "int64", "x": "float64", "y": "float64"}
NAN, INF = float("nan"), float("inf")


def lit(col_idx, op, v):
    if isinstance(v, float):
        return Insn(CMP_LIT, CMP[op], col_idx, 0, 0, v)
    return Insn(CMP_LIT, CMP[op], col_idx, 0, v, float(v))


def run_program(names, prog, row, dtypes):
    """postfix interpreter over one row (name -> value or None)."""
    st = []
    for i in prog:
        if i.opcode == CMP_LIT:
            dt = dtypes[names[i.col_a]]
            v = i.lit_f64 if dt == "f64" else i.lit_i64
            st.append(R._cmp(row[names[i.col_a]], v,
                             list(CMP)[i.cmp], dt))
        elif i.opcode == CMP_COL:
            st.append(R._cmp(row[names[i.col_a]], row[names[i.col_b]],
                             list(CMP)[i.cmp], dtypes[names[i.col_a]]))
        elif i.opcode == IS_NULL:
            st.append(row[names[i.col_a]] is None)
        elif i.opcode == IS_NOT_NULL:
            st.append(row[names[i.col_a]] is not None)
        elif i.opcode == CONST:
            st.append({0: False, 1: True, 2: None}[i.cmp])
        elif i.opcode == AND:
            b, a = st.pop(), st.pop()
            st.append(R.and3(a, b))
        elif i.opcode == OR:
            b, a = st.pop(), st.pop()
            st.append(R.or3(a, b))
        elif i.opcode == NOT:
            st.append(R.not3(st.pop()))
        else:
            raise AssertionError(i)
    assert len(st) == 1
    return st[0]


def test_module_imports_no_torch():
    import subprocess
    import sys
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path.insert(0, %r); import spark_amd.predicate; "
            "assert 'torch' not in sys.modules" % root)
    subprocess.run([sys.executable, "-c", code], check=True)


def test_opcodes_and_caps_mirror_the_header():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    h = open(os.path.join(root, "include", "gpuq.h")).read()
    defs = dict(re.findall(r"#define GPUQ_PRED_(\w+) (\d+)", h))
    for name in ("CMP_LIT", "CMP_COL", "IS_NULL", "IS_NOT_NULL", "CONST",
                 "AND", "OR", "NOT", "FALSE", "TRUE", "NULL", "MAX_INSNS",
                 "MAX_COLS", "MAX_DEPTH"):
        assert int(defs[name]) == getattr(P, name), name


def test_single_leaves():
    assert lower(Cmp("a", "<", 7), SCHEMA) == (["a"], [lit(0, "<", 7)])
    assert lower(Cmp("x", ">=", 2), SCHEMA) == (["x"], [lit(0, ">=", 2.0)])
    assert lower(IsNull("b"), SCHEMA) == (["b"], [Insn(IS_NULL, 0, 0)])
    assert lower(IsNotNull("b"), SCHEMA) == (["b"], [Insn(IS_NOT_NULL, 0, 0)])
    assert lower(Cmp("a", "==", Col("b")), SCHEMA) == \
        (["a", "b"], [Insn(CMP_COL, CMP["=="], 0, 1)])
    assert lower(Cmp("a", "==", None), SCHEMA) == (["a"], [Insn(CONST, NULL)])
    names, prog = lower(Cmp("x", "==", NAN), SCHEMA)
    assert prog[0].opcode == CMP_LIT and math.isnan(prog[0].lit_f64)


def test_between_is_two_leaves_and_an_and():
    assert lower(Between("a", 3, 9), SCHEMA) == \
        (["a"], [lit(0, ">=", 3), lit(0, "<=", 9), Insn(AND)])


def test_in_is_an_or_chain():
    assert lower(In("a", [1, 2, 3]), SCHEMA) == \
        (["a"], [lit(0, "==", 1), lit(0, "==", 2), Insn(OR),
                 lit(0, "==", 3), Insn(OR)])
    assert lower(In("a", [5]), SCHEMA) == (["a"], [lit(0, "==", 5)])
    assert lower(In("a", [4.0]), SCHEMA) == (["a"], [lit(0, "==", 4)])
    # a NULL literal contributes CONST NULL; the empty list is CONST FALSE
    assert lower(In("a", [1, None]), SCHEMA) == \
        (["a"], [lit(0, "==", 1), Insn(CONST, NULL), Insn(OR)])
    assert lower(In("a", []), SCHEMA) == (["a"], [Insn(CONST, FALSE)])


def test_not_in():
    assert lower(Not(In("x", [1.5, None])), SCHEMA) == \
        (["x"], [lit(0, "==", 1.5), Insn(CONST, NULL), Insn(OR), Insn(NOT)])


def test_nary_and_or_fold_left():
    p = And(Cmp("a", ">", 1), Cmp("b", ">", 2), Cmp("x", ">", 3.0))
    assert lower(p, SCHEMA) == \
        (["a", "b", "x"], [lit(0, ">", 1), lit(1, ">", 2), Insn(AND),
                           lit(2, ">", 3.0), Insn(AND)])
    q = Or(Cmp("a", ">", 1), Cmp("b", ">", 2), Cmp("x", ">", 3.0))
    assert [i.opcode for i in lower(q, SCHEMA)[1]] == \
        [CMP_LIT, CMP_LIT, OR, CMP_LIT, OR]
    assert P.stack_depth(lower(p, SCHEMA)[1]) == 2


def test_same_column_leaves_are_adjacent():
    # a .. b .. a .. b -> a a b b (first-occurrence order, stable inside)
    p = And(Cmp("a", ">=", 1), Cmp("b", "<", 24), Cmp("a", "<", 9),
            Not(Cmp("b", "==", 3)))
    names, prog = lower(p, SCHEMA)
    leaves = [(i.col_a, i.cmp) for i in prog if i.opcode == CMP_LIT]
    assert names == ["a", "b"]
    assert leaves == [(0, CMP[">="]), (0, CMP["<"]),
                      (1, CMP["<"]), (1, CMP["=="])]
    # Q6 shape: the shipdate pair and the BETWEEN pair each load once
    q6 = And(Cmp("a", ">=", 100), Between("x", 0.05, 0.07), Cmp("a", "<", 465),
             Cmp("y", "<", 24.0))
    names, prog = lower(q6, SCHEMA)
    cols = [i.col_a for i in prog if i.opcode == CMP_LIT]
    assert names == ["a", "x", "y"] and cols == [0, 0, 1, 1, 2]
    # an operand over two columns stays where it is
    r = Or(Cmp("a", "<", 0), And(Cmp("a", ">", 5), Cmp("b", ">", 5)),
           Cmp("a", "==", 3))
    cols = [i.col_a for i in lower(r, SCHEMA)[1] if i.opcode == CMP_LIT]
    assert cols == [0, 0, 0, 1]


@pytest.mark.parametrize("op", list(CMP))
@pytest.mark.parametrize("literal", [0.5, -0.5, 2.0, -7.25, 1e19, -1e19, 9.3e18,
                                     INF, -INF, NAN, float(1 << 53)])
def test_int_vs_float_literal_uses_filter_cmp_rewrite(op, literal):
    want_op, want_lit = P.rewrite_i64_float_cmp(op, literal)
    assert isinstance(want_lit, int)
    assert lower(Cmp("a", op, literal), SCHEMA) == \
        (["a"], [lit(0, want_op, want_lit)])


def test_rewrite_known_answers():
    rw = P.rewrite_i64_float_cmp
    assert rw("<", 0.5) == ("<=", 0)
    assert rw("<=", 0.5) == ("<=", 0)
    assert rw(">", 0.5) == (">=", 1)
    assert rw(">=", -0.5) == (">=", 0)
    assert rw("==", 0.5) == P.CMP_NONE and rw("!=", 0.5) == P.CMP_ALL
    assert rw("<", 2.0) == ("<", 2)
    assert rw("<", NAN) == P.CMP_ALL and rw(">", NAN) == P.CMP_NONE
    assert rw("<", INF) == P.CMP_ALL and rw(">=", INF) == P.CMP_NONE
    assert rw(">", -INF) == P.CMP_ALL and rw("<", -INF) == P.CMP_NONE
    assert rw("<", 1e19) == P.CMP_ALL and rw(">", 1e19) == P.CMP_NONE
    assert rw(">", -1e19) == P.CMP_ALL and rw("<", -1e19) == P.CMP_NONE
    # "all" / "none" stay comparisons against the column: a NULL row is NULL
    assert P.CMP_ALL == (">=", -(1 << 63)) and P.CMP_NONE == ("<", -(1 << 63))


def test_filter_cmp_uses_the_same_helper():
    gpuq = pytest.importorskip("spark_amd.gpuq")
    assert gpuq.rewrite_i64_float_cmp is P.rewrite_i64_float_cmp
    assert gpuq.CMP is P.CMP


@pytest.mark.parametrize("pred,msg", [
    (Cmp("nope", "<", 1), "unknown column"),
    (IsNull("nope"), "unknown column"),
    (Cmp("a", "<", Col("nope")), "unknown column"),
    (Cmp("a", "<", Col("x")), "dtypes differ"),
    (Cmp("x", "==", Col("b")), "dtypes differ"),
    (Cmp("s", "<", 1), "unsupported"),
    (IsNull("s"), "unsupported"),
    (In("a", [1, 2.5]), "non-integral"),
    (In("a", [NAN]), "non-integral"),
    (In("a", [INF]), "non-integral"),
    (Cmp("a", "<", 1 << 63), "exceeds int64"),
])
def test_lowering_rejects(pred, msg):
    schema = dict(SCHEMA, s="int32")
    with pytest.raises(ValueError, match=msg):
        lower(pred, schema)


def test_bad_operator_and_operands():
    with pytest.raises(ValueError):
        Cmp("a", "<>", 1)
    with pytest.raises(ValueError):
        And()
    with pytest.raises(ValueError):
        Not("a")


def right_nested(nleaves):
    p = Cmp("a", "!=", nleaves)
    for k in range(nleaves - 1, 0, -1):
        p = And(Cmp("a" if k % 2 else "b", "!=", k), p)
    return p


def test_depth_cap():
    names, prog = lower(right_nested(16), SCHEMA)
    assert P.stack_depth(prog) == 16 and len(prog) == 31
    with pytest.raises(ValueError, match="stack depth 17"):
        lower(right_nested(17), SCHEMA)


def test_instruction_cap():
    # left fold: depth 2 whatever the length; 16 leaves + 15 ANDs + NOT = 32
    p32 = Not(And(*[Cmp("a", "!=", k) for k in range(16)]))
    names, prog = lower(p32, SCHEMA)
    assert len(prog) == 32 and P.stack_depth(prog) == 2
    with pytest.raises(ValueError, match="33 instructions"):
        lower(Not(Not(And(*[Cmp("a", "!=", k) for k in range(16)]))), SCHEMA)


def test_column_cap():
    schema = {f"c{k}": "int64" for k in range(9)}
    lower(And(*[IsNotNull(f"c{k}") for k in range(8)]), schema)
    with pytest.raises(ValueError, match="9 columns"):
        lower(And(*[IsNotNull(f"c{k}") for k in range(9)]), schema)


def test_schema_accepts_torch_and_numpy_dtypes():
    np = pytest.importorskip("numpy")
    assert lower(Cmp("k", "<", 1), {"k": np.dtype("int64")})[1] == [lit(0, "<", 1)]
    torch = pytest.importorskip("torch")
    assert lower(Cmp("k", "<", 1), {"k": torch.float64})[1] == [lit(0, "<", 1.0)]


PREDS = [
    Between("a", -1, 1),
    In("a", [0, 2, None]),
    Not(In("a", [0, 2, None])),
    Not(In("x", [0.0, NAN])),
    In("a", []),
    Or(IsNull("a"), Cmp("a", ">", 0.5)),
    And(Cmp("a", ">=", 0), Cmp("x", "<", 1.0), Cmp("a", "<", 2),
        Not(Cmp("x", "==", Col("y")))),
    Or(Cmp("a", "<", Col("b")), And(IsNotNull("x"), Cmp("y", ">=", Col("x")))),
    Not(Or(Cmp("a", "<", -0.5), Cmp("x", ">", NAN), IsNull("y"))),
    right_nested(16),
]


@pytest.mark.parametrize("pred", PREDS, ids=[repr(p)[:60] for p in PREDS])
def test_lowered_program_means_what_the_tree_means(pred):
    dtypes = {"a": "i64", "b": "i64", "x": "f64", "y": "f64"}
    names, prog = lower(pred, SCHEMA)
    ivals = [None, -1, 0, 1, 2]
    fvals = [None, -0.0, 1.0, NAN]
    for a, b, x, y in itertools.product(ivals, ivals, fvals, fvals):
        row = {"a": a, "b": b, "x": x, "y": y}
        assert run_program(names, prog, row, dtypes) is \
            R.eval_row(pred, row, dtypes), row
