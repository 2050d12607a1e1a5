"""Lowering of SELECT-list expression trees (spark_amd.expression) to the
postfix program of gpuq_project_expr: the programs themselves, the depth of a
CASE chain, every refusal, the static nullability, and an independent stack /
type simulation every lowered program must pass. No GPU, no torch."""
import numpy as np
import pytest

from expr_gen import random_expr
from spark_amd import expression as E
from spark_amd.expression import (Abs, BinOp, CaseWhen, Cast, Coalesce,
                                  Compare, If, Insn, Lit, Neg)
from spark_amd.predicate import (And, Between, Cmp, Col, In, IsNotNull,
                                 IsNull, Not, Or)

SCHEMA = {"ep": "int64", "d": "int64", "t": "int64", "i": "int64",
          "j": "int64", "x": "float64", "y": "float64"}
I64, F64, BOOL = E.I64, E.F64, E.BOOL


def q1_outputs():
    disc_price = BinOp("*", Col("ep"), BinOp("-", Lit(100), Col("d")))
    charge = BinOp("*", BinOp("*", Col("ep"), BinOp("-", Lit(100), Col("d"))),
                   BinOp("+", Lit(100), Col("t")))
    return [("disc_price", disc_price), ("charge", charge)]


# ---------------- an independent simulation ----------------

def simulate(cols, prog, out_dtypes, schema):
    """Type-checks a program the way the header states the rules, written
    apart from both the lowering and the C entry point. Returns the peak
    depth."""
    code = {"int64": I64, "float64": F64}
    stack, written, peak = [], set(), 0
    for pc, ins in enumerate(prog):
        op, arg, dt = ins.opcode, ins.arg, ins.dtype
        where = f"insn {pc} {ins!r}"
        if op == E.COL:
            assert 0 <= arg < len(cols), where
            assert dt == code[schema[cols[arg]]], where
            stack.append(dt)
        elif op == E.LIT:
            assert arg in (0, 1) and dt in (I64, F64, BOOL), where
            if dt == I64:
                assert -(1 << 63) <= ins.lit_i64 < (1 << 63), where
            stack.append(dt)
        elif op == E.REF:
            assert arg in written, where
            assert dt == E.TYPE_CODE[out_dtypes[arg]], where
            stack.append(dt)
        elif op in (E.ARITH, E.CMP_OP):
            b, a = stack.pop(), stack.pop()
            assert a == b == dt and dt != BOOL, where
            assert 0 <= arg <= (3 if op == E.ARITH else 5), where
            stack.append(dt if op == E.ARITH else BOOL)
        elif op in (E.NEG, E.ABS):
            assert stack[-1] == dt != BOOL, where
        elif op == E.CAST:
            assert stack.pop() == dt, where
            assert (dt, arg) in ((I64, F64), (F64, I64), (BOOL, I64)), where
            stack.append(arg)
        elif op in (E.IS_NULL, E.IS_NOT_NULL):
            assert stack.pop() == dt, where
            stack.append(BOOL)
        elif op in (E.AND, E.OR):
            assert stack.pop() == BOOL and stack.pop() == BOOL and dt == BOOL, where
            stack.append(BOOL)
        elif op == E.NOT:
            assert stack[-1] == BOOL and dt == BOOL, where
        elif op == E.SELECT:
            cond, then, els = stack.pop(), stack.pop(), stack.pop()
            assert cond == BOOL and then == els == dt, where
            stack.append(dt)
        elif op == E.COALESCE:
            b, a = stack.pop(), stack.pop()
            assert a == b == dt, where
            stack.append(dt)
        elif op == E.OUT:
            assert arg not in written and 0 <= arg < len(out_dtypes), where
            assert stack.pop() == dt == E.TYPE_CODE[out_dtypes[arg]] != BOOL, where
            written.add(arg)
        else:
            raise AssertionError(where)
        peak = max(peak, len(stack))
    assert not stack and written == set(range(len(out_dtypes)))
    assert peak <= E.MAX_DEPTH and len(prog) <= E.MAX_INSNS
    assert len(cols) <= E.MAX_COLS
    return peak


def lower_ok(outputs, nullable=None):
    cols, prog, dts, nls = E.lower(outputs, SCHEMA, nullable)
    peak = simulate(cols, prog, dts, SCHEMA)
    assert peak == E.stack_depth(prog)
    return cols, prog, dts, nls


# ---------------- programs ----------------

def test_q1_program():
    cols, prog, dts, nls = lower_ok(q1_outputs(), nullable=["t"])
    assert cols == ["ep", "d", "t"]
    assert dts == ["i64", "i64"] and nls == [False, True]
    assert prog == [
        Insn(E.COL, 0, I64), Insn(E.LIT, 0, I64, 0, 100),
        Insn(E.COL, 1, I64), Insn(E.ARITH, 1, I64), Insn(E.ARITH, 2, I64),
        Insn(E.OUT, 0, I64),
        Insn(E.REF, 0, I64), Insn(E.LIT, 0, I64, 0, 100),
        Insn(E.COL, 2, I64), Insn(E.ARITH, 0, I64), Insn(E.ARITH, 2, I64),
        Insn(E.OUT, 1, I64)]
    assert E.stack_depth(prog) == 3


def test_ref_needs_the_whole_earlier_tree():
    a = BinOp("+", Col("i"), Col("j"))
    outs = [("s", a), ("u", BinOp("*", BinOp("+", Col("i"), Col("j")), 2)),
            ("v", BinOp("+", Col("j"), Col("i")))]        # not the same tree
    _, prog, _, _ = lower_ok(outs)
    assert [i.arg for i in prog if i.opcode == E.REF] == [0]
    # a bare column or literal output is never a REF target
    _, prog, _, _ = lower_ok([("c", Col("i")), ("e", BinOp("+", Col("i"), 1))])
    assert not [i for i in prog if i.opcode == E.REF]


def test_case_chain_folds_at_constant_depth():
    def arm(k, deep):
        v = Col("i")
        for _ in range(deep):
            v = BinOp("+", Lit(k), v)         # literal first: one level each
        return Compare(Col("j"), "==", k), v

    for deep in (0, 1, 3):
        cw = CaseWhen([arm(k, deep if k == 2 else 0) for k in range(5)],
                      else_=Lit(0))
        arm_depth = 1 + deep
        _, prog, _, _ = lower_ok([("c", cw)])
        assert E.stack_depth(prog) <= 3 + arm_depth
        assert sum(i.opcode == E.SELECT for i in prog) == 5
    # else-first: the program starts with the ELSE value
    _, prog, _, _ = lower_ok([("c", CaseWhen([(IsNull("i"), Lit(1))], else_=Lit(77)))])
    assert prog[0] == Insn(E.LIT, 0, I64, 0, 77)
    # without else_: the typed NULL literal
    _, prog, dts, nls = lower_ok([("c", CaseWhen([(IsNull("x"), Col("y"))]))])
    assert prog[0] == Insn(E.LIT, 1, F64) and dts == ["f64"] and nls == [True]


def test_literal_typing():
    _, prog, dts, _ = lower_ok([("a", BinOp("+", Col("x"), 1))])
    assert dts == ["f64"] and Insn(E.LIT, 0, F64, 0, 0, 1.0) in prog
    _, prog, dts, _ = lower_ok([("a", BinOp("+", Col("i"), 2.0))])
    assert dts == ["i64"] and Insn(E.LIT, 0, I64, 0, 2) in prog
    _, prog, dts, _ = lower_ok([("a", Coalesce(Col("i"), Col("j"), 0))])
    assert dts == ["i64"] and sum(i.opcode == E.COALESCE for i in prog) == 2
    _, _, dts, _ = lower_ok([("a", Lit(3)), ("b", Lit(2.5)), ("c", Lit(None, "f64"))])
    assert dts == ["i64", "f64", "f64"]
    # int64 column against a float literal: rewritten, never truncated
    _, prog, _, _ = lower_ok([("a", Cast(Compare(Col("i"), "<", 0.5), "i64"))])
    assert prog[1:3] == [Insn(E.LIT, 0, I64, 0, 0), Insn(E.CMP_OP, 2, I64)]
    _, prog, _, _ = lower_ok([("a", Cast(Compare(0.5, "<", Col("i")), "i64"))])
    assert prog[1:3] == [Insn(E.LIT, 0, I64, 0, 1), Insn(E.CMP_OP, 4, I64)]
    _, prog, _, _ = lower_ok([("a", Cast(Cmp("i", ">", 2.5), "i64"))])
    assert prog[1:3] == [Insn(E.LIT, 0, I64, 0, 3), Insn(E.CMP_OP, 4, I64)]


BAD = {
    "nonintegral_beside_i64": [("a", BinOp("+", Col("i"), 0.5))],
    "nan_beside_i64": [("a", BinOp("*", Col("i"), float("nan")))],
    "inexact_int_beside_f64": [("a", BinOp("+", Col("x"), (1 << 53) + 1))],
    "int_beyond_i64": [("a", BinOp("+", Col("i"), 1 << 63))],
    "two_dtypes_binop": [("a", BinOp("+", Col("i"), Col("x")))],
    "two_dtypes_compare": [("a", Cast(Compare(Col("i"), "<", Col("x")), "i64"))],
    "two_dtypes_cmp_cols": [("a", Cast(Cmp("i", "<", Col("x")), "i64"))],
    "two_dtypes_if": [("a", If(IsNull("i"), Col("i"), Col("x")))],
    "two_dtypes_case": [("a", CaseWhen([(IsNull("i"), Col("i"))], else_=Col("x")))],
    "two_dtypes_coalesce": [("a", Coalesce(Col("i"), Col("x")))],
    "typed_literal_mismatch": [("a", BinOp("+", Col("i"), Lit(1.0, "f64")))],
    "bool_output": [("a", Compare(Col("i"), "<", Col("j")))],
    "bool_output_pred": [("a", IsNull("i"))],
    "bool_operand": [("a", BinOp("+", Col("i"), Compare(Col("i"), "<", 1)))],
    "bool_to_f64": [("a", Cast(IsNull("i"), "f64"))],
    "unknown_column": [("a", BinOp("+", Col("nope"), 1))],
    "unknown_column_pred": [("a", Cast(IsNull("nope"), "i64"))],
    "untyped_null": [("a", Lit(None))],
    "in_nonintegral": [("a", Cast(In("i", [1, 2.5]), "i64"))],
    "too_many_outputs": [(f"o{k}", Col("i")) for k in range(5)],
    "no_outputs": [],
    "too_many_insns": [("a", Coalesce(*([Col("i")] * 25)))],      # 25 + 24 + OUT
    "too_deep": [("a", BinOp("+", Lit(1), BinOp("+", Lit(1), BinOp("+", Lit(1), BinOp(
        "+", Lit(1), BinOp("+", Lit(1), BinOp("+", Lit(1), BinOp("+", Lit(1), BinOp(
            "+", Lit(1), Col("i"))))))))))],                      # depth 9
}


@pytest.mark.parametrize("name", list(BAD))
def test_refusals(name):
    with pytest.raises(ValueError):
        E.lower(BAD[name], SCHEMA)


def test_too_many_columns():
    schema = {f"c{k}": "int64" for k in range(9)}
    e = Col("c0")
    for k in range(1, 9):
        e = BinOp("+", e, Col(f"c{k}"))
    with pytest.raises(ValueError, match="columns"):
        E.lower([("a", e)], schema)
    with pytest.raises(ValueError, match="unsupported"):
        E.lower([("a", Col("c"))], {"c": "int32"})
    for ctor in (lambda: BinOp("%", 1, 2), lambda: Compare(1, "~", 2),
                 lambda: Cast(Col("i"), "i32"), lambda: Lit("s"),
                 lambda: If(Col("i"), 1, 2), lambda: Coalesce(),
                 lambda: CaseWhen([])):
        with pytest.raises(ValueError):
            ctor()


def test_caps_exactly():
    # 24 operands: 24 pushes + 23 COALESCE + OUT = 48 instructions
    _, prog, _, _ = lower_ok([("a", Coalesce(*([Col("i")] * 24)))])
    assert len(prog) == E.MAX_INSNS
    e = Col("i")
    for _ in range(7):
        e = BinOp("+", Lit(1), e)
    _, prog, _, _ = lower_ok([("a", e)])
    assert E.stack_depth(prog) == E.MAX_DEPTH
    _, _, dts, _ = lower_ok([(f"o{k}", Neg(Col("i"))) for k in range(4)])
    assert len(dts) == E.MAX_OUTS


# ---------------- static nullability ----------------

def nl(e, nullable):
    return lower_ok([("a", e)], nullable)[3][0]


def test_out_nullable_rules():
    N = ["i", "x"]                       # i and x carry bitmaps, j and y do not
    assert nl(Col("i"), N) and not nl(Col("j"), N)
    assert nl(Col("j"), None)            # unknown: every column may
    assert nl(Lit(None, "i64"), N) and not nl(Lit(3), N)
    assert nl(BinOp("+", Col("i"), Col("j")), N)
    assert not nl(BinOp("*", Col("j"), 2), N)
    assert nl(BinOp("/", Col("j"), 2), N)                       # any divide
    assert nl(Neg(Col("i")), N) and not nl(Abs(Col("y")), N)
    assert nl(Cast(Col("x"), "i64"), N) and not nl(Cast(Col("j"), "f64"), N)
    assert nl(Cast(Compare(Col("i"), "<", Col("j")), "i64"), N)
    assert not nl(Cast(Compare(Col("j"), "<", 3), "i64"), N)
    assert nl(Cast(Cmp("j", "<", None), "i64"), N)
    assert nl(Cast(And(Cmp("j", "<", 1), Cmp("i", "<", 1)), "i64"), N)
    assert not nl(Cast(Or(Cmp("j", "<", 1), Cmp("y", "<", 1.0)), "i64"), N)
    assert nl(Cast(Not(Cmp("x", "<", 1.0)), "i64"), N)
    assert not nl(Cast(IsNull("i"), "i64"), N)
    assert not nl(Cast(IsNotNull("x"), "i64"), N)
    assert nl(Cast(In("j", [1, None]), "i64"), N)
    assert not nl(Cast(In("j", [1, 2]), "i64"), N)
    assert not nl(Cast(In("i", []), "i64"), N)
    assert nl(Cast(Between("i", 1, 2), "i64"), N)
    # If / CaseWhen: the value branches decide, not the condition
    assert not nl(If(Cmp("i", "<", 1), Col("j"), Lit(0)), N)
    assert nl(If(Cmp("j", "<", 1), Col("j"), Col("i")), N)
    assert nl(CaseWhen([(Cmp("j", "<", 1), Col("j"))]), N)      # no else
    assert not nl(CaseWhen([(Cmp("i", "<", 1), Col("j"))], else_=Lit(0)), N)
    # Coalesce: only if every operand is
    assert not nl(Coalesce(Col("i"), Col("j")), N)
    assert not nl(Coalesce(Col("i"), 0), N)
    assert nl(Coalesce(Col("i"), Lit(None, "i64")), N)
    # a REF carries the earlier output's nullability
    s = BinOp("+", Col("i"), Col("j"))
    assert lower_ok([("s", s), ("u", Neg(BinOp("+", Col("i"), Col("j"))))], N)[3] \
        == [True, True]


# ---------------- random trees pass the simulation ----------------

def test_random_trees_pass_the_simulation():
    rng = np.random.RandomState(20260)
    done = 0
    ops = set()
    while done < 300:
        outs = [(f"o{k}", random_expr(rng, rng.randint(1, 4),
                                      "i64" if rng.rand() < 0.5 else "f64",
                                      ["ep", "d", "t", "i", "j"], ["x", "y"]))
                for k in range(rng.randint(1, 5))]
        try:
            cols, prog, dts, nls = E.lower(outs, SCHEMA,
                                           nullable=["i", "x", "t"])
        except ValueError as err:
            assert "limit" in str(err) or "needs a dtype" in str(err), err
            continue
        simulate(cols, prog, dts, SCHEMA)
        ops |= {i.opcode for i in prog}
        done += 1
    assert ops >= set(range(16)) - {E.REF}
