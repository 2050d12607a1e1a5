"""Argument checks of gpuq_project_expr that need no GPU: the entry point
validates the whole program with a stack / type simulation before any HIP
call, so each rule is driven here through ctypes with fake, never
dereferenced pointers. Also: the columnar rule maps a ProjectExec with
expression entries to a GpuProjectExec with the same output."""
import ctypes
import os
import subprocess

import pytest

torch = pytest.importorskip("torch")

from spark_amd import expression as E  # noqa: E402
from spark_amd.expression import Insn  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I64, F64, BOOL, I32 = E.I64, E.F64, E.BOOL, 2
FAKE = 0x1000     # never dereferenced: every failing call stops at validation


@pytest.fixture(scope="module")
def gpuq():
    # always through make: a library older than its source lacks the entry
    # point tested here
    subprocess.run(["make", "-C", os.path.join(ROOT, "spark_amd", "csrc"), "-s"],
                   check=True)
    from spark_amd import gpuq as g
    return g


def call(gpuq, prog, n=8, col_dtypes=(I64, I64, F64), out_dtypes=(I64,),
         ncols=None, ninsns=None, nouts=None, outs=None, bits=None):
    L = gpuq.lib()
    cols = (gpuq._Col * max(len(col_dtypes), 1))(
        *[gpuq._Col(FAKE, FAKE if k == 1 else None, dt)
          for k, dt in enumerate(col_dtypes)])
    prog_arr = (gpuq._ExprInsn * max(len(prog), 1))(
        *[gpuq._ExprInsn(*i) for i in prog])
    k = max(len(out_dtypes), 1)
    vp = ctypes.c_void_p
    outs_arr = (vp * k)(*(outs if outs is not None else [FAKE] * len(out_dtypes)))
    bits_arr = (vp * k)(*(bits if bits is not None else [FAKE] * len(out_dtypes)))
    dts = (ctypes.c_int32 * k)(*out_dtypes)
    rc = L.gpuq_project_expr(
        None, n, cols, len(col_dtypes) if ncols is None else ncols,
        prog_arr, len(prog) if ninsns is None else ninsns,
        outs_arr, bits_arr, dts, len(out_dtypes) if nouts is None else nouts)
    return rc, L.gpuq_last_error().decode()


COL0 = Insn(E.COL, 0, I64)          # int64
COL1 = Insn(E.COL, 1, I64)          # int64 with a bitmap
COLF = Insn(E.COL, 2, F64)          # float64
LITI = Insn(E.LIT, 0, I64, 0, 5)
BTRUE = Insn(E.LIT, 0, BOOL, 0, 1)
OUT0 = Insn(E.OUT, 0, I64)
ADD = Insn(E.ARITH, 0, I64)
LT = Insn(E.CMP_OP, 1, I64)

# name -> (program, keyword overrides, what the message must name)
BAD = {
    "nrows_over_u32": ([COL0, OUT0], dict(n=0x100000000), "nrows"),
    "nrows_negative": ([COL0, OUT0], dict(n=-1), "nrows"),
    "too_many_columns": ([COL0, OUT0], dict(ncols=9), "columns"),
    "negative_columns": ([COL0, OUT0], dict(ncols=-1), "columns"),
    "no_insns": ([], {}, "instructions"),
    "too_many_insns": ([COL0, OUT0], dict(ninsns=49), "instructions"),
    "no_outputs": ([COL0, OUT0], dict(nouts=0), "outputs"),
    "too_many_outputs": ([COL0, OUT0], dict(nouts=5), "outputs"),
    "column_dtype": ([COL0, OUT0], dict(col_dtypes=(I32, I64, F64)), "column 0"),
    "column_dtype_bool": ([COL0, OUT0], dict(col_dtypes=(I64, BOOL, F64)), "column 1"),
    "output_dtype": ([COL0, OUT0], dict(out_dtypes=(I32,)), "output 0"),
    "output_dtype_bool": ([COL0, OUT0], dict(out_dtypes=(BOOL,)), "output 0"),
    "opcode_high": ([Insn(16, 0, I64)], {}, "bad opcode"),
    "opcode_negative": ([Insn(-1, 0, I64)], {}, "bad opcode"),
    "insn_dtype": ([Insn(E.LIT, 0, I32), OUT0], {}, "bad dtype"),
    "binop_rsub": ([COL0, LITI, Insn(E.ARITH, 4, I64), OUT0], {}, "bad binop"),
    "binop_negative": ([COL0, LITI, Insn(E.ARITH, -1, I64), OUT0], {}, "bad binop"),
    "comparison": ([COL0, LITI, Insn(E.CMP_OP, 6, I64), Insn(E.CAST, I64, BOOL), OUT0],
                   {}, "bad comparison"),
    "cast_pair_same": ([COL0, Insn(E.CAST, I64, I64), OUT0], {}, "bad cast"),
    "cast_bool_f64": ([BTRUE, Insn(E.CAST, F64, BOOL), Insn(E.OUT, 0, F64)],
                      dict(out_dtypes=(F64,)), "bad cast"),
    "cast_to_bool": ([COL0, Insn(E.CAST, BOOL, I64), OUT0], {}, "bad cast"),
    "null_literal_flag": ([Insn(E.LIT, 2, I64), OUT0], {}, "NULL-literal"),
    "bool_literal_value": ([Insn(E.LIT, 0, BOOL, 0, 2), Insn(E.CAST, I64, BOOL), OUT0],
                           {}, "bool literal"),
    "column_index": ([Insn(E.COL, 3, I64), OUT0], {}, "column index"),
    "column_index_negative": ([Insn(E.COL, -1, I64), OUT0], {}, "column index"),
    "output_index": ([COL0, Insn(E.OUT, 1, I64)], {}, "output index"),
    "ref_index": ([COL0, OUT0, Insn(E.REF, 1, I64), Insn(E.OUT, 0, I64)], {}, "output index"),
    "ref_before_out": ([Insn(E.REF, 0, I64), OUT0], {}, "not yet written"),
    "ref_before_out_2": ([COL0, OUT0, Insn(E.REF, 1, I64), Insn(E.OUT, 1, I64)],
                         dict(out_dtypes=(I64, I64)), "not yet written"),
    "out_twice": ([COL0, OUT0, COL0, OUT0], {}, "written twice"),
    "out_never": ([COL0, OUT0], dict(out_dtypes=(I64, I64)), "never written"),
    "col_declared_dtype": ([Insn(E.COL, 2, I64), OUT0], {}, "declared dtype"),
    "ref_declared_dtype": ([COL0, OUT0, Insn(E.REF, 0, F64), Insn(E.OUT, 1, F64)],
                           dict(out_dtypes=(I64, F64)), "declared dtype"),
    "arith_declared_dtype": ([COL0, LITI, Insn(E.ARITH, 0, F64), OUT0], {}, "declared dtype"),
    "neg_declared_dtype": ([COL0, Insn(E.NEG, 0, F64), OUT0], {}, "declared dtype"),
    "cast_declared_dtype": ([COL0, Insn(E.CAST, I64, F64), OUT0], {}, "declared dtype"),
    "is_null_declared_dtype": ([COL0, Insn(E.IS_NULL, 0, F64), Insn(E.CAST, I64, BOOL), OUT0],
                               {}, "declared dtype"),
    "and_declared_dtype": ([BTRUE, BTRUE, Insn(E.AND, 0, I64), Insn(E.CAST, I64, BOOL), OUT0],
                           {}, "declared dtype"),
    "select_declared_dtype": ([COL0, COL1, BTRUE, Insn(E.SELECT, 0, F64), OUT0],
                              {}, "declared dtype"),
    "out_declared_dtype": ([COL0, Insn(E.OUT, 0, F64)], {}, "declared dtype"),
    "out_dtype_vs_table": ([COLF, Insn(E.OUT, 0, F64)], {}, "declared dtype"),
    "arith_types_differ": ([COL0, COLF, ADD, OUT0], {}, "types differ"),
    "cmp_types_differ": ([COLF, COL0, LT, Insn(E.CAST, I64, BOOL), OUT0], {}, "types differ"),
    "select_types_differ": ([COL0, COLF, BTRUE, Insn(E.SELECT, 0, I64), OUT0],
                            {}, "types differ"),
    "coalesce_types_differ": ([COL0, COLF, Insn(E.COALESCE, 0, I64), OUT0], {}, "types differ"),
    "bool_to_arith": ([BTRUE, BTRUE, Insn(E.ARITH, 0, BOOL), OUT0], {}, "bool operand"),
    "bool_to_neg": ([BTRUE, Insn(E.NEG, 0, BOOL), OUT0], {}, "bool operand"),
    "bool_to_abs": ([BTRUE, Insn(E.ABS, 0, BOOL), OUT0], {}, "bool operand"),
    "bool_to_cmp": ([BTRUE, BTRUE, Insn(E.CMP_OP, 0, BOOL), Insn(E.CAST, I64, BOOL), OUT0],
                    {}, "bool operand"),
    "bool_to_out": ([BTRUE, Insn(E.OUT, 0, BOOL)], {}, "bool operand"),
    "int_to_and": ([COL0, BTRUE, Insn(E.AND, 0, BOOL), Insn(E.CAST, I64, BOOL), OUT0],
                   {}, "non-bool"),
    "int_to_or": ([BTRUE, COL0, Insn(E.OR, 0, BOOL), Insn(E.CAST, I64, BOOL), OUT0],
                  {}, "non-bool"),
    "int_to_not": ([COL0, Insn(E.NOT, 0, BOOL), Insn(E.CAST, I64, BOOL), OUT0], {}, "non-bool"),
    "int_select_condition": ([COL0, COL1, LITI, Insn(E.SELECT, 0, I64), OUT0], {}, "non-bool"),
    "underflow_arith": ([COL0, ADD, OUT0], {}, "underflow"),
    "underflow_out": ([OUT0], {}, "underflow"),
    "underflow_select": ([COL0, BTRUE, Insn(E.SELECT, 0, I64), OUT0], {}, "underflow"),
    "depth_9": ([LITI] * 9 + [ADD] * 8 + [OUT0], {}, "depth"),
    "ends_above_0": ([COL0, COL0, OUT0], {}, "leaves 1"),
    "null_output_buffer": ([COL0, OUT0], dict(outs=[None]), "no buffer"),
}


@pytest.mark.parametrize("name", list(BAD))
def test_rejected_before_any_hip_call(gpuq, name):
    prog, kw, needle = BAD[name]
    rc, msg = call(gpuq, prog, **kw)
    assert rc == 2, (name, rc, msg)
    assert msg.startswith("project_expr:") and needle in msg, (name, msg)


def test_zero_rows_launch_nothing(gpuq):
    # valid programs at nrows == 0 return GPUQ_OK without touching a pointer:
    # the largest legal shapes, a NULL output buffer and NULL bitmaps included
    progs = [
        [COL0, OUT0],
        [LITI] * 8 + [ADD] * 7 + [OUT0],                              # depth 8
        [COL0] + [COL1, Insn(E.COALESCE, 0, I64)] * 23 + [OUT0],       # 48 insns
        [COL0, COL1, LT, Insn(E.CAST, I64, BOOL), OUT0],
        [COL0, COL1, COL0, COL1, LT, Insn(E.SELECT, 0, I64), OUT0],
        [COLF, Insn(E.CAST, I64, F64), Insn(E.ABS, 0, I64), Insn(E.NEG, 0, I64), OUT0],
        [COL1, Insn(E.IS_NOT_NULL, 0, I64), BTRUE, Insn(E.OR, 0, BOOL),
         Insn(E.NOT, 0, BOOL), Insn(E.IS_NULL, 0, BOOL), Insn(E.CAST, I64, BOOL), OUT0],
        [Insn(E.LIT, 1, I64), OUT0],
    ]
    for prog in progs:
        assert len(prog) <= 48
        rc, msg = call(gpuq, prog, n=0, outs=[None], bits=[None])
        assert rc == 0, (prog, msg)
    rc, msg = call(gpuq, [COL0, Insn(E.OUT, 1, I64), Insn(E.REF, 1, I64),
                          Insn(E.CAST, F64, I64), Insn(E.OUT, 3, F64),
                          COLF, Insn(E.OUT, 2, F64), COL1, OUT0],
                   n=0, out_dtypes=(I64, I64, F64, F64))
    assert rc == 0, msg
    # no columns at all: a literal-only program
    rc, msg = call(gpuq, [LITI, OUT0], n=0, col_dtypes=(), ncols=0)
    assert rc == 0, msg


def test_caps_mirror_the_header(gpuq):
    header = open(os.path.join(ROOT, "include", "gpuq.h")).read()

    def define(name):
        for line in header.splitlines():
            parts = line.split()
            if len(parts) >= 3 and parts[0] == "#define" and parts[1] == name:
                return int(parts[2])
        raise KeyError(name)

    assert define("GPUQ_EXPR_MAX_INSNS") == E.MAX_INSNS == gpuq.EXPR_MAX_INSNS == 48
    assert define("GPUQ_EXPR_MAX_COLS") == E.MAX_COLS == gpuq.EXPR_MAX_COLS == 8
    assert define("GPUQ_EXPR_MAX_OUTS") == E.MAX_OUTS == gpuq.EXPR_MAX_OUTS == 4
    assert define("GPUQ_EXPR_MAX_DEPTH") == E.MAX_DEPTH == gpuq.EXPR_MAX_DEPTH == 8
    assert define("GPUQ_EXPR_BOOL") == E.BOOL != define("GPUQ_INT32")
    names = ["COL", "LIT", "REF", "ARITH", "NEG", "ABS", "CAST", "CMP", "IS_NULL",
             "IS_NOT_NULL", "AND", "OR", "NOT", "SELECT", "COALESCE", "OUT"]
    assert [define("GPUQ_EXPR_" + n) for n in names] == list(range(16))
    assert ctypes.sizeof(gpuq._ExprInsn) == 32
    assert gpuq.EXPR_TILE % 64 == 0


def test_rule_maps_expression_entries(gpuq):
    from spark_amd import exec as gx
    from spark_amd.expression import BinOp, CaseWhen, Cast, Lit
    from spark_amd.predicate import Cmp, Col
    child = gx.InputBatches([gx.ColumnarBatch(
        {"a": torch.zeros(4, dtype=torch.int64),
         "b": torch.zeros(4, dtype=torch.int64)})])
    projections = ["a",
                   ("s", BinOp("+", Col("a"), Col("b"))),
                   ("old", "a", "*", None, 3),
                   ("flag", Cast(Cmp("a", "<", Col("b")), "i64")),
                   ("c", CaseWhen([(Cmp("a", ">", 0), Lit(1))], else_=Lit(0)))]
    plan = gx.ProjectExec(projections, child)
    assert plan.output == ["a", "s", "old", "flag", "c"]
    gpu = gx.GpuColumnarRule().pre_columnar_transitions(plan)
    assert isinstance(gpu, gx.GpuProjectExec)
    assert gpu.output == plan.output and gpu.projections is projections
    # stacked projects are mapped one to one, not merged
    stacked = gx.ProjectExec([("t", BinOp("*", Col("s"), 2))], plan)
    g2 = gx.GpuColumnarRule().pre_columnar_transitions(stacked)
    assert isinstance(g2, gx.GpuProjectExec)
    assert isinstance(g2.children[0], gx.GpuProjectExec)
