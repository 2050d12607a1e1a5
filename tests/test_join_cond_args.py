"""The parts of the residual join condition that need no GPU.

gpuq_join_probe_keys_cond validates its arguments, the condition's column
table and the whole program before any HIP call, so each rule is driven here
through ctypes with fake, never dereferenced device pointers; the program
checks are the ones gpuq_filter_expr makes (one shared function), and
gpuq_filter_expr must still make them. Also: predicate.columns_of, the
`condition` keyword of the join nodes and its checks, and the columnar rule
carrying it onto the GPU nodes."""
import ctypes
import os
import subprocess

import pytest

torch = pytest.importorskip("torch")

from spark_amd import predicate as P  # noqa: E402
from spark_amd.predicate import (And, Between, Cmp, Col, In, Insn, IsNotNull,  # noqa: E402
                                 IsNull, Not, Or)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I64, F64, I32 = 0, 1, 2
FAKE = 0x1000     # never dereferenced: every failing call stops at validation
PREFIX = "join_keys probe_cond:"


@pytest.fixture(scope="module")
def gpuq():
    # always through make: a library older than its source lacks the entry
    # point tested here
    subprocess.run(["make", "-C", os.path.join(ROOT, "spark_amd", "csrc"), "-s"],
                   check=True)
    from spark_amd import gpuq as g
    return g


def cols_arr(gpuq, dtypes):
    return (gpuq._Col * max(len(dtypes), 1))(
        *[gpuq._Col(FAKE, FAKE if k == 1 else None, dt)
          for k, dt in enumerate(dtypes)])


def prog_arr(gpuq, prog):
    return (gpuq._PredInsn * max(len(prog), 1))(
        *[gpuq._PredInsn(*i) for i in prog])


def call(gpuq, prog, prows=8, key_dtypes=(I64, I64), nkeys=None, cap=16,
         brows=4, jt=0, cond_dtypes=(I64, I64, F64), sides=(0, 1, 1),
         ncond=None, ninsns=None, null_keys=False, null_cols=False,
         null_sides=False, null_prog=False):
    L = gpuq.lib()
    sides_a = (ctypes.c_int32 * max(len(sides), 1))(*sides)
    nm = ctypes.c_int64(-1)
    rc = L.gpuq_join_probe_keys_cond(
        None, prows, None if null_keys else cols_arr(gpuq, key_dtypes),
        len(key_dtypes) if nkeys is None else nkeys, FAKE, cap, brows, jt,
        None if null_cols else cols_arr(gpuq, cond_dtypes),
        None if null_sides else sides_a,
        len(cond_dtypes) if ncond is None else ncond,
        None if null_prog else prog_arr(gpuq, prog),
        len(prog) if ninsns is None else ninsns,
        FAKE, FAKE, 64, ctypes.byref(nm))
    return rc, L.gpuq_last_error().decode()


def call_filter(gpuq, prog, cond_dtypes=(I64, I64, F64), ninsns=None):
    L = gpuq.lib()
    rc = L.gpuq_filter_expr(None, 8, cols_arr(gpuq, cond_dtypes),
                            len(cond_dtypes), prog_arr(gpuq, prog),
                            len(prog) if ninsns is None else ninsns,
                            FAKE, FAKE, FAKE, 1 << 20)
    return rc, L.gpuq_last_error().decode()


LT = P.CMP["<"]
LEAF = Insn(P.CMP_LIT, LT, 0, 0, 5, 5.0)            # col0 < 5
LEAF_F = Insn(P.CMP_LIT, LT, 2, 0, 0, 0.5)          # col2 < 0.5
X_LT_Y = Insn(P.CMP_COL, LT, 0, 1)                  # probe col0 < build col1
GOOD = [X_LT_Y]

# what gpuq_join_probe_keys already rejects: name -> (kwargs, message part)
BAD_TABLE = {
    "nkeys_0": (dict(nkeys=0), "nkeys"),
    "nkeys_5": (dict(nkeys=5), "nkeys"),
    "capacity_not_pow2": (dict(cap=24), "power of two"),
    "capacity_0": (dict(cap=0), "power of two"),
    "build_rows_32bit": (dict(brows=1 << 31), "31-bit"),
    "build_rows_negative": (dict(brows=-1), "31-bit"),
    "null_aware_anti": (dict(jt=5), "null-aware anti"),
    "join_type_6": (dict(jt=6), "bad join_type"),
    "join_type_negative": (dict(jt=-1), "bad join_type"),
    "probe_rows_over_u32": (dict(prows=1 << 32), "32-bit"),
    "probe_rows_negative": (dict(prows=-1), "32-bit"),
    "key_columns_null": (dict(null_keys=True), "key columns missing"),
    "key_column_float": (dict(key_dtypes=(I64, F64)), "key col 1 must be int64"),
}

# the condition's own table
BAD_COND = {
    "no_condition_columns": (dict(ncond=0), "condition columns"),
    "too_many_condition_columns": (dict(ncond=9), "condition columns"),
    "negative_condition_columns": (dict(ncond=-1), "condition columns"),
    "null_cond_cols": (dict(null_cols=True), "condition columns missing"),
    "null_cond_sides": (dict(null_sides=True), "sides missing"),
    "null_prog": (dict(null_prog=True), "program missing"),
    "side_2": (dict(sides=(0, 2, 1)), "column 1 has side 2"),
    "side_negative": (dict(sides=(-1, 1, 1)), "column 0 has side -1"),
    "no_insns": (dict(ninsns=0), "instructions"),
    "too_many_insns": (dict(ninsns=33), "instructions"),
}

# every program error gpuq_filter_expr rejects: name -> (program, kwargs, part)
BAD_PROG = {
    "opcode_high": ([Insn(8)], {}, "bad opcode 8"),
    "opcode_negative": ([Insn(-1)], {}, "bad opcode -1"),
    "comparison_high": ([Insn(P.CMP_LIT, 6, 0)], {}, "bad comparison 6"),
    "comparison_negative": ([Insn(P.CMP_COL, -1, 0, 1)], {}, "bad comparison -1"),
    "const_value": ([Insn(P.CONST, 3)], {}, "bad constant 3"),
    "col_a_out_of_range": ([Insn(P.CMP_LIT, LT, 3)], {}, "column index 3"),
    "col_a_negative": ([Insn(P.IS_NULL, 0, -1)], {}, "column index -1"),
    "col_b_out_of_range": ([Insn(P.CMP_COL, LT, 0, 3)], {}, "column index 3"),
    "column_dtype_int32": (GOOD, dict(cond_dtypes=(I64, I32, F64)),
                           "column 1 has unsupported dtype 2"),
    "cmp_col_two_dtypes": ([Insn(P.CMP_COL, LT, 0, 2)], {}, "dtypes differ"),
    "underflow_and": ([LEAF, Insn(P.AND)], {}, "stack underflow"),
    "underflow_not": ([Insn(P.NOT)], {}, "stack underflow"),
    "depth_17": ([LEAF] * 17 + [Insn(P.AND)] * 15, {}, "stack depth exceeds 16"),
    "ends_at_depth_2": ([LEAF, LEAF_F], {}, "leaves 2 values"),
}


@pytest.mark.parametrize("name", list(BAD_TABLE))
def test_join_probe_keys_rejections_kept(gpuq, name):
    kw, needle = BAD_TABLE[name]
    rc, msg = call(gpuq, GOOD, **kw)
    assert rc == 2, (name, rc, msg)
    assert msg.startswith(PREFIX) and needle in msg, (name, msg)


@pytest.mark.parametrize("name", list(BAD_COND))
def test_condition_table_rejected_before_any_hip_call(gpuq, name):
    kw, needle = BAD_COND[name]
    rc, msg = call(gpuq, GOOD, **kw)
    assert rc == 2, (name, rc, msg)
    assert msg.startswith(PREFIX) and needle in msg, (name, msg)


@pytest.mark.parametrize("name", list(BAD_PROG))
def test_program_rejected_before_any_hip_call(gpuq, name):
    prog, kw, needle = BAD_PROG[name]
    assert len(prog) <= P.MAX_INSNS
    rc, msg = call(gpuq, prog, **kw)
    assert rc == 2, (name, rc, msg)
    assert msg.startswith(PREFIX) and needle in msg, (name, msg)


@pytest.mark.parametrize("name", list(BAD_PROG))
def test_filter_expr_still_rejects(gpuq, name):
    """the shared validation keeps gpuq_filter_expr's behaviour and words"""
    prog, kw, needle = BAD_PROG[name]
    rc, msg = call_filter(gpuq, prog, **kw)
    assert rc == 2, (name, rc, msg)
    assert msg.startswith("filter_expr:") and needle in msg, (name, msg)


def test_filter_expr_count_rules_unchanged(gpuq):
    rc, msg = call_filter(gpuq, GOOD, ninsns=0)
    assert rc == 2 and "filter_expr: 0 instructions, need 1..32" in msg
    rc, msg = call_filter(gpuq, GOOD, ninsns=33)
    assert rc == 2 and "filter_expr: 33 instructions, need 1..32" in msg
    rc, msg = call_filter(gpuq, GOOD, cond_dtypes=(I64,) * 9)
    assert rc == 2 and "filter_expr: 9 columns, need 0..8" in msg


def test_side_constants_mirror_the_header(gpuq):
    header = open(os.path.join(ROOT, "include", "gpuq.h")).read()
    assert "#define GPUQ_JOIN_SIDE_PROBE 0" in header
    assert "#define GPUQ_JOIN_SIDE_BUILD 1" in header
    assert (gpuq.JOIN_SIDE_PROBE, gpuq.JOIN_SIDE_BUILD) == (0, 1)


# ---------------- predicate.columns_of ----------------

def test_columns_of_first_use_order():
    assert P.columns_of(Cmp("x", "<", Col("y"))) == ["x", "y"]
    assert P.columns_of(Cmp("y", ">", 3)) == ["y"]
    assert P.columns_of(IsNull("a")) == ["a"]
    assert P.columns_of(IsNotNull(Col("a"))) == ["a"]
    assert P.columns_of(In("c", [1, None])) == ["c"]
    assert P.columns_of(Between("d", 0, 9)) == ["d"]
    assert P.columns_of(Not(Cmp("x", "==", Col("x")))) == ["x"]
    p = And(Cmp("px", "<", Col("by")),
            Or(IsNull("bz"), Cmp("pf", ">=", 0.5)),
            In("by", [3, None, 7]))
    assert P.columns_of(p) == ["px", "by", "bz", "pf"]
    with pytest.raises(ValueError):
        P.columns_of("x < y")


def test_columns_of_is_lowers_column_list():
    schema = {"a": "int64", "b": "int64", "c": "float64", "d": "float64"}
    preds = [
        Cmp("a", "<", Col("b")),
        And(Cmp("c", ">", 0.5), Cmp("a", "<", 3), Cmp("c", "<", Col("d"))),
        Or(Not(IsNull("d")), And(In("b", [1, 2]), Between("a", 0, 5),
                                 Cmp("b", "!=", None))),
        In("b", []),
    ]
    for p in preds:
        assert P.columns_of(p) == P.lower(p, schema)[0], p


# ---------------- nodes and rule ----------------

def scan(gx, **cols):
    return gx.InputBatches([gx.ColumnarBatch(
        {k: torch.zeros(4, dtype=dt) for k, dt in cols.items()})])


@pytest.fixture()
def sides():
    from spark_amd import exec as gx
    left = scan(gx, lk=torch.int64, x=torch.int64, both=torch.int64)
    right = scan(gx, rk=torch.int64, y=torch.int64, both=torch.int64)
    return gx, left, right


COND = Cmp("x", "<", Col("y"))


def test_rule_carries_condition_shj(sides):
    gx, left, right = sides
    for jt in ("inner", "left_outer", "left_semi", "left_anti"):
        node = gx.ShuffledHashJoinExec("lk", "rk", "right", left, right,
                                       join_type=jt, condition=COND)
        assert node.condition is COND
        gpu = gx.GpuColumnarRule().pre_columnar_transitions(node)
        assert type(gpu) is gx.GpuShuffledHashJoinExec
        assert gpu.condition is COND and gpu.join_type == jt
        assert gpu.output == node.output


def test_rule_carries_condition_smj_inside_the_resort(sides):
    gx, left, right = sides
    node = gx.SortMergeJoinExec(("lk", "x"), ("rk", "y"), left, right,
                                join_type="left_outer",
                                condition=COND)
    gpu = gx.GpuColumnarRule().pre_columnar_transitions(node)
    assert type(gpu) is gx.GpuSortExec           # the re-sort wrapper
    join = gpu.children[0]
    assert type(join) is gx.GpuShuffledHashJoinExec
    assert join.condition is COND and join.build_side == "right"
    # full outer declares no ordering: no wrapper, the condition still there
    node = gx.SortMergeJoinExec("lk", "rk", left, right,
                                join_type="full_outer", condition=COND)
    gpu = gx.GpuColumnarRule().pre_columnar_transitions(node)
    assert type(gpu) is gx.GpuShuffledHashJoinExec and gpu.condition is COND
    gpu = gx.GpuColumnarRule(preserve_smj_ordering=False) \
        .pre_columnar_transitions(
            gx.SortMergeJoinExec("lk", "rk", left, right, condition=COND))
    assert type(gpu) is gx.GpuShuffledHashJoinExec and gpu.condition is COND


def test_rule_carries_condition_bhj(sides):
    gx, left, right = sides
    node = gx.BroadcastHashJoinExec("lk", "rk", "right", left,
                                    gx.BroadcastExchangeExec(right),
                                    condition=COND)
    gpu = gx.GpuColumnarRule().pre_columnar_transitions(node)
    assert type(gpu) is gx.GpuBroadcastHashJoinExec
    assert gpu.condition is COND
    assert type(gpu.children[1]) is gx.GpuBroadcastExchangeExec


def test_without_condition_nothing_changes(sides):
    gx, left, right = sides
    cpu = [gx.ShuffledHashJoinExec("lk", "rk", "right", left, right),
           gx.ShuffledHashJoinExec("lk", "rk", "right", left, right, "left_semi"),
           gx.SortMergeJoinExec("lk", "rk", left, right),
           gx.SortMergeJoinExec("lk", "rk", left, right, "right_outer"),
           gx.BroadcastHashJoinExec("lk", "rk", "left", left, right),
           gx.BroadcastHashJoinExec("lk", "rk", "left", left, right, "inner")]
    both = ["lk", "x", "both", "rk", "y", "both"]
    outputs = [both, ["lk", "x", "both"], both, both, both, both]
    for node, out in zip(cpu, outputs):
        assert node.condition is None and node.output == out
    gpu = [gx.GpuShuffledHashJoinExec("lk", "rk", "right", left, right),
           gx.GpuShuffledHashJoinExec("lk", "rk", "right", left, right,
                                      "left_anti", True),
           gx.GpuShuffledHashJoinExec("lk", "rk", "right", left, right,
                                      join_type="left_anti",
                                      null_aware_anti=True),
           gx.GpuBroadcastHashJoinExec("lk", "rk", "left", left, right)]
    for node, out in zip(gpu, [both, both[:3], both[:3], both]):
        assert node.condition is None and node.output == out
    assert gpu[1].null_aware_anti and gpu[2].null_aware_anti
    for node in cpu:
        g = gx.GpuColumnarRule(preserve_smj_ordering=False) \
            .pre_columnar_transitions(node)
        assert g.condition is None and g.output == node.output


NODES = ["ShuffledHashJoinExec", "SortMergeJoinExec", "BroadcastHashJoinExec",
         "GpuShuffledHashJoinExec", "GpuBroadcastHashJoinExec"]


def make(gx, cls, left, right, **kw):
    if cls == "SortMergeJoinExec":
        return gx.SortMergeJoinExec("lk", "rk", left, right, **kw)
    return getattr(gx, cls)("lk", "rk", "right", left, right, **kw)


@pytest.mark.parametrize("cls", NODES)
def test_constructor_checks(sides, cls):
    gx, left, right = sides
    assert make(gx, cls, left, right, condition=COND).condition is COND
    with pytest.raises(ValueError, match="not a predicate"):
        make(gx, cls, left, right, condition="x < y")
    with pytest.raises(ValueError, match="not a predicate"):
        make(gx, cls, left, right, condition=("x", "<", "y"))
    with pytest.raises(ValueError, match="unknown column 'nope'"):
        make(gx, cls, left, right, condition=Cmp("x", "<", Col("nope")))
    with pytest.raises(ValueError, match="'both' is ambiguous"):
        make(gx, cls, left, right, condition=Cmp("both", "<", Col("y")))
    # a one-sided condition is legal, on either side
    make(gx, cls, left, right, condition=IsNotNull("x"))
    make(gx, cls, left, right, condition=Cmp("y", ">", 3))


def test_null_aware_anti_takes_no_condition(sides):
    gx, left, right = sides
    for cls in (gx.GpuShuffledHashJoinExec, gx.GpuBroadcastHashJoinExec):
        with pytest.raises(ValueError, match="null-aware"):
            cls("lk", "rk", "right", left, right, join_type="left_anti",
                null_aware_anti=True, condition=COND)


# ---------------- gpuq.lower_join_cond (pure Python) ----------------

def test_lower_join_cond_sides_and_errors(gpuq):
    probe = {"px": torch.zeros(3, dtype=torch.int64),
             "pf": torch.zeros(3, dtype=torch.float64),
             "both": torch.zeros(3, dtype=torch.int64)}
    build = {"by": torch.zeros(5, dtype=torch.int64),
             "bz": torch.zeros(5, dtype=torch.float64),
             "both": torch.zeros(5, dtype=torch.int64)}
    p = And(Cmp("px", "<", Col("by")),
            Or(IsNull("bz"), Cmp("pf", ">=", 0.5)), In("by", [3, None, 7]))
    names, sd, prog = gpuq.lower_join_cond(p, probe, build)
    assert names == ["px", "by", "bz", "pf"] and sd == [0, 1, 1, 0]
    assert (names, prog) == tuple(P.lower(p, {
        "px": "int64", "by": "int64", "bz": "float64", "pf": "float64"}))
    with pytest.raises(ValueError, match="ambiguous"):
        gpuq.lower_join_cond(Cmp("both", "<", Col("by")), probe, build)
    with pytest.raises(ValueError, match="unknown"):
        gpuq.lower_join_cond(Cmp("px", "<", Col("nope")), probe, build)
    with pytest.raises(ValueError, match="dtypes differ"):
        gpuq.lower_join_cond(Cmp("px", "<", Col("bz")), probe, build)
