"""CPU tests of sliding frames and first_value / last_value on the window plan
nodes: the RowsBetween frame type, the constructor checks of WindowExec and
GpuWindowExec, and the ColumnarRule carrying both through unchanged. No GPU
calls here."""
import dataclasses

import pytest

from spark_amd import exec as gx
from spark_amd.exec import RowsBetween, SortOrder, WindowExpr


class Scan(gx.SparkPlan):
    """leaf with a fixed schema and no data."""

    @property
    def output(self):
        return ["store", "day", "sales", "units"]


ORDER = [SortOrder("day")]
EXPRS = [WindowExpr("avg", "sales", "ma3", frame=RowsBetween(-2, 0)),
         WindowExpr("min", "units", "cmin", frame=RowsBetween(-1, 1)),
         WindowExpr("count", "units", "ahead", frame=RowsBetween(1, 3)),
         WindowExpr("count", None, "stars", frame=RowsBetween(None, -1)),
         WindowExpr("sum", "sales", "far", frame=RowsBetween(5000, 5002)),
         WindowExpr("max", "sales", "wide", frame=RowsBetween(-1000000, 1000000)),
         WindowExpr("first_value", "sales", "fv"),
         WindowExpr("first_value", "sales", "fv_rows", frame="rows"),
         WindowExpr("last_value", "sales", "lv", frame="partition"),
         WindowExpr("last_value", "units", "lv2", frame=RowsBetween(None, None)),
         WindowExpr("first_value", "units", "fv3", frame=RowsBetween(-3, -1)),
         WindowExpr("sum", "sales", "running", frame=RowsBetween(None, 0))]


def test_rows_between_is_a_frozen_value():
    f = RowsBetween(-6, 0)
    assert (f.lo, f.hi) == (-6, 0)
    assert f == RowsBetween(-6, 0) and f != RowsBetween(-6, 1)
    assert hash(f) == hash(RowsBetween(-6, 0))
    with pytest.raises(dataclasses.FrozenInstanceError):
        f.lo = 1
    assert RowsBetween(None, None).lo is None


def test_rewrite_keeps_frames_and_functions():
    cpu = gx.WindowExec(EXPRS, ["store"], ORDER, Scan())
    gpu = gx.GpuColumnarRule().pre_columnar_transitions(cpu)
    assert type(gpu) is gx.GpuWindowExec
    assert gpu.window_exprs == EXPRS
    assert [e.frame for e in gpu.window_exprs] == [e.frame for e in EXPRS]
    assert [e.fn for e in gpu.window_exprs][6:11] == \
        ["first_value", "first_value", "last_value", "last_value", "first_value"]
    assert gpu.partition_spec == ["store"] and gpu.order_spec == ORDER
    assert gpu.output == Scan().output + [e.name for e in EXPRS]


@pytest.mark.parametrize("cls", [gx.WindowExec, gx.GpuWindowExec])
def test_frame_of_returns_a_rows_between_as_it_is(cls):
    node = cls(EXPRS, ["store"], ORDER, Scan())
    assert node.frame_of(EXPRS[0]) == RowsBetween(-2, 0)
    assert node.frame_of(EXPRS[6]) == "range"          # the default, with ORDER BY
    assert node.frame_of(EXPRS[8]) == "partition"


@pytest.mark.parametrize("cls", [gx.WindowExec, gx.GpuWindowExec])
@pytest.mark.parametrize("exprs,order,match", [
    ([WindowExpr("row_number", None, "r", frame=RowsBetween(-1, 0))], ORDER,
     "takes no frame"),
    ([WindowExpr("rank", None, "r", frame=RowsBetween(None, 0))], ORDER,
     "takes no frame"),
    ([WindowExpr("dense_rank", None, "r", frame=RowsBetween(0, 0))], ORDER,
     "takes no frame"),
    ([WindowExpr("lag", "sales", "l", frame=RowsBetween(-1, 0))], ORDER,
     "takes no frame"),
    ([WindowExpr("lead", "sales", "l", frame=RowsBetween(0, 1))], ORDER,
     "takes no frame"),
    ([WindowExpr("sum", "sales", "s", frame=RowsBetween(1, 0))], ORDER, "lo > hi"),
    ([WindowExpr("sum", "sales", "s", frame=RowsBetween(-1, -2))], ORDER, "lo > hi"),
    ([WindowExpr("sum", "sales", "s", frame=RowsBetween(-1.0, 0))], ORDER,
     "not an int"),
    ([WindowExpr("sum", "sales", "s", frame=RowsBetween(0, "1"))], ORDER,
     "not an int"),
    ([WindowExpr("sum", "sales", "s", frame=RowsBetween(True, True))], ORDER,
     "not an int"),
    ([WindowExpr("sum", "sales", "s", frame=RowsBetween(-(1 << 31) - 1, 0))], ORDER,
     "int32"),
    ([WindowExpr("sum", "sales", "s", frame=RowsBetween(None, 1 << 31))], ORDER,
     "int32"),
    ([WindowExpr("sum", "sales", "s", frame=RowsBetween(1, None))], ORDER,
     "UNBOUNDED FOLLOWING"),
    ([WindowExpr("last_value", "sales", "s", frame=RowsBetween(0, None))], ORDER,
     "UNBOUNDED FOLLOWING"),
    ([WindowExpr("sum", "sales", "s", frame=RowsBetween(-1, 1))], [],
     "needs an ORDER BY"),
    ([WindowExpr("count", None, "s", frame=RowsBetween(None, None))], [],
     "needs an ORDER BY"),
    ([WindowExpr("first_value", "sales", "s")], [], "needs an ORDER BY"),
    ([WindowExpr("last_value", "sales", "s", frame="partition")], [],
     "needs an ORDER BY"),
    ([WindowExpr("first_value", None, "s")], ORDER, "needs a column"),
    ([WindowExpr("last_value", None, "s", frame="rows")], ORDER, "needs a column"),
    # what was refused before still is, with the same words
    ([WindowExpr("sum", "sales", "s", frame="sliding")], ORDER, "unknown frame"),
    ([WindowExpr("first_value", "sales", "s", frame=(-1, 1))], ORDER,
     "unknown frame"),
    ([WindowExpr("ntile", None, "t")], ORDER, "unknown function"),
    ([WindowExpr("nth_value", "sales", "t")], ORDER, "unknown function"),
])
def test_constructor_errors(cls, exprs, order, match):
    with pytest.raises(ValueError, match=match):
        cls(exprs, ["store"], order, Scan())


@pytest.mark.parametrize("cls", [gx.WindowExec, gx.GpuWindowExec])
def test_int32_edges_are_accepted(cls):
    lo, hi = -(1 << 31), (1 << 31) - 1
    cls([WindowExpr("sum", "sales", "a", frame=RowsBetween(lo, hi)),
         WindowExpr("sum", "sales", "b", frame=RowsBetween(None, lo)),
         WindowExpr("sum", "sales", "c", frame=RowsBetween(hi, hi))],
        ["store"], ORDER, Scan())


def test_cpu_placeholder_refuses_to_execute():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        next(gx.WindowExec(EXPRS, ["store"], ORDER, Scan()).execute_columnar())
