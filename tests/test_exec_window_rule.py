"""CPU tests of the window plan nodes: the ColumnarRule maps WindowExec
(execution/window/WindowExec.scala) to GpuWindowExec and keeps its arguments;
output, ordering and the requirements on the child; the constructor errors;
the CPU placeholder still refuses to run. No GPU calls here."""
import pytest

from spark_amd import exec as gx
from spark_amd.exec import SortOrder, WindowExpr


class Scan(gx.SparkPlan):
    """leaf with a fixed schema and no data."""

    @property
    def output(self):
        return ["store", "day", "sales", "units"]

    @property
    def output_ordering(self):
        return [SortOrder("store"), SortOrder("day", descending=True)]


ORDER = [SortOrder("day", descending=True)]
EXPRS = [WindowExpr("row_number", None, "rn"),
         WindowExpr("sum", "sales", "running", frame="rows"),
         WindowExpr("lag", "units", "prev_units", offset=2, default=0)]


def rewrite(plan):
    return gx.GpuColumnarRule().pre_columnar_transitions(plan)


def test_window_expr_defaults():
    e = WindowExpr("sum", "sales", "s")
    assert (e.fn, e.col, e.name, e.frame, e.offset, e.default) == \
        ("sum", "sales", "s", None, 1, None)


def test_rewrite_keeps_arguments():
    cpu = gx.WindowExec(EXPRS, ["store"], ORDER, Scan())
    gpu = rewrite(cpu)
    assert type(gpu) is gx.GpuWindowExec
    assert gpu.supports_columnar and not cpu.supports_columnar
    assert gpu.window_exprs == EXPRS
    assert gpu.partition_spec == ["store"]
    assert gpu.order_spec == ORDER
    assert isinstance(gpu.children[0], Scan)


def test_rewrite_descends_below_the_window():
    sort = gx.SortExec([SortOrder("store")] + ORDER, False,
                       gx.ShuffleExchangeExec(("store",), 4, Scan()))
    gpu = rewrite(gx.FilterExec("rn", "<=", 3,
                                gx.WindowExec(EXPRS[:1], ["store"], ORDER, sort)))
    assert type(gpu) is gx.GpuFilterExec
    win = gpu.children[0]
    assert type(win) is gx.GpuWindowExec
    assert type(win.children[0]) is gx.GpuSortExec
    assert type(win.children[0].children[0]) is gx.GpuShuffleExchangeExec


@pytest.mark.parametrize("cls", [gx.WindowExec, gx.GpuWindowExec])
def test_output_ordering_and_requirements(cls):
    node = cls(EXPRS, ["store"], ORDER, Scan())
    assert node.output == Scan().output + ["rn", "running", "prev_units"]
    assert node.output_ordering == Scan().output_ordering
    dist = node.required_child_distribution()
    assert len(dist) == 1
    assert (dist[0].kind, dist[0].keys) == ("clustered", ("store",))
    assert node.required_child_ordering() == [SortOrder("store")] + ORDER
    # a single name / SortOrder is accepted like a one-element list
    node = cls(EXPRS, "store", ORDER[0], Scan())
    assert node.partition_spec == ["store"] and node.order_spec == ORDER
    # two partition keys, no ORDER BY
    node = cls([WindowExpr("max", "sales", "m")], ["store", "day"], [], Scan())
    assert node.required_child_distribution()[0].keys == ("store", "day")
    assert node.required_child_ordering() == \
        [SortOrder("store"), SortOrder("day")]


def test_required_child_ordering_defaults_to_none():
    assert Scan().required_child_ordering() == []
    assert gx.GpuSortExec(ORDER, False, Scan()).required_child_ordering() == []


@pytest.mark.parametrize("cls", [gx.WindowExec, gx.GpuWindowExec])
def test_default_frames(cls):
    with_order = cls([WindowExpr("sum", "sales", "a"),
                      WindowExpr("sum", "sales", "b", frame="rows"),
                      WindowExpr("sum", "sales", "c", frame="partition")],
                     ["store"], ORDER, Scan())
    assert [with_order.frame_of(e) for e in with_order.window_exprs] == \
        ["range", "rows", "partition"]
    no_order = cls([WindowExpr("sum", "sales", "a"),
                    WindowExpr("sum", "sales", "b", frame="range"),
                    WindowExpr("sum", "sales", "c", frame="rows")],
                   ["store"], [], Scan())
    assert [no_order.frame_of(e) for e in no_order.window_exprs] == \
        ["partition", "partition", "rows"]


@pytest.mark.parametrize("cls", [gx.WindowExec, gx.GpuWindowExec])
@pytest.mark.parametrize("exprs,order,match", [
    ([WindowExpr("row_number", None, "sales")], ORDER, "already exists"),
    ([WindowExpr("sum", "sales", "s"), WindowExpr("min", "sales", "s")], ORDER,
     "already exists"),
    ([WindowExpr("row_number", None, "rn")], [], "needs an ORDER BY"),
    ([WindowExpr("rank", None, "r")], [], "needs an ORDER BY"),
    ([WindowExpr("dense_rank", None, "r")], [], "needs an ORDER BY"),
    ([WindowExpr("lag", "sales", "l")], [], "needs an ORDER BY"),
    ([WindowExpr("lead", "sales", "l")], [], "needs an ORDER BY"),
    ([WindowExpr("ntile", None, "t")], ORDER, "unknown function"),
    ([WindowExpr("sum", "sales", "s", frame="sliding")], ORDER, "unknown frame"),
    ([WindowExpr("rank", "sales", "r")], ORDER, "takes no column"),
    ([WindowExpr("sum", None, "s")], ORDER, "needs a column"),
])
def test_constructor_errors(cls, exprs, order, match):
    with pytest.raises(ValueError, match=match):
        cls(exprs, ["store"], order, Scan())


def test_count_star_and_aggregates_without_order_are_fine():
    node = gx.WindowExec([WindowExpr("count", None, "n"),
                          WindowExpr("avg", "sales", "a")], ["store"], [], Scan())
    assert node.output[-2:] == ["n", "a"]


def test_cpu_placeholder_refuses_to_execute():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        next(gx.WindowExec(EXPRS, ["store"], ORDER, Scan()).execute_columnar())
