"""CPU tests of the LIMIT plan nodes: the ColumnarRule maps
TakeOrderedAndProjectExec / LocalLimitExec / GlobalLimitExec /
CollectLimitExec (execution/limit.scala) to their GPU classes and keeps their
arguments; the CPU placeholders still refuse to run. No GPU calls here."""
import pytest

from spark_amd import exec as gx


class Scan(gx.SparkPlan):
    """leaf with a fixed schema and no data."""

    @property
    def output(self):
        return ["orderkey", "revenue", "date", "prio"]


ORDERS = [gx.SortOrder("revenue", descending=True), gx.SortOrder("date")]


def rewrite(plan):
    return gx.GpuColumnarRule().pre_columnar_transitions(plan)


def test_take_ordered_rewrite_keeps_arguments():
    cpu = gx.TakeOrderedAndProjectExec(10, ORDERS, ["orderkey", "revenue"], Scan())
    gpu = rewrite(cpu)
    assert type(gpu) is gx.GpuTakeOrderedAndProjectExec
    assert gpu.supports_columnar
    assert gpu.limit == 10
    assert gpu.sort_order is ORDERS and gpu.sort_orders == ORDERS
    assert gpu.project_list == ["orderkey", "revenue"]
    assert isinstance(gpu.children[0], Scan)


def test_take_ordered_output_and_ordering():
    for cls in (gx.TakeOrderedAndProjectExec, gx.GpuTakeOrderedAndProjectExec):
        node = cls(5, ORDERS, ["orderkey", "revenue"], Scan())
        assert node.output == ["orderkey", "revenue"]
        assert node.output_ordering == ORDERS
        node = cls(5, ORDERS[0], None, Scan())      # a single SortOrder
        assert node.output == Scan().output
        assert node.output_ordering == [ORDERS[0]]


def test_limit_rewrites_keep_limit_and_offset():
    gpu = rewrite(gx.LocalLimitExec(7, Scan()))
    assert type(gpu) is gx.GpuLocalLimitExec
    assert (gpu.limit, gpu.offset) == (7, 0)
    gpu = rewrite(gx.GlobalLimitExec(7, Scan(), offset=3))
    assert type(gpu) is gx.GpuGlobalLimitExec
    assert (gpu.limit, gpu.offset) == (7, 3)
    gpu = rewrite(gx.CollectLimitExec(9, Scan(), offset=2))
    assert type(gpu) is gx.GpuCollectLimitExec
    assert isinstance(gpu, gx.GpuGlobalLimitExec)
    assert (gpu.limit, gpu.offset) == (9, 2)
    for node in (gx.LocalLimitExec(1, Scan()), gx.GlobalLimitExec(1, Scan()),
                 gx.CollectLimitExec(1, Scan()), gpu):
        assert node.output == Scan().output


def test_limit_keeps_child_ordering():
    sort = gx.SortExec(ORDERS, False, Scan())
    gpu = rewrite(gx.GlobalLimitExec(3, gx.LocalLimitExec(3, sort)))
    assert type(gpu.children[0]) is gx.GpuLocalLimitExec
    assert type(gpu.children[0].children[0]) is gx.GpuSortExec
    assert gpu.output_ordering == ORDERS
    assert gpu.required_child_distribution()[0].kind == "all_tuples"


def test_rewrite_descends_through_limit_nodes():
    plan = gx.TakeOrderedAndProjectExec(
        4, ORDERS, None, gx.FilterExec("prio", "<", 3, Scan()))
    gpu = rewrite(plan)
    assert type(gpu.children[0]) is gx.GpuFilterExec


@pytest.mark.parametrize("make", [
    lambda: gx.TakeOrderedAndProjectExec(10, ORDERS, None, Scan()),
    lambda: gx.LocalLimitExec(10, Scan()),
    lambda: gx.GlobalLimitExec(10, Scan(), offset=1),
    lambda: gx.CollectLimitExec(10, Scan()),
])
def test_cpu_placeholders_refuse_to_execute(make):
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        next(make().execute_columnar())
