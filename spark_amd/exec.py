"""Host-side mirror of Spark's columnar physical-operator contract.

In a Spark deployment this layer is Scala: exec-node subclasses registered by
a ColumnarRule through SparkSessionExtensions.injectColumnar
(SparkSessionExtensions.scala:116,168), each overriding
supportsColumnar=true (SparkPlan.scala:92) and
doExecuteColumnar(): RDD[ColumnarBatch] (SparkPlan.scala:359) and calling
libgpuq over JNI (see INTEGRATION.md for that binding). This Python mirror
keeps the same node names, the same required-distribution semantics and the
same batch lifetime contract so the C-ABI is exercised exactly as the Scala
layer would; it is what tests and the TPC-H-style pipelines drive.

No CPU fallback anywhere: executing these nodes without the HIP engine (or
without a GPU) raises.
"""
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import torch

from . import expression
from .predicate import (And, Between, Cmp, Col, In, IsNotNull,  # noqa: F401
                        IsNull, Not, Or, Pred, columns_of)


class ColumnarBatch:
    """Device-resident batch (ColumnarBatch.java:61-123 access contract;
    Arrow-style columns: dense data + optional validity bitmap)."""

    def __init__(self, columns: Dict[str, torch.Tensor],
                 validity: Optional[Dict[str, torch.Tensor]] = None):
        self._cols = columns
        self._validity = validity or {}
        ns = {t.numel() for t in columns.values()}
        assert len(ns) == 1, "ragged batch"
        self._num_rows = ns.pop()
        self._closed = False

    def num_rows(self) -> int:
        return self._num_rows

    def column(self, name: str) -> torch.Tensor:
        assert not self._closed, "batch used after close()"
        return self._cols[name]

    def validity(self, name: str):
        return self._validity.get(name)

    def columns(self):
        return dict(self._cols)

    def close(self):
        # consumer closes (Columnar.scala:224-240 ColumnarToRowExec pattern);
        # device memory returns to the torch pool
        self._cols = {}
        self._validity = {}
        self._closed = True


@dataclass
class Distribution:
    """requiredChildDistribution analog (SparkPlan.scala:180 contract)."""
    kind: str                      # "unspecified" | "clustered" | "ordered"
    keys: Tuple[str, ...] = ()


class SparkPlan:
    """Physical operator (execution/SparkPlan.scala:65). Single-partition-
    per-rank execution model: executeColumnar() yields this rank's batches."""

    def __init__(self, *children: "SparkPlan"):
        self.children = list(children)

    @property
    def output(self) -> List[str]:
        raise NotImplementedError

    @property
    def supports_columnar(self) -> bool:
        return False

    def required_child_distribution(self) -> List[Distribution]:
        return [Distribution("unspecified") for _ in self.children]

    def required_child_ordering(self) -> list:
        """requiredChildOrdering (SparkPlan.scala): the SortOrders this node
        needs its child's rows in; EnsureRequirements puts a SortExec below
        a node whose child does not already deliver them."""
        return []

    @property
    def output_ordering(self) -> list:
        """outputOrdering (SparkPlan.scala:180 contract): the SortOrders
        this node's output satisfies. A replacement node must deliver AT
        LEAST what the node it replaces advertised — parents may have had
        their sorts elided against it (EnsureRequirements)."""
        return []

    def execute_columnar(self):
        """doExecuteColumnar (SparkPlan.scala:359)."""
        raise NotImplementedError(
            f"{type(self).__name__} does not support columnar execution")


# ---------------- CPU placeholders the rule replaces ----------------
# These mirror the Catalyst-produced nodes; they cannot execute here (the
# JVM engine isn't present) — they exist so the ColumnarRule's rewrite is
# the same shape as in Spark (SparkSessionExtensionSuite.scala:959-1000).

@dataclass
class SortOrder:
    key: str
    descending: bool = False
    nulls_first: Optional[bool] = None   # SortOrder.scala:35-45 defaults

    def __post_init__(self):
        if self.nulls_first is None:
            self.nulls_first = not self.descending


class _CpuNode(SparkPlan):
    def execute_columnar(self):
        raise RuntimeError(f"{type(self).__name__} is a CPU placeholder; "
                           "apply the ColumnarRule first (no CPU fallback)")


class SortExec(_CpuNode):
    """sort_order: one SortOrder or a list (multi-key ORDER BY,
    SortExec.scala sortOrder: Seq[SortOrder])."""

    def __init__(self, sort_order, global_sort: bool, child):
        super().__init__(child)
        self.sort_order, self.global_sort = sort_order, global_sort

    @property
    def sort_orders(self):
        return ([self.sort_order] if isinstance(self.sort_order, SortOrder)
                else list(self.sort_order))

    @property
    def output(self):
        return self.children[0].output

    @property
    def output_ordering(self):
        return self.sort_orders


class TakeOrderedAndProjectExec(_CpuNode):
    """ORDER BY ... LIMIT k as Catalyst plans it (execution/limit.scala
    TakeOrderedAndProjectExec), not Sort + Limit. sort_order: one SortOrder or
    a list; project_list: None (all child columns) or a list of column
    names."""

    def __init__(self, limit: int, sort_order, project_list, child):
        super().__init__(child)
        assert limit >= 0
        self.limit, self.sort_order = limit, sort_order
        self.project_list = project_list

    @property
    def sort_orders(self):
        return ([self.sort_order] if isinstance(self.sort_order, SortOrder)
                else list(self.sort_order))

    @property
    def output(self):
        if self.project_list is None:
            return self.children[0].output
        return list(self.project_list)

    @property
    def output_ordering(self):
        return self.sort_orders


class LocalLimitExec(_CpuNode):
    """First `limit` rows of each partition (limit.scala LocalLimitExec)."""

    def __init__(self, limit: int, child):
        super().__init__(child)
        assert limit >= 0
        self.limit = limit

    @property
    def output(self):
        return self.children[0].output

    @property
    def output_ordering(self):
        return self.children[0].output_ordering


class GlobalLimitExec(_CpuNode):
    """First `limit` rows after `offset` of the single partition
    (limit.scala GlobalLimitExec)."""

    def __init__(self, limit: int, child, offset: int = 0):
        super().__init__(child)
        assert limit >= 0 and offset >= 0
        self.limit, self.offset = limit, offset

    @property
    def output(self):
        return self.children[0].output

    @property
    def output_ordering(self):
        return self.children[0].output_ordering


class CollectLimitExec(GlobalLimitExec):
    """limit.scala CollectLimitExec: the same shape, as the plan's root."""


class HashAggregateExec(_CpuNode):
    """group_key: one column name or a tuple of names (composite GROUP BY,
    the UnsafeRow key-tuple case)."""

    def __init__(self, group_key, aggs: List[Tuple[str, str]], mode: str, child,
                 capacity: Optional[int] = None,
                 decimal_precision: Optional[Dict[str, int]] = None):
        super().__init__(child)
        self.group_key, self.aggs, self.mode = group_key, aggs, mode
        self.capacity = capacity
        self.decimal_precision = decimal_precision

    @property
    def group_keys(self):
        return (self.group_key,) if isinstance(self.group_key, str) else tuple(self.group_key)

    @property
    def output(self):
        out = list(self.group_keys)
        for fn, col in self.aggs:
            if fn == "sum_decimal":   # 128-bit result as (lo, hi) int64 words
                out += [f"sum_decimal_lo({col})", f"sum_decimal_hi({col})"]
            else:
                out.append(f"{fn}({col})")
        return out


def _join_key_tuples(left_key, right_key):
    """Join keys are one column name or a sequence of 1-4 names, the same
    count on both sides (HashJoin.scala leftKeys/rightKeys: Seq[Expression];
    the engine's composite table holds up to 4 int64 columns)."""
    lk = (left_key,) if isinstance(left_key, str) else tuple(left_key)
    rk = (right_key,) if isinstance(right_key, str) else tuple(right_key)
    assert len(lk) == len(rk), f"join key counts differ: {lk} vs {rk}"
    assert 1 <= len(lk) <= 4, f"join on {len(lk)} key columns (1-4 supported)"
    return lk, rk


def _check_join_condition(condition, left, right, null_aware_anti=False):
    """The residual join condition of a hash / sort-merge join node
    (HashJoin.scala boundCondition; SortMergeJoinExec.condition): None, or a
    Pred each of whose columns is on exactly one side."""
    if condition is None:
        return None
    if not isinstance(condition, Pred):
        raise ValueError(f"join condition {condition!r} is not a predicate")
    if null_aware_anti:
        # BroadcastHashJoinExec.scala: isNullAwareAntiJoin requires
        # condition.isEmpty
        raise ValueError("the null-aware anti join takes no condition")
    lo, ro = left.output, right.output
    for name in columns_of(condition):
        if name in lo and name in ro:
            raise ValueError(f"join condition column {name!r} is ambiguous: "
                             f"both sides have it")
        if name not in lo and name not in ro:
            raise ValueError(f"join condition reads unknown column {name!r}")
    return condition


class _JoinKeys:
    """left_key / right_key keep whatever the constructor was given (a name
    or a sequence); left_keys / right_keys are always tuples."""

    @property
    def left_keys(self):
        return _join_key_tuples(self.left_key, self.right_key)[0]

    @property
    def right_keys(self):
        return _join_key_tuples(self.left_key, self.right_key)[1]


class ShuffledHashJoinExec(_JoinKeys, _CpuNode):
    """join_type: "inner" | "left_outer" | "right_outer" | "left_semi" |
    "left_anti" (ShuffledHashJoinExec.scala joinType; the preserved side
    must stream, so left-preserving types build on the right and
    vice versa). left_key / right_key: a column name, or 1-4 names per side
    for a composite equi-join. condition: the non-equi remainder of the ON
    clause (a predicate over columns of both children), or None."""

    def __init__(self, left_key, right_key, build_side: str,
                 left, right, join_type: str = "inner", condition=None):
        super().__init__(left, right)
        _join_key_tuples(left_key, right_key)
        self.left_key, self.right_key, self.build_side = left_key, right_key, build_side
        self.join_type = join_type
        self.condition = _check_join_condition(condition, left, right)

    @property
    def output(self):
        if self.join_type in ("left_semi", "left_anti"):
            return self.children[0].output
        return self.children[0].output + self.children[1].output


class SortMergeJoinExec(_JoinKeys, _CpuNode):
    """CPU placeholder (joins/SortMergeJoinExec.scala:135). The GPU plan
    replaces SMJ with the hash join — both fill the same equi-join plan slot
    with identical ClusteredDistribution requirements (ShuffledJoin.scala:
    57-69), and on GPU the hash build/probe dominates sort+merge for
    co-partitioned batches."""

    def __init__(self, left_key, right_key, left, right,
                 join_type: str = "inner", condition=None):
        super().__init__(left, right)
        _join_key_tuples(left_key, right_key)
        self.left_key, self.right_key = left_key, right_key
        self.join_type = join_type
        self.condition = _check_join_condition(condition, left, right)

    @property
    def output(self):
        return self.children[0].output + self.children[1].output

    @property
    def output_ordering(self):
        # SMJ's output ordering follows the join type
        # (SortMergeJoinExec.scala outputOrdering via getKeyOrdering:
        # inner/left-ish -> left keys, RightOuter -> right keys,
        # FullOuter -> none)
        if self.join_type == "full_outer":
            return []
        if self.join_type == "right_outer":
            return [SortOrder(k) for k in self.right_keys]
        return [SortOrder(k) for k in self.left_keys]


class ShuffleExchangeExec(_CpuNode):
    def __init__(self, keys: Tuple[str, ...], num_partitions: int, child):
        super().__init__(child)
        self.keys, self.num_partitions = keys, num_partitions

    @property
    def output(self):
        return self.children[0].output


def _filter_args(args):
    """FilterExec(col, op, literal, child) or FilterExec(condition, child)
    -> (col, op, literal, condition, child); the form not used is None."""
    if len(args) == 4:
        return args[0], args[1], args[2], None, args[3]
    if len(args) == 2:
        if not isinstance(args[0], Pred):
            raise TypeError(f"filter condition {args[0]!r} is not a predicate")
        return None, None, None, args[0], args[1]
    raise TypeError("expected (col, op, literal, child) or (condition, child)")


class FilterExec(_CpuNode):
    """FilterExec(col, op, literal, child): one col OP literal comparison.
    FilterExec(condition, child): a predicate tree (spark_amd.predicate), the
    shape of basicPhysicalOperators.scala FilterExec(condition, child)."""

    def __init__(self, *args):
        col, op, literal, condition, child = _filter_args(args)
        super().__init__(child)
        self.col, self.op, self.literal = col, op, literal
        self.condition = condition

    @property
    def output(self):
        return self.children[0].output


def _is_expr_entry(p) -> bool:
    """(out_name, expr): the expression form of a projection entry"""
    return isinstance(p, tuple) and len(p) == 2 and expression.is_expr(p[1])


class ProjectExec(_CpuNode):
    """projections: list of (out_name, a, op, b_or_None, literal_or_None),
    (out_name, expr) with an expression tree of spark_amd.expression, plus
    pass-through column names."""

    def __init__(self, projections, child):
        super().__init__(child)
        self.projections = projections

    @property
    def output(self):
        return [p if isinstance(p, str) else p[0] for p in self.projections]


WINDOW_RANK_FNS = ("row_number", "rank", "dense_rank")
WINDOW_AGG_FNS = ("count", "sum", "min", "max", "avg")
WINDOW_SHIFT_FNS = ("lag", "lead")
WINDOW_VALUE_FNS = ("first_value", "last_value")
WINDOW_FRAMES = ("rows", "range", "partition")


@dataclass(frozen=True)
class RowsBetween:
    """ROWS BETWEEN lo AND hi: signed row offsets from the current row
    (negative PRECEDING, 0 CURRENT ROW, positive FOLLOWING), None for
    UNBOUNDED PRECEDING (lo) / UNBOUNDED FOLLOWING (hi). Row i of the
    partition [pb, pe] sees the rows max(pb, i + lo) .. min(pe, i + hi); the
    frame is empty when that range is."""
    lo: Optional[int]
    hi: Optional[int]


@dataclass
class WindowExpr:
    """One window expression of a WindowExec (WindowExec.scala
    windowExpression). fn: row_number / rank / dense_rank / count / sum / min
    / max / avg / lag / lead. col: the argument column, None for the rank
    functions and COUNT(*). frame, for the aggregates: "rows" (ROWS BETWEEN
    UNBOUNDED PRECEDING AND CURRENT ROW), "range" (RANGE ... CURRENT ROW:
    peers share a value) or "partition" (the whole partition); None is
    Spark's default, "range" with an ORDER BY and "partition" without one.
    A RowsBetween(lo, hi) is a sliding ROWS frame; it needs an ORDER BY, as
    do first_value / last_value (ignoreNulls = false), which take any frame
    an aggregate takes. offset / default are lag's and lead's (ignoreNulls =
    false)."""
    fn: str
    col: Optional[str]
    name: str
    frame: object = None
    offset: int = 1
    default: object = None


def _rows_between_check(e, order_spec):
    """a RowsBetween frame on expression e, as gpuq_window_slide takes it."""
    f = e.frame
    if e.fn in WINDOW_RANK_FNS + WINDOW_SHIFT_FNS:
        raise ValueError(f"window: {e.fn} takes no frame, got {f!r}")
    for b in (f.lo, f.hi):
        if b is None:
            continue
        if isinstance(b, bool) or not isinstance(b, int):
            raise ValueError(f"window: frame offset {b!r} is not an int")
        if not -(1 << 31) <= b < (1 << 31):
            raise ValueError(f"window: frame offset {b} does not fit int32")
    if f.lo is not None and f.hi is None:
        raise ValueError(f"window: {f!r} (k .. UNBOUNDED FOLLOWING) unsupported")
    if f.lo is not None and f.lo > f.hi:
        raise ValueError(f"window: {f!r} has lo > hi")
    if not order_spec:
        raise ValueError(f"window: a sliding frame {f!r} needs an ORDER BY")


def _window_check(window_exprs, partition_spec, order_spec, child):
    """the constructor checks shared by WindowExec and GpuWindowExec;
    returns (window_exprs, partition_spec, order_spec) as lists."""
    window_exprs = list(window_exprs)
    partition_spec = ([partition_spec] if isinstance(partition_spec, str)
                      else list(partition_spec))
    order_spec = ([order_spec] if isinstance(order_spec, SortOrder)
                  else list(order_spec))
    names = list(child.output)
    for e in window_exprs:
        if e.fn not in (WINDOW_RANK_FNS + WINDOW_AGG_FNS + WINDOW_SHIFT_FNS
                        + WINDOW_VALUE_FNS):
            raise ValueError(f"window: unknown function {e.fn!r}")
        if isinstance(e.frame, RowsBetween):
            _rows_between_check(e, order_spec)
        elif e.frame is not None and e.frame not in WINDOW_FRAMES:
            raise ValueError(f"window: unknown frame {e.frame!r}")
        if e.fn in WINDOW_VALUE_FNS and not order_spec:
            raise ValueError(f"window: {e.fn} needs an ORDER BY")
        if e.fn in WINDOW_RANK_FNS and e.col is not None:
            raise ValueError(f"window: {e.fn} takes no column")
        if e.fn not in WINDOW_RANK_FNS and e.fn != "count" and e.col is None:
            raise ValueError(f"window: {e.fn} needs a column")
        if e.fn in WINDOW_RANK_FNS + WINDOW_SHIFT_FNS and not order_spec:
            raise ValueError(f"window: {e.fn} needs an ORDER BY")
        if e.name in names:
            raise ValueError(f"window: output column {e.name!r} already exists")
        names.append(e.name)
    return window_exprs, partition_spec, order_spec


class _WindowSpec:
    """what WindowExec and GpuWindowExec share: output = child's output plus
    one column per expression, the child's ordering kept, rows clustered on
    the partition keys and sorted by (partition keys ascending, order spec)
    (WindowExec.scala requiredChildDistribution / requiredChildOrdering)."""

    @property
    def output(self):
        return list(self.children[0].output) + [e.name for e in self.window_exprs]

    @property
    def output_ordering(self):
        return self.children[0].output_ordering

    def required_child_distribution(self):
        return [Distribution("clustered", tuple(self.partition_spec))]

    def required_child_ordering(self):
        return [SortOrder(k) for k in self.partition_spec] + list(self.order_spec)

    def frame_of(self, e: "WindowExpr"):
        """the frame an aggregate runs under: Spark's default when none is
        given, and "range" without an ORDER BY is the whole partition (every
        row is a peer of every other). A RowsBetween is returned as it is."""
        frame = e.frame or ("range" if self.order_spec else "partition")
        if frame == "range" and not self.order_spec:
            frame = "partition"
        return frame


class WindowExec(_WindowSpec, _CpuNode):
    """window_exprs: WindowExprs; partition_spec: column names (PARTITION
    BY); order_spec: SortOrders (ORDER BY) (execution/window/
    WindowExec.scala)."""

    def __init__(self, window_exprs, partition_spec, order_spec, child):
        super().__init__(child)
        self.window_exprs, self.partition_spec, self.order_spec = \
            _window_check(window_exprs, partition_spec, order_spec, child)


class RangeExec(_CpuNode):
    """CPU placeholder for RangeExec (basicPhysicalOperators.scala:630)."""

    def __init__(self, n: int, start: int = 0, step: int = 1, name: str = "id"):
        super().__init__()
        self.n, self.start, self.step, self.name = n, start, step, name

    @property
    def output(self):
        return [self.name]


class BroadcastHashJoinExec(_JoinKeys, _CpuNode):
    """CPU placeholder (joins/BroadcastHashJoinExec.scala:40): equi-join
    with a broadcast (small) build side; inner unless join_type says
    otherwise."""

    def __init__(self, left_key, right_key, build_side: str,
                 left, right, join_type: str = "inner", condition=None):
        super().__init__(left, right)
        assert build_side in ("left", "right")
        _join_key_tuples(left_key, right_key)
        self.left_key, self.right_key, self.build_side = left_key, right_key, build_side
        self.join_type = join_type
        self.condition = _check_join_condition(condition, left, right)

    @property
    def output(self):
        return self.children[0].output + self.children[1].output


class BroadcastExchangeExec(_CpuNode):
    def __init__(self, child):
        super().__init__(child)

    @property
    def output(self):
        return self.children[0].output


class ParquetScanExec(_CpuNode):
    """CPU placeholder for FileSourceScanExec over a Parquet file
    (DataSourceScanExec.scala:735)."""

    def __init__(self, path: str, columns: Optional[List[str]] = None):
        super().__init__()
        self.path, self.columns = path, columns

    @property
    def output(self):
        if self.columns:
            return list(self.columns)
        import pyarrow.parquet as pq
        return [f.name for f in pq.ParquetFile(self.path).schema_arrow]


class GpuParquetScanExec(SparkPlan):
    """Replaces FileSourceScanExec's columnar Parquet path (SURVEY
    §8(f).1 full form; VectorizedParquetRecordReader.java:67): pyarrow
    decodes row groups on the host, columns normalize to the engine's
    types (decimal(<=18,s) -> scaled int64, date32 -> int64 days,
    dictionary strings -> int64 ids) and ride pinned-host -> HBM copies
    with their Arrow validity bitmaps. One ColumnarBatch per row group.
    Dictionaries for string columns are exposed on `dictionaries` after
    execution (host-side decode concern, not engine compute)."""

    def __init__(self, path: str, columns: Optional[List[str]] = None):
        super().__init__()
        self.path, self.columns = path, columns
        self.dictionaries: Dict[str, list] = {}

    @property
    def output(self):
        return ParquetScanExec(self.path, self.columns).output

    @property
    def supports_columnar(self):
        return True

    def execute_columnar(self):
        import pyarrow.parquet as pq
        from .parquet_io import read_row_group_to_device
        pf = pq.ParquetFile(self.path)
        for rg in range(pf.num_row_groups):
            cols, validity, dicts = read_row_group_to_device(
                pf, rg, columns=self.columns)
            self.dictionaries.update(dicts)
            yield ColumnarBatch(cols, validity=validity or None)


class InputBatches(SparkPlan):
    """Leaf: pre-materialized device batches (scan stand-in)."""

    def __init__(self, batches: List[ColumnarBatch]):
        super().__init__()
        self._batches = batches

    @property
    def output(self):
        return list(self._batches[0].columns().keys())

    @property
    def supports_columnar(self):
        return True

    def execute_columnar(self):
        yield from self._batches


# ---------------- GPU exec nodes ----------------

def concat_batches(batches):
    """Concatenate a partition's batches into one (whole-partition
    operators: sort, join build). Validity bitmaps concatenate through
    the u8 wire form (row counts are not byte-aligned)."""
    from . import gpuq
    if len(batches) == 1:
        return batches[0]
    names = list(batches[0].columns().keys())
    cols = {n: torch.cat([b.column(n) for b in batches]) for n in names}
    validity = {}
    for n in names:
        if any(b.validity(n) is not None for b in batches):
            parts = []
            for b in batches:
                v = b.validity(n)
                nn = b.num_rows()
                if v is None:
                    parts.append(torch.ones(nn, dtype=torch.uint8,
                                            device="cuda"))
                else:
                    parts.append(gpuq.bits_to_u8(v, nn))
            validity[n] = gpuq.u8_to_bits(torch.cat(parts))
    for b in batches:
        b.close()
    return ColumnarBatch(cols, validity=validity or None)


class GpuSortExec(SparkPlan):
    """Replaces SortExec (SortExec.scala:75-126): radix-eligible
    int64/float64 keys (canUseRadixSort analog). Multi-key ORDER BY
    composes as successive STABLE radix passes from the last sort key to
    the first — the stability the kernel guarantees makes the composition
    exactly the lexicographic order SortExec produces."""

    def __init__(self, sort_order, global_sort: bool, child):
        super().__init__(child)
        self.sort_order, self.global_sort = sort_order, global_sort

    @property
    def sort_orders(self):
        return ([self.sort_order] if isinstance(self.sort_order, SortOrder)
                else list(self.sort_order))

    @property
    def output(self):
        return self.children[0].output

    @property
    def output_ordering(self):
        return self.sort_orders

    @property
    def supports_columnar(self):
        return True

    def required_child_distribution(self):
        if self.global_sort:
            return [Distribution("ordered", tuple(o.key for o in self.sort_orders))]
        return [Distribution("unspecified")]

    @staticmethod
    def _sort_pass(batch, o):
        """one stable sort of the whole batch by o (keys + payload +
        validity bitmaps through the same permutation)."""
        from . import gpuq
        keys = batch.column(o.key)
        kvalid = batch.validity(o.key)
        perm, skeys = gpuq.sort_perm(keys, desc=o.descending,
                                     nulls_first=o.nulls_first,
                                     key_validity=kvalid)
        cols = {o.key: skeys}
        validity = {}
        if kvalid is not None:
            validity[o.key] = gpuq.gather_bits(kvalid, perm)
        for name, t in batch.columns().items():
            if name != o.key:
                cols[name] = gpuq.gather(t, perm)
                v = batch.validity(name)
                if v is not None:
                    validity[name] = gpuq.gather_bits(v, perm)
        batch.close()
        return ColumnarBatch(cols, validity=validity or None)

    def execute_columnar(self):
        import torch.distributed as dist
        from . import gpuq  # noqa: F401 (engine presence check)
        orders = self.sort_orders
        # SortExec sorts the WHOLE partition (one sorter per task): a
        # multi-batch child (e.g. Parquet row groups) concatenates first
        batches = list(self.children[0].execute_columnar())
        assert batches, "sort over a batchless child"
        for batch in [concat_batches(batches)]:
            if (self.global_sort and dist.is_initialized()
                    and dist.get_world_size() > 1):
                # global ORDER BY: range exchange on the PRIMARY key first
                # (the EnsureRequirements RangePartitioning insertion,
                # exchange/EnsureRequirements.scala:296); after the local
                # sort below, rank-major order is global order. Multi-key
                # global sort would need tie-aware range bounds — the
                # single-key contract is asserted.
                assert len(orders) == 1, \
                    "multi-key global ORDER BY across ranks unsupported"
                from .exchange import range_exchange
                o = orders[0]
                payload = {n_: t for n_, t in batch.columns().items()
                           if n_ != o.key}
                validity = {n_: batch.validity(n_) for n_ in batch.columns()
                            if batch.validity(n_) is not None}
                k, payload, validity = range_exchange(
                    batch.column(o.key), payload, desc=o.descending,
                    nulls_first=o.nulls_first,
                    key_validity=batch.validity(o.key),
                    validity={n_: v for n_, v in validity.items()
                              if n_ != o.key},
                    key_name=o.key)
                cols = {o.key: k}
                cols.update(payload)
                batch.close()
                batch = ColumnarBatch(cols, validity=validity or None)
            for o in reversed(orders):
                batch = self._sort_pass(batch, o)
            yield batch


def _gather_batch(batch, perm):
    """every column and bitmap of batch through one row permutation (gather
    / gather_bits: the bitmap comes out clean, nothing is sliced)."""
    from . import gpuq
    cols, validity = {}, {}
    for name, t in batch.columns().items():
        cols[name] = gpuq.gather(t, perm)
        v = batch.validity(name)
        if v is not None and perm.numel():
            validity[name] = gpuq.gather_bits(v, perm)
    batch.close()
    return ColumnarBatch(cols, validity=validity or None)


def _row_range(lo: int, hi: int):
    """identity permutation over rows [lo, hi) (int32, the gather kernels'
    u32 row ids)."""
    return torch.arange(lo, hi, dtype=torch.int32, device="cuda")


# TakeOrdered runs sort + head instead of the select when
# limit > rows * TOPK_SORT_FRACTION: the largest measured k/n at which
# topk_perm still beats sort + head beyond the run-to-run spread, for int64
# and float64 keys at 2^26 and 2^28 rows (DESIGN.md "Top-K (radix select)",
# table rows "n/8"; at n/2 the sort wins).
TOPK_SORT_FRACTION = 1.0 / 8


class GpuTakeOrderedAndProjectExec(SparkPlan):
    """Replaces TakeOrderedAndProjectExec (limit.scala): per child batch, a
    radix select on the first sort key (gpuq.topk_candidates; boundary ties
    kept whole when further keys break them) leaves at most limit rows plus
    ties, which alone are gathered and stable-sorted from the last key to the
    first; the heads of all batches concatenate in batch order and reduce once
    more the same way. Every stage is stable and keeps input order, so the
    result equals the first `limit` rows of GpuSortExec over the concatenated
    child, boundary ties included, while memory stays bounded by batches x
    limit rows. Above limit > rows * TOPK_SORT_FRACTION a batch is sorted
    whole instead (identical result)."""

    def __init__(self, limit: int, sort_order, project_list, child):
        super().__init__(child)
        assert limit >= 0
        self.limit, self.sort_order = limit, sort_order
        self.project_list = project_list

    @property
    def sort_orders(self):
        return ([self.sort_order] if isinstance(self.sort_order, SortOrder)
                else list(self.sort_order))

    @property
    def output(self):
        if self.project_list is None:
            return self.children[0].output
        return list(self.project_list)

    @property
    def output_ordering(self):
        return self.sort_orders

    @property
    def supports_columnar(self):
        return True

    def _head(self, batch):
        """the first min(limit, rows) rows of batch in sort order."""
        from . import gpuq
        orders = self.sort_orders
        rows = batch.num_rows()
        keep = min(self.limit, rows)
        if rows == 0:
            return batch
        if self.limit <= rows * TOPK_SORT_FRACTION:
            o = orders[0]
            rids, _, _ = gpuq.topk_candidates(
                batch.column(o.key), self.limit, desc=o.descending,
                nulls_first=o.nulls_first, key_validity=batch.validity(o.key),
                keep_ties=len(orders) > 1)
            batch = _gather_batch(batch, rids)
        for o in reversed(orders):
            batch = GpuSortExec._sort_pass(batch, o)
        if batch.num_rows() > keep:
            batch = _gather_batch(batch, _row_range(0, keep))
        return batch

    def execute_columnar(self):
        import torch.distributed as dist
        from . import gpuq  # noqa: F401 (engine presence check)
        # the merge across ranks would be a broadcast_gather of the local
        # heads plus one more reduction
        assert not (dist.is_initialized() and dist.get_world_size() > 1), \
            "multi-rank TakeOrdered unsupported"
        child = self.children[0].execute_columnar()
        if self.limit == 0:
            first = next(child)
            heads = [ColumnarBatch({n_: t[:0]
                                    for n_, t in first.columns().items()})]
            first.close()
        else:
            heads = [self._head(b) for b in child]
        assert heads, "TakeOrdered over a batchless child"
        out = heads[0] if len(heads) == 1 else self._head(concat_batches(heads))
        if self.project_list is not None:
            cols = {n_: out.column(n_) for n_ in self.project_list}
            validity = {n_: out.validity(n_) for n_ in self.project_list
                        if out.validity(n_) is not None}
            out = ColumnarBatch(cols, validity=validity or None)
        yield out


class GpuLocalLimitExec(SparkPlan):
    """Replaces LocalLimitExec (limit.scala): the first `limit` rows across
    the child's batches in order; no batch is pulled once they are out. Data
    columns are tensor slices; bitmaps go through gather_bits with an
    identity row range, because the cut is not byte-aligned."""

    offset = 0

    def __init__(self, limit: int, child):
        super().__init__(child)
        assert limit >= 0
        self.limit = limit

    @property
    def output(self):
        return self.children[0].output

    @property
    def output_ordering(self):
        return self.children[0].output_ordering

    @property
    def supports_columnar(self):
        return True

    @staticmethod
    def _slice(batch, lo: int, hi: int):
        from . import gpuq
        cols = {n_: t[lo:hi] for n_, t in batch.columns().items()}
        validity = {}
        if hi > lo:
            rows = _row_range(lo, hi)
            for n_ in cols:
                v = batch.validity(n_)
                if v is not None:
                    validity[n_] = gpuq.gather_bits(v, rows)
        batch.close()
        return ColumnarBatch(cols, validity=validity or None)

    def execute_columnar(self):
        from . import gpuq  # noqa: F401 (engine presence check)
        skip, remaining = self.offset, self.limit
        empty = None            # schema carrier if no row comes out
        emitted = False
        for batch in self.children[0].execute_columnar():
            rows = batch.num_rows()
            lo = min(skip, rows)
            skip -= lo
            take = min(rows - lo, remaining)
            remaining -= take
            if take == rows:
                emitted = True
                yield batch
            elif take > 0:
                emitted = True
                yield self._slice(batch, lo, lo + take)
            elif empty is None:
                empty = self._slice(batch, 0, 0)
            if remaining == 0:
                break
        if not emitted:
            assert empty is not None, "limit over a batchless child"
            yield empty


class GpuGlobalLimitExec(GpuLocalLimitExec):
    """Replaces GlobalLimitExec (limit.scala): the first `limit` rows after
    `offset` of the single partition (AllTuples)."""

    def __init__(self, limit: int, child, offset: int = 0):
        super().__init__(limit, child)
        assert offset >= 0
        self.offset = offset

    def required_child_distribution(self):
        return [Distribution("all_tuples")]

    def execute_columnar(self):
        import torch.distributed as dist
        assert not (dist.is_initialized() and dist.get_world_size() > 1), \
            "multi-rank GlobalLimit unsupported"
        yield from super().execute_columnar()


class GpuCollectLimitExec(GpuGlobalLimitExec):
    """Replaces CollectLimitExec: GlobalLimit as the plan's root."""


class GpuHashAggregateExec(SparkPlan):
    """Replaces HashAggregateExec (HashAggregateExec.scala:99-151).
    mode: "partial" | "final" | "complete" (AggUtils.scala:126-195 split).

    Partial mode outputs the aggregation BUFFER columns (the
    aggBufferAttributes analog, e.g. Average.scala's (sum, count) pair;
    Sum/Min/Max carry a count companion for NULL-ness), which travel
    through the exchange; final mode merges them exactly: partial sums
    merge with the same-dtype SUM op (int64 counts merge as wrapping i64
    adds, never as f64 — Sum.scala mergeExpressions / Count.scala), and
    partial MIN/MAX merge with MIN/MAX over non-NULL partials. A result is
    NULL iff the merged count of non-null inputs is 0.

    "sum_decimal" is the exact SUM over a decimal(p <= 18, s) column carried
    as scaled int64 (Sum.scala's Decimal path; "sum" on the same column
    keeps the wrapping LongType result). Its buffer is a 128-bit (lo, hi)
    word pair plus a count — dsum_lo(c), dsum_hi(c), count(c) — merged in
    final mode as a 128-bit add. Final/complete output is two int64 columns
    sum_decimal_lo(c), sum_decimal_hi(c) sharing one validity bitmap: valid
    iff count(c) > 0 and |sum| < 10^min(38, p+10) (non-ANSI overflow is
    NULL). decimal_precision maps column -> input precision p (default 18).

    group_key: one name or a tuple (composite GROUP BY via
    gpuq_hash_agg_keys; the reference's UnsafeRow key-tuple path,
    UnsafeFixedWidthAggregationMap.java:39)."""

    def __init__(self, group_key, aggs: List[Tuple[str, str]], mode: str,
                 child, capacity: Optional[int] = None,
                 decimal_precision: Optional[Dict[str, int]] = None):
        super().__init__(child)
        assert mode in ("partial", "final", "complete")
        self.group_key, self.aggs, self.mode = group_key, aggs, mode
        self.capacity = capacity
        self.decimal_precision = decimal_precision
        fns = {fn for fn, _ in self.aggs}
        assert fns <= {"sum", "count", "count*", "avg", "min", "max",
                       "sum_decimal"}, f"unsupported aggs {fns}"
        for c, p in (decimal_precision or {}).items():
            assert 1 <= p <= 18, f"decimal precision {p} of {c} not in [1,18]"

    @property
    def group_keys(self):
        if self.group_key is None:
            return ()
        return (self.group_key,) if isinstance(self.group_key, str) else tuple(self.group_key)

    @staticmethod
    def agg_out_name(fn: str, col) -> str:
        return "count(1)" if fn == "count*" else f"{fn}({col})"

    @classmethod
    def _out_names(cls, fn: str, col) -> List[str]:
        """final/complete output columns of one aggregate."""
        if fn == "sum_decimal":
            return [f"sum_decimal_lo({col})", f"sum_decimal_hi({col})"]
        return [cls.agg_out_name(fn, col)]

    def _result_precision(self, col: str) -> int:
        # Sum.scala resultType: decimal(min(38, p + 10), s)
        return min(38, (self.decimal_precision or {}).get(col, 18) + 10)

    def _buffer_cols(self, fn: str, col: str) -> List[str]:
        """agg buffer column names (partial-mode output schema)."""
        if fn == "sum_decimal":
            return [f"dsum_lo({col})", f"dsum_hi({col})", f"count({col})"]
        if fn == "sum":
            return [f"sum({col})", f"count({col})"]
        if fn == "count":
            return [f"count({col})"]
        if fn == "count*":
            return ["count(1)"]
        if fn == "avg":
            return [f"avg_sum({col})", f"count({col})"]
        return [f"{fn}({col})", f"count({col})"]  # min/max

    @property
    def output(self):
        keys = list(self.group_keys)
        if self.mode == "partial":
            seen, bufs = set(), []
            for fn, col in self.aggs:
                for b in self._buffer_cols(fn, col):
                    if b not in seen:
                        seen.add(b); bufs.append(b)
            return keys + bufs
        return keys + [n for fn, col in self.aggs
                       for n in self._out_names(fn, col)]

    @property
    def supports_columnar(self):
        return True

    def required_child_distribution(self):
        if self.mode == "final":
            return [Distribution("clustered", self.group_keys)]
        return [Distribution("unspecified")]

    def execute_columnar(self):
        # HashAggregateExec aggregates the WHOLE partition (one
        # TungstenAggregationIterator per task), not one table per input
        # batch: all child batches accumulate into a single hash table
        # (the kernel's first_batch/finalize contract) and ONE result
        # batch emits per partition.
        batches = list(self.children[0].execute_columnar())
        assert batches, "aggregate over a batchless child"
        yield self._agg_batches(batches)

    # ---- spec construction ----

    def _input_specs(self, batch):
        """specs over RAW input rows (partial/complete) + per-buffer slots.
        Returns (specs, buffer_slot: name -> accumulator word index; a
        128-bit spec owns two adjacent words)."""
        from . import gpuq
        specs, slot = [], {}

        def add(name, spec, hi_name=None):
            if name not in slot:
                slot[name] = self._nwords(specs)
                if hi_name is not None:
                    slot[hi_name] = slot[name] + 1
                specs.append(spec)

        for fn, col in self.aggs:
            if fn == "count*":
                add("count(1)", ("count*",))
                continue
            t = batch.column(col)
            v = batch.validity(col)
            if fn == "avg":
                ts = gpuq.cast_i64_f64(t) if t.dtype == torch.int64 else t
                add(f"avg_sum({col})", ("sum", ts, v))
                add(f"count({col})", ("count", t, v))
            elif fn == "count":
                add(f"count({col})", ("count", t, v))
            elif fn == "sum_decimal":
                # the count companion is unconditional: the buffer layout
                # must not depend on a batch's validity or on the mode
                add(f"dsum_lo({col})", ("sum_dec128", t, v), f"dsum_hi({col})")
                add(f"count({col})", ("count", t, v))
            else:
                add(f"{fn}({col})", (fn, t, v))
                # count companion tracks NULL-ness (result NULL iff no
                # non-null input). In complete mode over a non-null column
                # every group is non-empty, so the companion is redundant.
                if v is not None or self.mode != "complete":
                    add(f"count({col})", ("count", t, v))
        if not specs:
            # pure GROUP BY (no aggregate expressions — the SELECT DISTINCT
            # shape): the kernel wants >= 1 spec; count rows and discard
            add("__rows__", ("count*",))
        return specs, slot

    def _merge_specs(self, batch):
        """specs over PARTIAL BUFFER columns (final mode): same-dtype SUM
        for sums/counts, MIN/MAX over non-NULL partials."""
        specs, slot = [], {}

        def add(name, kind, hi_name=None):
            if name in slot:
                return
            t = batch.column(name)
            v = batch.validity(name)
            slot[name] = self._nwords(specs)
            if hi_name is None:
                specs.append((kind, t, v))
            else:
                slot[hi_name] = slot[name] + 1
                specs.append((kind, t, v, batch.column(hi_name)))

        for fn, col in self.aggs:
            for b in self._buffer_cols(fn, col):
                if b.startswith("dsum_lo"):
                    add(b, "merge_dec128", f"dsum_hi({col})")
                elif b.startswith("dsum_hi"):
                    pass              # the hi word of the pair above
                elif b.startswith("count"):
                    add(b, "sum")     # SUM_I64: exact merged counts
                elif b.startswith("min"):
                    add(b, "min")
                elif b.startswith("max"):
                    add(b, "max")
                else:
                    add(b, "sum")
        if not specs:
            slot["__rows__"] = len(specs)
            specs.append(("count*",))
        return specs, slot

    @staticmethod
    def _nwords(specs) -> int:
        """accumulator words (= kernel specs) a spec list expands to."""
        return sum(2 if s[0] in ("sum_dec128", "merge_dec128") else 1
                   for s in specs)

    def _agg_batches(self, batches):
        from . import gpuq
        keys = self.group_keys
        total = sum(b.num_rows() for b in batches)
        cap = self.capacity or (1 << max(10, int(total).bit_length()))
        if self.mode == "final":
            per_specs = [self._merge_specs(b) for b in batches]
        else:
            per_specs = [self._input_specs(b) for b in batches]
        slot = per_specs[0][1]
        mg = min(total, cap) + 2
        nspecs = self._nwords(per_specs[0][0])
        last_i = len(batches) - 1
        if len(keys) == 0:
            # global aggregate (empty grouping): one output row even on
            # empty input — COUNT 0, SUM/MIN/MAX/AVG NULL (AggUtils
            # emptyInputAggBuffer)
            if total == 0:
                cols, validity = {}, {}
                dev = "cuda"
                b0 = batches[0]

                def src_dtype(name):
                    base = name.split("(", 1)[1][:-1]
                    try:
                        return b0.column(base).dtype
                    except KeyError:
                        return torch.float64
                names = (list(slot) if self.mode == "partial"
                         else [n for fn, col in self.aggs
                               for n in self._out_names(fn, col)])
                for name in names:
                    if name.startswith("count"):
                        cols[name] = torch.zeros(1, dtype=torch.int64, device=dev)
                    elif name.startswith(("dsum_", "sum_decimal_")):
                        cols[name] = torch.zeros(1, dtype=torch.int64, device=dev)
                        validity[name] = torch.zeros(1, dtype=torch.uint8,
                                                     device=dev)
                    elif name.startswith(("min(", "max(", "sum(")):
                        cols[name] = torch.zeros(1, dtype=src_dtype(name),
                                                 device=dev)
                        validity[name] = torch.zeros(1, dtype=torch.uint8,
                                                     device=dev)
                    else:  # avg / avg_sum: f64
                        cols[name] = torch.zeros(1, dtype=torch.float64,
                                                 device=dev)
                        validity[name] = torch.zeros(1, dtype=torch.uint8,
                                                     device=dev)
                for b in batches:
                    b.close()
                return ColumnarBatch(cols, validity=validity or None)
            ws = gpuq.agg_multi_workspace(cap, nspecs)
            res = None
            for i, (b, (specs, _)) in enumerate(zip(batches, per_specs)):
                key0 = gpuq.range_i64(b.num_rows(), 0, 0)  # one group
                res = gpuq.hash_agg_multi(key0, specs, cap, workspace=ws,
                                          first_batch=(i == 0),
                                          finalize=(i == last_i),
                                          max_groups=mg)
            ok, okv, accs = res
            key_cols, key_valid = {}, {}
        elif len(keys) == 1:
            k = keys[0]
            ws = gpuq.agg_multi_workspace(cap, nspecs)
            res = None
            any_kv = any(b.validity(k) is not None for b in batches)
            for i, (b, (specs, _)) in enumerate(zip(batches, per_specs)):
                res = gpuq.hash_agg_multi(
                    b.column(k), specs, cap, workspace=ws,
                    key_validity=b.validity(k),
                    first_batch=(i == 0), finalize=(i == last_i),
                    max_groups=mg)
            ok, okv, accs = res
            key_cols = {k: ok}
            # NULL-key group: okv==0 row. Only materialize a bitmap when
            # some input batch's key was nullable.
            key_valid = {}
            if any_kv:
                key_valid[k] = gpuq.u8_to_bits(okv)
        else:
            kcs = [[b.column(k) for k in keys] for b in batches]
            kvs = [[b.validity(k) for k in keys] for b in batches]
            packed = None
            if (len(keys) == 2
                    and all(v[0] is None and v[1] is None for v in kvs)
                    and kcs[0][0].dtype == torch.int64
                    and kcs[0][1].dtype == torch.int64):
                # narrow-tuple pack rule: when the GLOBAL key ranges fit,
                # pack (k1,k2) into one int64 so the single-key path
                # (incl. its per-block LDS tables at low cardinality —
                # the TPC-H Q1 (returnflag, linestatus) shape) runs
                # instead of the verify-slot composite table
                mm = [(gpuq.minmax_i64(kc[0]), gpuq.minmax_i64(kc[1]))
                      for kc in kcs]
                if all(a[2] and b_[2] for a, b_ in mm):
                    mn0 = min(a[0] for a, _ in mm)
                    mx0 = max(a[1] for a, _ in mm)
                    mn1 = min(b_[0] for _, b_ in mm)
                    mx1 = max(b_[1] for _, b_ in mm)
                    shift = max(1, int(mx1 - mn1).bit_length())
                    if (mx0 - mn0) < (1 << (63 - shift)):
                        packed = [gpuq.pack2_i64(kc[0], kc[1], mn0, mn1,
                                                 shift) for kc in kcs]
            if packed is not None:
                ws = gpuq.agg_multi_workspace(cap, nspecs)
                res = None
                for i, (pk, (specs, _)) in enumerate(zip(packed, per_specs)):
                    res = gpuq.hash_agg_multi(pk, specs, cap, workspace=ws,
                                              first_batch=(i == 0),
                                              finalize=(i == last_i),
                                              max_groups=mg)
                ok, okv, accs = res
                k0, k1 = gpuq.unpack2_i64(ok, mn0, mn1, shift)
                key_cols = {keys[0]: k0, keys[1]: k1}
                key_valid = {}
            else:
                ws = torch.empty(
                    gpuq.lib().gpuq_hash_agg_keys_workspace_bytes(
                        cap, len(keys), nspecs),
                    dtype=torch.uint8, device="cuda")
                res = None
                for i, (kc, kv, (specs, _)) in enumerate(
                        zip(kcs, kvs, per_specs)):
                    res = gpuq.hash_agg_keys(
                        kc, specs, cap, key_validities=kv, workspace=ws,
                        first_batch=(i == 0), finalize=(i == last_i),
                        max_groups=mg)
                okeys, kmask, accs = res
                key_cols = dict(zip(keys, okeys))
                key_valid = {}
                for c, k in enumerate(keys):
                    if any(v[c] is not None for v in kvs):
                        key_valid[k] = gpuq.maskbit_to_bits(kmask, c)
        cols, validity = dict(key_cols), dict(key_valid)
        if self.mode == "partial":
            for name, j in slot.items():
                if name == "__rows__":
                    continue
                cols[name] = accs[j]
                # partial sum/min/max of an all-NULL group is NULL (its
                # count companion is 0); counts themselves are never NULL
                if not name.startswith("count"):
                    base = name.split("(", 1)[1][:-1]
                    validity[name] = gpuq.nonzero_to_bits(
                        accs[slot[f"count({base})"]])
        else:
            for fn, col in self.aggs:
                out = self.agg_out_name(fn, col)
                if fn == "count*":
                    cols[out] = accs[slot["count(1)"]]
                    continue
                if fn == "count":
                    cols[out] = accs[slot[f"count({col})"]]
                    continue
                cnt_slot = slot.get(f"count({col})")
                if fn == "sum_decimal":
                    lo = accs[slot[f"dsum_lo({col})"]]
                    hi = accs[slot[f"dsum_hi({col})"]]
                    # NULL iff no non-null input OR the sum no longer fits
                    # decimal(min(38, p+10), s) (Sum.scala, non-ANSI)
                    bits = gpuq.dec128_overflow_to_null(
                        lo, hi, self._result_precision(col),
                        gpuq.nonzero_to_bits(accs[cnt_slot]))
                    for n_, t_ in zip(self._out_names(fn, col), (lo, hi)):
                        cols[n_] = t_
                        validity[n_] = bits
                    continue
                if fn == "avg":
                    # Average.evaluateExpression: sum / cast(count)
                    cols[out] = gpuq.project_binop(
                        accs[slot[f"avg_sum({col})"]], "/",
                        b=gpuq.cast_i64_f64(accs[cnt_slot]))
                else:
                    cols[out] = accs[slot[f"{fn}({col})"]]
                # SQL NULL iff no non-null input (Sum/Min/Max/Average.scala);
                # no companion => non-null complete-mode input, always valid
                if cnt_slot is not None:
                    validity[out] = gpuq.nonzero_to_bits(accs[cnt_slot])
        for b in batches:
            b.close()
        return ColumnarBatch(cols, validity=validity or None)


class GpuShuffleExchangeExec(SparkPlan):
    """Replaces ShuffleExchangeExec (ShuffleExchangeExec.scala:277-470):
    on-device radix partition + RCCL all-to-all (spark_amd/exchange.py).
    Runs only under torch.distributed; num_partitions == world size."""

    def __init__(self, keys: Tuple[str, ...], child):
        super().__init__(child)
        assert 1 <= len(keys) <= 4, "1..4 int64 partition key columns"
        self.keys = tuple(keys)

    @property
    def output(self):
        return self.children[0].output

    @property
    def supports_columnar(self):
        return True

    # --- ShuffleExchangeLike mirror (ShuffleExchangeExec.scala:51-151) ---
    # AQE materializes each shuffle stage and reads its map-output stats
    # (AdaptiveSparkPlanExec.scala:784, QueryStageExec.materialize :69);
    # these fields are what a Scala GpuShuffleExchangeExec would return from
    # mapOutputStatisticsFuture/runtimeStatistics, with per-partition byte
    # sizes taken from gpuq_partition_perm's counts (no per-row CPU work).

    @property
    def num_mappers(self) -> int:
        import torch.distributed as dist
        return dist.get_world_size() if dist.is_initialized() else 1

    @property
    def num_partitions(self) -> int:
        return self.num_mappers

    def runtime_statistics(self):
        """(total bytes written, rows) of this rank's map output —
        ShuffleExchangeLike.runtimeStatistics (:146)."""
        return dict(self._stats) if hasattr(self, "_stats") else None

    def get_shuffle_partitions(self, specs):
        """AQE getShuffleRDD(partitionSpecs) analog
        (ShuffleExchangeExec.scala:141, ShuffledRowRDD.scala:33
        CoalescedPartitionSpec): serve coalesced partition ranges straight
        from this rank's partition-contiguous map output, no re-partition.
        specs: list of (start_partition, end_partition) half-open ranges.
        Returns one ColumnarBatch per spec (this rank's contribution)."""
        assert hasattr(self, "_map_outputs"), "execute_columnar first"
        from . import gpuq
        out = []
        for start, end in specs:
            parts = []
            for cols, validity, offsets in self._map_outputs:
                lo, hi = offsets[start], offsets[end]
                sl = {n_: t[lo:hi] for n_, t in cols.items()}
                va = {}
                for n_, u8 in validity.items():
                    if hi > lo:
                        va[n_] = gpuq.u8_to_bits(u8[lo:hi])
                parts.append(ColumnarBatch(sl, validity=va or None))
            out.append(concat_batches(parts) if len(parts) > 1 else parts[0])
        return out

    def execute_columnar(self):
        import torch.distributed as dist
        from . import gpuq
        from .exchange import exchange_columns
        assert dist.is_initialized(), "GpuShuffleExchangeExec needs torch.distributed"
        world = self.num_partitions
        for batch in self.children[0].execute_columnar():
            kcols = [batch.column(k) for k in self.keys]
            kvals = [batch.validity(k) for k in self.keys]
            if len(self.keys) == 1:
                perm, counts = gpuq.partition_perm(kcols[0], world,
                                                   key_validity=kvals[0])
            else:
                perm, counts = gpuq.partition_perm_multi(kcols, world,
                                                         key_validities=kvals)
            cols, vcols = {}, {}
            row_bytes = 0
            for name, t in batch.columns().items():
                cols[name] = gpuq.gather(t, perm)
                row_bytes += t.element_size()
                v = batch.validity(name)
                if v is not None:
                    # bitmaps travel as u8 columns: partition split points
                    # are not byte-aligned (repacked on receive)
                    pv = gpuq.gather_bits(v, perm)
                    vcols[name] = gpuq.bits_to_u8(pv, t.numel())
                    row_bytes += 1
            in_splits = counts.cpu().tolist()
            self._stats = {"bytes_by_partition": [c * row_bytes for c in in_splits],
                           "rows_written": int(sum(in_splits))}
            offsets = [0]
            for c in in_splits:
                offsets.append(offsets[-1] + c)
            if not hasattr(self, "_map_outputs"):
                self._map_outputs = []
            self._map_outputs.append((cols, vcols, offsets))
            wire = dict(cols)
            wire.update({f"__valid__{n}": u8 for n, u8 in vcols.items()})
            out, _ = exchange_columns(wire, in_splits)
            batch.close()
            validity = {}
            for name in list(out):
                if name.startswith("__valid__"):
                    u8 = out.pop(name)
                    validity[name[len("__valid__"):]] = gpuq.u8_to_bits(u8)
            yield ColumnarBatch(out, validity=validity or None)


class GpuShuffledHashJoinExec(_JoinKeys, SparkPlan):
    """Replaces ShuffledHashJoinExec inner join
    (ShuffledHashJoinExec.scala:103-132). Both children must already be
    clustered on the join key (ShuffledJoin.scala:57-69) — i.e. fed by (our)
    exchanges, as EnsureRequirements would arrange. One key column runs the
    single-key (LongHashedRelation-style) kernels; 2-4 key columns run the
    composite-key table (gpuq_join_*_keys). condition: the residual join
    condition (HashJoin.scala boundCondition), a predicate over columns of
    both children that a key-equal pair must make TRUE to count as a match;
    with one, any key count runs the composite-key table and the probe
    evaluates the condition itself (gpuq_join_probe_keys_cond)."""

    def __init__(self, left_key, right_key, build_side: str,
                 left, right, join_type: str = "inner",
                 null_aware_anti: bool = False, condition=None):
        super().__init__(left, right)
        self.condition = _check_join_condition(condition, left, right,
                                               null_aware_anti)
        assert build_side in ("left", "right")
        assert join_type in ("inner", "left_outer", "right_outer",
                             "left_semi", "left_anti", "full_outer")
        lk, _ = _join_key_tuples(left_key, right_key)
        # NOT IN rewrite (BroadcastHashJoinExec.scala:48,137
        # isNullAwareAntiJoin): empty build -> all probe rows; any NULL
        # build key -> empty result; NULL probe keys are filtered
        assert not null_aware_anti or join_type == "left_anti"
        # isNullAwareAntiJoin requires leftKeys.length == 1
        assert not null_aware_anti or len(lk) == 1, \
            "null-aware anti join is single-key only"
        self.null_aware_anti = null_aware_anti
        # the preserved/streamed side must be the PROBE side
        # (HashJoin.scala buildSide constraints; full outer preserves both
        # — either side may build)
        if join_type in ("left_outer", "left_semi", "left_anti"):
            assert build_side == "right", f"{join_type} builds on the right"
        if join_type == "right_outer":
            assert build_side == "left", "right_outer builds on the left"
        self.left_key, self.right_key, self.build_side = left_key, right_key, build_side
        self.join_type = join_type

    @property
    def output(self):
        if self.join_type in ("left_semi", "left_anti"):
            return self.children[0].output
        return self.children[0].output + self.children[1].output

    @property
    def supports_columnar(self):
        return True

    def required_child_distribution(self):
        return [Distribution("clustered", self.left_keys),
                Distribution("clustered", self.right_keys)]

    def _join_output(self, build, probe_cols, probe_validity, op, ob):
        """One output batch from matched (probe_rid, build_rid) pairs: build
        columns gathered by ob (NIL -> NULL for the outer types), probe
        columns by op (NIL -> NULL for full outer); a probe column whose
        name the build side already uses gets a `#probe` suffix."""
        from . import gpuq
        semi = self.join_type in ("left_semi", "left_anti")
        outer = self.join_type in ("left_outer", "right_outer", "full_outer")
        full = self.join_type == "full_outer"
        cols, validity = {}, {}
        if not semi:
            for name, t in build.columns().items():
                if outer:
                    # unmatched probe rows pair with NIL -> NULL build
                    cols[name], validity[name] = gpuq.gather_nullable(
                        t, ob, validity=build.validity(name))
                else:
                    cols[name] = gpuq.gather(t, ob)
                    v = build.validity(name)
                    if v is not None:
                        validity[name] = gpuq.gather_bits(v, ob)
        for name, t in probe_cols.items():
            v = probe_validity.get(name)
            if name in cols:
                name = f"{name}#probe"
            if full:
                # build-side unmatched rows carry NIL probe rids
                cols[name], validity[name] = gpuq.gather_nullable(
                    t, op, validity=v)
            else:
                cols[name] = gpuq.gather(t, op)
                if v is not None:
                    validity[name] = gpuq.gather_bits(v, op)
        return ColumnarBatch(cols, validity=validity or None)

    def _execute_composite(self, gpuq, build, bkeys, pkeys, jt, probe_iter):
        """2-4 key columns, or any key count with a residual condition: one
        composite-key table over the concatenated build side, probed
        batch-at-a-time (the condition, if any, evaluated by the probe).
        Full outer emits the unmatched build rows ONCE, after the last probe
        batch, from the matched bits the probes accumulated."""
        bn = build.num_rows()
        nkeys = len(bkeys)
        cap = 1 << max(4, int(bn * 2 - 1).bit_length() if bn else 4)
        ws = gpuq.join_build_keys(
            [build.column(k) for k in bkeys], cap,
            key_validities=[build.validity(k) for k in bkeys])
        full = self.join_type == "full_outer"
        probe_dtypes = None
        bcols = build.columns()
        bvalid = {n_: build.validity(n_) for n_ in bcols}
        for probe in probe_iter:
            pk = [probe.column(k) for k in pkeys]
            pkv = [probe.validity(k) for k in pkeys]
            pcols = probe.columns()
            pvalid = {n_: probe.validity(n_) for n_ in pcols}
            if self.condition is not None:
                cond = gpuq.lower_join_cond(self.condition, pcols, bcols)
            out_cap = max(int(probe.num_rows() * 2) + 64, 64)
            while True:
                if self.condition is None:
                    op, ob, nm = gpuq.join_probe_keys(
                        pk, ws, cap, bn, out_cap, key_validities=pkv,
                        join_type=jt)
                else:
                    op, ob, nm = gpuq.join_probe_keys_cond(
                        pk, ws, cap, bn, out_cap, cond, pcols, bcols,
                        probe_validities=pvalid, build_validities=bvalid,
                        key_validities=pkv, join_type=jt)
                if op is not None:
                    break
                out_cap = nm + 64
            probe_dtypes = {n_: t.dtype for n_, t in pcols.items()}
            out = self._join_output(
                build, pcols, pvalid, op, ob)
            probe.close()
            yield out
        if full:
            # the NULL probe columns need the probe schema
            assert probe_dtypes is not None, \
                "full outer join over a batchless probe child"
            op, ob, nu = gpuq.join_keys_unmatched_build(ws, cap, bn, nkeys)
            if nu:
                # every op entry is NIL: the one-row sources are never read
                null_src = {n_: torch.zeros(1, dtype=dt, device=ob.device)
                            for n_, dt in probe_dtypes.items()}
                yield self._join_output(build, null_src, {}, op, ob)
        build.close()

    def execute_columnar(self):
        from . import gpuq
        bi = 0 if self.build_side == "left" else 1
        build_b = list(self.children[bi].execute_columnar())
        assert build_b, "join build over a batchless child"
        # buildHashedRelation materializes the whole build side per
        # partition: multi-batch children concatenate
        build = concat_batches(build_b)
        jt = {"inner": gpuq.JOIN_INNER, "left_outer": gpuq.JOIN_OUTER,
              "right_outer": gpuq.JOIN_OUTER, "left_semi": gpuq.JOIN_SEMI,
              "left_anti": gpuq.JOIN_ANTI,
              "full_outer": gpuq.JOIN_FULL}[self.join_type]
        bkeys = self.left_keys if self.build_side == "left" else self.right_keys
        pkeys = self.right_keys if self.build_side == "left" else self.left_keys
        if len(bkeys) > 1 or self.condition is not None:
            yield from self._execute_composite(
                gpuq, build, bkeys, pkeys, jt,
                self.children[1 - bi].execute_columnar())
            return
        bkey, pkey = bkeys[0], pkeys[0]
        bk = build.column(bkey)
        bn = bk.numel()
        if self.null_aware_anti:
            if bn == 0:
                # NOT IN (empty) is true for every row, NULL included
                yield from self.children[1 - bi].execute_columnar()
                build.close()
                return
            _, _, valid_cnt = gpuq.minmax_i64(bk,
                                              validity=build.validity(bkey))
            if valid_cnt < bn:
                # any NULL in the build side: NOT IN is never true
                for probe in self.children[1 - bi].execute_columnar():
                    empty = {n_: t[:0] for n_, t in probe.columns().items()}
                    probe.close()
                    yield ColumnarBatch(empty)
                build.close()
                return
            jt = gpuq.JOIN_ANTI_NULLAWARE
        cap = 1 << max(4, int(bn * 2 - 1).bit_length() if bn else 4)
        ws = gpuq.join_build(bk, cap, key_validity=build.validity(bkey))
        # the probe (streamed) side is consumed batch-at-a-time
        # (ShuffledHashJoinExec.doExecute streams streamedIter)
        for probe in self.children[1 - bi].execute_columnar():
            pk = probe.column(pkey)
            out_cap = max(int(probe.num_rows() * 2) + 64, 64)
            while True:
                op, ob, nm = gpuq.join_probe(pk, ws, cap, bn, out_cap,
                                             key_validity=probe.validity(pkey),
                                             join_type=jt)
                if op is not None:
                    break
                out_cap = nm + 64
            pcols = probe.columns()
            out = self._join_output(
                build, pcols, {n_: probe.validity(n_) for n_ in pcols}, op, ob)
            probe.close()
            yield out
        build.close()


class GpuRangeExec(SparkPlan):
    """Replaces RangeExec: generates the id column directly in HBM (the
    scan-feed adjacency, SURVEY §8(f).1 — no RowToColumnar CPU tax)."""

    def __init__(self, n: int, start: int = 0, step: int = 1, name: str = "id"):
        super().__init__()
        self.n, self.start, self.step, self.name = n, start, step, name

    @property
    def output(self):
        return [self.name]

    @property
    def supports_columnar(self):
        return True

    def execute_columnar(self):
        from . import gpuq
        yield ColumnarBatch({self.name: gpuq.range_i64(self.n, self.start, self.step)})


class GpuFilterExec(SparkPlan):
    """Replaces FilterExec: stable compaction on device,
    then payload gather by the passing-row permutation. The four-argument
    form (col, op, literal, child) runs one comparison through
    gpuq_filter_cmp; the two-argument form (condition, child) evaluates a
    predicate tree in one fused pass through gpuq_filter_expr."""

    def __init__(self, *args):
        col, op, literal, condition, child = _filter_args(args)
        super().__init__(child)
        self.col, self.op, self.literal = col, op, literal
        self.condition = condition

    @property
    def output(self):
        return self.children[0].output

    @property
    def output_ordering(self):
        # stable compaction preserves the child's order (FilterExec does)
        return self.children[0].output_ordering

    @property
    def supports_columnar(self):
        return True

    def execute_columnar(self):
        from . import gpuq
        for batch in self.children[0].execute_columnar():
            if self.condition is not None:
                names = batch.columns()
                perm, cnt = gpuq.filter_expr(
                    names, self.condition,
                    validities={k: batch.validity(k) for k in names
                                if batch.validity(k) is not None})
            else:
                perm, cnt = gpuq.filter_cmp(batch.column(self.col), self.op,
                                            self.literal,
                                            validity=batch.validity(self.col))
            cols, validity = {}, {}
            for name, t in batch.columns().items():
                cols[name] = gpuq.gather(t, perm)
                v = batch.validity(name)
                if v is not None and cnt:
                    validity[name] = gpuq.gather_bits(v, perm)
            batch.close()
            yield ColumnarBatch(cols, validity=validity or None)


class GpuProjectExec(SparkPlan):
    """Replaces ProjectExec; pass-through entries keep their
    column and its validity bitmap. A 5-tuple entry is one binary operation
    through gpuq_project_binop_nullable: its row is NULL iff an input row is
    NULL or the op is a division by zero (Spark non-ANSI). All (out_name,
    expr) entries of the node are evaluated together by one
    gpuq_project_expr call per batch (more only if they exceed that call's
    output, column, instruction or depth caps), each input column read once.
    A computed column carries a bitmap unless nothing in it can be NULL."""

    def __init__(self, projections, child):
        super().__init__(child)
        self.projections = projections
        self._lowered = {}      # (schema, nullable columns) -> chunks

    def _expr_chunks(self, batch):
        """the node's expression entries lowered for this batch's schema:
        [(out_names, lowered program tuple)], one gpuq_project_expr call each"""
        entries = [p for p in self.projections if _is_expr_entry(p)]
        if not entries:
            return []
        cols = batch.columns()
        nullable = tuple(k for k in cols if batch.validity(k) is not None)
        key = (tuple((k, str(t.dtype)) for k, t in cols.items()), nullable)
        if key not in self._lowered:
            schema = {k: t.dtype for k, t in cols.items()}
            chunks, cur, cur_low = [], [], None
            for ent in entries:
                try:
                    low = expression.lower(cur + [ent], schema, nullable)
                except ValueError:
                    if not cur:
                        raise
                    chunks.append(([n for n, _ in cur], cur_low))
                    cur = []
                    low = expression.lower([ent], schema, nullable)
                cur, cur_low = cur + [ent], low
            chunks.append(([n for n, _ in cur], cur_low))
            self._lowered[key] = chunks
        return self._lowered[key]

    @property
    def output(self):
        return [p if isinstance(p, str) else p[0] for p in self.projections]

    @property
    def supports_columnar(self):
        return True

    def execute_columnar(self):
        from . import gpuq
        for batch in self.children[0].execute_columnar():
            cols, validity = {}, {}
            computed = {}
            for out_names, low in self._expr_chunks(batch):
                in_cols = batch.columns()
                computed.update(gpuq.project_expr_program(
                    in_cols, low[0], low[1], out_names, low[2], low[3],
                    validities={k: batch.validity(k) for k in low[0]
                                if batch.validity(k) is not None}))
            for p in self.projections:
                if isinstance(p, str):
                    cols[p] = batch.column(p)
                    v = batch.validity(p)
                elif _is_expr_entry(p):
                    p = p[0]
                    cols[p], v = computed[p]
                else:
                    out_name, a, op, b, lit = p
                    p = out_name
                    cols[p], v = gpuq.project_binop_nullable(
                        batch.column(a), op,
                        b=batch.column(b) if b is not None else None,
                        literal=lit, a_validity=batch.validity(a),
                        b_validity=batch.validity(b) if b is not None else None)
                if v is not None:
                    validity[p] = v
            batch.close()
            yield ColumnarBatch(cols, validity=validity or None)


class GpuWindowExec(_WindowSpec, SparkPlan):
    """Replaces WindowExec (execution/window/WindowExec.scala). As in Spark
    the rows arrive clustered on the partition keys and sorted by (partition
    keys, order keys) — the SortExec EnsureRequirements put below this node;
    nothing is sorted here. A whole-partition operator: the child's batches
    are concatenated, the partition / peer-group bitmaps are computed once
    and every expression is one segmented scan (gpuq_window_scan) or shift
    (gpuq_window_shift) under them. Yields one batch: every input column and
    bitmap untouched, plus one column per expression. avg (float64 only) is
    windowed SUM / cast(windowed COUNT), NULL where the count is 0. A
    RowsBetween frame other than (None, 0) / (None, None), and first_value /
    last_value, run through gpuq_window_slide."""

    def __init__(self, window_exprs, partition_spec, order_spec, child):
        super().__init__(child)
        self.window_exprs, self.partition_spec, self.order_spec = \
            _window_check(window_exprs, partition_spec, order_spec, child)

    @property
    def supports_columnar(self):
        return True

    def _eval(self, gpuq, e, batch, n, part_bits, peer_bits, ws):
        """(column, validity or None) of one expression."""
        if e.fn in WINDOW_RANK_FNS:
            return gpuq.window_scan(e.fn, "rows", part_bits, peer_bits, n=n,
                                    workspace=ws)
        val = batch.column(e.col) if e.col is not None else None
        valid = batch.validity(e.col) if e.col is not None else None
        if e.fn in WINDOW_SHIFT_FNS:
            off = -e.offset if e.fn == "lag" else e.offset
            return gpuq.window_shift(val, off, part_bits, validity=valid,
                                     default=e.default, workspace=ws)
        frame = self.frame_of(e)
        if e.fn in WINDOW_VALUE_FNS:
            return self._eval_value(gpuq, e, frame, val, valid, part_bits)
        if isinstance(frame, RowsBetween):
            if frame.lo is not None or frame.hi not in (None, 0):
                return self._eval_slide(gpuq, e, frame, val, valid, n, part_bits)
            frame = "rows" if frame.hi == 0 else "partition"
        if e.fn != "avg":
            return gpuq.window_scan(e.fn, frame, part_bits, peer_bits, val=val,
                                    validity=valid, n=n, workspace=ws)
        if val.dtype != torch.float64:
            raise ValueError(f"window: avg({e.col}) over {val.dtype} "
                             "unsupported (float64 columns only)")
        total, tvalid = gpuq.window_scan("sum", frame, part_bits, peer_bits,
                                         val=val, validity=valid, workspace=ws)
        cnt, _ = gpuq.window_scan("count", frame, part_bits, peer_bits,
                                  val=val, validity=valid, workspace=ws)
        # x / 0 is NULL: the rows whose frame holds no non-NULL value
        return gpuq.project_binop_nullable(total, "/", b=gpuq.cast_i64_f64(cnt),
                                           a_validity=tvalid)

    @staticmethod
    def _eval_value(gpuq, e, frame, val, valid, part_bits):
        """first_value / last_value: the value and NULL-ness of the frame's
        first / last row. Under "rows", "range" and the default frame the
        first row is the partition's; the last row of a RANGE frame is the
        peer group's, which is not built."""
        if not isinstance(frame, RowsBetween):
            if e.fn == "last_value" and frame == "range":
                raise ValueError(
                    f"window: last_value({e.col}) under the RANGE frame "
                    "unsupported (give a ROWS frame)")
            frame = RowsBetween(None, None if frame == "partition" else 0)
        return gpuq.window_slide(e.fn, frame.lo, frame.hi, part_bits, val=val,
                                 validity=valid)

    @staticmethod
    def _eval_slide(gpuq, e, frame, val, valid, n, part_bits):
        """an aggregate over a sliding frame (gpuq_window_slide)."""
        if e.fn != "avg":
            return gpuq.window_slide(e.fn, frame.lo, frame.hi, part_bits,
                                     val=val, validity=valid, n=n)
        if val.dtype != torch.float64:
            raise ValueError(f"window: avg({e.col}) over {val.dtype} "
                             "unsupported (float64 columns only)")
        ws = gpuq.window_slide_workspace(n, frame.lo, frame.hi)
        total, tvalid = gpuq.window_slide("sum", frame.lo, frame.hi, part_bits,
                                          val=val, validity=valid, workspace=ws)
        cnt, _ = gpuq.window_slide("count", frame.lo, frame.hi, part_bits,
                                   val=val, validity=valid, workspace=ws)
        # x / 0 is NULL: the rows whose frame holds no non-NULL value
        return gpuq.project_binop_nullable(total, "/", b=gpuq.cast_i64_f64(cnt),
                                           a_validity=tvalid)

    def execute_columnar(self):
        import torch.distributed as dist
        from . import gpuq
        assert (self.partition_spec or not dist.is_initialized()
                or dist.get_world_size() == 1), \
            "multi-rank window without PARTITION BY unsupported"
        batches = list(self.children[0].execute_columnar())
        assert batches, "window over a batchless child"
        batch = concat_batches(batches)
        n = batch.num_rows()
        keys = list(self.partition_spec) + [o.key for o in self.order_spec]
        part_bits, peer_bits = gpuq.window_boundaries(
            [batch.column(k) for k in keys],
            [batch.validity(k) for k in keys], len(self.partition_spec), n=n)
        ws = gpuq.window_workspace(n)
        cols = batch.columns()
        validity = {k: batch.validity(k) for k in cols
                    if batch.validity(k) is not None}
        for e in self.window_exprs:
            cols[e.name], v = self._eval(gpuq, e, batch, n, part_bits,
                                         peer_bits, ws)
            if v is not None:
                validity[e.name] = v
        yield ColumnarBatch(cols, validity=validity or None)


class GpuBroadcastExchangeExec(SparkPlan):
    """Replaces BroadcastExchangeExec: RCCL all-gather of the build-side
    batch across ranks (single-rank: identity). Unlike the shuffled
    exchange there is no partitioning — every rank gets the whole
    relation."""

    def __init__(self, child):
        super().__init__(child)

    @property
    def output(self):
        return self.children[0].output

    @property
    def supports_columnar(self):
        return True

    def execute_columnar(self):
        import torch.distributed as dist
        from . import gpuq
        from .exchange import broadcast_gather, _unpack_validity_wire
        for batch in self.children[0].execute_columnar():
            if dist.is_initialized() and dist.get_world_size() > 1:
                wire = batch.columns()
                n = batch.num_rows()
                for name in list(wire):
                    v = batch.validity(name)
                    if v is not None:
                        wire[f"__valid__{name}"] = gpuq.bits_to_u8(v, n)
                cols = broadcast_gather(wire)
                validity = _unpack_validity_wire(gpuq, cols)
                batch.close()
                yield ColumnarBatch(cols, validity=validity or None)
            else:
                yield batch


class GpuBroadcastHashJoinExec(GpuShuffledHashJoinExec):
    """Replaces BroadcastHashJoinExec: identical device-side build/probe
    kernels; the build child is expected to be a GpuBroadcastExchangeExec,
    and the PROBE side needs no distribution at all (BroadcastDistribution,
    joins/BroadcastHashJoinExec.scala:60-66)."""

    def required_child_distribution(self):
        dists = [Distribution("unspecified"), Distribution("unspecified")]
        dists[0 if self.build_side == "left" else 1] = Distribution("broadcast")
        return dists


class GpuColumnarRule:
    """The injected rule (ColumnarRule, Columnar.scala:36-50; injection via
    SparkSessionExtensions.injectColumnar:168; applied at
    QueryExecution.scala:798 / AdaptiveSparkPlanExec.scala:184-186).
    preColumnarTransitions swaps CPU nodes for GPU subclasses — the
    SparkSessionExtensionSuite.scala:959-1000 pattern."""

    def __init__(self, preserve_smj_ordering: bool = True):
        self.preserve_smj_ordering = preserve_smj_ordering

    def pre_columnar_transitions(self, plan: SparkPlan) -> SparkPlan:
        children = [self.pre_columnar_transitions(c) for c in plan.children]
        if isinstance(plan, SortExec):
            return GpuSortExec(plan.sort_order, plan.global_sort, *children)
        if isinstance(plan, TakeOrderedAndProjectExec):
            return GpuTakeOrderedAndProjectExec(
                plan.limit, plan.sort_order, plan.project_list, *children)
        if isinstance(plan, LocalLimitExec):
            return GpuLocalLimitExec(plan.limit, *children)
        if isinstance(plan, CollectLimitExec):   # before its base class
            return GpuCollectLimitExec(plan.limit, *children,
                                       offset=plan.offset)
        if isinstance(plan, GlobalLimitExec):
            return GpuGlobalLimitExec(plan.limit, *children,
                                      offset=plan.offset)
        if isinstance(plan, HashAggregateExec):
            return GpuHashAggregateExec(
                plan.group_key, plan.aggs, plan.mode, *children,
                capacity=plan.capacity,
                decimal_precision=plan.decimal_precision)
        if isinstance(plan, ShuffledHashJoinExec):
            return GpuShuffledHashJoinExec(plan.left_key, plan.right_key,
                                           plan.build_side, *children,
                                           join_type=plan.join_type,
                                           condition=plan.condition)
        if isinstance(plan, SortMergeJoinExec):
            # SMJ -> GPU hash join (same slot, same required distribution;
            # build on the right side as SHJ's default would choose). SMJ
            # advertises outputOrdering on the streamed keys — parents may
            # have had sorts elided against it — so re-sort the hash join's
            # output to honor the contract (one radix pass; the GPU sort
            # node's output_ordering then matches what SMJ declared).
            build = "left" if plan.join_type == "right_outer" else "right"
            j = GpuShuffledHashJoinExec(plan.left_key, plan.right_key,
                                        build, *children,
                                        join_type=plan.join_type,
                                        condition=plan.condition)
            declared = plan.output_ordering
            if self.preserve_smj_ordering and declared:
                return GpuSortExec(declared, False, j)
            return j
        if isinstance(plan, ShuffleExchangeExec):
            return GpuShuffleExchangeExec(plan.keys, *children)
        if isinstance(plan, FilterExec):
            if plan.condition is not None:
                return GpuFilterExec(plan.condition, *children)
            return GpuFilterExec(plan.col, plan.op, plan.literal, *children)
        if isinstance(plan, ProjectExec):
            return GpuProjectExec(plan.projections, *children)
        if isinstance(plan, WindowExec):
            return GpuWindowExec(plan.window_exprs, plan.partition_spec,
                                 plan.order_spec, *children)
        if isinstance(plan, RangeExec):
            return GpuRangeExec(plan.n, plan.start, plan.step, plan.name)
        if isinstance(plan, ParquetScanExec):
            return GpuParquetScanExec(plan.path, plan.columns)
        if isinstance(plan, BroadcastExchangeExec):
            return GpuBroadcastExchangeExec(*children)
        if isinstance(plan, BroadcastHashJoinExec):
            return GpuBroadcastHashJoinExec(plan.left_key, plan.right_key,
                                            plan.build_side, *children,
                                            join_type=plan.join_type,
                                            condition=plan.condition)
        plan.children = children
        return plan

    def post_columnar_transitions(self, plan: SparkPlan) -> SparkPlan:
        # Spark inserts Row<->Columnar transitions here (Columnar.scala:564-614);
        # in this mirror every node is columnar, nothing to insert.
        return plan
