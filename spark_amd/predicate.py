"""WHERE-clause predicate trees and their lowering to the postfix program
gpuq_filter_expr interprets (include/gpuq.h, GPUQ_PRED_*).

Pure Python: nothing here touches the device, so plans can be built, lowered
and checked without one. The node classes mirror the Catalyst expressions a
FilterExec condition is made of (And, Or, Not, In, IsNull, IsNotNull, the
binary comparisons with an AttributeReference on either side); the kernel
sees only CMP_LIT / CMP_COL / IS_NULL / IS_NOT_NULL / CONST / AND / OR / NOT.

Three-valued (Kleene) logic throughout, as Spark evaluates it: a comparison
with a NULL operand is NULL, AND is FALSE if either side is FALSE else NULL
if either is NULL, OR is the dual, NOT NULL is NULL, and WHERE keeps a row
only when the whole predicate is TRUE.
"""
import math
from typing import NamedTuple

CMP = {"==": 0, "<": 1, "<=": 2, ">": 3, ">=": 4, "!=": 5}

# opcodes and caps: mirrors of the #defines in include/gpuq.h
CMP_LIT, CMP_COL, IS_NULL, IS_NOT_NULL, CONST, AND, OR, NOT = range(8)
FALSE, TRUE, NULL = 0, 1, 2
MAX_INSNS = 32
MAX_COLS = 8
MAX_DEPTH = 16

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1

_OPNAMES = ("CMP_LIT", "CMP_COL", "IS_NULL", "IS_NOT_NULL", "CONST", "AND",
            "OR", "NOT")


class Insn(NamedTuple):
    """One postfix instruction (gpuq_pred_insn). cmp is a CMP code for
    CMP_LIT / CMP_COL and FALSE / TRUE / NULL for CONST; col_a / col_b index
    the column list lower() returns."""
    opcode: int
    cmp: int = 0
    col_a: int = 0
    col_b: int = 0
    lit_i64: int = 0
    lit_f64: float = 0.0

    def __repr__(self):
        return (f"Insn({_OPNAMES[self.opcode]}, cmp={self.cmp}, a={self.col_a}, "
                f"b={self.col_b}, i={self.lit_i64}, f={self.lit_f64!r})")


# ---------------- predicate nodes ----------------

class Col:
    """A column reference on the right-hand side of a comparison."""

    def __init__(self, name: str):
        self.name = name

    def __repr__(self):
        return f"Col({self.name!r})"


def _name(col) -> str:
    return col.name if isinstance(col, Col) else col


class Pred:
    pass


class Cmp(Pred):
    """col OP rhs; rhs is a Python literal (None = the NULL literal) or
    Col(name); op is a key of CMP."""

    def __init__(self, col, op: str, rhs):
        if op not in CMP:
            raise ValueError(f"unknown comparison {op!r}")
        self.col, self.op, self.rhs = _name(col), op, rhs

    def __repr__(self):
        return f"Cmp({self.col!r}, {self.op!r}, {self.rhs!r})"


class IsNull(Pred):
    def __init__(self, col):
        self.col = _name(col)

    def __repr__(self):
        return f"IsNull({self.col!r})"


class IsNotNull(Pred):
    def __init__(self, col):
        self.col = _name(col)

    def __repr__(self):
        return f"IsNotNull({self.col!r})"


class In(Pred):
    """col IN (values); None in the list is a NULL literal."""

    def __init__(self, col, values):
        self.col, self.values = _name(col), list(values)

    def __repr__(self):
        return f"In({self.col!r}, {self.values!r})"


class Between(Pred):
    """lo <= col AND col <= hi."""

    def __init__(self, col, lo, hi):
        self.col, self.lo, self.hi = _name(col), lo, hi

    def __repr__(self):
        return f"Between({self.col!r}, {self.lo!r}, {self.hi!r})"


class _Nary(Pred):
    def __init__(self, *ps):
        if not ps:
            raise ValueError(f"{type(self).__name__} needs an operand")
        for p in ps:
            if not isinstance(p, Pred):
                raise ValueError(f"{type(self).__name__} operand {p!r} is "
                                 f"not a predicate")
        self.ps = list(ps)

    def __repr__(self):
        return f"{type(self).__name__}({', '.join(map(repr, self.ps))})"


class And(_Nary):
    pass


class Or(_Nary):
    pass


class Not(Pred):
    def __init__(self, p):
        if not isinstance(p, Pred):
            raise ValueError(f"Not operand {p!r} is not a predicate")
        self.p = p

    def __repr__(self):
        return f"Not({self.p!r})"


# ---------------- int64 column vs float literal ----------------

# "every valid row" / "no row", kept as comparisons against the column so
# that a NULL row still evaluates to NULL, not to a constant
CMP_ALL = (">=", I64_MIN)
CMP_NONE = ("<", I64_MIN)


def rewrite_i64_float_cmp(op: str, literal: float):
    """(op, int literal) equivalent to `int64 column OP float literal` under
    Spark's cast-to-double comparison: k < 0.5 becomes k <= 0, never a
    truncation (k < 0.5 must keep k == 0). +/-inf and NaN literals become
    CMP_ALL / CMP_NONE (NaN is greater than every double a bigint casts
    to)."""
    if math.isnan(literal):
        return CMP_ALL if op in ("<", "<=", "!=") else CMP_NONE
    if math.isinf(literal):
        all_ops = ("<", "<=") if literal > 0 else (">", ">=")
        return CMP_ALL if op in all_ops or op == "!=" else CMP_NONE
    if literal != int(literal) or not (I64_MIN <= int(literal) <= I64_MAX):
        f = math.floor(literal)
        if op == "==":
            return CMP_NONE
        if op == "!=":
            return CMP_ALL
        if op in ("<", "<="):
            # col < L  <=>  col <= floor(L)
            if f > I64_MAX:
                return CMP_ALL
            return ("<=", f) if f >= I64_MIN else CMP_NONE
        # > / >= : col > L  <=>  col >= floor(L) + 1
        g = f + 1
        if g < I64_MIN:
            return CMP_ALL
        return (">=", g) if g <= I64_MAX else CMP_NONE
    return op, int(literal)


# ---------------- lowering ----------------

def _dtype_code(dtype) -> str:
    s = str(dtype)
    if s in ("torch.int64", "int64", "i64"):
        return "i64"
    if s in ("torch.float64", "float64", "f64"):
        return "f64"
    raise ValueError(f"unsupported predicate column dtype {dtype!r}")


def _single_col(p):
    """the column every leaf of p loads as its col_a, or None if they differ
    (then p takes no part in the same-column grouping)."""
    if isinstance(p, (Cmp, IsNull, IsNotNull, In, Between)):
        return p.col
    if isinstance(p, Not):
        return _single_col(p.p)
    cols = {_single_col(q) for q in p.ps}
    return cols.pop() if len(cols) == 1 else None


def _group_by_col(ps):
    """Stable regrouping of the operands of one And / Or (both commute under
    Kleene logic): operands on one column follow its first occurrence, so the
    kernel's one-entry column cache serves them with one load."""
    groups, where = [], {}
    for p in ps:
        c = _single_col(p)
        if c is not None and c in where:
            groups[where[c]].append(p)
        else:
            if c is not None:
                where[c] = len(groups)
            groups.append([p])
    return [p for g in groups for p in g]


class _Lowering:
    def __init__(self, schema):
        self.schema = schema
        self.cols = []
        self.prog = []

    def col(self, name):
        if name not in self.schema:
            raise ValueError(f"unknown column {name!r}")
        code = _dtype_code(self.schema[name])
        if name not in self.cols:
            self.cols.append(name)
        return self.cols.index(name), code

    def cmp_lit(self, name, op, literal):
        ia, dt = self.col(name)
        if literal is None:          # col OP NULL is NULL whatever the row
            self.prog.append(Insn(CONST, NULL))
            return
        if dt == "f64":
            self.prog.append(Insn(CMP_LIT, CMP[op], ia, 0, 0, float(literal)))
            return
        if isinstance(literal, float):
            op, literal = rewrite_i64_float_cmp(op, literal)
        literal = int(literal)
        if not I64_MIN <= literal <= I64_MAX:
            raise ValueError(f"literal {literal!r} exceeds int64")
        self.prog.append(Insn(CMP_LIT, CMP[op], ia, 0, literal, float(literal)))

    def emit(self, p):
        if isinstance(p, Cmp):
            if isinstance(p.rhs, Col):
                ia, da = self.col(p.col)
                ib, db = self.col(p.rhs.name)
                if da != db:
                    raise ValueError(
                        f"comparison of {p.col!r} ({da}) with {p.rhs.name!r} "
                        f"({db}): dtypes differ, project a cast first")
                self.prog.append(Insn(CMP_COL, CMP[p.op], ia, ib))
            else:
                self.cmp_lit(p.col, p.op, p.rhs)
        elif isinstance(p, IsNull):
            self.prog.append(Insn(IS_NULL, 0, self.col(p.col)[0]))
        elif isinstance(p, IsNotNull):
            self.prog.append(Insn(IS_NOT_NULL, 0, self.col(p.col)[0]))
        elif isinstance(p, Between):
            self.cmp_lit(p.col, ">=", p.lo)
            self.cmp_lit(p.col, "<=", p.hi)
            self.prog.append(Insn(AND))
        elif isinstance(p, In):
            _, dt = self.col(p.col)
            if not p.values:
                self.prog.append(Insn(CONST, FALSE))
            for k, v in enumerate(p.values):
                if dt == "i64" and isinstance(v, float) \
                        and not (math.isfinite(v) and v == int(v)):
                    raise ValueError(f"non-integral literal {v!r} in an IN "
                                     f"list on int64 column {p.col!r}")
                self.cmp_lit(p.col, "==", v)
                if k:
                    self.prog.append(Insn(OR))
        elif isinstance(p, (And, Or)):
            join = Insn(AND if isinstance(p, And) else OR)
            for k, q in enumerate(_group_by_col(p.ps)):
                self.emit(q)
                if k:
                    self.prog.append(join)
        elif isinstance(p, Not):
            self.emit(p.p)
            self.prog.append(Insn(NOT))
        else:
            raise ValueError(f"not a predicate: {p!r}")


def columns_of(pred):
    """-> the column names pred references, each once, in order of first use.
    Needs no schema: a join node uses it to tell which side each column of its
    residual condition comes from. The walk is lower()'s (the operands of an
    And / Or regrouped by column), so for a predicate that lowers the result
    is lower()'s column list."""
    names = []

    def use(name):
        if name not in names:
            names.append(name)

    def walk(p):
        if isinstance(p, Cmp):
            use(p.col)
            if isinstance(p.rhs, Col):
                use(p.rhs.name)
        elif isinstance(p, (IsNull, IsNotNull, In, Between)):
            use(p.col)
        elif isinstance(p, (And, Or)):
            for q in _group_by_col(p.ps):
                walk(q)
        elif isinstance(p, Not):
            walk(p.p)
        else:
            raise ValueError(f"not a predicate: {p!r}")

    walk(pred)
    return names


def stack_depth(program) -> int:
    """Largest evaluation-stack depth of a postfix program."""
    depth = peak = 0
    for insn in program:
        depth += {AND: -1, OR: -1, NOT: 0}.get(insn.opcode, 1)
        peak = max(peak, depth)
    return peak


def lower(pred, schema):
    """-> (column_names, program): the columns the predicate reads, in order
    of first use, and the postfix instruction list over them. schema maps a
    column name to its dtype (torch / numpy dtype or "int64" / "float64").
    Raises ValueError for an unknown column, a dtype other than int64 /
    float64, a column-vs-column comparison of different dtypes, a non-integral
    literal in an IN list on an int64 column, and a program over the caps
    (MAX_INSNS instructions, MAX_COLS columns, stack depth MAX_DEPTH)."""
    lo = _Lowering(schema)
    lo.emit(pred)
    depth = stack_depth(lo.prog)
    if depth > MAX_DEPTH:
        raise ValueError(f"predicate needs stack depth {depth}, the limit is "
                         f"{MAX_DEPTH}")
    if len(lo.prog) > MAX_INSNS:
        raise ValueError(f"predicate lowers to {len(lo.prog)} instructions, "
                         f"the limit is {MAX_INSNS}")
    if len(lo.cols) > MAX_COLS:
        raise ValueError(f"predicate reads {len(lo.cols)} columns, the limit "
                         f"is {MAX_COLS}")
    return lo.cols, lo.prog
