"""SELECT-list expression trees and their lowering to the typed postfix
program gpuq_project_expr interprets (include/gpuq.h, GPUQ_EXPR_*).

Pure Python, like predicate.py: nothing here touches the device. The node
classes mirror the Catalyst expressions a ProjectExec list is made of
(Add / Subtract / Multiply / Divide, UnaryMinus, Abs, Cast, the binary
comparisons, If, CaseWhen, Coalesce); any predicate.Pred is accepted wherever
a boolean is wanted. The kernel sees only the sixteen opcodes below.

Typing is decided here, never on the device: every instruction carries its
operand type, "i64", "f64" or the stack-only "bool". Nothing is promoted
implicitly: operands of two dtypes need an explicit Cast. An untyped literal
(Lit(3), or a bare Python number) takes the type of its sibling operand, and
lowering refuses where that would lose information.

NULL rules (Spark, non-ANSI) are those of the header: arithmetic and
comparisons are NULL if an operand is, x / 0 is NULL, If / CaseWhen take the
else branch on a NULL condition, Coalesce takes the first non-NULL operand.
"""
import math
from typing import NamedTuple

from .predicate import (CMP, I64_MAX, I64_MIN, And, Between, Cmp, Col, In,
                        IsNotNull, IsNull, Not, Or, Pred, _dtype_code,
                        rewrite_i64_float_cmp)

# opcodes, type codes and caps: mirrors of the #defines in include/gpuq.h
(COL, LIT, REF, ARITH, NEG, ABS, CAST, CMP_OP, IS_NULL, IS_NOT_NULL, AND, OR,
 NOT, SELECT, COALESCE, OUT) = range(16)
I64, F64, BOOL = 0, 1, 3
MAX_INSNS = 48
MAX_COLS = 8
MAX_OUTS = 4
MAX_DEPTH = 8

BINOP = {"+": 0, "-": 1, "*": 2, "/": 3}
TYPE_CODE = {"i64": I64, "f64": F64, "bool": BOOL}
TYPE_NAME = {v: k for k, v in TYPE_CODE.items()}

_OPNAMES = ("COL", "LIT", "REF", "ARITH", "NEG", "ABS", "CAST", "CMP",
            "IS_NULL", "IS_NOT_NULL", "AND", "OR", "NOT", "SELECT",
            "COALESCE", "OUT")
# values popped by each opcode; every opcode but OUT pushes one
POPS = (0, 0, 0, 2, 1, 1, 1, 2, 1, 1, 2, 2, 1, 3, 2, 1)


class Insn(NamedTuple):
    """One postfix instruction (gpuq_expr_insn)."""
    opcode: int
    arg: int = 0
    dtype: int = I64
    pad: int = 0
    lit_i64: int = 0
    lit_f64: float = 0.0

    def __repr__(self):
        return (f"Insn({_OPNAMES[self.opcode]}, arg={self.arg}, "
                f"{TYPE_NAME.get(self.dtype, self.dtype)}, i={self.lit_i64}, "
                f"f={self.lit_f64!r})")


# ---------------- expression nodes ----------------

class Expr:
    pass


def _operand(e):
    """a node as given, or a bare Python number / None as an untyped literal"""
    if isinstance(e, (Expr, Col, Pred)):
        return e
    if e is None or isinstance(e, (int, float)):
        return Lit(e)
    raise ValueError(f"not an expression: {e!r}")


def _bool_operand(p):
    if not isinstance(p, Pred):
        raise ValueError(f"condition {p!r} is not a predicate")
    return p


class Lit(Expr):
    """A literal; value None is the NULL literal. dtype "i64" / "f64" fixes
    the type, None leaves it to the sibling operand."""

    def __init__(self, value, dtype=None):
        if dtype is not None:
            dtype = _dtype_code(dtype)
        if isinstance(value, bool) or \
                not (value is None or isinstance(value, (int, float))):
            raise ValueError(f"unsupported literal {value!r}")
        self.value, self.dtype = value, dtype

    def __repr__(self):
        return f"Lit({self.value!r})" if self.dtype is None \
            else f"Lit({self.value!r}, {self.dtype!r})"


class BinOp(Expr):
    def __init__(self, op: str, a, b):
        if op not in BINOP:
            raise ValueError(f"unknown arithmetic operator {op!r}")
        self.op, self.a, self.b = op, _operand(a), _operand(b)

    def __repr__(self):
        return f"BinOp({self.op!r}, {self.a!r}, {self.b!r})"


class Neg(Expr):
    def __init__(self, e):
        self.e = _operand(e)

    def __repr__(self):
        return f"Neg({self.e!r})"


class Abs(Expr):
    def __init__(self, e):
        self.e = _operand(e)

    def __repr__(self):
        return f"Abs({self.e!r})"


class Cast(Expr):
    """Cast(e, "i64" | "f64"): int64 <-> float64, or a boolean to 0 / 1."""

    def __init__(self, e, to: str):
        self.e, self.to = _operand(e), _dtype_code(to)

    def __repr__(self):
        return f"Cast({self.e!r}, {self.to!r})"


class Compare(Pred):
    """a OP b with an expression on either side."""

    def __init__(self, a, op: str, b):
        if op not in CMP:
            raise ValueError(f"unknown comparison {op!r}")
        self.a, self.op, self.b = _operand(a), op, _operand(b)

    def __repr__(self):
        return f"Compare({self.a!r}, {self.op!r}, {self.b!r})"


class If(Expr):
    def __init__(self, cond, then, else_):
        self.cond = _bool_operand(cond)
        self.then, self.else_ = _operand(then), _operand(else_)

    def __repr__(self):
        return f"If({self.cond!r}, {self.then!r}, {self.else_!r})"


class CaseWhen(Expr):
    """CASE WHEN c1 THEN v1 ... [ELSE e] END; without else_ a row no arm
    takes is NULL."""

    def __init__(self, branches, else_=None):
        self.branches = [(_bool_operand(c), _operand(v)) for c, v in branches]
        if not self.branches:
            raise ValueError("CaseWhen needs a branch")
        self.else_ = None if else_ is None else _operand(else_)

    def __repr__(self):
        return f"CaseWhen({self.branches!r}, else_={self.else_!r})"


class Coalesce(Expr):
    def __init__(self, *es):
        if not es:
            raise ValueError("Coalesce needs an operand")
        self.es = [_operand(e) for e in es]

    def __repr__(self):
        return f"Coalesce({', '.join(map(repr, self.es))})"


def is_expr(e) -> bool:
    """what a ProjectExec entry (out_name, e) may hold"""
    return isinstance(e, (Expr, Col, Pred))


# ---------------- structural identity (for REF) ----------------

def _key(e):
    if isinstance(e, Col):
        return ("Col", e.name)
    if isinstance(e, Lit):
        return ("Lit", repr(e.value), e.dtype)
    if isinstance(e, BinOp):
        return ("BinOp", e.op, _key(e.a), _key(e.b))
    if isinstance(e, (Neg, Abs)):
        return (type(e).__name__, _key(e.e))
    if isinstance(e, Cast):
        return ("Cast", e.to, _key(e.e))
    if isinstance(e, Compare):
        return ("Compare", e.op, _key(e.a), _key(e.b))
    if isinstance(e, If):
        return ("If", _key(e.cond), _key(e.then), _key(e.else_))
    if isinstance(e, CaseWhen):
        return ("CaseWhen", tuple((_key(c), _key(v)) for c, v in e.branches),
                None if e.else_ is None else _key(e.else_))
    if isinstance(e, Coalesce):
        return ("Coalesce",) + tuple(_key(x) for x in e.es)
    if isinstance(e, Cmp):
        rhs = _key(e.rhs) if isinstance(e.rhs, Col) else repr(e.rhs)
        return ("Cmp", e.col, e.op, rhs)
    if isinstance(e, (IsNull, IsNotNull)):
        return (type(e).__name__, e.col)
    if isinstance(e, In):
        return ("In", e.col, tuple(repr(v) for v in e.values))
    if isinstance(e, Between):
        return ("Between", e.col, repr(e.lo), repr(e.hi))
    if isinstance(e, (And, Or)):
        return (type(e).__name__,) + tuple(_key(p) for p in e.ps)
    if isinstance(e, Not):
        return ("Not", _key(e.p))
    raise ValueError(f"not an expression: {e!r}")


# ---------------- lowering ----------------

def _literal(value, dt: str) -> Insn:
    """LIT of type dt ("i64" / "f64" / "bool") for a Python value"""
    code = TYPE_CODE[dt]
    if value is None:
        return Insn(LIT, 1, code)
    if dt == "bool":
        return Insn(LIT, 0, BOOL, 0, 1 if value else 0)
    if dt == "i64":
        if isinstance(value, float):
            if not math.isfinite(value) or value != int(value):
                raise ValueError(f"non-integral literal {value!r} beside an "
                                 f"int64 operand (cast the operand to f64)")
            value = int(value)
        if not I64_MIN <= value <= I64_MAX:
            raise ValueError(f"literal {value!r} exceeds int64")
        return Insn(LIT, 0, I64, 0, value, 0.0)
    if isinstance(value, int):
        try:
            exact = int(float(value)) == value
        except OverflowError:
            exact = False
        if not exact:
            raise ValueError(f"literal {value!r} is not exactly representable "
                             f"as float64")
    return Insn(LIT, 0, F64, 0, 0, float(value))


class _Lowering:
    def __init__(self, schema, nullable):
        self.schema = schema
        self.nullable = nullable      # names with a bitmap; None = all
        self.cols = []
        self.prog = []
        self.done = []                # (key, dtype, nullable) per output

    def col(self, name):
        """-> (dtype, nullable); pushes the column"""
        if name not in self.schema:
            raise ValueError(f"unknown column {name!r}")
        dt = _dtype_code(self.schema[name])
        if name not in self.cols:
            self.cols.append(name)
        self.prog.append(Insn(COL, self.cols.index(name), TYPE_CODE[dt]))
        return dt, self.nullable is None or name in self.nullable

    def type_of(self, e):
        """static type of a node; None for an untyped literal"""
        if isinstance(e, Pred):
            return "bool"
        if isinstance(e, Col):
            if e.name not in self.schema:
                raise ValueError(f"unknown column {e.name!r}")
            return _dtype_code(self.schema[e.name])
        if isinstance(e, Lit):
            return e.dtype
        if isinstance(e, Cast):
            return e.to
        if isinstance(e, BinOp):
            return self.unify([e.a, e.b], e)
        if isinstance(e, (Neg, Abs)):
            return self.type_of(e.e)
        if isinstance(e, If):
            return self.unify([e.then, e.else_], e)
        if isinstance(e, CaseWhen):
            vals = [v for _, v in e.branches]
            return self.unify(vals + ([] if e.else_ is None else [e.else_]), e)
        if isinstance(e, Coalesce):
            return self.unify(e.es, e)
        raise ValueError(f"not an expression: {e!r}")

    def unify(self, es, where):
        """the one type sibling operands share; None if all are untyped"""
        types = {t for t in map(self.type_of, es) if t is not None}
        if len(types) > 1:
            raise ValueError(f"operands of {where!r} have dtypes "
                             f"{sorted(types)}: no implicit promotion, add "
                             f"a Cast")
        return types.pop() if types else None

    @staticmethod
    def natural(es, where):
        """type for siblings that are all untyped literals"""
        vals = [e.value for e in es if isinstance(e, Lit) and e.value is not None]
        if not vals:
            raise ValueError(f"{where!r}: a NULL literal needs a dtype")
        return "f64" if any(isinstance(v, float) for v in vals) else "i64"

    def siblings(self, es, where, want):
        t = self.unify(es, where) or want
        if t is None:
            t = self.natural(es, where)
        if t == "bool":
            raise ValueError(f"{where!r}: a boolean operand, use "
                             f"Cast(..., \"i64\") for a 0 / 1 value")
        return t

    def emit(self, e, want=None):
        """pushes e; -> (dtype, nullable). want types an untyped literal."""
        if not isinstance(e, (Lit, Col, Pred)):   # an output is never a bool
            k = _key(e)
            for j, (kj, dj, nj) in enumerate(self.done):
                if kj == k:
                    self.prog.append(Insn(REF, j, TYPE_CODE[dj]))
                    return dj, nj
        if isinstance(e, Pred):
            return "bool", self.emit_pred(e)
        if isinstance(e, Col):
            return self.col(e.name)
        if isinstance(e, Lit):
            dt = e.dtype or want or self.natural([e], e)
            self.prog.append(_literal(e.value, dt))
            return dt, e.value is None
        if isinstance(e, BinOp):
            dt = self.siblings([e.a, e.b], e, want)
            _, na = self.emit(e.a, dt)
            _, nb = self.emit(e.b, dt)
            self.prog.append(Insn(ARITH, BINOP[e.op], TYPE_CODE[dt]))
            return dt, na or nb or e.op == "/"
        if isinstance(e, (Neg, Abs)):
            dt, nl = self.emit(e.e, want)
            if dt == "bool":
                raise ValueError(f"{e!r}: a boolean operand")
            self.prog.append(Insn(NEG if isinstance(e, Neg) else ABS, 0,
                                  TYPE_CODE[dt]))
            return dt, nl
        if isinstance(e, Cast):
            src, nl = self.emit(e.e)
            if src == "bool" and e.to != "i64":
                raise ValueError(f"{e!r}: a boolean casts to i64 only")
            if src != e.to:
                self.prog.append(Insn(CAST, TYPE_CODE[e.to], TYPE_CODE[src]))
            return e.to, nl
        if isinstance(e, If):
            dt = self.siblings([e.then, e.else_], e, want)
            _, ne = self.emit(e.else_, dt)
            _, nt = self.emit(e.then, dt)
            self.emit_pred(e.cond)
            self.prog.append(Insn(SELECT, 0, TYPE_CODE[dt]))
            return dt, nt or ne
        if isinstance(e, CaseWhen):
            vals = [v for _, v in e.branches]
            dt = self.siblings(vals + ([] if e.else_ is None else [e.else_]),
                               e, want)
            if e.else_ is None:
                self.prog.append(_literal(None, dt))
                nl = True
            else:
                _, nl = self.emit(e.else_, dt)
            for cond, val in reversed(e.branches):     # else-first
                _, nv = self.emit(val, dt)
                self.emit_pred(cond)
                self.prog.append(Insn(SELECT, 0, TYPE_CODE[dt]))
                nl = nl or nv
            return dt, nl
        if isinstance(e, Coalesce):
            dt = self.siblings(e.es, e, want)
            nl = True
            for k, x in enumerate(e.es):
                _, nx = self.emit(x, dt)
                if k:
                    self.prog.append(Insn(COALESCE, 0, TYPE_CODE[dt]))
                nl = nl and nx
            return dt, nl
        raise ValueError(f"not an expression: {e!r}")

    # ---- predicates on the generic opcodes ----

    def cmp_lit(self, name, op, literal):
        """col OP literal -> nullable"""
        if name not in self.schema:
            raise ValueError(f"unknown column {name!r}")
        if literal is None:          # col OP NULL is NULL whatever the row
            self.prog.append(_literal(None, "bool"))
            return True
        dt = _dtype_code(self.schema[name])
        if dt == "i64" and isinstance(literal, float):
            op, literal = rewrite_i64_float_cmp(op, literal)
        _, nl = self.col(name)
        self.prog.append(_literal(literal, dt))
        self.prog.append(Insn(CMP_OP, CMP[op], TYPE_CODE[dt]))
        return nl

    def emit_pred(self, p):
        """pushes a BOOL; -> nullable"""
        if not isinstance(p, Pred):
            raise ValueError(f"not a predicate: {p!r}")
        if isinstance(p, Compare):
            a, op, b = p.a, p.op, p.b
            ta, tb = self.type_of(a), self.type_of(b)
            # int64 expression against an untyped float literal: Spark's
            # cast-to-double comparison, rewritten to an exact integer one
            if tb == "i64" and isinstance(a, Lit) and ta is None \
                    and isinstance(a.value, float):
                a, b, ta, tb = b, a, tb, ta
                op = {"<": ">", "<=": ">=", ">": "<", ">=": "<="}.get(op, op)
            if ta == "i64" and isinstance(b, Lit) and tb is None \
                    and isinstance(b.value, float):
                op, lit = rewrite_i64_float_cmp(op, b.value)
                _, na = self.emit(a, "i64")
                self.prog.append(_literal(lit, "i64"))
                self.prog.append(Insn(CMP_OP, CMP[op], I64))
                return na
            dt = self.siblings([a, b], p, None)
            _, na = self.emit(a, dt)
            _, nb = self.emit(b, dt)
            self.prog.append(Insn(CMP_OP, CMP[op], TYPE_CODE[dt]))
            return na or nb
        if isinstance(p, Cmp):
            if isinstance(p.rhs, Col):
                da, na = self.col(p.col)
                db, nb = self.col(p.rhs.name)
                if da != db:
                    raise ValueError(
                        f"comparison of {p.col!r} ({da}) with {p.rhs.name!r} "
                        f"({db}): dtypes differ, add a Cast")
                self.prog.append(Insn(CMP_OP, CMP[p.op], TYPE_CODE[da]))
                return na or nb
            return self.cmp_lit(p.col, p.op, p.rhs)
        if isinstance(p, (IsNull, IsNotNull)):
            dt, _ = self.col(p.col)
            self.prog.append(Insn(IS_NULL if isinstance(p, IsNull)
                                  else IS_NOT_NULL, 0, TYPE_CODE[dt]))
            return False
        if isinstance(p, Between):
            nlo = self.cmp_lit(p.col, ">=", p.lo)
            nhi = self.cmp_lit(p.col, "<=", p.hi)
            self.prog.append(Insn(AND, 0, BOOL))
            return nlo or nhi
        if isinstance(p, In):
            if p.col not in self.schema:
                raise ValueError(f"unknown column {p.col!r}")
            dt = _dtype_code(self.schema[p.col])
            if not p.values:
                self.prog.append(_literal(False, "bool"))
                return False
            nl = False
            for k, v in enumerate(p.values):
                if dt == "i64" and isinstance(v, float) \
                        and not (math.isfinite(v) and v == int(v)):
                    raise ValueError(f"non-integral literal {v!r} in an IN "
                                     f"list on int64 column {p.col!r}")
                nl = self.cmp_lit(p.col, "==", v) or nl
                if k:
                    self.prog.append(Insn(OR, 0, BOOL))
            return nl
        if isinstance(p, (And, Or)):
            nl = False
            for k, q in enumerate(p.ps):
                nl = self.emit_pred(q) or nl
                if k:
                    self.prog.append(Insn(AND if isinstance(p, And) else OR,
                                          0, BOOL))
            return nl
        if isinstance(p, Not):
            nl = self.emit_pred(p.p)
            self.prog.append(Insn(NOT, 0, BOOL))
            return nl
        raise ValueError(f"not a predicate: {p!r}")


def stack_depth(program) -> int:
    """Largest evaluation-stack depth of a postfix program."""
    depth = peak = 0
    for insn in program:
        depth += (0 if insn.opcode == OUT else 1) - POPS[insn.opcode]
        peak = max(peak, depth)
    return peak


def lower(outputs, schema, nullable=None):
    """-> (column_names, program, out_dtypes, out_nullable) for an ordered
    [(name, expr)] list: the columns the expressions read, in order of first
    use, one postfix program that ends each output with an OUT, and per output
    its dtype ("i64" / "f64") and whether it can hold a NULL.

    schema maps a column name to its dtype (torch / numpy dtype or "int64" /
    "float64"); nullable is the collection of column names that carry a
    validity bitmap (None: every column may). Outputs lower in order; a
    subtree structurally equal to the whole tree of an earlier output of the
    list lowers to a REF of it. CaseWhen lowers else-first, so a chain folds
    at constant depth.

    Raises ValueError for an unknown column, operands of two dtypes with no
    Cast, a literal that does not fit its sibling's type exactly (a
    non-integral float beside int64, an int float64 cannot represent), a
    boolean output (use Cast(..., "i64")), and a program over the caps
    (MAX_INSNS instructions, MAX_COLS columns, MAX_OUTS outputs, stack depth
    MAX_DEPTH)."""
    outputs = list(outputs)
    if not 1 <= len(outputs) <= MAX_OUTS:
        raise ValueError(f"{len(outputs)} outputs, the limit is 1..{MAX_OUTS}")
    lo = _Lowering(schema, None if nullable is None else set(nullable))
    out_dtypes, out_nullable = [], []
    for k, (name, e) in enumerate(outputs):
        e = _operand(e)
        dt, nl = lo.emit(e)
        if dt == "bool":
            raise ValueError(f"output {name!r} is a boolean: use "
                             f"Cast(..., \"i64\") for a 0 / 1 column")
        lo.prog.append(Insn(OUT, k, TYPE_CODE[dt]))
        lo.done.append((_key(e), dt, nl))
        out_dtypes.append(dt)
        out_nullable.append(nl)
    depth = stack_depth(lo.prog)
    if depth > MAX_DEPTH:
        raise ValueError(f"expressions need stack depth {depth}, the limit "
                         f"is {MAX_DEPTH}")
    if len(lo.prog) > MAX_INSNS:
        raise ValueError(f"expressions lower to {len(lo.prog)} instructions, "
                         f"the limit is {MAX_INSNS}")
    if len(lo.cols) > MAX_COLS:
        raise ValueError(f"expressions read {len(lo.cols)} columns, the "
                         f"limit is {MAX_COLS}")
    return lo.cols, lo.prog, out_dtypes, out_nullable
