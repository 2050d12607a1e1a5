"""Seeded random SELECT-list expression trees for the lowering and GPU parity
tests: every node class of spark_amd.expression and every predicate class,
typed consistently (no implicit promotion), over caller-given int64 and
float64 column names."""
from spark_amd.expression import (Abs, BinOp, CaseWhen, Cast, Coalesce,
                                  Compare, If, Lit, Neg)
from spark_amd.predicate import (And, Between, Cmp, Col, In, IsNotNull,
                                 IsNull, Not, Or)


def random_pred(rng, depth, icols, fcols):
    k = rng.randint(9)
    allc = list(icols) + list(fcols)
    c = str(allc[rng.randint(len(allc))])
    isf = c in fcols
    if depth == 0 or k == 0:
        lit = float(rng.randint(-4, 5)) / 2 if (isf or rng.rand() < 0.3) \
            else int(rng.randint(-3, 4))
        return Cmp(c, ["==", "<", "<=", ">", ">=", "!="][rng.randint(6)], lit)
    if k == 1:
        return (IsNull if rng.rand() < 0.5 else IsNotNull)(c)
    if k == 2:
        return Between(c, -1.0 if isf else -1, 3.0 if isf else 3)
    if k == 3:
        vals = [float(v) if isf else int(v) for v in rng.randint(-2, 5, size=rng.randint(0, 4))]
        if rng.rand() < 0.3:
            vals.append(None)
        return In(c, vals)
    if k == 4:
        t = "i64" if rng.rand() < 0.5 else "f64"
        return Compare(random_expr(rng, depth - 1, t, icols, fcols),
                       ["==", "<", "<=", ">", ">=", "!="][rng.randint(6)],
                       random_expr(rng, depth - 1, t, icols, fcols))
    if k == 5:
        return Not(random_pred(rng, depth - 1, icols, fcols))
    if k == 6:
        same = [o for o in (fcols if isf else icols) if o != c]
        if same:
            return Cmp(c, "<=", Col(str(same[rng.randint(len(same))])))
    return (And if k % 2 else Or)(random_pred(rng, depth - 1, icols, fcols),
                                  random_pred(rng, depth - 1, icols, fcols))


def random_expr(rng, depth, dt, icols, fcols):
    cols = icols if dt == "i64" else fcols

    def lit():
        return Lit(int(rng.randint(-5, 6))) if dt == "i64" \
            else Lit(float(rng.randint(-5, 6)) / 2)

    def sub():
        return random_expr(rng, depth - 1, dt, icols, fcols)

    def pred():
        return random_pred(rng, depth - 1, icols, fcols)

    if depth == 0 or rng.rand() < 0.2:
        return Col(str(cols[rng.randint(len(cols))])) if rng.rand() < 0.7 else lit()
    k = rng.randint(8)
    if k == 0:
        return BinOp("+-*/"[rng.randint(4)], sub(), sub())
    if k == 1:
        return (Neg if rng.rand() < 0.5 else Abs)(sub())
    if k == 2:
        other = "f64" if dt == "i64" else "i64"
        return Cast(random_expr(rng, depth - 1, other, icols, fcols), dt)
    if k == 3:
        return If(pred(), sub(), sub())
    if k == 4:
        return CaseWhen([(pred(), sub()) for _ in range(rng.randint(1, 4))],
                        else_=sub() if rng.rand() < 0.5 else None)
    if k == 5:
        return Coalesce(*[sub() for _ in range(rng.randint(1, 4))])
    if k == 6 and dt == "i64":
        return Cast(pred(), "i64")
    return BinOp("*", sub(), lit())
