"""GPU parity for the residual join condition (gpuq_join_probe_keys_cond and
the `condition` of the hash-join nodes) against tests/join_cond_ref.py, the
nested-loop reference. Pair lists compare sorted; node outputs compare as
multisets of full rows, float columns by their bit patterns (NaN, -0.0)."""
import functools

import numpy as np
import pytest

import join_cond_ref as R
from spark_amd.predicate import And, Between, Cmp, Col, In, IsNull, Not, Or

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

I64_MIN = -(1 << 63)
NIL = R.NIL
NAN = float("nan")
JT_NAMES = {R.INNER: "inner", R.OUTER: "left_outer", R.SEMI: "left_semi",
            R.ANTI: "left_anti", R.FULL: "full_outer"}
# neither a multiple of the probe kernels' chunks (4096, and 1024 for the
# conditioned probe) nor of the wave (64); several blocks
BUILD_ROWS, PROBE_ROWS = 10_007, 13_003
CAP = 1 << 15


@pytest.fixture(scope="module")
def gq():
    from spark_amd import gpuq
    assert torch.cuda.is_available()
    return gpuq


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def pack_validity(valid_bool):
    return torch.from_numpy(np.packbits(valid_bool, bitorder="little")).cuda()


def pair_list(op, ob):
    p = op.cpu().numpy().view(np.uint32).tolist()
    b = ob.cpu().numpy().view(np.uint32).tolist()
    return sorted(zip(p, b))


# ---------------- data ----------------

# value tables: -1, 0 and INT64_MIN are ordinary key components
VALS0 = np.array([-1, 0, I64_MIN] + list(range(3, 6000)), dtype=np.int64)
VALS1 = np.array(list(range(2, 100)) + [I64_MIN, -1], dtype=np.int64)
VALS2 = np.array([-1, 0], dtype=np.int64)
VALS3 = np.array([I64_MIN, 7], dtype=np.int64)
TABLES = [VALS0, VALS1, VALS2, VALS3]
# (build, probe) domain sizes per column: 3000 build tuples against 6000
# probe tuples whatever nkeys is
DOMAINS = {1: [(3000, 6000)],
           2: [(60, 60), (50, 100)],
           4: [(15, 15), (50, 100), (2, 2), (2, 2)]}
# float operands: every special value, few enough distinct ones for ties
FLOATS = np.array([NAN, 0.0, -0.0, np.inf, -np.inf, 0.25, 0.5, 0.75])


def gen_keys(rng, n, nkeys, side):
    keys = [TABLES[c][rng.randint(0, DOMAINS[nkeys][c][side], size=n)]
            for c in range(nkeys)]
    # a NULL in exactly one key column of ~1/16 of the rows
    valid = [np.ones(n, bool) for _ in range(nkeys)]
    rows = np.flatnonzero(rng.randint(0, 16, size=n) == 0)
    for r, c in zip(rows, rng.randint(0, nkeys, size=len(rows))):
        valid[c][r] = False
    return keys, valid


def gen_i64(rng, n):
    return (rng.randint(0, 100, size=n).astype(np.int64),
            rng.randint(0, 8, size=n) != 0, "i64")


def gen_f64(rng, n):
    return (FLOATS[rng.randint(0, len(FLOATS), size=n)],
            rng.randint(0, 8, size=n) != 0, "f64")


class Case:
    """one seeded data set; probe = left (lk*, px, pf, pid), build = right
    (rk*, by, bz, bg, bid). pid / bid number the rows and have no NULLs."""

    def __init__(self, nkeys, seed, bn=BUILD_ROWS, pn=PROBE_ROWS, extra=None):
        rng = np.random.RandomState(seed)
        self.nkeys = nkeys
        self.bk, self.bv = gen_keys(rng, bn, nkeys, 0)
        self.pk, self.pv = gen_keys(rng, pn, nkeys, 1)
        self.bcols = {"by": gen_i64(rng, bn), "bz": gen_i64(rng, bn),
                      "bg": gen_f64(rng, bn)}
        self.pcols = {"px": gen_i64(rng, pn), "pf": gen_f64(rng, pn)}
        if extra is not None:
            extra(self)
        self.bn, self.pn = len(self.bk[0]), len(self.pk[0])
        self.bcols["bid"] = (np.arange(self.bn, dtype=np.int64), None, "i64")
        self.pcols["pid"] = (np.arange(self.pn, dtype=np.int64), None, "i64")
        self._verd = {}
        self._dev = None

    @functools.cached_property
    def cands(self):
        return R.candidate_lists(list(zip(self.pk, self.pv)),
                                 list(zip(self.bk, self.bv)))

    def verd(self, name):
        if name not in self._verd:
            self._verd[name] = R.verdicts(self.cands, self.pcols, self.bcols,
                                          CONDS[name])
        return self._verd[name]

    def expected(self, name, jt, n=None):
        """reference pairs / unmatched build rows for the first n probe rows"""
        return R.join_pairs(self.verd(name)[:n], jt, self.bn)

    # ---- device side ----
    def dev(self):
        if self._dev is None:
            d = {}
            d["bk"] = [to_dev(k) for k in self.bk]
            d["bv"] = [pack_validity(v) for v in self.bv]
            d["bcols"] = {k: to_dev(c[0]) for k, c in self.bcols.items()}
            d["bvalid"] = {k: pack_validity(c[1]) for k, c in self.bcols.items()
                           if c[1] is not None}
            self._dev = d
        return self._dev

    def table(self, gq):
        d = self.dev()
        if "ws" not in d:
            d["ws"] = gq.join_build_keys(d["bk"], CAP, key_validities=d["bv"])
        return d["ws"]

    def probe_side(self, lo=0, hi=None):
        """(keys, key bitmaps, columns, column bitmaps) of probe rows lo:hi"""
        hi = self.pn if hi is None else hi
        return ([to_dev(k[lo:hi]) for k in self.pk],
                [pack_validity(v[lo:hi]) for v in self.pv],
                {k: to_dev(c[0][lo:hi]) for k, c in self.pcols.items()},
                {k: pack_validity(c[1][lo:hi]) for k, c in self.pcols.items()
                 if c[1] is not None})

    def probe(self, gq, cond, jt, n=None, out_cap=None):
        d = self.dev()
        ws = self.table(gq)
        pk, pkv, pc, pcv = self.probe_side(0, n)
        rows = self.pn if n is None else n
        out_cap = 16 * rows + self.bn + 64 if out_cap is None else out_cap
        return gq.join_probe_keys_cond(
            pk, ws, CAP, self.bn, out_cap, cond, pc, d["bcols"],
            probe_validities=pcv, build_validities=d["bvalid"],
            key_validities=pkv, join_type=jt)

    def unmatched(self, gq):
        uo, ub, nu = gq.join_keys_unmatched_build(self.table(gq), CAP, self.bn,
                                                  self.nkeys)
        got = pair_list(uo, ub)
        assert nu == len(got) and all(p == NIL for p, _ in got)
        return [b for _, b in got]

    # ---- node level: rows as tuples, floats as bit patterns ----
    def lnames(self):
        return [f"lk{c}" for c in range(self.nkeys)] + list(self.pcols)

    def rnames(self):
        return [f"rk{c}" for c in range(self.nkeys)] + list(self.bcols)

    def _side_rows(self, keys, valid, cols):
        data = [(k, v) for k, v in zip(keys, valid)]
        data += [(c[0].view(np.int64) if c[2] == "f64" else c[0],
                  c[1] if c[1] is not None else np.ones(len(c[0]), bool))
                 for c in cols.values()]
        return [tuple(int(x[i]) if v[i] else None for x, v in data)
                for i in range(len(keys[0]))]

    @functools.cached_property
    def prows(self):
        return self._side_rows(self.pk, self.pv, self.pcols)

    @functools.cached_property
    def brows(self):
        return self._side_rows(self.bk, self.bv, self.bcols)

    def expected_rows(self, name, jt):
        """build columns first, then probe columns, as _join_output lays
        them out; semi / anti carry the probe columns only"""
        pairs, unmatched = self.expected(name, jt)
        pnull = (None,) * len(self.lnames())
        bnull = (None,) * len(self.rnames())
        if jt in (R.SEMI, R.ANTI):
            return sort_rows(self.prows[i] for i, _ in pairs)
        rows = [(self.brows[j] if j != NIL else bnull) + self.prows[i]
                for i, j in pairs]
        rows += [self.brows[j] + pnull for j in unmatched]
        return sort_rows(rows)

    def batches(self, gx, splits=None):
        """-> (probe InputBatches split at `splits`, build InputBatches)"""
        splits = splits or [0, self.pn]
        left = []
        for lo, hi in zip(splits, splits[1:]):
            pk, pkv, pc, pcv = self.probe_side(lo, hi)
            cols = {f"lk{c}": t for c, t in enumerate(pk)}
            cols.update(pc)
            val = {f"lk{c}": t for c, t in enumerate(pkv)}
            val.update(pcv)
            left.append(gx.ColumnarBatch(cols, validity=val))
        d = self.dev()
        cols = {f"rk{c}": t.clone() for c, t in enumerate(d["bk"])}
        cols.update({k: t.clone() for k, t in d["bcols"].items()})
        val = {f"rk{c}": t.clone() for c, t in enumerate(d["bv"])}
        val.update({k: t.clone() for k, t in d["bvalid"].items()})
        return (gx.InputBatches(left),
                gx.InputBatches([gx.ColumnarBatch(cols, validity=val)]))

    def keys(self):
        return (tuple(f"lk{c}" for c in range(self.nkeys)),
                tuple(f"rk{c}" for c in range(self.nkeys)))


def sort_rows(rows):
    return sorted(rows, key=lambda r: tuple((x is None, x or 0) for x in r))


def batch_rows(batch, names):
    """device batch -> list of row tuples, None where the bitmap says NULL,
    float columns as their int64 bit patterns"""
    n = batch.num_rows()
    cols = []
    for name in names:
        t = batch.column(name)
        if t.dtype == torch.float64:
            t = t.view(torch.int64)
        data = t.cpu().numpy()
        v = batch.validity(name)
        ok = (np.unpackbits(v.cpu().numpy(), count=n, bitorder="little")
              .astype(bool) if v is not None else np.ones(n, bool))
        cols.append([int(x) if o else None for x, o in zip(data, ok)])
    return list(zip(*cols)) if cols else []


CONDS = {
    "x<y": Cmp("px", "<", Col("by")),
    # the Q21 shape (l2.l_suppkey <> l1.l_suppkey) on doubles: NaN == NaN and
    # -0.0 == 0.0 are ties, so they FAIL !=
    "f!=g": Cmp("pf", "!=", Col("bg")),
    "compound": And(Cmp("px", "<", Col("by")),
                    Or(IsNull("bz"), Cmp("pf", ">=", 0.5)),
                    In("by", [3, None, 7])),
    # the IN list above lets only a handful of pairs pass; this one is
    # balanced, and uses NOT / BETWEEN / a probe-side IN with a NULL
    "compound2": Or(And(Cmp("px", "<", Col("by")), Cmp("pf", ">=", 0.5)),
                    Not(Between("bz", 10, 90)),
                    In("px", [1, 2, None])),
    "probe_only": Cmp("px", ">=", 40),
    "build_only": Or(Cmp("bg", "<", 0.5), IsNull("by")),
    "never": Cmp("px", "<", I64_MIN),
    "always": Cmp("pid", ">=", I64_MIN),
}


@functools.lru_cache(maxsize=None)
def parity_case(nkeys):
    return Case(nkeys, seed=7100 + nkeys)


# ---------------- 0. the input has every leg (CPU, reference only) ----------

@pytest.mark.parametrize("nkeys", [1, 2, 4])
def test_condition_leg_coverage(nkeys):
    """conditions on the input, not measurements: each share of the probe
    rows (of the candidate pairs for the last) is at least 3 %, so a seed
    change cannot silently remove a leg of the kernel"""
    case = parity_case(nkeys)
    verd = case.verd("x<y")
    pn = case.pn
    matched = [r for r in verd if r]
    npass = lambda r: sum(1 for _, t in r if t is True)
    share = {
        "key-matched, no passing pair": sum(npass(r) == 0 for r in matched),
        "some but not all pass": sum(0 < npass(r) < len(r) for r in matched),
        "all pass": sum(npass(r) == len(r) for r in matched),
        "three or more passing pairs": sum(npass(r) >= 3 for r in matched),
        ">= 3 candidates, first two not both passing": sum(
            len(r) >= 3 and not (r[0][1] is True and r[1][1] is True)
            for r in matched),
    }
    for what, count in share.items():
        assert count / pn >= 0.03, (what, count / pn)
    pairs = [t for r in verd for _, t in r]
    assert sum(t is None for t in pairs) / len(pairs) >= 0.03
    # ~1/16 NULL-key rows per side, every key column has some
    for valid in (case.bv, case.pv):
        nulls = sum((~v).astype(int) for v in valid)
        assert nulls.max() == 1 and 0.03 < (nulls == 1).mean() < 0.10
        assert all((~v).any() for v in valid)
    # the float operands meet at NaN and at the two zeros, both as ties
    fg = case.verd("f!=g")
    pf, bg = case.pcols["pf"], case.bcols["bg"]
    ties = [(i, j) for i, r in enumerate(fg) for j, t in r if t is False]
    assert any(np.isnan(pf[0][i]) and np.isnan(bg[0][j]) for i, j in ties)
    assert any(pf[0][i] == 0 and np.signbit(pf[0][i]) != np.signbit(bg[0][j])
               and bg[0][j] == 0 for i, j in ties)
    # the compound condition passes somewhere, and not everywhere
    comp = [t for r in case.verd("compound") for _, t in r]
    assert 0 < sum(t is True for t in comp) < len(comp)
    assert any(t is None for t in comp) and any(t is False for t in comp)


# ---------------- 1. parity: keys x join types x conditions ----------------

@pytest.mark.parametrize("name", ["x<y", "f!=g", "compound", "compound2",
                                  "probe_only", "build_only"])
@pytest.mark.parametrize("jt", [R.INNER, R.OUTER, R.SEMI, R.ANTI, R.FULL])
@pytest.mark.parametrize("nkeys", [1, 2, 4])
def test_parity(gq, nkeys, jt, name):
    case = parity_case(nkeys)
    exp, exp_unmatched = case.expected(name, jt)
    if jt == R.FULL:
        # matched bits accumulate across probes: start from a fresh table
        case.dev().pop("ws", None)
    op, ob, n = case.probe(gq, CONDS[name], jt)
    assert n == len(exp)
    assert pair_list(op, ob) == exp
    if jt == R.FULL:
        assert case.unmatched(gq) == exp_unmatched
        case.dev().pop("ws", None)


@pytest.mark.parametrize("nkeys", [1, 2, 4])
def test_always_false(gq, nkeys):
    case = parity_case(nkeys)
    cond = CONDS["never"]
    every = [(i, NIL) for i in range(case.pn)]
    case.dev().pop("ws", None)
    for jt, exp in ((R.INNER, []), (R.SEMI, []), (R.ANTI, every),
                    (R.OUTER, every), (R.FULL, every)):
        op, ob, n = case.probe(gq, cond, jt)
        assert n == len(exp) and pair_list(op, ob) == exp, jt
    assert case.unmatched(gq) == list(range(case.bn))
    case.dev().pop("ws", None)


@pytest.mark.parametrize("jt", [R.INNER, R.OUTER, R.SEMI, R.ANTI, R.FULL])
@pytest.mark.parametrize("nkeys", [1, 2, 4])
def test_always_true_is_the_unconditioned_probe(gq, nkeys, jt):
    """ties the new kernel to the old one: a condition that holds for every
    pair (a comparison on a column without NULLs) must give exactly what
    gpuq_join_probe_keys gives over the same table"""
    case = parity_case(nkeys)
    d = case.dev()
    pk, pkv, _, _ = case.probe_side()
    out_cap = 4 * case.pn + case.bn
    d.pop("ws", None)
    op0, ob0, n0 = gq.join_probe_keys(pk, case.table(gq), CAP, case.bn,
                                      out_cap, key_validities=pkv,
                                      join_type=jt)
    old = pair_list(op0, ob0)
    old_unmatched = case.unmatched(gq) if jt == R.FULL else []
    d.pop("ws", None)
    op, ob, n = case.probe(gq, CONDS["always"], jt)
    assert n == n0 and n0 > 0
    assert pair_list(op, ob) == old
    if jt == R.FULL:
        assert case.unmatched(gq) == old_unmatched
    d.pop("ws", None)


# ---------------- 2. edges ----------------

@pytest.mark.parametrize("n", [0, 1, 1023, 1024, 1025, 4095, 4096, 4097])
def test_probe_row_counts(gq, n):
    case = parity_case(2)
    for jt in (R.INNER, R.OUTER, R.SEMI, R.ANTI, R.FULL):
        exp, _ = case.expected("x<y", jt, n)
        op, ob, nm = case.probe(gq, CONDS["x<y"], jt, n=n)
        assert nm == len(exp), (jt, nm)
        assert pair_list(op, ob) == exp, jt
    case.dev().pop("ws", None)


def test_empty_build_side(gq):
    case = Case(2, seed=7205, bn=0, pn=1_003)
    assert case.bn == 0
    every = [(i, NIL) for i in range(case.pn)]
    for jt, exp in ((R.INNER, []), (R.SEMI, []), (R.OUTER, every),
                    (R.ANTI, every), (R.FULL, every)):
        op, ob, n = case.probe(gq, CONDS["x<y"], jt)
        assert n == len(exp) and pair_list(op, ob) == exp, jt
    assert case.unmatched(gq) == []


def long_chain_case():
    """key (5000, 5000) — outside every value table — on 300 build rows and
    70 probe rows (more than one wave). by = 0 for build rows 0 and 1 (px is
    never below 0, so the first two inserted never pass), 99 for the last
    one (passes whenever px is below 99) and scattered values in between:
    which candidates pass differs from probe row to probe row, and nearly
    every one has more than two passing pairs, so phase B walks its chain
    again."""
    far, dup, npr = 5000, 300, 70

    def extra(c):
        rng = np.random.RandomState(99)
        by = rng.randint(0, 100, size=dup).astype(np.int64)
        by[:2] = 0
        by[-1] = 99
        ok = rng.randint(0, 8, size=dup) != 0
        ok[[0, 1, dup - 1]] = True
        c.bk = [np.append(k, np.full(dup, far, np.int64)) for k in c.bk]
        c.bv = [np.append(v, np.ones(dup, bool)) for v in c.bv]
        for name, (vals, valid, dt) in list(c.bcols.items()):
            tail_v, tail_ok = (by, ok) if name == "by" else (vals[:dup], valid[:dup])
            c.bcols[name] = (np.append(vals, tail_v), np.append(valid, tail_ok), dt)
        c.pk = [np.append(k, np.full(npr, far, np.int64)) for k in c.pk]
        c.pv = [np.append(v, np.ones(npr, bool)) for v in c.pv]
        px = np.arange(npr, dtype=np.int64) + 20
        for name, (vals, valid, dt) in list(c.pcols.items()):
            tail_v, tail_ok = ((px, np.ones(npr, bool)) if name == "px"
                               else (vals[:npr], valid[:npr]))
            c.pcols[name] = (np.append(vals, tail_v), np.append(valid, tail_ok), dt)

    return Case(2, seed=7301, bn=2_001, pn=3_001, extra=extra)


def test_long_chain_scattered_passes(gq):
    case = long_chain_case()
    dup, npr = 300, 70
    first, last = case.bn - dup, case.bn - 1
    verd = case.verd("x<y")
    for r in verd[-npr:]:
        assert [j for j, _ in r] == list(range(first, case.bn))
        passing = [j for j, t in r if t is True]
        assert first not in passing and first + 1 not in passing
        assert last in passing and 2 < len(passing) < dup - 2
    assert len({tuple(t for _, t in r) for r in verd[-npr:]}) > 30
    for jt in (R.INNER, R.OUTER, R.SEMI, R.ANTI, R.FULL):
        exp, exp_unmatched = case.expected("x<y", jt)
        case.dev().pop("ws", None)
        op, ob, n = case.probe(gq, CONDS["x<y"], jt)
        assert n == len(exp) and pair_list(op, ob) == exp, jt
        if jt == R.FULL:
            assert case.unmatched(gq) == exp_unmatched


@pytest.mark.parametrize("jt", [R.INNER, R.OUTER, R.SEMI, R.ANTI, R.FULL])
def test_output_overflow_and_retry(gq, jt):
    case = parity_case(2)
    exp, exp_unmatched = case.expected("x<y", jt)
    assert len(exp) > 1000
    case.dev().pop("ws", None)
    op, ob, n = case.probe(gq, CONDS["x<y"], jt, out_cap=len(exp) - 1)
    assert op is None and ob is None and n == len(exp)
    op, ob, n2 = case.probe(gq, CONDS["x<y"], jt, out_cap=n)
    assert n2 == n and pair_list(op, ob) == exp
    if jt == R.FULL:
        # the matched bits were set twice; the unmatched list is still right
        assert case.unmatched(gq) == exp_unmatched
    case.dev().pop("ws", None)


def test_lowered_triple_and_row_count_check(gq):
    case = parity_case(2)
    d = case.dev()
    pk, pkv, pc, pcv = case.probe_side()
    triple = gq.lower_join_cond(CONDS["x<y"], pc, d["bcols"])
    assert triple[0] == ["px", "by"] and triple[1] == [0, 1]
    op, ob, n = gq.join_probe_keys_cond(
        pk, case.table(gq), CAP, case.bn, 4 * case.pn, triple, pc, d["bcols"],
        probe_validities=pcv, build_validities=d["bvalid"], key_validities=pkv)
    assert pair_list(op, ob) == case.expected("x<y", R.INNER)[0]
    short = dict(d["bcols"], by=d["bcols"]["by"][:100])
    with pytest.raises(ValueError, match="'by' has 100 rows"):
        gq.join_probe_keys_cond(pk, case.table(gq), CAP, case.bn, 64,
                                CONDS["x<y"], pc, short)
    case.dev().pop("ws", None)


# ---------------- 3. node level ----------------

def run_node(plan, names):
    outs = list(plan.execute_columnar())
    for out in outs:
        assert list(out.columns().keys()) == names
    return outs, [r for out in outs for r in batch_rows(out, names)]


@pytest.mark.parametrize("jt", [R.INNER, R.OUTER, R.SEMI, R.ANTI, R.FULL])
def test_node_two_probe_batches_through_the_rule(gq, jt):
    from spark_amd import exec as gx
    case = parity_case(2)
    left, right = case.batches(gx, [0, 6_001, case.pn])
    lk, rk = case.keys()
    node = gx.ShuffledHashJoinExec(lk, rk, "right", left, right,
                                   join_type=JT_NAMES[jt],
                                   condition=CONDS["x<y"])
    plan = gx.GpuColumnarRule().pre_columnar_transitions(node)
    assert type(plan) is gx.GpuShuffledHashJoinExec
    assert plan.condition is CONDS["x<y"]
    names = (case.lnames() if jt in (R.SEMI, R.ANTI)
             else case.rnames() + case.lnames())
    outs, got = run_node(plan, names)
    exp = case.expected_rows("x<y", jt)
    assert len(got) == len(exp) and sort_rows(got) == exp
    # NULLs of the payload columns came through (bitmaps survive the
    # gather): columns the condition does not read, so a NULL there says
    # nothing about the pair
    payload = [("pf", "pid")] + ([] if jt in (R.SEMI, R.ANTI)
                                 else [("bg", "bid"), ("bz", "bid")])
    for col, rid in payload:
        k, i = names.index(col), names.index(rid)
        assert any(r[k] is None and r[i] is not None for r in got)
        assert any(r[k] is not None and r[i] is not None for r in got)
    if jt == R.FULL:
        # one batch per probe batch, then ONE batch of unmatched build rows
        assert len(outs) == 3
        pid = names.index("pid")
        _, unmatched = case.expected("x<y", jt)
        tail = batch_rows(outs[2], names)
        assert sorted(r[names.index("bid")] for r in tail) == unmatched
        assert all(r[pid] is None for r in tail)
        for out in outs[:2]:
            assert all(r[pid] is not None for r in batch_rows(out, names))
        # key-equal build rows whose pairs all fail are among them
        failing = {j for r in case.verd("x<y") for j, _ in r} - \
            {j for r in case.verd("x<y") for j, t in r if t is True}
        assert len(failing) > 100 and failing <= set(unmatched)
    else:
        assert len(outs) == 2


def test_node_right_outer_builds_on_the_left(gq):
    from spark_amd import exec as gx
    case = parity_case(1)
    probe, build = case.batches(gx)
    lk, rk = case.keys()
    # the build side (rk*, by, ...) is the LEFT child here
    plan = gx.GpuShuffledHashJoinExec(rk, lk, "left", build, probe,
                                      join_type="right_outer",
                                      condition=CONDS["compound"])
    names = case.rnames() + case.lnames()
    assert plan.output == names
    _, got = run_node(plan, names)
    exp = case.expected_rows("compound", R.OUTER)
    assert len(got) == len(exp) and sort_rows(got) == exp


def test_node_broadcast_join_through_the_rule(gq):
    from spark_amd import exec as gx
    case = parity_case(4)
    left, right = case.batches(gx, [0, 4_000, case.pn])
    lk, rk = case.keys()
    node = gx.BroadcastHashJoinExec(lk, rk, "right", left,
                                    gx.BroadcastExchangeExec(right),
                                    join_type="left_anti",
                                    condition=CONDS["f!=g"])
    plan = gx.GpuColumnarRule().pre_columnar_transitions(node)
    assert type(plan) is gx.GpuBroadcastHashJoinExec
    _, got = run_node(plan, case.lnames())
    exp = case.expected_rows("f!=g", R.ANTI)
    assert len(got) == len(exp) and sort_rows(got) == exp


def test_node_single_key_sort_merge_through_the_rule(gq):
    """nkeys == 1 with a condition runs the composite table with one key;
    the SMJ mapping keeps its re-sort wrapper around the conditioned join"""
    from spark_amd import exec as gx
    case = parity_case(1)
    left, right = case.batches(gx)
    node = gx.SortMergeJoinExec("lk0", "rk0", left, right,
                                join_type="left_semi",
                                condition=CONDS["x<y"])
    plan = gx.GpuColumnarRule().pre_columnar_transitions(node)
    assert type(plan) is gx.GpuSortExec
    assert plan.children[0].condition is CONDS["x<y"]
    names = case.lnames()
    outs = list(plan.execute_columnar())
    got = [r for out in outs for r in batch_rows(out, names)]
    exp = case.expected_rows("x<y", R.SEMI)
    assert len(got) == len(exp) and sort_rows(got) == exp
    keys = [r[0] for r in got]
    assert keys == sorted(keys, key=lambda k: (k is not None, k or 0))
