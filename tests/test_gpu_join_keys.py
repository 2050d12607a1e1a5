"""GPU parity for the composite-key hash join (gpuq_join_*_keys and the
2-4 key path of GpuShuffledHashJoinExec) against a plain Python dict join.
All key and payload data are int64, so every comparison is exact; join
order is unspecified, so results compare as multisets of full rows."""
import collections
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

I64_MIN = -(1 << 63)
NIL = 0xFFFFFFFF
JOIN_TYPES = ["inner", "left_outer", "left_semi", "left_anti", "full_outer"]
# neither a multiple of JOIN_CHUNK (4096) nor of the wave (64); several blocks
BUILD_ROWS, PROBE_ROWS = 10_007, 13_003


@pytest.fixture(scope="module")
def gq():
    from spark_amd import gpuq
    assert torch.cuda.is_available()
    return gpuq


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def pack_validity(valid_bool):
    return torch.from_numpy(np.packbits(valid_bool, bitorder="little")).cuda()


def sort_rows(rows):
    return sorted(rows, key=lambda r: tuple((x is None, x or 0) for x in r))


def batch_rows(batch, names):
    """device batch -> list of row tuples, None where the bitmap says NULL"""
    n = batch.num_rows()
    cols = []
    for name in names:
        data = batch.column(name).cpu().numpy()
        v = batch.validity(name)
        ok = (np.unpackbits(v.cpu().numpy(), count=n, bitorder="little")
              .astype(bool) if v is not None else np.ones(n, bool))
        cols.append([int(x) if o else None for x, o in zip(data, ok)])
    return list(zip(*cols)) if cols else []


def pair_list(op, ob):
    p = op.cpu().numpy().view(np.uint32).tolist()
    b = ob.cpu().numpy().view(np.uint32).tolist()
    return sorted(zip(p, b))


# ---------------- data + reference ----------------

# value tables: -1, 0 and INT64_MIN are ordinary key components; tables 0
# and 1 overlap, so (a, b) and (b, a) both occur
VALS0 = np.array([-1, 0, I64_MIN] + list(range(3, 60)), dtype=np.int64)
VALS1 = np.array(list(range(2, 100)) + [I64_MIN, -1], dtype=np.int64)
VALS2 = np.array([-1, 0], dtype=np.int64)
VALS3 = np.array([I64_MIN, 7], dtype=np.int64)
# (build, probe) domain sizes per column: 3000 build tuples against 6000
# probe tuples whatever nkeys is, so ~3.3 build rows per tuple, about half
# the probe rows unmatched, inner output ~1.7x the probe rows
DOMAINS = {2: [(60, 60), (50, 100)],
           3: [(30, 30), (50, 100), (2, 2)],
           4: [(15, 15), (50, 100), (2, 2), (2, 2)]}
TABLES = [VALS0, VALS1, VALS2, VALS3]


def gen_side(rng, n, nkeys, side):
    keys = [TABLES[c][rng.randint(0, DOMAINS[nkeys][c][side], size=n)]
            for c in range(nkeys)]
    # a NULL in exactly one key column of ~6% of the rows, per-column bitmaps
    valid = [np.ones(n, bool) for _ in range(nkeys)]
    rows = np.flatnonzero(rng.randint(0, 16, size=n) == 0)
    which = rng.randint(0, nkeys, size=len(rows))
    for r, c in zip(rows, which):
        valid[c][r] = False
    pay = rng.randint(-(1 << 62), 1 << 62, size=n).astype(np.int64)
    return keys, valid, pay


def tuple_or_none(keys, valid, i):
    if not all(v[i] for v in valid):
        return None
    return tuple(int(k[i]) for k in keys)


class Case:
    """one seeded data set + its dict-join reference"""

    def __init__(self, nkeys, seed, bn=BUILD_ROWS, pn=PROBE_ROWS, extra=None):
        rng = np.random.RandomState(seed)
        self.nkeys = nkeys
        self.bk, self.bv, self.bp = gen_side(rng, bn, nkeys, 0)
        self.pk, self.pv, self.pp = gen_side(rng, pn, nkeys, 1)
        if extra is not None:
            extra(self)
        self.bn, self.pn = len(self.bp), len(self.pp)
        self.table = collections.defaultdict(list)
        for j in range(self.bn):
            t = tuple_or_none(self.bk, self.bv, j)
            if t is not None:
                self.table[t].append(j)
        self.hits = []
        for i in range(self.pn):
            t = tuple_or_none(self.pk, self.pv, i)
            self.hits.append(self.table.get(t, []) if t is not None else [])

    def check_coverage(self):
        """the properties the parity data must have, asserted on the CPU so
        a seed change cannot silently remove them"""
        dup = collections.Counter(len(v) for v in self.table.values())
        assert dup[1] and dup[2] and sum(c for d, c in dup.items() if d >= 3)
        unmatched = sum(1 for h in self.hits if not h) / self.pn
        assert 0.35 < unmatched < 0.65
        tuples = set(self.table)
        firsts = collections.Counter(t[0] for t in tuples)
        assert max(firsts.values()) > 1     # same first column, later differs
        assert any(t[0] != t[1] and (t[1], t[0]) + t[2:] in tuples
                   for t in tuples)          # (a, b) and (b, a)
        comps = {x for t in tuples for x in t}
        assert {-1, 0, I64_MIN} <= comps
        ptuples = {tuple_or_none(self.pk, self.pv, i) for i in range(self.pn)}
        assert {-1, 0, I64_MIN} <= {x for t in ptuples if t for x in t}
        for valid, n in ((self.bv, self.bn), (self.pv, self.pn)):
            nulls = sum((~v).astype(int) for v in valid)
            assert nulls.max() == 1 and (nulls == 1).sum() > 50
            assert all((~v).any() for v in valid)   # every column has NULLs
        inner = sum(len(h) for h in self.hits)
        assert inner < 4 * self.pn

    # rows as the join node lays them out: build columns, then probe columns
    def brow(self, j):
        if j is None:
            return (None,) * (self.nkeys + 1)
        return tuple(int(k[j]) if v[j] else None
                     for k, v in zip(self.bk, self.bv)) + (int(self.bp[j]),)

    def prow(self, i):
        if i is None:
            return (None,) * (self.nkeys + 1)
        return tuple(int(k[i]) if v[i] else None
                     for k, v in zip(self.pk, self.pv)) + (int(self.pp[i]),)

    def expected_pairs(self, jt):
        """(probe_rid or None, build_rid or None)"""
        exp = []
        for i, h in enumerate(self.hits):
            if jt == "inner":
                exp += [(i, j) for j in h]
            elif jt in ("left_outer", "full_outer"):
                exp += [(i, j) for j in h] if h else [(i, None)]
            elif jt == "left_semi":
                exp += [(i, None)] if h else []
            else:
                exp += [] if h else [(i, None)]
        if jt == "full_outer":
            matched = {j for h in self.hits for j in h}
            exp += [(None, j) for j in range(self.bn) if j not in matched]
        return exp

    def expected_rows(self, jt):
        if jt in ("left_semi", "left_anti"):
            return sort_rows(self.prow(i) for i, _ in self.expected_pairs(jt))
        return sort_rows(self.brow(j) + self.prow(i)
                         for i, j in self.expected_pairs(jt))

    def names(self, jt):
        ln = [f"lk{c}" for c in range(self.nkeys)] + ["lp"]
        rn = [f"rk{c}" for c in range(self.nkeys)] + ["rp"]
        return ln if jt in ("left_semi", "left_anti") else rn + ln

    def probe_batch(self, gx, lo=0, hi=None):
        hi = self.pn if hi is None else hi
        cols = {f"lk{c}": to_dev(self.pk[c][lo:hi]) for c in range(self.nkeys)}
        cols["lp"] = to_dev(self.pp[lo:hi])
        return gx.ColumnarBatch(cols, validity={
            f"lk{c}": pack_validity(self.pv[c][lo:hi])
            for c in range(self.nkeys)})

    def build_batch(self, gx):
        cols = {f"rk{c}": to_dev(self.bk[c]) for c in range(self.nkeys)}
        cols["rp"] = to_dev(self.bp)
        return gx.ColumnarBatch(cols, validity={
            f"rk{c}": pack_validity(self.bv[c]) for c in range(self.nkeys)})

    def run(self, jt, splits=None):
        from spark_amd import exec as gx
        splits = splits or [0, self.pn]
        left = gx.InputBatches([self.probe_batch(gx, a, b)
                                for a, b in zip(splits, splits[1:])])
        right = gx.InputBatches([self.build_batch(gx)])
        node = gx.ShuffledHashJoinExec(
            tuple(f"lk{c}" for c in range(self.nkeys)),
            tuple(f"rk{c}" for c in range(self.nkeys)),
            "right", left, right, join_type=jt)
        plan = gx.GpuColumnarRule().pre_columnar_transitions(node)
        assert type(plan) is gx.GpuShuffledHashJoinExec
        return list(plan.execute_columnar())


@functools.lru_cache(maxsize=None)
def parity_case(nkeys):
    return Case(nkeys, seed=1000 + nkeys)


# ---------------- 1. parity through the rule ----------------

@pytest.mark.parametrize("jt", JOIN_TYPES)
@pytest.mark.parametrize("nkeys", [2, 3, 4])
def test_join_keys_parity(gq, nkeys, jt):
    case = parity_case(nkeys)
    case.check_coverage()
    names = case.names(jt)
    got = []
    for out in case.run(jt):
        assert list(out.columns().keys()) == names
        got += batch_rows(out, names)
    exp = case.expected_rows(jt)
    assert len(got) == len(exp)
    assert sort_rows(got) == exp


# ---------------- 2. full outer, probe side in three batches ----------------

def test_full_outer_three_probe_batches(gq):
    far = 1000   # outside every value table

    def extra(c):
        # a build row whose tuple only the LAST probe row carries
        c.bk = [np.append(k, far) for k in c.bk]
        c.bv = [np.append(v, True) for v in c.bv]
        c.bp = np.append(c.bp, 77)
        c.pk = [np.append(k, far) for k in c.pk]
        c.pv = [np.append(v, True) for v in c.pv]
        c.pp = np.append(c.pp, 88)

    case = Case(2, seed=2002, extra=extra)
    late = case.bn - 1
    splits = [0, 4001, 9000, case.pn]
    matchers = [i for i, h in enumerate(case.hits) if late in h]
    assert matchers == [case.pn - 1] and matchers[0] >= splits[2]
    # rows that only a later batch matches exist in bulk too
    first_batch_matched = {j for h in case.hits[:splits[1]] for j in h}
    all_matched = {j for h in case.hits for j in h}
    assert len(all_matched - first_batch_matched) > 100
    assert len(all_matched) < case.bn

    names = case.names("full_outer")
    outs = case.run("full_outer", splits)
    # one batch per probe batch + ONE trailing batch of unmatched build rows
    assert len(outs) == 4
    got = [r for out in outs for r in batch_rows(out, names)]
    assert sort_rows(got) == case.expected_rows("full_outer")
    null_probe = (None,) * 3
    null_ext = [r for r in got if r[3:] == null_probe]
    # each unmatched build row exactly once (payloads identify build rows)
    unmatched = [j for j in range(case.bn) if j not in all_matched]
    assert sort_rows(r[:3] for r in null_ext) == \
        sort_rows(case.brow(j) for j in unmatched)
    assert len(set(case.bp.tolist())) == case.bn
    assert not any(r[2] == 77 for r in null_ext)
    assert [r for r in got if r[2] == 77] == [(far, far, 77, far, far, 88)]
    # the first three batches hold no NULL-extended build row at all
    for out in outs[:3]:
        assert not any(r[3:] == null_probe and r[2] is not None
                       for r in batch_rows(out, names))


# ---------------- 3. nkeys == 1 against the single-key join ----------------

def single_key_data():
    rng = np.random.RandomState(3003)
    bn, pn = 5_003, 7_001
    bk = rng.randint(-1, 3000, size=bn).astype(np.int64)
    pk = rng.randint(-1, 6000, size=pn).astype(np.int64)
    bk[::97] = -1
    pk[::89] = -1
    bv = rng.randint(0, 20, size=bn) != 0
    pv = rng.randint(0, 20, size=pn) != 0
    return bk, bv, pk, pv


@pytest.mark.parametrize("jt", [0, 1, 2, 3, 4])
def test_single_key_through_keys_entry_points(gq, jt):
    bk, bv, pk, pv = single_key_data()
    assert (bk[bv] == -1).sum() > 10 and (pk[pv] == -1).sum() > 10
    bn, pn = len(bk), len(pk)
    cap = 1 << 14
    dbk, dpk = to_dev(bk), to_dev(pk)
    dbv, dpv = pack_validity(bv), pack_validity(pv)
    out_cap = 4 * pn + bn
    ws1 = gq.join_build(dbk, cap, key_validity=dbv)
    op1, ob1, n1 = gq.join_probe(dpk, ws1, cap, bn, out_cap,
                                 key_validity=dpv, join_type=jt)
    ws = gq.join_build_keys([dbk], cap, key_validities=[dbv])
    op, ob, n = gq.join_probe_keys([dpk], ws, cap, bn, out_cap,
                                   key_validities=[dpv], join_type=jt)
    got = pair_list(op, ob)
    if jt == 4:
        assert not any(p == NIL for p, _ in got)   # probe half only
        uo, ub, nu = gq.join_keys_unmatched_build(ws, cap, bn, 1)
        assert nu == len(uo) and nu > 0
        got = sorted(got + pair_list(uo, ub))
        n += nu
    assert n == n1 and n1 > 0
    assert got == pair_list(op1, ob1)


# ---------------- 4. small table, heavy linear probing ----------------

@pytest.mark.parametrize("ndistinct", [8, 15])
def test_small_table_linear_probing(gq, ndistinct):
    rng = np.random.RandomState(4000 + ndistinct)
    tuples = [(int(a), int(b)) for a, b in
              zip(rng.randint(-5, 5, size=64), rng.randint(-5, 5, size=64))]
    tuples = list(dict.fromkeys(tuples))[:ndistinct]
    assert len(tuples) == ndistinct
    build = tuples + [tuples[i % ndistinct] for i in (0, 0, 3, 5, 5, 5)]
    misses = [(a, b) for a in range(-5, 5) for b in range(-5, 5)
              if (a, b) not in set(tuples)][:40]
    probe = tuples + misses + tuples[::2]
    table = collections.defaultdict(list)
    for j, t in enumerate(build):
        table[t].append(j)
    exp = sorted((i, j) for i, t in enumerate(probe) for j in table.get(t, []))
    bcols = [to_dev(np.array([t[c] for t in build], dtype=np.int64))
             for c in range(2)]
    pcols = [to_dev(np.array([t[c] for t in probe], dtype=np.int64))
             for c in range(2)]
    ws = gq.join_build_keys(bcols, 16)
    op, ob, n = gq.join_probe_keys(pcols, ws, 16, len(build), 1024)
    assert n == len(exp)
    assert pair_list(op, ob) == exp
    # anti join over the same table: exactly the misses
    op, ob, n = gq.join_probe_keys(pcols, ws, 16, len(build), 1024,
                                   join_type=gq.JOIN_ANTI)
    assert sorted(p for p, _ in pair_list(op, ob)) == \
        [i for i, t in enumerate(probe) if t not in table]


# ---------------- 5. edges ----------------

@pytest.mark.parametrize("jt", ["inner", "left_outer"])
def test_empty_build_side(gq, jt):
    case = Case(2, seed=5005, bn=0, pn=1_003)
    assert case.bn == 0
    names = case.names(jt)
    got = [r for out in case.run(jt) for r in batch_rows(out, names)]
    exp = case.expected_rows(jt)
    assert len(exp) == (0 if jt == "inner" else case.pn)
    assert sort_rows(got) == exp


def test_empty_probe_batch(gq):
    case = parity_case(2)
    cap = 1 << 15
    ws = gq.join_build_keys([to_dev(k) for k in case.bk], cap,
                            key_validities=[pack_validity(v) for v in case.bv])
    empty = [torch.empty(0, dtype=torch.int64, device="cuda")] * 2
    for jt in (gq.JOIN_INNER, gq.JOIN_OUTER, gq.JOIN_ANTI, gq.JOIN_FULL):
        op, ob, n = gq.join_probe_keys(empty, ws, cap, case.bn, 64,
                                       join_type=jt)
        assert n == 0 and op.numel() == 0 and ob.numel() == 0
    # through the node: an empty batch between two real ones
    names = case.names("left_outer")
    outs = case.run("left_outer", [0, 5000, 5000, case.pn])
    assert [o.num_rows() for o in outs][1] == 0
    got = [r for out in outs for r in batch_rows(out, names)]
    assert sort_rows(got) == case.expected_rows("left_outer")


def test_probe_output_overflow_and_retry(gq):
    case = parity_case(2)
    cap = 1 << 15
    ws = gq.join_build_keys([to_dev(k) for k in case.bk], cap,
                            key_validities=[pack_validity(v) for v in case.bv])
    pk = [to_dev(k) for k in case.pk]
    pv = [pack_validity(v) for v in case.pv]
    exp = sorted(case.expected_pairs("inner"))
    assert len(exp) > 1000
    op, ob, n = gq.join_probe_keys(pk, ws, cap, case.bn, 1000,
                                   key_validities=pv)
    assert op is None and ob is None and n == len(exp)
    op, ob, n2 = gq.join_probe_keys(pk, ws, cap, case.bn, n,
                                    key_validities=pv)
    assert n2 == n and pair_list(op, ob) == exp


# ---------------- 6. build-table overflow ----------------

def test_build_table_overflow_is_bounded(gq):
    a = np.arange(17, dtype=np.int64)
    cols = [to_dev(a), to_dev(a * 3 - 20)]
    with pytest.raises(gq.GpuqError, match="overflow"):
        gq.join_build_keys(cols, 16)
    torch.cuda.synchronize()
    # the process carries on: a normal join right after
    ws = gq.join_build_keys(cols, 64)
    op, ob, n = gq.join_probe_keys(cols, ws, 64, 17, 64)
    assert n == 17 and pair_list(op, ob) == [(i, i) for i in range(17)]


# ---------------- 7. TPC-H Q5 shape end to end ----------------

def test_q5_shape_end_to_end(gq):
    from spark_amd import exec as gx
    rng = np.random.RandomState(7007)
    n_region, n_nation, n_supp, n_cust, n_ord, n_li = 5, 25, 200, 1_500, 6_000, 24_000
    nation_region = (np.arange(n_nation) % n_region).astype(np.int64)
    s_nation = rng.randint(0, n_nation, size=n_supp).astype(np.int64)
    c_nation = rng.randint(0, n_nation, size=n_cust).astype(np.int64)
    o_cust = rng.randint(0, n_cust, size=n_ord).astype(np.int64)
    o_date = rng.randint(0, 3 * 365, size=n_ord).astype(np.int64)
    l_order = rng.randint(0, n_ord, size=n_li).astype(np.int64)
    l_supp = rng.randint(0, n_supp, size=n_li).astype(np.int64)
    l_price = rng.randint(100, 100_000, size=n_li).astype(np.int64)  # cents
    l_disc = rng.randint(0, 11, size=n_li).astype(np.int64)          # percent
    d0, d1, region = 365, 730, 2

    # expected, by plain loops: revenue in cents * percent
    exp = collections.defaultdict(int)
    for li in range(n_li):
        o = int(l_order[li])
        if not d0 <= o_date[o] < d1:
            continue
        cn = int(c_nation[o_cust[o]])
        s = int(l_supp[li])
        if s_nation[s] != cn:           # the second equi-condition
            continue
        if nation_region[cn] != region:
            continue
        exp[cn] += int(l_price[li]) * (100 - int(l_disc[li]))
    assert len(exp) >= 2

    def scan(**cols):
        return gx.InputBatches([gx.ColumnarBatch(
            {k: to_dev(v) for k, v in cols.items()})])

    ar = lambda n: np.arange(n, dtype=np.int64)
    customer = scan(c_custkey=ar(n_cust), c_nationkey=c_nation)
    orders = scan(o_orderkey=ar(n_ord), o_custkey=o_cust, o_orderdate=o_date)
    lineitem = scan(l_orderkey=l_order, l_suppkey=l_supp,
                    l_extendedprice=l_price, l_discount=l_disc)
    supplier = scan(s_suppkey=ar(n_supp), s_nationkey=s_nation)
    nation = scan(n_nationkey=ar(n_nation), n_regionkey=nation_region)
    regions = scan(r_regionkey=ar(n_region))

    co = gx.ShuffledHashJoinExec("o_custkey", "c_custkey", "right",
                                 orders, customer)
    co = gx.FilterExec("o_orderdate", "<", d1,
                       gx.FilterExec("o_orderdate", ">=", d0, co))
    col = gx.ShuffledHashJoinExec("l_orderkey", "o_orderkey", "right",
                                  lineitem, co)
    cols_ = gx.ShuffledHashJoinExec(("l_suppkey", "c_nationkey"),
                                    ("s_suppkey", "s_nationkey"), "right",
                                    col, supplier)
    n_ = gx.ShuffledHashJoinExec("s_nationkey", "n_nationkey", "right",
                                 cols_, nation)
    r_ = gx.ShuffledHashJoinExec("n_regionkey", "r_regionkey", "right",
                                 n_, regions)
    f = gx.FilterExec("r_regionkey", "==", region, r_)
    p = gx.ProjectExec(["n_nationkey", "l_extendedprice",
                        ("one_minus_disc", "l_discount", "rsub", None, 100)], f)
    p = gx.ProjectExec(["n_nationkey",
                        ("revenue", "l_extendedprice", "*", "one_minus_disc",
                         None)], p)
    agg = gx.HashAggregateExec("n_nationkey", [("sum", "revenue")], "complete", p)
    plan = gx.SortExec(gx.SortOrder("sum(revenue)", descending=True), False, agg)

    gpu = gx.GpuColumnarRule().pre_columnar_transitions(plan)
    composite = gpu.children[0].children[0].children[0].children[0] \
        .children[0].children[0].children[0]
    assert isinstance(composite, gx.GpuShuffledHashJoinExec)
    assert composite.left_keys == ("l_suppkey", "c_nationkey")
    outs = list(gpu.execute_columnar())
    assert len(outs) == 1
    got = batch_rows(outs[0], ["n_nationkey", "sum(revenue)"])
    assert sorted(got) == sorted(exp.items())
    rev = [r for _, r in got]
    assert all(a >= b for a, b in zip(rev, rev[1:]))
