"""GPU checks of the exact 128-bit decimal SUM (spec ops 8/9/10, the
"sum_decimal" aggregate and the decimal-overflow-to-NULL kernel). The only
reference is Python int arithmetic, so every comparison is exact."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
LDS_CAP = 1024       # cap * (1 + 3..4 words) * 8 <= 64 KB: per-block LDS tables
GLOBAL_CAP = 16384   # past 64 KB: the global table
CAPS = [LDS_CAP, GLOBAL_CAP]


@pytest.fixture(scope="module")
def gq():
    from spark_amd import gpuq
    assert torch.cuda.is_available()
    return gpuq


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def pack_validity(valid_bool):
    return torch.from_numpy(np.packbits(valid_bool, bitorder="little")).cuda()


def unpack_validity(bits, n):
    return np.unpackbits(bits.cpu().numpy(), count=n,
                         bitorder="little").astype(bool)


def i64(x):
    """low 64 bits of a Python int as a signed int64 value."""
    x &= M64
    return x - (1 << 64) if x >> 63 else x


def split128(x):
    """Python int in [-2^127, 2^127) -> (lo, hi) signed int64 words."""
    return i64(x), i64(x >> 64)


def i64_array(values):
    return np.array([int(v) for v in values], dtype=np.int64)


def random_values(seed, n):
    """full-range int64 values, ~25 % NULL."""
    rng = np.random.default_rng(seed)
    vals = rng.integers(-(1 << 63), (1 << 63) - 1, size=n, dtype=np.int64,
                        endpoint=True)
    valid = rng.random(n) >= 0.25
    return vals, valid


# ---------- 1. carry edges, one group ----------

EDGE_CASES = {
    "lo_wraps_to_zero": [2**63 - 1, 2**63 - 1, 2],
    "carry_cancels_sign_extension": [-1, 1],
    "three_int64_min": [-2**63] * 3,
    "one_slot_2_pow_74": [2**62] * 4096,
}


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("case", sorted(EDGE_CASES))
def test_carry_edges_one_group(gq, case, cap):
    vals = EDGE_CASES[case]
    v = to_dev(i64_array(vals))
    keys = to_dev(np.full(len(vals), 7, dtype=np.int64))
    ok, okv, accs = gq.hash_agg_multi(
        keys, [("sum_dec128", v), ("count", v)], cap)
    assert ok.cpu().tolist() == [7] and okv.cpu().tolist() == [1]
    assert len(accs) == 3
    assert gq.dec128_to_pyints(accs[0], accs[1]) == [sum(vals)]
    assert accs[2].cpu().tolist() == [len(vals)]
    if case == "lo_wraps_to_zero":
        assert accs[0].cpu().tolist() == [0] and accs[1].cpu().tolist() == [1]
    if case == "carry_cancels_sign_extension":
        assert accs[0].cpu().tolist() == [0] and accs[1].cpu().tolist() == [0]


# ---------- 2. random full-range values, both special slots ----------

N = 20_000
ALL_NULL_KEY = 3


def single_key_data():
    rng = np.random.default_rng(11)
    keys = rng.integers(-1, 6, size=N, endpoint=True).astype(np.int64)
    kvalid = rng.random(N) >= 0.1
    vals, valid = random_values(12, N)
    valid[kvalid & (keys == ALL_NULL_KEY)] = False
    return keys, kvalid, vals, valid


def reference(key_tuples, vals, valid):
    """key tuple -> [exact sum of non-NULL values, count non-NULL, rows]."""
    ref = {}
    for kt, v, ok in zip(key_tuples, vals.tolist(), valid.tolist()):
        r = ref.setdefault(kt, [0, 0, 0])
        if ok:
            r[0] += v
            r[1] += 1
        r[2] += 1
    return ref


@pytest.mark.parametrize("cap", CAPS)
def test_random_full_range_single_key(gq, cap):
    keys, kvalid, vals, valid = single_key_data()
    ref = reference([(int(k) if kv else None,)
                     for k, kv in zip(keys, kvalid)], vals, valid)
    dv, dvv = to_dev(vals), pack_validity(valid)
    ok, okv, accs = gq.hash_agg_multi(
        to_dev(keys), [("sum_dec128", dv, dvv), ("count", dv, dvv), ("count*",)],
        cap, key_validity=pack_validity(kvalid))
    sums = gq.dec128_to_pyints(accs[0], accs[1])
    got = {}
    for k, kv, s, c, r in zip(ok.cpu().tolist(), okv.cpu().tolist(), sums,
                              accs[2].cpu().tolist(), accs[3].cpu().tolist()):
        got[(k if kv else None,)] = [s, c, r]
    assert (-1,) in ref and (None,) in ref       # both special slots in play
    assert ref[(ALL_NULL_KEY,)][:2] == [0, 0]
    assert got == ref


# ---------- 3. carry state across a batch boundary ----------

@pytest.mark.parametrize("cap", CAPS)
def test_two_batches_one_workspace(gq, cap):
    rng = np.random.default_rng(21)
    n = 4096
    keys = rng.integers(0, 3, size=2 * n, endpoint=True).astype(np.int64)
    pos = rng.integers(1 << 61, (1 << 63) - 1, size=n, dtype=np.int64)
    neg = -rng.integers(1 << 62, (1 << 63) - 1, size=n, dtype=np.int64) - 1
    assert sum(pos.tolist()) > 2**64 and sum(neg.tolist()) < -2**64
    ws = gq.agg_multi_workspace(cap, 3)
    res = gq.hash_agg_multi(
        to_dev(keys[:n]), [("sum_dec128", to_dev(pos)), ("count*",)], cap,
        workspace=ws, first_batch=True, finalize=False)
    assert res is None
    ok, okv, accs = gq.hash_agg_multi(
        to_dev(keys[n:]), [("sum_dec128", to_dev(neg)), ("count*",)], cap,
        workspace=ws, first_batch=False, finalize=True)
    vals = np.concatenate([pos, neg])
    ref = reference([(int(k),) for k in keys], vals, np.ones(2 * n, dtype=bool))
    got = {(k,): [s, c, c] for k, s, c in zip(
        ok.cpu().tolist(), gq.dec128_to_pyints(accs[0], accs[1]),
        accs[2].cpu().tolist())}
    assert got == ref


# ---------- 4. composite keys ----------

def test_random_full_range_composite_keys(gq):
    rng = np.random.default_rng(31)
    k1 = rng.integers(-1, 3, size=N, endpoint=True).astype(np.int64)
    k2 = rng.integers(0, 2, size=N, endpoint=True).astype(np.int64)
    v1 = rng.random(N) >= 0.1
    v2 = rng.random(N) >= 0.1
    vals, valid = random_values(32, N)
    valid[v1 & v2 & (k1 == 2) & (k2 == 1)] = False     # an all-NULL group
    ref = reference([(int(a) if va else None, int(b) if vb else None)
                     for a, va, b, vb in zip(k1, v1, k2, v2)], vals, valid)
    dv, dvv = to_dev(vals), pack_validity(valid)
    okeys, kmask, accs = gq.hash_agg_keys(
        [to_dev(k1), to_dev(k2)],
        [("sum_dec128", dv, dvv), ("count", dv, dvv), ("count*",)], 1 << 10,
        key_validities=[pack_validity(v1), pack_validity(v2)])
    sums = gq.dec128_to_pyints(accs[0], accs[1])
    got = {}
    for a, b, m, s, c, r in zip(okeys[0].cpu().tolist(), okeys[1].cpu().tolist(),
                                kmask.cpu().tolist(), sums,
                                accs[2].cpu().tolist(), accs[3].cpu().tolist()):
        got[(a if m & 1 else None, b if m & 2 else None)] = [s, c, r]
    assert ref[(2, 1)][:2] == [0, 0]
    assert got == ref


# ---------- 5. operator level ----------

def run_plan(node):
    from spark_amd import exec as gx
    outs = list(gx.GpuColumnarRule().pre_columnar_transitions(node)
                .execute_columnar())
    assert len(outs) == 1
    return outs[0]


def concat_partials(partials):
    """what the exchange would deliver to the final-mode node."""
    from spark_amd import exec as gx
    cols, validity = {}, {}
    for name in partials[0].columns():
        cols[name] = torch.cat([p.column(name) for p in partials])
        vs = [p.validity(name) for p in partials]
        if any(v is not None for v in vs):
            cat = [np.ones(p.num_rows(), dtype=bool) if v is None
                   else unpack_validity(v, p.num_rows())
                   for p, v in zip(partials, vs)]
            validity[name] = pack_validity(np.concatenate(cat))
    return gx.ColumnarBatch(cols, validity=validity or None)


def operator_data():
    """values around +-9e17, three quarters positive: groups pass 2^63."""
    rng = np.random.default_rng(41)
    mag = rng.integers(8 * 10**17, 92 * 10**16, size=N, dtype=np.int64)
    vals = np.where(rng.random(N) < 0.75, mag, -mag)
    valid = rng.random(N) >= 0.25
    k1 = rng.integers(0, 3, size=N, endpoint=True).astype(np.int64)
    k2 = rng.integers(10, 11, size=N, endpoint=True).astype(np.int64)
    k1_valid = rng.random(N) >= 0.1
    return vals, valid, k1, k2, k1_valid


# shape -> (group_key, nullable first key)
SHAPES = {"single": ("k1", False), "packed": (("k1", "k2"), False),
          "composite": (("k1", "k2"), True)}


def operator_result(out, names):
    """output batch -> {key tuple: (exact sum | None, wrapped sum | None,
    count*)}."""
    n = out.num_rows()
    kcols = []
    for k in names:
        col = out.column(k).cpu().tolist()
        v = out.validity(k)
        kv = unpack_validity(v, n) if v is not None else np.ones(n, dtype=bool)
        kcols.append([c if ok else None for c, ok in zip(col, kv)])
    lo, hi = out.column("sum_decimal_lo(v)"), out.column("sum_decimal_hi(v)")
    from spark_amd import gpuq
    exact = gpuq.dec128_to_pyints(lo, hi)
    vlo = unpack_validity(out.validity("sum_decimal_lo(v)"), n)
    vhi = unpack_validity(out.validity("sum_decimal_hi(v)"), n)
    assert (vlo == vhi).all()
    wrapped = out.column("sum(v)").cpu().tolist()
    vw = unpack_validity(out.validity("sum(v)"), n)
    star = out.column("count(1)").cpu().tolist()
    return {tuple(kc[i] for kc in kcols):
            (exact[i] if vlo[i] else None, wrapped[i] if vw[i] else None,
             star[i]) for i in range(n)}


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_operator_complete_and_partial_final(gq, shape):
    from spark_amd import exec as gx
    group_key, nullable = SHAPES[shape]
    names = (group_key,) if isinstance(group_key, str) else group_key
    vals, valid, k1, k2, k1_valid = operator_data()
    keycols = {"k1": k1, "k2": k2}
    ref = {}
    tuples = [tuple(None if (nullable and k == "k1" and not k1_valid[i])
                    else int(keycols[k][i]) for k in names) for i in range(N)]
    for kt, (s, c, r) in reference(tuples, vals, valid).items():
        ref[kt] = (s if c else None, i64(s) if c else None, r)
    assert any(s is not None and abs(s) >= 2**63 for s, _, _ in ref.values())

    def batch(lo, hi):
        cols = {k: to_dev(keycols[k][lo:hi]) for k in names}
        cols["v"] = to_dev(vals[lo:hi])
        validity = {"v": pack_validity(valid[lo:hi])}
        if nullable:
            validity["k1"] = pack_validity(k1_valid[lo:hi])
        return gx.ColumnarBatch(cols, validity=validity)

    aggs = [("sum_decimal", "v"), ("sum", "v"), ("count*", None)]
    prec = {"v": 18}
    complete = run_plan(gx.HashAggregateExec(
        group_key, aggs, "complete", gx.InputBatches([batch(0, N)]),
        decimal_precision=prec))
    assert operator_result(complete, names) == ref

    # two partial nodes = two ranks; concat = the exchange; then final
    half = N // 2 + 1
    partials = [run_plan(gx.HashAggregateExec(
        group_key, aggs, "partial", gx.InputBatches([batch(lo, hi)]),
        decimal_precision=prec)) for lo, hi in ((0, half), (half, N))]
    for p in partials:
        assert {"dsum_lo(v)", "dsum_hi(v)", "count(v)"} <= set(p.columns())
    final = run_plan(gx.HashAggregateExec(
        group_key, aggs, "final", gx.InputBatches([concat_partials(partials)]),
        decimal_precision=prec))
    assert operator_result(final, names) == ref


# ---------- 6. overflow-to-NULL through final mode ----------

def test_final_mode_overflow_to_null(gq):
    from spark_amd import exec as gx
    half = 5 * 10**27                      # p = 18 -> bound 10^28 < 2^127
    rows = [(0, half, 1), (0, half - 1, 1),        # 10^28 - 1: valid
            (1, half, 1), (1, half, 1),            # 10^28: NULL
            (2, -half, 1), (2, -(half - 1), 1),    # -(10^28 - 1): valid
            (3, -half, 1), (3, -half, 1),          # -10^28: NULL
            (4, 0, 0), (4, 0, 0)]                  # no non-null input: NULL
    words = [split128(x) for _, x, _ in rows]
    pvalid = pack_validity(np.array([c > 0 for _, _, c in rows]))
    merged = gx.ColumnarBatch(
        {"k": to_dev(i64_array(k for k, _, _ in rows)),
         "dsum_lo(v)": to_dev(i64_array(w[0] for w in words)),
         "dsum_hi(v)": to_dev(i64_array(w[1] for w in words)),
         "count(v)": to_dev(i64_array(c for _, _, c in rows))},
        validity={"dsum_lo(v)": pvalid, "dsum_hi(v)": pvalid})
    out = run_plan(gx.HashAggregateExec(
        "k", [("sum_decimal", "v")], "final", gx.InputBatches([merged]),
        decimal_precision={"v": 18}))
    n = out.num_rows()
    assert n == 5
    sums = gq.dec128_to_pyints(out.column("sum_decimal_lo(v)"),
                               out.column("sum_decimal_hi(v)"))
    vlo = unpack_validity(out.validity("sum_decimal_lo(v)"), n)
    vhi = unpack_validity(out.validity("sum_decimal_hi(v)"), n)
    got = {k: (s if a and b else None) for k, s, a, b in
           zip(out.column("k").cpu().tolist(), sums, vlo, vhi)}
    assert got == {0: 10**28 - 1, 1: None, 2: -(10**28 - 1), 3: None, 4: None}


# ---------- 7. the overflow kernel alone ----------

@pytest.mark.parametrize("precision", [1, 19, 28, 38])
def test_dec128_overflow_to_null_alone(gq, precision):
    n = 67                                 # ragged last validity byte
    bound = 10**precision
    edge = [bound - 1, -(bound - 1), bound, -bound, 0, 2**127 - 1, -2**127,
            bound + 1, -(bound + 1), 1, -1]
    xs = [edge[i % len(edge)] for i in range(n)]
    incoming = np.array([i % 5 != 2 for i in range(n)])
    words = [split128(x) for x in xs]
    lo = to_dev(i64_array(w[0] for w in words))
    hi = to_dev(i64_array(w[1] for w in words))
    assert gq.dec128_to_pyints(lo, hi) == xs
    bits = gq.dec128_overflow_to_null(lo, hi, precision, pack_validity(incoming))
    expect = [bool(inc) and -bound < x < bound for inc, x in zip(incoming, xs)]
    assert unpack_validity(bits, n).tolist() == expect
    # no incoming bitmap: every row starts valid
    bits = gq.dec128_overflow_to_null(lo, hi, precision)
    assert unpack_validity(bits, n).tolist() == [-bound < x < bound for x in xs]


# ---------- 8. empty-input global aggregate ----------

def test_empty_input_global_aggregate(gq):
    from spark_amd import exec as gx
    empty = gx.ColumnarBatch({"v": torch.empty(0, dtype=torch.int64,
                                               device="cuda")})
    out = run_plan(gx.HashAggregateExec(
        None, [("sum_decimal", "v")], "complete", gx.InputBatches([empty])))
    assert out.num_rows() == 1
    for name in ("sum_decimal_lo(v)", "sum_decimal_hi(v)"):
        assert out.column(name).cpu().tolist() == [0]
        assert unpack_validity(out.validity(name), 1).tolist() == [False]


# ---------- 9. ABI misuse ----------

def test_abi_misuse_is_rejected_before_any_launch(gq):
    L = gq.lib()
    n, cap = 8, 1024
    keys = to_dev(np.zeros(n, dtype=np.int64))
    vi = to_dev(np.arange(n, dtype=np.int64))
    vf = to_dev(np.arange(n, dtype=np.float64))
    cols = (gq._Col * 2)(gq._col(vi), gq._col(vf))
    outs = [torch.zeros(cap + 2, dtype=torch.int64, device="cuda")
            for _ in range(3)]
    outp = (ctypes.c_void_p * 3)(*[t.data_ptr() for t in outs])
    ok = torch.empty(cap + 2, dtype=torch.int64, device="cuda")
    okv = torch.empty(cap + 2, dtype=torch.uint8, device="cuda")
    ws = gq.agg_multi_workspace(cap, 3)
    ng = ctypes.c_int64(0)

    def call(ops, cids):
        k = len(ops)
        return L.gpuq_hash_agg_multi(
            gq._stream(), n, gq._col(keys), cols,
            (ctypes.c_int32 * k)(*ops), (ctypes.c_int32 * k)(*cids), k,
            ws.data_ptr(), cap, 1, 1, ok.data_ptr(), okv.data_ptr(), outp,
            ctypes.byref(ng))

    # a valid pairing is accepted and computes
    assert call([8, 9, 2], [0, 0, 0]) == 0
    assert ng.value == 1
    assert gq.dec128_to_pyints(outs[0][:1], outs[1][:1]) == [sum(range(n))]
    assert outs[2][:1].cpu().tolist() == [n]

    ws.fill_(0xAB)       # a launched init kernel would overwrite this
    torch.cuda.synchronize()
    for ops, cids in [([2, 8], [0, 0]),        # op 8 as the last spec
                      ([8, 3], [0, 0]),        # op 8 followed by op 3
                      ([9], [0]),              # a bare op 9
                      ([2, 9], [0, 0]),        # op 9 after a non-dec128 op
                      ([8, 9], [1, 1])]:       # op 8 on a float64 column
        assert call(ops, cids) == 2, (ops, cids)           # GPUQ_ERR_INVALID
        assert L.gpuq_last_error() != b""
    torch.cuda.synchronize()
    assert bool((ws == 0xAB).all())
