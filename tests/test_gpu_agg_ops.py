"""GPU checks of the hash aggregates' ops 0-7 (SUM / COUNT / MIN / MAX over
int64 and float64) on every entry point and table path, against the plain
reference in tests/agg_ref.py.

Every comparison is `==` on {key tuple: [result per spec]} over ALL groups;
the single exception is the cancelling float SUM of case (e), held to
agg_ref.sum_error_bound. Float SUM columns hold integer-valued doubles in
[-2^20, 2^20], so every partial sum is an integer below 2^41, exactly
representable, and the float64 SUM is the same in any order: a lost, doubled
or mis-merged update changes it. Floats are compared with their sign bit
(norm()), NaN as "is NaN".

Table paths. gpuq_hash_agg_multi builds in per-block LDS tables that merge
into the global table iff lds_bytes = cap * (1 + nspecs) * 8 <= 65536, else
directly in the global table; gpuq_hash_agg_i64_f64 takes its LDS kernel iff
cap <= 2048; GPUQ_NO_LDS_AGG (read per call) forces the global path of both.
gpuq_hash_agg_keys has one (global) path. Each case names its arithmetic."""
import functools
import math

import numpy as np
import pytest

import agg_ref

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
N = 20_000

# the full op list: 6 value ops, a COUNT per value column, COUNT(*)
FULL_SPECS = [("sum", "a"), ("sum", "b"), ("min", "c"), ("max", "c"),
              ("min", "d"), ("max", "d"), ("count", "a"), ("count", "b"),
              ("count", "c"), ("count", "d"), ("count*", None)]
# 11 specs -> 12 words = 96 B per slot
FULL_LDS_CAP = 512       # 512 * 12 * 8 = 49152 <= 65536: LDS tables + merge
FULL_GLOBAL_CAP = 1024   # 1024 * 12 * 8 = 98304 > 65536: global table
FULL_CAPS = [FULL_LDS_CAP, FULL_GLOBAL_CAP]


@pytest.fixture(scope="module")
def gq():
    from spark_amd import gpuq
    assert torch.cuda.is_available()
    return gpuq


@pytest.fixture(autouse=True)
def default_paths(monkeypatch):
    """a case takes the path its capacity selects unless it says otherwise."""
    monkeypatch.delenv("GPUQ_NO_LDS_AGG", raising=False)


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def pack_validity(valid_bool):
    return torch.from_numpy(np.packbits(valid_bool, bitorder="little")).cuda()


def f64_from_bits(words):
    return np.array(words, dtype=np.uint64).view(np.float64)


# quiet NaN, negative NaN, NaN with a payload, +-inf, both zeros
SPECIALS = f64_from_bits([0x7FF8000000000000, 0xFFF8000000000000,
                          0x7FF8000000ABCDEF, 0x7FF0000000000000,
                          0xFFF0000000000000, 0x8000000000000000, 0])
NANS, NEG_ZERO = SPECIALS[:3], SPECIALS[5]


def norm(x):
    """a result value made comparable with ==: NaN -> "nan", other floats
    carry their sign so that -0.0 != +0.0."""
    if isinstance(x, float):
        return "nan" if math.isnan(x) else (x, math.copysign(1.0, x))
    return x


def value_columns(rng, n):
    """name -> [values, valid]: a = integer-valued doubles (SUM f64), b =
    full-range int64 (SUM i64, wraps), c = full-range int64 (MIN / MAX), d =
    doubles with ~30 % specials (MIN / MAX f64). One bitmap per column."""
    d = rng.standard_normal(n) * 1e3
    pick = rng.random(n) < 0.3
    d[pick] = SPECIALS[rng.integers(0, len(SPECIALS), size=int(pick.sum()))]
    cols = {
        "a": rng.integers(-(1 << 20), 1 << 20, size=n, endpoint=True)
                .astype(np.float64),
        "b": rng.integers(I64_MIN, I64_MAX, size=n, dtype=np.int64, endpoint=True),
        "c": rng.integers(I64_MIN, I64_MAX, size=n, dtype=np.int64, endpoint=True),
        "d": d,
    }
    return {name: [v, rng.random(n) >= 0.25] for name, v in cols.items()}


def plant(cols, rng, all_null=None, only_i64_max=None, only_i64_min=None,
          only_neg_zero=None, both_zeros=None, only_nans=None,
          neg_zero_is_min=None, zero_is_max=None):
    """each argument is a row mask (or None) of one group."""
    def rows(sel):
        return int(sel.sum())
    if all_null is not None:
        for name in cols:
            cols[name][1][all_null] = False
    if only_i64_max is not None:                # encodes to the MIN init word
        cols["c"][0][only_i64_max] = I64_MAX
    if only_i64_min is not None:                # encodes to the MAX init word
        cols["c"][0][only_i64_min] = I64_MIN
    d = cols["d"][0]
    if only_neg_zero is not None:
        d[only_neg_zero] = NEG_ZERO
    if both_zeros is not None:
        d[both_zeros] = np.where(rng.random(rows(both_zeros)) < 0.5, NEG_ZERO, 0.0)
    if only_nans is not None:
        d[only_nans] = NANS[rng.integers(0, 3, size=rows(only_nans))]
    if neg_zero_is_min is not None:
        d[neg_zero_is_min] = np.where(rng.random(rows(neg_zero_is_min)) < 0.5,
                                      NEG_ZERO, 2.5)
    if zero_is_max is not None:
        d[zero_is_max] = np.where(rng.random(rows(zero_is_max)) < 0.5,
                                  NEG_ZERO, -2.5)


def ref_specs(speclist, cols, lo=0, hi=None):
    return [("count*",) if kind == "count*" else
            (kind, cols[c][0][lo:hi], cols[c][1][lo:hi]) for kind, c in speclist]


def dev_specs(speclist, cols, lo=0, hi=None):
    dev = {c: (to_dev(cols[c][0][lo:hi]), pack_validity(cols[c][1][lo:hi]))
           for _, c in speclist if c is not None}
    return [("count*",) if kind == "count*" else (kind,) + dev[c]
            for kind, c in speclist]


def reference(speclist, key_cols, key_valids, cols):
    ref = agg_ref.aggregate(key_cols, key_valids, ref_specs(speclist, cols))
    return {kt: [norm(x) for x in r] for kt, r in ref.items()}


def result_dict(speclist, key_tuples, accs):
    """kernel output -> the reference's dict. A SUM / MIN / MAX whose paired
    COUNT is 0 is None: its accumulator word is the op's init, not a value."""
    accs = [a.cpu().tolist() for a in accs]
    count_of = {c: j for j, (kind, c) in enumerate(speclist) if kind == "count"}
    out = {}
    for g, kt in enumerate(key_tuples):
        row = []
        for j, (kind, c) in enumerate(speclist):
            x = accs[j][g]
            if kind in ("sum", "min", "max") and accs[count_of[c]][g] == 0:
                x = None
            row.append(norm(x))
        assert kt not in out, f"group {kt} emitted twice"
        out[kt] = row
    assert len(out) == len(key_tuples)
    return out


def single_tuples(ok, okv):
    return [(k if v else None,) for k, v in zip(ok.cpu().tolist(),
                                                okv.cpu().tolist())]


def multi_result(speclist, res):
    ok, okv, accs = res
    return result_dict(speclist, single_tuples(ok, okv), accs)


def run_multi(gq, keys, kvalid, cols, speclist, cap, lo=0, hi=None, **kw):
    res = gq.hash_agg_multi(
        to_dev(keys[lo:hi]), dev_specs(speclist, cols, lo, hi), cap,
        key_validity=None if kvalid is None else pack_validity(kvalid[lo:hi]),
        **kw)
    return None if res is None else multi_result(speclist, res)


def agg_result(res, with_count=True):
    """hash_agg / hash_agg_partitioned output -> {key: [sum, count]}."""
    ok, okv, osum, osv, ocnt = (t.cpu().tolist() for t in res)
    out = {}
    for k, kv, s, sv, c in zip(ok, okv, osum, osv, ocnt):
        kt = (k if kv else None,)
        assert kt not in out, f"group {kt} emitted twice"
        out[kt] = [norm(s) if sv else None, c] if with_count else [norm(s)]
    return out


# ---------- shared single-key input ----------

K = 150                  # ordinary keys 0..K, plus -1 and ~10 % NULL
ALL_NULL_KEY, IMAX_KEY, IMIN_KEY = 3, 5, 6
NEG_ZERO_KEY, ZEROS_KEY, NANS_KEY, ZERO_MIN_KEY, ZERO_MAX_KEY = 7, 8, 9, 10, 11


@functools.lru_cache(maxsize=None)
def single_key_data():
    rng = np.random.default_rng(101)
    keys = rng.integers(-1, K, size=N, endpoint=True).astype(np.int64)
    kvalid = rng.random(N) >= 0.1
    cols = value_columns(rng, N)

    def grp(k):
        return kvalid & (keys == k)
    plant(cols, rng, grp(ALL_NULL_KEY), grp(IMAX_KEY), grp(IMIN_KEY),
          grp(NEG_ZERO_KEY), grp(ZEROS_KEY), grp(NANS_KEY), grp(ZERO_MIN_KEY),
          grp(ZERO_MAX_KEY))
    return keys, kvalid, cols


@functools.lru_cache(maxsize=None)
def single_key_ref(specs):
    keys, kvalid, cols = single_key_data()
    return reference(list(specs), [keys], [kvalid], cols)


def spec_index(speclist, kind, col):
    return speclist.index((kind, col))


# ---------- a. all ops, both paths, single key ----------

@pytest.mark.parametrize("cap", FULL_CAPS)
def test_all_ops_single_key(gq, cap):
    keys, kvalid, cols = single_key_data()
    ref = single_key_ref(tuple(FULL_SPECS))
    # the input holds what it is meant to hold
    assert (-1,) in ref and (None,) in ref       # both special slots in play
    assert len(ref) == K + 3
    assert ref[(ALL_NULL_KEY,)][:10] == [None] * 6 + [0] * 4
    assert ref[(ALL_NULL_KEY,)][10] > 0
    i_min_c, i_max_c = 2, 3
    i_min_d, i_max_d = 4, 5
    assert ref[(IMAX_KEY,)][i_min_c] == I64_MAX
    assert ref[(IMIN_KEY,)][i_max_c] == I64_MIN
    plus_zero = (0.0, 1.0)
    assert ref[(NEG_ZERO_KEY,)][i_min_d] == plus_zero
    assert ref[(NEG_ZERO_KEY,)][i_max_d] == plus_zero
    assert ref[(ZEROS_KEY,)][i_min_d:i_max_d + 1] == [plus_zero, plus_zero]
    assert ref[(NANS_KEY,)][i_min_d:i_max_d + 1] == ["nan", "nan"]
    assert ref[(ZERO_MIN_KEY,)][i_min_d] == plus_zero
    assert ref[(ZERO_MAX_KEY,)][i_max_d] == plus_zero
    assert any(r[i_max_d] == "nan" and r[i_min_d] != "nan" for r in ref.values())
    got = run_multi(gq, keys, kvalid, cols, FULL_SPECS, cap)
    assert got == ref


# ---------- b. LDS against global on the same input ----------

def test_multi_lds_equals_global(gq, monkeypatch):
    keys, kvalid, cols = single_key_data()
    lds = run_multi(gq, keys, kvalid, cols, FULL_SPECS, FULL_LDS_CAP)
    monkeypatch.setenv("GPUQ_NO_LDS_AGG", "1")
    glob = run_multi(gq, keys, kvalid, cols, FULL_SPECS, FULL_LDS_CAP)
    assert lds == glob
    assert lds == single_key_ref(tuple(FULL_SPECS))


HASH_AGG_LDS_CAP = 1024      # <= AGG_LDS_CAP (2048): k_agg_build_lds
HASH_AGG_GLOBAL_CAP = 4096   # > 2048: k_agg_build


def run_hash_agg(gq, keys, kvalid, col, cap, ops=None):
    kw = {} if ops is None else {"ops": ops}
    return gq.hash_agg(
        to_dev(keys), to_dev(col[0]), cap,
        key_validity=None if kvalid is None else pack_validity(kvalid),
        val_validity=None if col[1] is None else pack_validity(col[1]), **kw)


def test_hash_agg_lds_equals_global(gq, monkeypatch):
    keys, kvalid, cols = single_key_data()
    ref = single_key_ref((("sum", "a"), ("count", "a")))
    lds = agg_result(run_hash_agg(gq, keys, kvalid, cols["a"], HASH_AGG_LDS_CAP))
    monkeypatch.setenv("GPUQ_NO_LDS_AGG", "1")
    glob = agg_result(run_hash_agg(gq, keys, kvalid, cols["a"], HASH_AGG_LDS_CAP))
    assert lds == glob
    assert ref[(ALL_NULL_KEY,)] == [None, 0]
    assert lds == ref
    # and the capacity that selects the global kernel by itself
    assert agg_result(run_hash_agg(gq, keys, kvalid, cols["a"],
                                   HASH_AGG_GLOBAL_CAP)) == ref


# ---------- c. the 64 KB boundary ----------

BOUNDARY = {
    # 2048 * (1 + 3) * 8 = 65536: the largest LDS table, exactly 64 KB
    "lds_2048x3": (2048, [("min", "c"), ("max", "c"), ("count", "c")]),
    # 2048 * (1 + 4) * 8 = 81920: the first size on the global path
    "global_2048x4": (2048, [("sum", "a"), ("count", "a"), ("min", "d"),
                             ("count", "d")]),
    # the exec default capacity: 1024 * (1 + 7) * 8 = 65536, LDS
    "lds_1024x7": (1024, [("sum", "a"), ("count", "a"), ("sum", "b"),
                          ("count", "b"), ("max", "d"), ("count", "d"),
                          ("count*", None)]),
}


@pytest.mark.parametrize("case", sorted(BOUNDARY))
def test_lds_boundary(gq, case):
    cap, specs = BOUNDARY[case]
    lds_bytes = cap * (1 + len(specs)) * 8
    assert (lds_bytes <= 65536) == case.startswith("lds")
    assert lds_bytes == 65536 or case == "global_2048x4"
    keys, kvalid, cols = single_key_data()
    assert run_multi(gq, keys, kvalid, cols, specs, cap) == \
        single_key_ref(tuple(specs))


# ---------- d. two batches in one workspace ----------

CUT = N // 2 + 1
B1_ONLY, BOTH, B2_ONLY = (0, 49), (50, 99), (100, 149)
NULL_THEN_VALUE_KEY, B2_IMAX_KEY = 60, 120


@functools.lru_cache(maxsize=None)
def two_batch_data():
    rng = np.random.default_rng(202)
    keys = np.concatenate([
        rng.integers(-1, BOTH[1], size=CUT, endpoint=True),
        rng.integers(BOTH[0] - 1, B2_ONLY[1], size=N - CUT, endpoint=True)])
    keys[keys == BOTH[0] - 1] = -1
    keys = keys.astype(np.int64)
    kvalid = rng.random(N) >= 0.1
    cols = value_columns(rng, N)
    first = np.arange(N) < CUT

    def grp(k):
        return kvalid & (keys == k)
    plant(cols, rng, grp(ALL_NULL_KEY), grp(IMAX_KEY), grp(IMIN_KEY),
          grp(NEG_ZERO_KEY), grp(ZEROS_KEY), grp(NANS_KEY))
    plant(cols, rng, all_null=grp(NULL_THEN_VALUE_KEY) & first,
          only_i64_max=grp(B2_IMAX_KEY), only_i64_min=grp(BOTH[0] + 5),
          only_neg_zero=grp(BOTH[0] + 6))
    for name in cols:                      # non-NULL in batch 2 for certain
        cols[name][1][grp(NULL_THEN_VALUE_KEY) & ~first] = True
    return keys, kvalid, cols


@pytest.mark.parametrize("cap", FULL_CAPS)
def test_two_batches_one_workspace(gq, cap):
    keys, kvalid, cols = two_batch_data()
    ref = reference(FULL_SPECS, [keys], [kvalid], cols)
    b1 = {int(k) for k, v in zip(keys[:CUT], kvalid[:CUT]) if v}
    b2 = {int(k) for k, v in zip(keys[CUT:], kvalid[CUT:]) if v}
    assert set(range(*B1_ONLY)) <= b1 - b2 and set(range(*B2_ONLY)) <= b2 - b1
    assert set(range(*BOTH)) | {-1} <= b1 & b2
    assert not kvalid[:CUT].all() and not kvalid[CUT:].all()   # NULL keys in both
    first = reference(FULL_SPECS, [keys[:CUT]], [kvalid[:CUT]],
                      {c: [v[:CUT], ok[:CUT]] for c, (v, ok) in cols.items()})
    assert first[(NULL_THEN_VALUE_KEY,)][:10] == [None] * 6 + [0] * 4
    assert None not in ref[(NULL_THEN_VALUE_KEY,)]
    assert ref[(ALL_NULL_KEY,)][:6] == [None] * 6
    assert ref[(B2_IMAX_KEY,)][2] == I64_MAX and ref[(BOTH[0] + 5,)][3] == I64_MIN
    ws = gq.agg_multi_workspace(cap, len(FULL_SPECS))
    assert run_multi(gq, keys, kvalid, cols, FULL_SPECS, cap, 0, CUT,
                     workspace=ws, first_batch=True, finalize=False) is None
    got = run_multi(gq, keys, kvalid, cols, FULL_SPECS, cap, CUT, N,
                    workspace=ws, first_batch=False, finalize=True)
    assert got == ref


# ---------- e. non-finite and cancelling float SUMs ----------

SUM_SPECS = [("sum", "a"), ("count", "a")]
SUM_LDS_CAP = 1024       # 1024 * 3 * 8 = 24576 <= 65536; hash_agg: <= 2048
SUM_GLOBAL_CAP = 4096    # 4096 * 3 * 8 = 98304 > 65536; hash_agg: > 2048


@functools.lru_cache(maxsize=None)
def non_finite_data():
    """300 rows per group, shuffled over several blocks. Group 0: finite and
    one +inf; 1: +inf and -inf; 2: a NaN among finite; 3: only -0.0;
    4: finite only; 5: finite and -inf; NULL key: a NaN and -inf."""
    rng = np.random.default_rng(303)
    per = 300
    keys = np.repeat(np.arange(7, dtype=np.int64), per)
    kvalid = keys != 6
    v = rng.integers(-(1 << 20), 1 << 20, size=len(keys),
                     endpoint=True).astype(np.float64)
    v[0 * per + 17] = math.inf
    v[1 * per + 5], v[1 * per + 250] = math.inf, -math.inf
    v[2 * per + 99] = NANS[2]
    v[3 * per:4 * per] = NEG_ZERO
    v[5 * per + 1] = -math.inf
    v[6 * per + 3], v[6 * per + 4] = NANS[1], -math.inf
    valid = rng.random(len(keys)) >= 0.2
    valid[[17, per + 5, per + 250, 2 * per + 99, 5 * per + 1,
           6 * per + 3, 6 * per + 4]] = True
    p = rng.permutation(len(keys))
    return keys[p], kvalid[p], {"a": [v[p], valid[p]]}


@pytest.mark.parametrize("cap", [SUM_LDS_CAP, SUM_GLOBAL_CAP])
def test_non_finite_float_sums(gq, cap):
    keys, kvalid, cols = non_finite_data()
    ref = reference(SUM_SPECS, [keys], [kvalid], cols)
    assert [ref[(k,)][0] for k in (0, 1, 2, 3, 5, None)] == \
        [(math.inf, 1.0), "nan", "nan", (0.0, 1.0), (-math.inf, -1.0), "nan"]
    assert run_multi(gq, keys, kvalid, cols, SUM_SPECS, cap) == ref
    assert agg_result(run_hash_agg(gq, keys, kvalid, cols["a"], cap)) == ref


@pytest.mark.parametrize("cap", [SUM_LDS_CAP, SUM_GLOBAL_CAP])
def test_cancelling_float_sum_within_the_derived_bound(gq, cap):
    """the one tolerance in this file: (n - 1) * 2^-53 * sum|v|, the bound of
    recursive summation in any order, around the correctly rounded sum."""
    rng = np.random.default_rng(304)
    v = rng.permutation(np.array([1e16, 1.0, -1e16] * 1000))
    keys = np.full(len(v), 12, dtype=np.int64)
    exact = math.fsum(v.tolist())
    bound = agg_ref.sum_error_bound(v.tolist())
    assert exact == 1000.0
    ok, okv, accs = gq.hash_agg_multi(to_dev(keys), [("sum", to_dev(v)),
                                                     ("count*",)], cap)
    assert single_tuples(ok, okv) == [(12,)]
    assert accs[1].cpu().tolist() == [len(v)]
    got = accs[0].cpu().tolist()[0]
    assert abs(got - exact) <= bound, ("hash_agg_multi", got, exact, bound)
    res = agg_result(gq.hash_agg(to_dev(keys), to_dev(v), cap))
    assert list(res) == [(12,)] and res[(12,)][1] == len(v)
    got = res[(12,)][0][0]
    assert abs(got - exact) <= bound, ("hash_agg", got, exact, bound)


# ---------- f. grid-stride rows ----------

STRIDE_SPECS = [("sum", "a"), ("count", "a"), ("sum", "b"), ("count", "b"),
                ("min", "c"), ("max", "c"), ("count", "c"), ("count*", None)]


def test_grid_stride_rows(gq):
    """the hash kernels launch at most 2048 blocks of 256 threads; 257 rows
    more give the first 257 threads a second loop iteration. 8 specs:
    512 * 9 * 8 = 36864 <= 65536, the LDS path."""
    n, cap = 2048 * 256 + 257, 512
    rng = np.random.default_rng(404)
    keys = rng.integers(-1, 46, size=n, endpoint=True).astype(np.int64)
    kvalid = rng.random(n) >= 0.1
    cols = value_columns(rng, n)
    tail = np.arange(n) >= 2048 * 256
    keys[tail], kvalid[tail] = 47, True       # a group of second iterations only
    cols["c"][0][tail], cols["c"][1][tail] = I64_MAX, True
    ref = agg_ref.np_aggregate(keys, kvalid, ref_specs(STRIDE_SPECS, cols))
    ref = {kt: [norm(x) for x in r] for kt, r in ref.items()}
    assert len(ref) == 50 and (-1,) in ref and (None,) in ref
    assert ref[(47,)][4] == I64_MAX and ref[(47,)][7] == 257
    assert run_multi(gq, keys, kvalid, cols, STRIDE_SPECS, cap) == ref


# ---------- g. composite keys ----------

KEYS_CAP = 16384         # < 10^4 groups; gpuq_hash_agg_keys has one path
KEY_VALUES = np.array([-1, 0, 1, 2, I64_MIN, I64_MAX], dtype=np.int64)
EVERY_COLUMN = [None, -1, 0, 1, 2, I64_MIN, I64_MAX]


@functools.lru_cache(maxsize=None)
def composite_data(nkeys):
    rng = np.random.default_rng(500 + nkeys)
    kcols = [KEY_VALUES[rng.integers(0, len(KEY_VALUES), size=N)]
             for _ in range(nkeys)]
    small = 40 if nkeys == 1 else 3           # small random ints mixed in
    kcols = [np.where(rng.random(N) < 0.6, k,
                      rng.integers(-small, small, size=N, endpoint=True))
             .astype(np.int64) for k in kcols]
    kvalids = [rng.random(N) >= 0.12 for _ in range(nkeys)]
    # three rows in each half with one value, or NULL, in every key column
    for i, value in enumerate(EVERY_COLUMN):
        for row in [base + 3 * i + r for base in (0, CUT) for r in range(3)]:
            for k, kv in zip(kcols, kvalids):
                k[row], kv[row] = value or 0, value is not None
    cols = value_columns(rng, N)

    def grp(value):
        sel = np.ones(N, dtype=bool)
        for k, kv in zip(kcols, kvalids):
            sel &= kv & (k == value)
        return sel
    all_null_keys = np.ones(N, dtype=bool)
    for kv in kvalids:
        all_null_keys &= ~kv
    plant(cols, rng, all_null=grp(2), only_i64_max=grp(1), only_i64_min=grp(0),
          only_neg_zero=grp(I64_MAX), only_nans=grp(I64_MIN),
          both_zeros=all_null_keys)
    ref = reference(FULL_SPECS, kcols, kvalids, cols)
    return kcols, kvalids, cols, ref


def run_keys(gq, kcols, kvalids, cols, speclist, cap, lo=0, hi=None, **kw):
    res = gq.hash_agg_keys(
        [to_dev(k[lo:hi]) for k in kcols], dev_specs(speclist, cols, lo, hi),
        cap, key_validities=[pack_validity(v[lo:hi]) for v in kvalids], **kw)
    if res is None:
        return None
    okeys, kmask, accs = res
    okeys = [k.cpu().tolist() for k in okeys]
    tuples = [tuple(okeys[c][g] if (m >> c) & 1 else None
                    for c in range(len(kcols)))
              for g, m in enumerate(kmask.cpu().tolist())]
    return result_dict(speclist, tuples, accs)


@pytest.mark.parametrize("batches", [1, 2])
@pytest.mark.parametrize("nkeys", [1, 2, 4])
def test_composite_keys(gq, nkeys, batches):
    kcols, kvalids, cols, ref = composite_data(nkeys)
    every = lambda v: (v,) * nkeys                          # noqa: E731
    assert every(None) in ref                  # NULL in every key column at once
    assert every(-1) in ref and every(I64_MIN) in ref and every(I64_MAX) in ref
    assert ref[every(2)][:10] == [None] * 6 + [0] * 4
    assert ref[every(1)][2] == I64_MAX and ref[every(0)][3] == I64_MIN
    assert ref[every(I64_MAX)][4:6] == [(0.0, 1.0)] * 2
    assert len(ref) > (40 if nkeys == 1 else 6 ** nkeys)
    if batches == 1:
        got = run_keys(gq, kcols, kvalids, cols, FULL_SPECS, KEYS_CAP)
    else:
        ws = torch.empty(gq.lib().gpuq_hash_agg_keys_workspace_bytes(
            KEYS_CAP, nkeys, len(FULL_SPECS)), dtype=torch.uint8, device="cuda")
        assert run_keys(gq, kcols, kvalids, cols, FULL_SPECS, KEYS_CAP, 0, CUT,
                        workspace=ws, first_batch=True, finalize=False) is None
        got = run_keys(gq, kcols, kvalids, cols, FULL_SPECS, KEYS_CAP, CUT, N,
                       workspace=ws, first_batch=False, finalize=True)
    assert got == ref


# signatures: the composite table compares a 64-bit splitmix64 chain over the
# tuple before the stored keys. Restated here to build tuples that collide.
_M = (1 << 64) - 1


def _splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & _M
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M
    return x ^ (x >> 31)


def _signature(tup):
    s = 0x243F6A8885A308D3
    for c, k in enumerate(tup):
        s = _splitmix64(((s ^ (k & _M)) + c) & _M)
    return s


def _home(oracle, tup, cap):
    h = 42
    for k in tup:
        h = oracle.hash_long(k, h)
    return h & (cap - 1)


def test_composite_keys_with_equal_signatures_stay_apart(gq):
    """pairs of two-column tuples with the SAME 64-bit signature, the same
    NULL mask and the same home slot: whichever comes second walks over the
    first one's slot and must tell the tuples apart by their stored keys."""
    import oracle
    cap, pairs = 16, []
    a2 = 1000
    for a1 in range(5):
        b1 = 7 * a1 + 3
        while True:           # (a1, b1) and (a2, b2) chain to one signature
            a2 += 1
            s1 = _splitmix64(0x243F6A8885A308D3 ^ a1)
            s2 = _splitmix64(0x243F6A8885A308D3 ^ a2)
            b2 = agg_ref.wrap_i64(s1 ^ b1 ^ s2)
            if _home(oracle, (a1, b1), cap) == _home(oracle, (a2, b2), cap):
                break
        assert _signature((a1, b1)) == _signature((a2, b2)) > 1
        pairs += [(a1, b1), (a2, b2)]
    assert len(set(pairs)) == 10
    rng = np.random.default_rng(606)
    n = 4096
    pick = rng.integers(0, len(pairs), size=n)
    kcols = [np.array([pairs[i][c] for i in pick], dtype=np.int64)
             for c in range(2)]
    kvalids = [np.ones(n, dtype=bool)] * 2
    cols = value_columns(rng, n)
    specs = [("sum", "b"), ("count", "b"), ("min", "c"), ("count", "c"),
             ("count*", None)]
    ref = reference(specs, kcols, kvalids, cols)
    assert set(ref) == set(pairs)
    assert run_keys(gq, kcols, kvalids, cols, specs, cap) == ref


# ---------- h. tight tables ----------

TIGHT_CAP, TIGHT_KEYS = 16, 14       # load 14/16; 16 * 12 * 8 = 1536 B: LDS


def tight_keys(home_of):
    """14 keys, three of them at home slot cap - 1: all but the first of
    those to arrive wrap to slot 0 and on."""
    last, rest, k = [], [], 0
    while len(last) < 3 or len(rest) < TIGHT_KEYS - 3:
        (last if home_of(k) == TIGHT_CAP - 1 else rest).append(k)
        k += 1
    keys = last[:3] + rest[:TIGHT_KEYS - 3]
    assert sum(home_of(k) == TIGHT_CAP - 1 for k in keys) >= 2
    return np.array(keys, dtype=np.int64)


@pytest.mark.parametrize("path", ["lds", "global"])
def test_tight_table_multi(gq, monkeypatch, path):
    import oracle
    if path == "global":
        monkeypatch.setenv("GPUQ_NO_LDS_AGG", "1")
    rng = np.random.default_rng(707)
    distinct = tight_keys(lambda k: oracle.hash_long(k, 42) & (TIGHT_CAP - 1))
    keys = distinct[rng.integers(0, TIGHT_KEYS, size=N)]
    kvalid = rng.random(N) >= 0.05
    keys[rng.random(N) < 0.05] = -1       # the special slots take no table slot
    cols = value_columns(rng, N)
    ref = reference(FULL_SPECS, [keys], [kvalid], cols)
    assert len(ref) == TIGHT_KEYS + 2
    assert run_multi(gq, keys, kvalid, cols, FULL_SPECS, TIGHT_CAP) == ref


def test_tight_table_keys(gq):
    import oracle
    rng = np.random.default_rng(708)
    distinct = tight_keys(lambda k: _home(oracle, (k, 0), TIGHT_CAP))
    kcols = [distinct[rng.integers(0, TIGHT_KEYS, size=N)],
             np.zeros(N, dtype=np.int64)]
    kvalids = [np.ones(N, dtype=bool)] * 2
    cols = value_columns(rng, N)
    ref = reference(FULL_SPECS, kcols, kvalids, cols)
    assert len(ref) == TIGHT_KEYS
    assert run_keys(gq, kcols, kvalids, cols, FULL_SPECS, TIGHT_CAP) == ref


# ---------- i. overflow is reported ----------

def overflow_input(distinct):
    rng = np.random.default_rng(808)
    keys = rng.permutation(np.arange(N, dtype=np.int64) % distinct)
    v = rng.integers(-5, 5, size=N, endpoint=True)
    return keys, {"a": [v.astype(np.float64), np.ones(N, dtype=bool)],
                  "b": [v.astype(np.int64), np.ones(N, dtype=bool)]}


# kernel, capacity, distinct keys. A block holds 256 rows.
OVERFLOW = {
    # 64 * 3 * 8 B: LDS. ~190 distinct keys per block > 64 slots: a block's
    # own table overflows and the thread leaves before the flush barrier
    "multi_lds_block_table": ("multi", 64, 200),
    # 512 * 3 * 8 = 12288 B: LDS. <= 256 distinct keys per block fit, the
    # 2000 distinct keys of all blocks overflow the global table in the merge
    "multi_lds_merge": ("multi", 512, 2000),
    # 4096 * 3 * 8 = 98304 B: global
    "multi_global": ("multi", 4096, 6000),
    "hash_agg_lds_block_table": ("agg", 64, 200),      # 64 <= 2048: LDS
    "hash_agg_lds_merge": ("agg", 512, 2000),
    "keys": ("keys", 64, 200),
}


@pytest.mark.parametrize("case", sorted(OVERFLOW))
def test_overflow_is_reported(gq, case):
    kernel, cap, distinct = OVERFLOW[case]
    keys, cols = overflow_input(distinct)
    with pytest.raises(gq.GpuqError, match="overflow"):
        if kernel == "multi":
            run_multi(gq, keys, None, cols, SUM_SPECS, cap)
        elif kernel == "agg":
            gq.hash_agg(to_dev(keys), to_dev(cols["a"][0]), cap)
        else:
            gq.hash_agg_keys([to_dev(keys), to_dev(keys)],
                             dev_specs(SUM_SPECS, cols), cap)
    torch.cuda.synchronize()
    # the library is usable afterwards
    small = np.arange(8, dtype=np.int64)
    ok, okv, accs = gq.hash_agg_multi(to_dev(small), [("count*",)], 64)
    assert sorted(ok.cpu().tolist()) == list(range(8))


# ---------- j. the partitioned path at small shapes ----------

PART_CHUNK, PART_TILE = 16384, 262144
SUM, COUNT = 1, 2


def part_input(n, pattern, seed):
    rng = np.random.default_rng(seed)
    if pattern == "groups":
        keys = rng.integers(-1, 300, size=n, endpoint=True).astype(np.int64)
    else:
        keys = rng.permutation(np.arange(n, dtype=np.int64) * 2654435761 + 17)
        if pattern == "hot":              # one key holds ~90 % of the rows
            keys[rng.random(n) < 0.9] = 123456789
        keys[rng.random(n) < 0.02] = -1
    kvalid = rng.random(n) >= 0.1
    if n >= 2:
        keys[0], kvalid[0], kvalid[1] = -1, True, False
    vals = rng.integers(-(1 << 20), 1 << 20, size=n, endpoint=True)
    return keys, kvalid, vals.astype(np.float64)


# name -> (rows, key pattern, capacity, seed)
PART_CASES = {
    # chunk edges: one row short of, exactly, and one row past one chunk
    "chunk_minus_1": (PART_CHUNK - 1, "groups", 1024, 901),
    "chunk": (PART_CHUNK, "groups", 1024, 902),
    "chunk_plus_1": (PART_CHUNK + 1, "groups", 1024, 903),
    # one row past the scatter tile: a second scatter block with one row
    "tile_plus_1": (PART_TILE + 1, "groups", 1024, 904),
    # two chunks of ~16384 distinct keys each against the 4096-slot LDS
    # table: the mid-chunk flush runs several times in every chunk
    "all_distinct": (2 * PART_CHUNK, "distinct", 1 << 16, 905),
    "hot_key": (2 * PART_CHUNK, "hot", 1 << 16, 906),
}


@pytest.mark.parametrize("ops", [SUM | COUNT, SUM])
@pytest.mark.parametrize("case", sorted(PART_CASES))
def test_partitioned_small_shapes(gq, case, ops):
    n, pattern, cap, seed = PART_CASES[case]
    keys, kvalid, vals = part_input(n, pattern, seed)
    specs = [("sum", vals), ("count", vals)] if ops & COUNT else [("sum", vals)]
    ref = agg_ref.np_aggregate(keys, kvalid, specs)
    ref = {kt: [norm(x) for x in r] for kt, r in ref.items()}
    assert (-1,) in ref and (None,) in ref       # both special slots in play
    if pattern == "distinct":
        assert len(ref) > 0.85 * n
    if pattern == "hot":
        assert (123456789,) in ref
        assert 0.05 * n < len(ref) < 0.15 * n
    got = agg_result(gq.hash_agg_partitioned(
        to_dev(keys), to_dev(vals), cap, key_validity=pack_validity(kvalid),
        ops=ops), with_count=bool(ops & COUNT))
    assert got == ref


@pytest.mark.parametrize("ops", [SUM | COUNT, SUM])
@pytest.mark.parametrize("row", ["ordinary", "minus_one", "null"])
def test_partitioned_one_row(gq, row, ops):
    """N = 1 holds one kind of key, so each kind gets its own run."""
    keys = np.array([-1 if row == "minus_one" else 41], dtype=np.int64)
    kvalid = np.array([row != "null"])
    vals = np.array([-7.0])
    want = [(-7.0, -1.0), 1] if ops & COUNT else [(-7.0, -1.0)]
    got = agg_result(gq.hash_agg_partitioned(
        to_dev(keys), to_dev(vals), 1024, key_validity=pack_validity(kvalid),
        ops=ops), with_count=bool(ops & COUNT))
    assert got == {(None,) if row == "null" else (int(keys[0]),): want}
