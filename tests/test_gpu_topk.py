"""Top-K by radix select: gpuq.topk_candidates / topk_perm and the
TakeOrderedAndProject / Limit exec nodes.

The reference is always the CPU oracle's stable sort: topk_perm must equal
oracle.sort_perm(...)[:k] bit for bit (permutation and keys), the candidate
set and its counts are recomputed here with numpy from that permutation, and
the exec nodes must equal GpuSortExec + head on the same batch, every column
and every bitmap.
"""
import ctypes
import time

import numpy as np
import pytest

import oracle

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SIGN = np.uint64(1 << 63)


@pytest.fixture(scope="module")
def gq():
    from spark_amd import gpuq
    assert torch.cuda.is_available()
    return gpuq


@pytest.fixture(scope="module")
def gx():
    from spark_amd import exec as gx_
    return gx_


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def pack(valid):
    return np.packbits(valid, bitorder="little")


def encode(keys):
    """ascending sort encoding: equal codes <=> equal in sort order."""
    if keys.dtype == np.float64:
        k = keys.copy()
        k[k == 0.0] = 0.0                       # -0.0 -> 0.0
        bits = k.view(np.uint64).copy()
        bits[np.isnan(k)] = np.uint64(0x7ff8000000000000)
        neg = (bits >> np.uint64(63)).astype(bool)
        return bits ^ np.where(neg, np.uint64(0xFFFFFFFFFFFFFFFF), SIGN)
    return keys.view(np.uint64) ^ SIGN


def oracle_perm(keys, desc, nulls_first, valid):
    return oracle.sort_perm(keys, desc=desc, nulls_first=nulls_first,
                            validity=None if valid is None else pack(valid))


def same_keys(got, want):
    if want.dtype == np.float64:
        # without a bitmap the engine emits the canonical NaN and +0.0
        return bool(((got == want) | (np.isnan(got) & np.isnan(want))).all())
    return bool((got == want).all())


def check_perm(gq, keys, ks, desc=False, nulls_first=None, valid=None, dk=None):
    """topk_perm against the oracle head for every k in ks."""
    exp = oracle_perm(keys, desc, nulls_first, valid)
    dk = to_dev(keys) if dk is None else dk
    dv = None if valid is None else to_dev(pack(valid))
    n = len(keys)
    for k in ks:
        perm, skeys = gq.topk_perm(dk, k, desc=desc, nulls_first=nulls_first,
                                   key_validity=dv)
        kk = max(min(k, n), 0)
        assert perm.numel() == kk and skeys.numel() == kk, (n, k)
        got = perm.cpu().numpy().astype(np.uint32)
        assert (got == exp[:kk].astype(np.uint32)).all(), (n, k, desc, nulls_first)
        assert same_keys(skeys.cpu().numpy(), keys[exp[:kk]]), (n, k)
    return exp


def ks_for(n):
    ks = {1, 2, 63, 64, 65, n // 10, n // 3, n // 2, (2 * n) // 3,
          n - 1, n, n + 1, 10 * n}
    return sorted(k for k in ks if k >= 1)


# ---------- sizes ----------

EMIT_TILE = 2048      # gpuq.TOPK_EMIT_TILE, rows per emit block
SIZES = [1, 7, 8, 9, 63, 64, 65, 255, 256, 257,
         EMIT_TILE - 1, EMIT_TILE, EMIT_TILE + 1,
         2048 * 256 + 1]                      # the first size that grid-strides


@pytest.mark.parametrize("n", SIZES)
def test_sizes(gq, n):
    assert gq.TOPK_EMIT_TILE == EMIT_TILE
    keys = oracle.gen_i64(seed=300 + n, n=n)
    ks = sorted({k for k in (1, 2, 63, 64, 65, n - 1, n, n + 1, 10 * n) if k >= 1})
    check_perm(gq, keys, ks)


@pytest.mark.parametrize("n", [7, 65, EMIT_TILE + 1])
def test_sizes_with_nulls_desc(gq, n):
    keys = oracle.gen_i64(seed=400 + n, n=n, range_=50)
    valid = np.random.default_rng(n).random(n) >= 0.3
    check_perm(gq, keys, ks_for(n), desc=True, nulls_first=True, valid=valid)


def test_empty(gq):
    dk = to_dev(oracle.gen_i64(seed=1, n=100))
    for k in (0, -3):
        perm, skeys = gq.topk_perm(dk, k)
        assert perm.numel() == 0 and skeys.numel() == 0
        rids, nb, nt = gq.topk_candidates(dk, k, keep_ties=True)
        assert rids.numel() == 0 and (nb, nt) == (0, 0)
    empty = torch.empty(0, dtype=torch.int64, device="cuda")
    perm, skeys = gq.topk_perm(empty, 5)
    assert perm.numel() == 0 and skeys.numel() == 0
    assert skeys.dtype == torch.int64
    rids, nb, nt = gq.topk_candidates(empty, 5)
    assert rids.numel() == 0 and (nb, nt) == (0, 0)


# ---------- key shapes ----------

N_SHAPE = 5003        # three emit blocks, no multiple of 8 or 64


def shape_keys(name, n=N_SHAPE):
    rng = np.random.default_rng(13)
    if name == "full":                # all eight bytes active
        return oracle.gen_i64(seed=11, n=n)
    if name == "range1000":            # two bytes active
        return oracle.gen_i64(seed=12, n=n, range_=1000)
    if name == "low_byte":
        return (np.int64(0x1234567800) << 8) | rng.integers(0, 256, n).astype(np.int64)
    if name == "top_byte":
        top = rng.integers(0, 256, n).astype(np.uint64) << np.uint64(56)
        return (top | np.uint64(0x00ABCDEF01234567)).view(np.int64)
    if name == "all_equal":            # bits_changed == 0
        return np.full(n, -77, dtype=np.int64)
    if name == "two_values":           # 30% / 70%: cuts fall in the larger group
        return np.where(rng.random(n) < 0.3, np.int64(-5), np.int64(1 << 40))
    raise KeyError(name)


SHAPES = ["full", "range1000", "low_byte", "top_byte", "all_equal", "two_values"]


@pytest.mark.parametrize("desc", [False, True])
@pytest.mark.parametrize("name", SHAPES)
def test_shapes(gq, name, desc):
    keys = shape_keys(name)
    n = len(keys)
    exp = check_perm(gq, keys, ks_for(n), desc=desc)
    if name == "all_equal":            # T is the whole input: the first k rows
        assert (exp[:100] == np.arange(100)).all()


@pytest.mark.parametrize("nulls_first", [False, True])
@pytest.mark.parametrize("desc", [False, True])
@pytest.mark.parametrize("name", SHAPES)
def test_shapes_with_nulls(gq, name, desc, nulls_first):
    keys = shape_keys(name)
    n = len(keys)
    valid = np.random.default_rng(7).random(n) >= 0.2
    check_perm(gq, keys, ks_for(n), desc=desc, nulls_first=nulls_first, valid=valid)


def f64_specials(n=301):
    rng = np.random.default_rng(3)
    keys = rng.standard_normal(n)
    nan_bits = np.array([0x7ff8000000000000, 0x7ff8000000000001,
                         0xfff8000000000000, 0x7ff0000000000001,
                         0xffffffffffffffff], dtype=np.uint64).view(np.float64)
    keys[0:40] = np.tile([0.0, -0.0], 20)
    keys[40:80] = np.tile(nan_bits, 8)
    keys[80:100] = np.inf
    keys[100:120] = -np.inf
    return keys[rng.permutation(n)].copy()


@pytest.mark.parametrize("nulls_first", [False, True])
@pytest.mark.parametrize("desc", [False, True])
def test_f64_tie_groups_every_cut(gq, desc, nulls_first):
    """-0.0/0.0, five NaN payloads and both infinities as tie groups; every k
    from 1 to n + 1, so the cut falls at each position of each group."""
    keys = f64_specials()
    n = len(keys)
    check_perm(gq, keys, range(1, n + 2), desc=desc, nulls_first=nulls_first)
    valid = np.random.default_rng(4).random(n) >= 0.15
    check_perm(gq, keys, range(1, n + 2, 3), desc=desc, nulls_first=nulls_first,
               valid=valid)


def test_f64_unit_range(gq):
    n = 20011
    keys = oracle.gen_f64_unit(seed=21, n=n)
    check_perm(gq, keys, ks_for(n))
    check_perm(gq, keys, ks_for(n), desc=True)


# ---------- NULL counts around k ----------

@pytest.mark.parametrize("desc", [False, True])
@pytest.mark.parametrize("nulls_first", [False, True])
def test_null_count_around_k(gq, desc, nulls_first):
    """nulls first: nnull below, equal to and above k; nulls last: nvalid
    below, equal to and above k. n is no multiple of 8."""
    n = 1003
    keys = oracle.gen_i64(seed=31, n=n, range_=40)
    valid = np.ones(n, dtype=bool)
    valid[np.random.default_rng(5).choice(n, 100, replace=False)] = False
    edge = 100 if nulls_first else n - 100      # size of the group that sorts first
    ks = [1, edge - 1, edge, edge + 1, edge + 7, n]
    check_perm(gq, keys, ks, desc=desc, nulls_first=nulls_first, valid=valid)


@pytest.mark.parametrize("nulls_first", [False, True])
def test_all_null(gq, nulls_first):
    n = 301
    keys = oracle.gen_i64(seed=32, n=n)
    valid = np.zeros(n, dtype=bool)
    check_perm(gq, keys, [1, 8, 300, 301, 400], nulls_first=nulls_first, valid=valid)
    rids, nb, nt = gq.topk_candidates(to_dev(keys), 8, nulls_first=nulls_first,
                                      key_validity=to_dev(pack(valid)))
    assert (nb, nt) == (0, n)
    assert (rids.cpu().numpy() == np.arange(8)).all()


# ---------- select paths ----------

def path_counts(gq, dk, k):
    """(topk_hist launches, topk_collect launches) of one topk_candidates."""
    gq.profiling(True)
    try:
        gq.kernel_stats_reset()
        gq.topk_candidates(dk, k)
        torch.cuda.synchronize()
        return gq.kernel_stats("topk_hist")[1], gq.kernel_stats("topk_collect")[1]
    finally:
        gq.profiling(False)
        gq.kernel_stats_reset()


def skewed_keys(shared_bytes, n, seed):
    """60% of the rows share their top `shared_bytes` bytes (random below),
    the rest are full-range."""
    rng = np.random.default_rng(seed)
    keys = oracle.gen_i64(seed=seed, n=n).view(np.uint64).copy()
    big = rng.random(n) < 0.6
    low_bits = np.uint64(8 * (8 - shared_bytes))
    low = keys & ((np.uint64(1) << low_bits) - np.uint64(1))
    head = (np.uint64(0x5A5A5A5A5A5A5A5A) >> low_bits) << low_bits
    keys[big] = head | low[big]
    return keys.view(np.int64), big


def test_path_all_levels_on_column(gq):
    """More than half the rows share the top seven bytes and the cut falls in
    that bucket: every level's bucket exceeds TOPK_COMPACT_MAX, so all eight
    levels stream the column and nothing is collected."""
    n = 2 * gq.TOPK_COMPACT_MAX + 5
    keys, big = skewed_keys(7, n, seed=41)
    exp = oracle_perm(keys, False, None, None)
    pos = np.flatnonzero(big[exp])              # sorted positions of the bucket
    assert len(pos) > gq.TOPK_COMPACT_MAX
    k = int(pos[len(pos) // 2]) + 1
    dk = to_dev(keys)
    assert path_counts(gq, dk, k) == (8, 0)
    perm, skeys = gq.topk_perm(dk, k)
    assert (perm.cpu().numpy().astype(np.uint32) == exp[:k].astype(np.uint32)).all()
    assert (skeys.cpu().numpy() == keys[exp[:k]]).all()


def test_path_compaction_after_some_level(gq):
    """The same size with three shared bytes: after bytes 7, 6, 5 the bucket
    is still the whole big group, so byte 4 streams the column too; its
    bucket (~1/256 of the group) is collected while byte 3 is counted, and
    bytes 2..0 read the collected keys."""
    n = 2 * gq.TOPK_COMPACT_MAX + 5
    keys, big = skewed_keys(3, n, seed=42)
    exp = oracle_perm(keys, False, None, None)
    pos = np.flatnonzero(big[exp])
    k = int(pos[len(pos) // 2]) + 1
    dk = to_dev(keys)
    assert path_counts(gq, dk, k) == (4 + 3, 1)
    perm, _ = gq.topk_perm(dk, k)
    assert (perm.cpu().numpy().astype(np.uint32) == exp[:k].astype(np.uint32)).all()
    # first-level bucket already small: collected right after level 0
    assert path_counts(gq, dk, 10) == (1 + 6, 1)
    perm, _ = gq.topk_perm(dk, 10)
    assert (perm.cpu().numpy().astype(np.uint32) == exp[:10].astype(np.uint32)).all()


# ---------- topk_candidates directly ----------

def expected_candidates(keys, valid, exp, k, keep_ties):
    """(sorted row ids, n_before, n_tie) from the oracle permutation."""
    n = len(keys)
    kk = min(k, n)
    code = encode(keys)
    isnull = np.zeros(n, dtype=bool) if valid is None else ~valid
    code = np.where(isnull, np.uint64(0), code)
    pivot = exp[kk - 1]
    in_t = (code == code[pivot]) & (isnull == isnull[pivot])
    t_sorted = in_t[exp]                       # contiguous in the sorted order
    n_before = int(np.argmax(t_sorted))
    n_tie = int(in_t.sum())
    assert t_sorted[n_before:n_before + n_tie].all()
    before = exp[:n_before]
    t_rows = np.flatnonzero(in_t)              # input order
    take = t_rows if keep_ties else t_rows[:kk - n_before]
    return np.sort(np.concatenate([before, take])), n_before, n_tie


@pytest.mark.parametrize("keep_ties", [False, True])
@pytest.mark.parametrize("desc", [False, True])
def test_candidates(gq, desc, keep_ties):
    cases = [
        (oracle.gen_i64(seed=51, n=N_SHAPE, range_=30), None),
        (oracle.gen_i64(seed=52, n=N_SHAPE, range_=30),
         np.random.default_rng(52).random(N_SHAPE) >= 0.25),
        (oracle.gen_i64(seed=53, n=N_SHAPE), None),
        (f64_specials(), None),
        (f64_specials(), np.random.default_rng(54).random(301) >= 0.25),
    ]
    for keys, valid in cases:
        n = len(keys)
        dk = to_dev(keys)
        dv = None if valid is None else to_dev(pack(valid))
        for nulls_first in (False, True):
            exp = oracle_perm(keys, desc, nulls_first, valid)
            for k in (1, 2, 64, n // 3, n // 2, n - 1, n, n + 9):
                rids, nb, nt = gq.topk_candidates(
                    dk, k, desc=desc, nulls_first=nulls_first, key_validity=dv,
                    keep_ties=keep_ties)
                want, wb, wt = expected_candidates(keys, valid, exp, k, keep_ties)
                got = rids.cpu().numpy().astype(np.uint32).astype(np.int64)
                assert (nb, nt) == (wb, wt), (n, k, nulls_first)
                assert (np.diff(got) > 0).all(), "rids strictly ascending"
                assert len(got) == len(want) and (got == want).all(), (n, k)
                if not keep_ties:
                    assert len(got) == min(k, n)


def raw_candidates(gq, dk, k, keep_ties, cap, ws=None, fill=-1):
    n = dk.numel()
    ws = gq.topk_workspace(n) if ws is None else ws
    rids = torch.full((max(cap, 1),), fill, dtype=torch.int32, device="cuda")
    counts = (ctypes.c_int64 * 3)(-9, -9, -9)
    rc = gq.lib().gpuq_topk_candidates(
        torch.cuda.current_stream().cuda_stream, n, gq._col(dk), 0, 1, k,
        int(keep_ties), rids.data_ptr(), cap, counts, ws.data_ptr(), ws.numel())
    torch.cuda.synchronize()
    return rc, list(counts), rids


@pytest.mark.parametrize("keep_ties", [False, True])
def test_overflow_leaves_output_untouched(gq, keep_ties):
    keys = oracle.gen_i64(seed=61, n=N_SHAPE, range_=10)
    dk = to_dev(keys)
    k = 100
    rids, nb, nt = gq.topk_candidates(dk, k, keep_ties=keep_ties)
    n_cand = rids.numel()
    assert n_cand == (nb + nt if keep_ties else k)
    rc, counts, out = raw_candidates(gq, dk, k, keep_ties, n_cand - 1)
    assert rc == 3                                  # GPUQ_ERR_OVERFLOW
    assert counts == [n_cand, nb, nt]
    assert (out.cpu().numpy() == -1).all(), "poisoned out_rids stays untouched"
    rc, counts, out = raw_candidates(gq, dk, k, keep_ties, n_cand)
    assert rc == 0 and counts == [n_cand, nb, nt]
    assert (out.cpu().numpy() == rids.cpu().numpy()).all()


def test_keep_ties_retries_at_reported_size(gq):
    # 3000 rows tie at the cut: more than the first guess max(2k, 1024)
    keys = np.concatenate([np.zeros(3000, dtype=np.int64),
                           np.arange(1, 501, dtype=np.int64)])
    rids, nb, nt = gq.topk_candidates(to_dev(keys), 5, keep_ties=True)
    assert (nb, nt) == (0, 3000)
    assert (rids.cpu().numpy() == np.arange(3000)).all()


def test_invalid_arguments(gq):
    dk = to_dev(oracle.gen_i64(seed=62, n=100))
    rc, counts, _ = raw_candidates(gq, dk, 5, False, 5,
                                   ws=torch.empty(64, dtype=torch.uint8, device="cuda"))
    assert rc == 2 and counts == [0, 0, 0]          # short workspace
    d32 = torch.zeros(100, dtype=torch.int32, device="cuda")
    rc, counts, _ = raw_candidates(gq, d32, 5, False, 5)
    assert rc == 2 and counts == [0, 0, 0]          # unsupported dtype
    rc, counts, out = raw_candidates(gq, dk, 0, False, 5)
    assert rc == 0 and counts == [0, 0, 0]
    assert (out.cpu().numpy() == -1).all()
    assert gq.lib().gpuq_topk_workspace_bytes(1 << 32) > 0   # pure arithmetic


# ---------- seeded random loop ----------

def test_random_loop(gq):
    rng = np.random.default_rng(2024)
    t0 = time.monotonic()
    done = 0
    for it in range(200):
        if time.monotonic() - t0 > 10.0:
            break
        n = int(rng.integers(1, 50_001))
        if rng.random() < 0.5:
            range_ = int(rng.choice([0, 2, 300, 70_000, 1 << 33]))
            keys = oracle.gen_i64(seed=1000 + it, n=n, range_=range_)
            if rng.random() < 0.3:
                keys = keys - np.int64(range_ // 2)        # both signs
        else:
            keys = oracle.gen_f64_unit(seed=1000 + it, n=n)
            mode = rng.integers(0, 3)
            if mode == 1:
                keys = np.round(keys * 50) - 25             # heavy ties, both signs
            elif mode == 2:
                keys = (keys - 0.5) * 1e300
        density = float(rng.choice([0.0, 0.0, 0.01, 0.5, 0.99]))
        valid = None if density == 0.0 else rng.random(n) >= density
        k = int(rng.choice([1, int(rng.integers(1, n + 1)), n, n + 3,
                            max(1, n // 100)]))
        check_perm(gq, keys, [k], desc=bool(rng.integers(0, 2)),
                   nulls_first=bool(rng.integers(0, 2)), valid=valid)
        done += 1
    assert done >= 20, f"only {done} iterations in 10 s"


# ---------- exec nodes ----------

ROWS = 1003


def make_columns(rows=ROWS, seed=71):
    """revenue has ~12 distinct values (heavy ties at any cut) and a few
    NULLs; date breaks the ties; orderkey / prio are nullable payload."""
    rng = np.random.default_rng(seed)
    cols = {
        "orderkey": np.arange(rows, dtype=np.int64) * 3 + 1,
        "revenue": rng.integers(0, 12, rows).astype(np.float64) * 1.5,
        "date": rng.integers(0, 40, rows).astype(np.int64),
        "prio": rng.standard_normal(rows),
    }
    valid = {
        "orderkey": rng.random(rows) >= 0.1,
        "revenue": rng.random(rows) >= 0.05,
        "prio": rng.random(rows) >= 0.3,
    }
    return cols, valid


def make_batch(gx, cols, valid, lo=0, hi=None):
    hi = len(next(iter(cols.values()))) if hi is None else hi
    return gx.ColumnarBatch(
        {n_: to_dev(c[lo:hi]) for n_, c in cols.items()},
        validity={n_: to_dev(pack(v[lo:hi])) for n_, v in valid.items()})


def batch_to_host(gq, batch, names):
    """{name: (int64 bit view of the data, bool validity)}"""
    rows = batch.num_rows()
    out = {}
    for n_ in names:
        data = batch.column(n_).cpu().numpy()
        v = batch.validity(n_)
        if v is None or rows == 0:
            vb = np.ones(rows, dtype=bool)
        else:
            assert v.numel() == (rows + 7) // 8
            vb = gq.bits_to_u8(v, rows).cpu().numpy().astype(bool)
            # a clean bitmap: no stray bits past the last row
            assert (v.cpu().numpy() == pack(vb)).all()
        out[n_] = (data.view(np.int64), vb)
    return out


def orders_of(gx):
    return [gx.SortOrder("revenue", descending=True), gx.SortOrder("date")]


@pytest.fixture(scope="module")
def sorted_ref(gq, gx):
    """GpuSortExec over the whole batch, computed once."""
    cols, valid = make_columns()
    plan = gx.GpuSortExec(orders_of(gx), False,
                          gx.InputBatches([make_batch(gx, cols, valid)]))
    (out,) = list(plan.execute_columnar())
    return batch_to_host(gq, out, list(cols))


def assert_head(got, ref, names, keep):
    for n_ in names:
        data, vb = got[n_]
        assert len(data) == keep
        assert (vb == ref[n_][1][:keep]).all(), n_
        assert (data == ref[n_][0][:keep]).all(), n_


PROJECT = ["orderkey", "revenue", "prio"]
SPLITS = [(0, 333), (333, 334 + 333 + 5), (334 + 333 + 5, ROWS)]   # 333 / 339 / 331 rows


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("limit", [1, 10, ROWS, ROWS + 5, 0])
def test_take_ordered_and_project(gq, gx, sorted_ref, limit, split):
    cols, valid = make_columns()
    parts = SPLITS if split else [(0, ROWS)]
    assert all((hi - lo) % 8 for lo, hi in parts)
    child = gx.InputBatches([make_batch(gx, cols, valid, lo, hi) for lo, hi in parts])
    plan = gx.GpuColumnarRule().pre_columnar_transitions(
        gx.TakeOrderedAndProjectExec(limit, orders_of(gx), PROJECT, child))
    (out,) = list(plan.execute_columnar())
    assert list(out.columns()) == PROJECT
    keep = min(limit, ROWS)
    assert out.num_rows() == keep
    assert_head(batch_to_host(gq, out, PROJECT), sorted_ref, PROJECT, keep)


def emit_launches(gq, plan):
    gq.profiling(True)
    try:
        gq.kernel_stats_reset()
        outs = list(plan.execute_columnar())
        torch.cuda.synchronize()
        return outs, gq.kernel_stats("topk_emit")[1]
    finally:
        gq.profiling(False)
        gq.kernel_stats_reset()


def test_take_ordered_routing(gq, gx, sorted_ref):
    """limit above rows * TOPK_SORT_FRACTION sorts the batch whole; at or
    below it the select runs. Same rows either way."""
    cols, valid = make_columns()
    names = list(cols)
    cut = int(ROWS * gx.TOPK_SORT_FRACTION)
    for limit, selects in ((cut, 1), (cut + 1, 0), (ROWS // 2, 0)):
        plan = gx.GpuTakeOrderedAndProjectExec(
            limit, orders_of(gx), None, gx.InputBatches([make_batch(gx, cols, valid)]))
        (out,), launches = emit_launches(gq, plan)
        assert launches == selects, limit
        assert_head(batch_to_host(gq, out, names), sorted_ref, names, limit)


def test_take_ordered_single_key(gq, gx):
    cols, valid = make_columns()
    names = list(cols)
    order = gx.SortOrder("revenue")
    (ref,) = list(gx.GpuSortExec(order, False, gx.InputBatches(
        [make_batch(gx, cols, valid)])).execute_columnar())
    ref = batch_to_host(gq, ref, names)
    child = gx.InputBatches([make_batch(gx, cols, valid, lo, hi) for lo, hi in SPLITS])
    (out,) = list(gx.GpuTakeOrderedAndProjectExec(
        17, order, None, child).execute_columnar())
    assert_head(batch_to_host(gq, out, names), ref, names, 17)


def host_rows(cols, valid, names):
    rows = len(next(iter(cols.values())))
    return {n_: (cols[n_].view(np.int64),
                 valid.get(n_, np.ones(rows, dtype=bool))) for n_ in names}


@pytest.mark.parametrize("limit,offset", [(400, 300), (5, 0), (50, 990), (0, 3),
                                          (2000, 0), (10, 5000)])
def test_global_limit_offset_across_batches(gq, gx, limit, offset):
    """offset 300 / limit 400 starts inside the first batch (333 rows) and
    ends inside the third; the cuts are not byte-aligned."""
    cols, valid = make_columns()
    names = list(cols)
    child = gx.InputBatches([make_batch(gx, cols, valid, lo, hi) for lo, hi in SPLITS])
    plan = gx.GpuColumnarRule().pre_columnar_transitions(
        gx.GlobalLimitExec(limit, child, offset=offset))
    outs = list(plan.execute_columnar())
    assert outs
    want = host_rows(cols, valid, names)
    lo, hi = min(offset, ROWS), min(offset + limit, ROWS)
    got = [batch_to_host(gq, b, names) for b in outs]
    assert sum(b.num_rows() for b in outs) == hi - lo
    for n_ in names:
        data = np.concatenate([g[n_][0] for g in got])
        vb = np.concatenate([g[n_][1] for g in got])
        assert (data == want[n_][0][lo:hi]).all(), n_
        assert (vb == want[n_][1][lo:hi]).all(), n_


def test_local_limit_stops_pulling(gq, gx):
    cols, valid = make_columns()
    names = list(cols)
    pulled = []

    class Child(gx.SparkPlan):
        output = names
        supports_columnar = True

        def execute_columnar(self):
            for i, (lo, hi) in enumerate(SPLITS):
                # 400 rows end inside the second batch: the third is never asked for
                assert i < 2, "pulled past the batch that completes the limit"
                pulled.append(i)
                yield make_batch(gx, cols, valid, lo, hi)

    plan = gx.GpuColumnarRule().pre_columnar_transitions(
        gx.LocalLimitExec(400, Child()))
    outs = list(plan.execute_columnar())
    assert pulled == [0, 1]
    assert [b.num_rows() for b in outs] == [333, 67]
    want = host_rows(cols, valid, names)
    got = [batch_to_host(gq, b, names) for b in outs]
    for n_ in names:
        assert (np.concatenate([g[n_][0] for g in got]) == want[n_][0][:400]).all()
        assert (np.concatenate([g[n_][1] for g in got]) == want[n_][1][:400]).all()
