"""Sort with the fused first pass: a histogram-only pre-pass, then the first
scatter pass reads the raw key column, encodes in registers and synthesises
the row ids.

Every case compares the permutation and the sorted keys bit for bit with the
CPU oracle's stable sort (NaN compares as NaN), checks that the key tensor is
unchanged, and proves which path ran from the launch counts of two profiling
tags: `sort_hist` (the histogram-only pre-pass) and `encode` (the kernel that
materialises the encoded keys and the identity row ids).

  fused:    sort_hist = 1, encode = 0
  fused, every encoded key equal (no pass runs, so the pairs are materialised
            for the zero-pass tail): sort_hist = 1, encode = 1
  unfused:  sort_hist = 0, encode = 1

Not covered: the lookback-timeout redo, which cannot be reached on purpose
(it materialises with `encode` before its hist+scan passes; read the code).
"""
import numpy as np
import pytest

import oracle

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SIGN = np.uint64(1 << 63)
TILE = 5632           # rows per scatter block at the default 256 x 22 geometry
SIZES = [1, 2, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 17, 65536]

FUSED, FUSED_MATERIALISED, UNFUSED = (0, 1), (1, 1), (1, 0)   # (encode, sort_hist)


@pytest.fixture(scope="module")
def gq():
    from spark_amd import gpuq
    assert torch.cuda.is_available()
    return gpuq


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def encode(keys):
    """Order-preserving u64 encoding of the ascending sort."""
    if keys.dtype == np.float64:
        k = keys.copy()
        k[k == 0.0] = 0.0                       # -0.0 -> 0.0
        b = k.view(np.uint64).copy()
        b[np.isnan(k)] = np.uint64(0x7ff8000000000000)
        neg = (b >> np.uint64(63)).astype(bool)
        return b ^ np.where(neg, np.uint64(0xFFFFFFFFFFFFFFFF), SIGN)
    return keys.view(np.uint64) ^ SIGN


def sort_counted(gq, dev, **kw):
    """Sort `dev` with profiling on; returns (perm, keys, plan, (encode
    launches, sort_hist launches)) as host values."""
    gq.profiling(True)
    try:
        gq.kernel_stats_reset()
        perm, skeys = gq.sort_perm(dev, **kw)
        plan = gq.sort_last_plan()
        counts = (gq.kernel_stats("encode")[1], gq.kernel_stats("sort_hist")[1])
    finally:
        gq.profiling(False)
        gq.kernel_stats_reset()
    return perm.cpu().numpy().astype(np.uint32), skeys.cpu().numpy(), plan, counts


def check(gq, keys, path, desc=False, valid=None, dev=None):
    """`dev` is the device tensor holding `keys` (made here if not given)."""
    if dev is None:
        dev = torch.from_numpy(np.ascontiguousarray(keys)).cuda()
    kw, okw = {}, {}
    if valid is not None:
        packed = np.packbits(valid, bitorder="little")
        kw["key_validity"] = torch.from_numpy(packed).cuda()
        okw["validity"] = packed
    perm, got, plan, counts = sort_counted(gq, dev, desc=desc, **kw)
    assert (bits(dev.cpu().numpy()) == bits(keys)).all(), "key column was written"
    exp = oracle.sort_perm(keys, desc=desc, **okw)
    assert (perm == exp.astype(np.uint32)).all()
    want = keys[exp]
    if keys.dtype == np.float64:
        # the engine emits the canonical NaN and +0.0
        assert ((got == want) | (np.isnan(got) & np.isnan(want))).all()
    else:
        assert (got == want).all()
    assert counts == path, f"(encode, sort_hist) launches {counts}, expected {path}"
    return plan, perm, got


def fused_path(keys):
    enc = encode(keys)
    return FUSED_MATERIALISED if (enc == enc[0]).all() else FUSED


def f64_keys(n, seed):
    """Normals with the special values in the first 100 rows: +-0.0, NaNs
    (canonical, and a negative one with a payload), +-inf, denormals."""
    keys = np.random.default_rng(seed).standard_normal(n)
    special = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 5e-324, -5e-324,
                        1e-310, -1e-310, 0.0], dtype=np.float64)
    special[9] = np.array([0xfff0000000000123], dtype=np.uint64).view(np.float64)[0]
    m = min(n, 100)
    keys[:m] = np.tile(special, 10)[:m]
    return keys


# ---------- fused path ----------

@pytest.mark.parametrize("desc", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_fused_i64(gq, n, desc):
    # full-range keys: the prefix plan from 3 tiles up, the classic one below
    keys = oracle.gen_i64(seed=3000 + n, n=n)
    plan, _, _ = check(gq, keys, fused_path(keys), desc=desc)
    if n >= 3 * TILE + 17:
        assert plan[1] >= 2 and plan[2] == 0


@pytest.mark.parametrize("desc", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_fused_f64(gq, n, desc):
    # n = 1 is one key and n = 2 is (0.0, -0.0): every encoded key equal
    keys = f64_keys(n, seed=n)
    check(gq, keys, fused_path(keys), desc=desc)


def test_fused_f64_every_bit_pattern(gq):
    # all 8 bytes active: the prefix plan, and NaNs of every payload
    n = 65536
    keys = oracle.gen_i64(seed=78, n=n).view(np.float64).copy()
    keys[:100] = f64_keys(100, seed=0)
    plan, _, _ = check(gq, keys, FUSED)
    assert plan[1] >= 2 and plan[2] == 0


@pytest.mark.parametrize("desc", [False, True])
def test_classic_several_passes(gq, desc):
    keys = oracle.gen_i64(seed=41, n=65536, range_=1 << 20)
    plan, _, _ = check(gq, keys, FUSED, desc=desc)
    assert plan == (0, 0, 0)


@pytest.mark.parametrize("desc", [False, True])
@pytest.mark.parametrize("dtype", [np.int64, np.float64])
@pytest.mark.parametrize("n", [65, TILE + 1, 65536])
def test_classic_one_active_byte(gq, n, dtype, desc):
    # the first pass is also the final pass: it reads the raw column and
    # writes the permutation and the decoded keys
    keys = oracle.gen_i64(seed=42, n=n, range_=200)
    if dtype == np.float64:
        # 1.0 + k * 2^-52: only the lowest mantissa byte varies
        keys = (np.float64(1.0).view(np.uint64) + keys.view(np.uint64)).view(np.float64)
    enc = encode(keys)
    changed = int(np.bitwise_and.reduce(enc)) ^ int(np.bitwise_or.reduce(enc))
    assert 0 < changed < 256
    plan, _, _ = check(gq, keys, FUSED, desc=desc)
    assert plan == (0, 0, 0)


@pytest.mark.parametrize("n", [1, TILE + 1])
def test_all_keys_equal(gq, n):
    keys = np.full(n, -7, dtype=np.int64)
    _, perm, got = check(gq, keys, FUSED_MATERIALISED)
    assert (perm == np.arange(n, dtype=np.uint32)).all()
    assert (got == -7).all()


@pytest.mark.parametrize("n", [TILE + 1, 3 * TILE + 17])
def test_sliced_key_tensor(gq, n):
    # the key column starts 24 bytes into its allocation
    keys = oracle.gen_i64(seed=5, n=n + 3)
    dev = torch.from_numpy(keys).cuda()
    check(gq, keys[3:], FUSED, dev=dev[3:])
    assert (dev.cpu().numpy() == keys).all()


def fallback_keys(n=65536, seed=13):
    # the construction of tests/test_gpu_sort_prefix.py: every window byte
    # looks uniform to the gate, yet there are only 256 window values
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 256, n).astype(np.uint64)
    low = rng.integers(0, 1 << 32, n).astype(np.uint64)
    return (v * np.uint64(0x0101010100000000) + low).view(np.int64)


def test_tiefix_overflow_redo_reads_raw_column(gq):
    plan, _, _ = check(gq, fallback_keys(), FUSED)    # the redo did not materialise
    assert plan[1] >= 2 and plan[2] == 1


# ---------- unfused paths ----------

def test_nulls_stay_unfused(gq):
    n = 3 * TILE + 17
    keys = oracle.gen_i64(seed=6, n=n)
    valid = np.random.default_rng(6).random(n) >= 0.10
    check(gq, keys, UNFUSED, valid=valid)


def test_hist_scan_stays_unfused(gq, monkeypatch):
    monkeypatch.setenv("GPUQ_NO_ONESWEEP", "1")
    keys = oracle.gen_i64(seed=7, n=3 * TILE + 17)
    check(gq, keys, UNFUSED)


def test_aliased_out_keys_stays_unfused(gq):
    # sorting the keys in place: the column is an output, so it is
    # materialised before any pass
    keys = oracle.gen_i64(seed=8, n=TILE + 1, range_=200)
    dev = torch.from_numpy(keys).cuda()
    gq.profiling(True)
    try:
        gq.kernel_stats_reset()
        perm, skeys = gq.sort_perm(dev, out_keys=dev)
        counts = (gq.kernel_stats("encode")[1], gq.kernel_stats("sort_hist")[1])
    finally:
        gq.profiling(False)
        gq.kernel_stats_reset()
    exp = oracle.sort_perm(keys)
    assert (perm.cpu().numpy().astype(np.uint32) == exp.astype(np.uint32)).all()
    assert (skeys.cpu().numpy() == keys[exp]).all()
    assert counts == UNFUSED


@pytest.mark.parametrize("n", [65536, 1 << 20])
def test_kill_switch(gq, monkeypatch, n):
    keys = oracle.gen_i64(seed=9000 + n, n=n)
    _, perm0, keys0 = check(gq, keys, FUSED)
    monkeypatch.setenv("GPUQ_SORT_NO_FUSED_ENCODE", "1")
    _, perm1, keys1 = check(gq, keys, UNFUSED)
    assert (perm0 == perm1).all() and (keys0 == keys1).all()
