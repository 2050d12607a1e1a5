"""Prefix-plan sort: radix only the leading key bytes, fix ties in one pass.

Every case compares the permutation and the sorted keys bit for bit with the
CPU oracle's stable sort and asserts, through gpuq.sort_last_plan(), which
plan ran. The expected plan is computed here from the rule in DESIGN.md
("Sort: prefix plan"), on the encoded keys, independently of the engine:

  need     = ceil(log2(n)) + 2 changed bits
  window   = the top H active bytes, H the smallest count reaching `need`
  deferred = the active bytes below the window; at least 2, else classic
  gate     = n * prod_{window bytes} sum_v p_v^2 <= 1, else classic
"""
import numpy as np
import pytest

import oracle

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SIGN = np.uint64(1 << 63)
TIE_MAX = 32          # GPUQ_SORT_TIE_MAX
TIEFIX_TILE = 2048    # rows per tie-fix block


@pytest.fixture(scope="module")
def gq():
    from spark_amd import gpuq
    assert torch.cuda.is_available()
    return gpuq


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def encode(keys):
    """Order-preserving u64 encoding of the ascending sort (the descending
    one is its complement: same changed bits, same byte statistics)."""
    if keys.dtype == np.float64:
        k = keys.copy()
        k[k == 0.0] = 0.0                       # -0.0 -> 0.0
        bits = k.view(np.uint64).copy()
        bits[np.isnan(k)] = np.uint64(0x7ff8000000000000)
        neg = (bits >> np.uint64(63)).astype(bool)
        return bits ^ np.where(neg, np.uint64(0xFFFFFFFFFFFFFFFF), SIGN)
    return keys.view(np.uint64) ^ SIGN


def expected_plan(enc):
    """(window_passes, deferred_bytes) by the rule; (0, 0) = classic plan."""
    n = len(enc)
    changed = int(np.bitwise_and.reduce(enc)) ^ int(np.bitwise_or.reduce(enc))
    need = (n - 1).bit_length() + 2
    active = [b for b in range(8) if (changed >> (8 * b)) & 0xff]
    window, bits = [], 0
    for b in reversed(active):
        window.append(b)
        bits += bin((changed >> (8 * b)) & 0xff).count("1")
        if bits >= need:
            break
    if bits < need:
        return 0, 0
    deferred = [b for b in active if b < window[-1]]
    if len(deferred) < 2:
        return 0, 0
    est = float(n)
    for b in window:
        byte = ((enc >> np.uint64(8 * b)) & np.uint64(0xff)).astype(np.int64)
        p = np.bincount(byte, minlength=256) / float(n)
        est *= float((p * p).sum())
    if est > 1.0:
        return 0, 0
    return len(window), len(deferred)


def check(gq, keys, desc=False, valid=None, nulls_first=None):
    """Sort on the device, compare with the oracle; returns the plan."""
    kw, okw = {}, {}
    if valid is not None:
        kw["key_validity"] = torch.from_numpy(
            np.packbits(valid, bitorder="little")).cuda()
        okw["validity"] = np.packbits(valid, bitorder="little")
    perm, skeys = gq.sort_perm(to_dev(keys), desc=desc, nulls_first=nulls_first, **kw)
    plan = gq.sort_last_plan()
    exp = oracle.sort_perm(keys, desc=desc, nulls_first=nulls_first, **okw)
    got_perm = perm.cpu().numpy().astype(np.uint32)
    assert (got_perm == exp.astype(np.uint32)).all()
    got, want = skeys.cpu().numpy(), keys[exp]
    if keys.dtype == np.float64:
        # the engine emits the canonical NaN and +0.0 (as the classic plan does)
        assert ((got == want) | (np.isnan(got) & np.isnan(want))).all()
    else:
        assert (got == want).all()
    return plan, got_perm, got


def assert_rule(plan, enc, must_prefix):
    wp, db = expected_plan(enc)
    if must_prefix:
        assert db >= 2, "the case was built to select the prefix plan"
    assert plan == (wp, db, 0)


# ---------- prefix path taken ----------

SIZES = [2, 65, 5632 * 3 + 17, 1 << 16, 1 << 20]


@pytest.mark.parametrize("desc", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_prefix_i64_full_range(gq, n, desc):
    keys = oracle.gen_i64(seed=1000 + n, n=n)
    plan, _, _ = check(gq, keys, desc=desc)
    # from one scatter tile up the window is a strict subset of the 8 bytes
    assert_rule(plan, encode(keys), must_prefix=n >= 5632 * 3 + 17)


@pytest.mark.parametrize("desc", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_prefix_f64_normals(gq, n, desc):
    keys = np.random.default_rng(n).standard_normal(n)
    if n >= 100:
        keys[:100] = np.repeat([0.0, -0.0, np.nan, np.inf, -np.inf], 20)
    plan, _, _ = check(gq, keys, desc=desc)
    # normals crowd the exponent bytes: the rule (gate included) decides
    assert_rule(plan, encode(keys), must_prefix=False)


@pytest.mark.parametrize("desc", [False, True])
def test_prefix_f64_wide(gq, desc):
    # every bit pattern: all 8 bytes active and uniform, ~0.1% NaNs that
    # collapse to one canonical key (a long run of fully equal keys)
    n = 1 << 16
    keys = oracle.gen_i64(seed=77, n=n).view(np.float64).copy()
    keys[:100] = np.repeat([0.0, -0.0, np.nan, np.inf, -np.inf], 20)
    plan, _, _ = check(gq, keys, desc=desc)
    assert_rule(plan, encode(keys), must_prefix=True)


@pytest.mark.parametrize("nulls_first", [False, True])
@pytest.mark.parametrize("desc", [False, True])
@pytest.mark.parametrize("n", [5632 * 3 + 17, 1 << 16])
def test_prefix_i64_with_nulls(gq, n, desc, nulls_first):
    keys = oracle.gen_i64(seed=2000 + n, n=n)
    valid = np.random.default_rng(n).random(n) >= 0.10
    plan, _, _ = check(gq, keys, desc=desc, valid=valid, nulls_first=nulls_first)
    assert_rule(plan, encode(keys[valid]), must_prefix=True)


def test_prefix_hist_scan_variant(gq, monkeypatch):
    monkeypatch.setenv("GPUQ_NO_ONESWEEP", "1")
    keys = oracle.gen_i64(seed=31, n=1 << 16)
    plan, _, _ = check(gq, keys)
    assert_rule(plan, encode(keys), must_prefix=True)


# ---------- run edges ----------

def build_run_edges(n=1 << 16, seed=5):
    """Keys laid out in sorted order as runs that share the top 24 bits, then
    shuffled. Unsorted runs (random low bits) of 1, 2, 31 and 32 rows and
    fully-equal runs of 33 and 1000 rows sit at both array ends and across
    tie-fix block boundaries; everything else is single rows."""
    rng = np.random.default_rng(seed)
    special = {}                       # sorted start position -> (len, equal)
    special[0] = (TIE_MAX, False)      # an unsorted 32-run at the array start
    b = TIEFIX_TILE
    layout = [(1, False, 0), (2, False, 1), (31, False, 15), (32, False, 16),
              (32, False, 31), (32, False, 1), (33, True, 16), (33, True, 32),
              (1000, True, 500), (31, False, 30), (2, False, 1), (33, True, 1)]
    for k, (ln, equal, before) in enumerate(layout, start=1):
        special[k * b - before] = (ln, equal)   # `before` rows left of the edge
    special[n - 33] = (33, True)       # an equal 33-run at the array end
    lens, equal = [], []
    pos = 0
    for start in sorted(special):
        assert start >= pos
        lens += [1] * (start - pos)
        equal += [False] * (start - pos)
        lens.append(special[start][0])
        equal.append(special[start][1])
        pos = start + special[start][0]
    assert pos == n
    nruns = len(lens)
    win = np.sort(rng.choice(1 << 24, size=nruns, replace=False)).astype(np.uint64)
    enc = np.empty(n, dtype=np.uint64)
    pos = 0
    for w, ln, eq in zip(win, lens, equal):
        low = rng.integers(0, 1 << 40, size=1 if eq else ln, dtype=np.uint64)
        enc[pos:pos + ln] = (w << np.uint64(40)) | low
        pos += ln
    keys = (enc ^ SIGN).view(np.int64)
    return keys[rng.permutation(n)].copy()


@pytest.mark.parametrize("desc", [False, True])
def test_run_edges(gq, desc):
    keys = build_run_edges()
    plan, _, _ = check(gq, keys, desc=desc)
    wp, db = expected_plan(encode(keys))
    assert (wp, db) == (3, 5)          # the window is exactly the run key
    assert plan == (3, 5, 0)           # no fallback


def test_heavy_duplicates(gq):
    vals = oracle.gen_i64(seed=9, n=2000)
    keys = vals[np.random.default_rng(9).integers(0, 2000, 200_000)]
    plan, _, _ = check(gq, keys)
    assert_rule(plan, encode(keys), must_prefix=True)


# ---------- fallback, gate, kill switch ----------

def fallback_keys(n=65536, seed=13):
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 256, n).astype(np.uint64)
    low = rng.integers(0, 1 << 32, n).astype(np.uint64)
    return (v * np.uint64(0x0101010100000000) + low).view(np.int64)


def test_device_fallback(gq):
    # every window byte looks uniform to the gate, yet there are only 256
    # window values: ~256-row unsorted runs overflow the tie-fix
    keys = fallback_keys()
    wp, db = expected_plan(encode(keys))
    assert db >= 2
    plan, _, _ = check(gq, keys)
    assert plan == (wp, db, 1)


def test_device_fallback_with_nulls(gq):
    keys = fallback_keys(seed=14)
    valid = np.random.default_rng(14).random(len(keys)) >= 0.10
    wp, db = expected_plan(encode(keys[valid]))
    assert db >= 2
    plan, _, _ = check(gq, keys, valid=valid)
    assert plan == (wp, db, 1)


def test_gate_rejects_clustered_keys(gq):
    """Two high bytes that are each 0x00 or 0xFF contribute 16 changed bits but
    only 4 window values; with a uniform third byte the window has 24 bits and
    the estimate is 65536 * 0.5 * 0.5 / 256 = 64 > 1 (real runs: ~64 unsorted
    rows). The gate must pick the classic plan before any prefix work."""
    n = 65536
    rng = np.random.default_rng(17)
    hi = rng.integers(0, 2, (2, n)).astype(np.uint64) * np.uint64(0xff)
    low48 = rng.integers(0, 1 << 48, n).astype(np.uint64)
    keys = ((hi[0] << np.uint64(56)) | (hi[1] << np.uint64(48)) | low48).view(np.int64)
    assert expected_plan(encode(keys)) == (0, 0)
    plan, _, _ = check(gq, keys)
    assert plan == (0, 0, 0)           # classic plan, no prefix work


def test_one_bit_high_byte(gq):
    """(c << 56) | low48 with c in {0, 1}: byte 7 adds one changed bit, byte 6
    is constant, so 18 bits need bytes 7, 5, 4, 3. Those 25 bits spread 65536
    rows thinly (estimate 65536 * 0.5 / 256^3 = 0.002, longest real run 2):
    the rule takes the prefix plan here, 4 passes instead of 7."""
    n = 65536
    rng = np.random.default_rng(17)
    c = rng.integers(0, 2, n).astype(np.uint64)
    low48 = rng.integers(0, 1 << 48, n).astype(np.uint64)
    keys = ((c << np.uint64(56)) | low48).view(np.int64)
    assert expected_plan(encode(keys)) == (4, 3)
    plan, _, _ = check(gq, keys)
    assert plan == (4, 3, 0)


def test_kill_switch(gq, monkeypatch):
    n = SIZES[-1]
    keys = oracle.gen_i64(seed=1000 + n, n=n)
    plan, perm0, keys0 = check(gq, keys)
    assert plan[1] >= 2 and plan[2] == 0
    monkeypatch.setenv("GPUQ_SORT_NO_PREFIX", "1")
    plan, perm1, keys1 = check(gq, keys)
    assert plan == (0, 0, 0)
    assert (perm0 == perm1).all() and (keys0 == keys1).all()
