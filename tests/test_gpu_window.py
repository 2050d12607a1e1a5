"""GPU parity for the window kernels (gpuq_window_boundaries / _scan / _shift),
their Python wrappers and GpuWindowExec against tests/window_ref.py.

Exactness: the bitmaps, the rank ops, COUNT, int64 SUM / MIN / MAX, float64
MIN / MAX, shift and every validity bitmap are compared bit for bit. float64
SUM is bit-exact on integer-valued doubles (every partial sum is exact, so
the order of the additions cannot show); on values in [0, 1) it is held to the
project's 1e-6 relative tolerance: for non-negative addends any summation
order is within (m-1) * 2^-53 relative of the true sum, so with m < 2^24 the
reference and the kernel each stay below 2^-29 ~ 2e-9.

Sizes: 1, 2; 63 / 64 / 65 (one bitmap word, one wave round); 255 / 256 / 257
(one round of a block); WIN_TILE - 1 / WIN_TILE / WIN_TILE + 1 (one block);
3 * WIN_TILE + 1 (carries through several tiles); and BIG = WIN_CARRY_SPAN *
WIN_TILE + WIN_TILE + 1, which makes each walk of the carry kernel take a
second step. Sizes up to 257 are compared with the row-by-row reference, the
larger ones with its vectorised forms (test_window_ref.py checks those against
the row-by-row ones).
"""
import functools
import zlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import window_ref as R  # noqa: E402
from spark_amd import gpuq as G  # noqa: E402

T = G.WIN_TILE
SMALL = [1, 2, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 3 * T + 1]
BIG = G.WIN_CARRY_SPAN * T + T + 1
ROW_BY_ROW_MAX = 257
NAN, INF = float("nan"), float("inf")
FSPECIAL = np.array([NAN, INF, -INF, -0.0, 0.0, 1.5, -3.0, 7.0])
FRAMES = ("rows", "range", "partition")


@pytest.fixture(scope="module")
def gq():
    assert torch.cuda.is_available()
    return G


def test_constants_mirror_the_kernels():
    assert G.WIN_TILE == 2048 and G.WIN_CARRY_SPAN == 2048
    assert BIG < 1 << 24        # the float-sum tolerance argument above


# ---------------- helpers ----------------

def dev(a):
    return torch.from_numpy(np.array(a)).cuda()      # a writable copy


def dev_bits(flags):
    return dev(R.bits_of(flags).view(np.int64))


def dev_valid(ok):
    return None if ok is None else dev(np.packbits(ok, bitorder="little"))


def host_bits(t, n):
    """validity bitmap tensor -> bool array of n rows; also checks the spare
    bits of the last byte are zero."""
    raw = t.cpu().numpy()
    assert raw.dtype == np.uint8 and len(raw) == (n + 7) // 8
    bits = np.unpackbits(raw, bitorder="little")
    assert not bits[n:].any()
    return bits[:n].astype(bool)


def same_bits(got, want):
    """bit-for-bit equality of two 8-byte columns."""
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    assert got.dtype == want.dtype, (got.dtype, want.dtype)
    return np.array_equal(got.view(np.uint64), want.view(np.uint64))


def ref_scan(op, frame, part, peer, vals=None, ok=None):
    """(out, ok) from the row-by-row reference for short inputs, from the
    vectorised one otherwise; NULL rows hold 0."""
    if len(part) > ROW_BY_ROW_MAX:
        return R.np_scan(op, frame, part, peer, vals, ok)
    dt = "f64" if vals is not None and vals.dtype == np.float64 else "i64"
    lst = None if vals is None else R.to_list(vals, ok)
    out = R.scan(op, frame, part.tolist(), peer.tolist(), lst, dt)
    odt = np.float64 if dt == "f64" and op in ("sum", "min", "max") else np.int64
    o, ook = R.from_list(out, odt)
    return o, (ook if ok is not None and op in ("sum", "min", "max") else None)


def ref_shift(vals, ok, offset, part, default):
    if len(part) > ROW_BY_ROW_MAX:
        return R.np_shift(vals, ok, offset, part, default)
    out = R.shift(R.to_list(vals, ok), offset, part.tolist(), default)
    return R.from_list(out, vals.dtype)


# ---------------- boundary placements ----------------

def _groups(n, sizes):
    """bool start flags for consecutive groups of the given sizes (cycled)."""
    flags = np.zeros(n, dtype=bool)
    i = k = 0
    while i < n:
        flags[i] = True
        i += sizes[k % len(sizes)]
        k += 1
    return flags


def _peers_within(part, rng, straddle=()):
    """peer starts: the partition starts plus random extra ones; no peer
    start in [a, b] for each (a, b) of straddle (a peer group across it)."""
    peer = part | (rng.rand(len(part)) < 0.4)
    for a, b in straddle:
        lo, hi = max(a, 1), min(b, len(part) - 1)
        if lo <= hi:
            peer[lo:hi + 1] = part[lo:hi + 1]
    return peer


@functools.lru_cache(maxsize=None)
def placement(name, n):
    """(part, peer, ok): bool arrays; ok = the value column's validity, or
    None for a column without a bitmap."""
    rng = np.random.RandomState(zlib.crc32(f"{name}/{n}".encode()))
    ok = rng.rand(n) >= 0.3
    if name == "one":                       # one partition over the whole input
        part = np.zeros(n, dtype=bool)
        part[0] = True
        peer = _peers_within(part, rng, [(T - 2, T + 2)])
    elif name == "one_no_bitmap":
        part = np.zeros(n, dtype=bool)
        part[0] = True
        peer = _peers_within(part, rng)
        ok = None
    elif name == "each":                    # every row its own partition
        part = np.ones(n, dtype=bool)
        peer = part.copy()
    elif name == "edges":
        # starts on the first and on the last row of a tile, on rows 63 / 64 /
        # 65, and a peer group straddling each tile edge in between
        part = np.zeros(n, dtype=bool)
        at = [0, 63, 64, 65, T - 1, T, 2 * T - 1, 2 * T, 3 * T]
        part[[a for a in at if a < n]] = True
        peer = _peers_within(part, rng, [(T + 1, T + 9), (2 * T - 9, 2 * T - 2)])
        peer[min(2 * T + 100, n - 1)] = True
        peer[2 * T + 101:3 * T] = False     # a group running to the tile's end
    elif name == "far_end":
        # a partition that ends several tiles after its first rows
        part = np.zeros(n, dtype=bool)
        part[[a for a in (0, 10, n - 7) if 0 <= a < n]] = True
        peer = _peers_within(part, rng, [(T - 50, 2 * T + 50)])
    elif name == "null_run":
        # a partition beginning with a NULL run longer than a tile, and an
        # all-NULL partition after it
        part = np.zeros(n, dtype=bool)
        part[[a for a in (0, 100, 2 * T + 400, 2 * T + 900) if a < n]] = True
        peer = _peers_within(part, rng)
        ok[100:100 + T + 150] = False
        ok[2 * T + 400:2 * T + 900] = False
    elif name.startswith("random"):         # random sizes, NULL density by name
        density = {"random0": 0.0, "random3": 0.3, "random1": 1.0}[name]
        part = _groups(n, rng.choice([1, 2, 5, 40, 64, 300, 1000, 2500],
                                     size=64).tolist())
        peer = _peers_within(part, rng)
        ok = rng.rand(n) >= density
    else:
        raise KeyError(name)
    for a in (part, peer, ok):
        if a is not None:
            a.setflags(write=False)
    return part, peer, ok


@functools.lru_cache(maxsize=None)
def values(n):
    """int64 values (wrap past 2^63 in long partitions), integer-valued
    doubles, doubles with NaN / inf / signed zeros, doubles in [0, 1)."""
    rng = np.random.RandomState(77 + n % 9973)
    xi = rng.randint(-(1 << 62), 1 << 62, size=n).astype(np.int64)
    xd = rng.randint(-50, 51, size=n).astype(np.float64)
    xs = FSPECIAL[rng.randint(0, len(FSPECIAL), size=n)]
    xu = rng.rand(n)
    for a in (xi, xd, xs, xu):
        a.setflags(write=False)
    return xi, xd, xs, xu


def check_all_ops(gq, name, n):
    part, peer, ok = placement(name, n)
    xi, xd, xs, _ = values(n)
    dpart, dpeer, dok = dev_bits(part), dev_bits(peer), dev_valid(ok)
    ws = gq.window_workspace(n)
    for op in R.RANK_OPS:
        out, bits = gq.window_scan(op, "rows", dpart, dpeer, n=n, workspace=ws)
        want, _ = ref_scan(op, "rows", part, peer)
        assert bits is None and same_bits(out, want), (op, name, n)
    dcols = {"i": (xi, dev(xi)), "d": (xd, dev(xd)), "s": (xs, dev(xs))}
    for frame in FRAMES:
        out, bits = gq.window_scan("count", frame, dpart, dpeer, n=n, workspace=ws)
        want, _ = ref_scan("count", frame, part, peer)
        assert bits is None and same_bits(out, want), ("count*", frame, name, n)
        for col, ops in (("i", ("count", "sum", "min", "max")), ("d", ("sum",)),
                         ("s", ("min", "max"))):
            h, d = dcols[col]
            for op in ops:
                out, bits = gq.window_scan(op, frame, dpart, dpeer, val=d,
                                           validity=dok, workspace=ws)
                want, wok = ref_scan(op, frame, part, peer, h, ok)
                assert same_bits(out, want), (op, col, frame, name, n)
                if wok is None:
                    assert bits is None
                else:
                    assert np.array_equal(host_bits(bits, n), wok), \
                        (op, col, frame, name, n)


# ---------------- scans ----------------

@pytest.mark.parametrize("n", SMALL)
@pytest.mark.parametrize("name", ["one", "each", "random3"])
def test_scan_sizes(gq, name, n):
    check_all_ops(gq, name, n)


@pytest.mark.parametrize("name", ["one_no_bitmap", "edges", "far_end", "null_run",
                                  "random0", "random1"])
def test_scan_placements(gq, name):
    check_all_ops(gq, name, 3 * T + 1)


@pytest.mark.parametrize("name", ["one", "random3"])
def test_scan_across_a_carry_step(gq, name):
    check_all_ops(gq, name, BIG)


def test_null_partition_key_group_and_key_kernel_feed_the_scan(gq):
    """bitmaps from window_boundaries itself: two partition keys, the NULL
    group of the first, then every op."""
    n = T + 77
    rng = np.random.RandomState(5)
    p = np.repeat(np.arange(n // 50 + 1), 50)[:n].astype(np.int64)
    p_ok = (p % 5) != 4
    p[~p_ok] = rng.randint(0, 99, size=int((~p_ok).sum()))   # garbage under NULL
    o = (np.arange(n) // 3).astype(np.float64)
    part, peer = R.np_boundaries([(p, p_ok), (o, None)], 1)
    assert part.sum() == n // 50 + 1        # NULL rows of one run are one group
    dpart, dpeer = gq.window_boundaries([dev(p), dev(o)], [dev_valid(p_ok), None], 1)
    assert same_bits(dpart, R.bits_of(part).view(np.int64))
    assert same_bits(dpeer, R.bits_of(peer).view(np.int64))
    xi = values(n)[0]
    out, _ = gq.window_scan("sum", "range", dpart, dpeer, val=dev(xi))
    assert same_bits(out, R.np_scan("sum", "range", part, peer, xi)[0])


@pytest.mark.parametrize("n", [T + 1, BIG])
@pytest.mark.parametrize("name", ["one", "random3"])
def test_float_sum_tolerance(gq, name, n):
    part, peer, ok = placement(name, n)
    xu = values(n)[3]
    dpart, dpeer = dev_bits(part), dev_bits(peer)
    for frame in FRAMES:
        out, bits = gq.window_scan("sum", frame, dpart, dpeer, val=dev(xu),
                                   validity=dev_valid(ok))
        want, wok = R.np_scan("sum", frame, part, peer, xu, ok)
        assert np.array_equal(host_bits(bits, n), wok)
        np.testing.assert_allclose(out.cpu().numpy(), want, rtol=1e-6, atol=0)


def test_int64_sum_wraps_past_2_63(gq):
    n = 300
    part = np.zeros(n, dtype=bool)
    part[0] = True
    x = np.full(n, (1 << 62) + 12345, dtype=np.int64)
    want = R.np_scan("sum", "rows", part, part, x)[0]
    assert (want < 0).any() and (want > 0).any()
    out, _ = gq.window_scan("sum", "rows", dev_bits(part), dev_bits(part), val=dev(x))
    assert same_bits(out, want)


def test_count_and_rank_accept_a_validity_buffer(gq):
    """the C entry point fills a bitmap given for a never-NULL op."""
    n = 131
    part, peer, _ = placement("random3", n)
    dpart, dpeer = dev_bits(part), dev_bits(peer)
    ws = gq.window_workspace(n)
    for op in (gq.WIN_OP["row_number"], gq.WIN_OP["dense_rank"], gq.WIN_OP["count"]):
        out = torch.empty(n, dtype=torch.int64, device="cuda")
        bits = torch.zeros((n + 7) // 8, dtype=torch.uint8, device="cuda")
        rc = gq.lib().gpuq_window_scan(
            0, n, op, 0, gq._Col(None, None, 0), dpart.data_ptr(), dpeer.data_ptr(),
            out.data_ptr(), bits.data_ptr(), ws.data_ptr(), ws.numel())
        torch.cuda.synchronize()
        assert rc == 0 and host_bits(bits, n).all()


# ---------------- boundaries ----------------

@functools.lru_cache(maxsize=None)
def key_columns(n):
    """8 sorted-looking key columns: runs of equal values, int64 / float64
    mixed, some with bitmaps; the float ones hold -0.0 / 0.0 and NaN runs."""
    rng = np.random.RandomState(31 + n)
    cols = []
    for c in range(8):
        run = [40, 7, 3, 1, 64, 2, 300, 5][c]
        base = np.arange(n) // run
        if c % 2 == 0:
            v = (base * 3 - 10).astype(np.int64)
        else:
            v = FSPECIAL[base % len(FSPECIAL)].copy()
            flip = rng.rand(n) < 0.5
            v = np.where((v == 0.0) & flip, -v, v)     # mix the zero signs
        ok = None
        if c in (0, 1, 5, 6):
            ok = (base % 4) != 1
            v = np.where(ok, v, rng.randint(0, 9, size=n).astype(v.dtype))
        cols.append((v, ok))
    return cols


@pytest.mark.parametrize("n", SMALL)
@pytest.mark.parametrize("nkeys,npart", [(0, 0), (1, 0), (1, 1), (2, 1), (8, 4)])
def test_boundaries(gq, n, nkeys, npart):
    cols = key_columns(n)[:nkeys]
    if nkeys == 0:
        part = np.zeros(n, dtype=bool)
        part[0] = True
        peer = part
    elif n <= ROW_BY_ROW_MAX:
        lists = [R.to_list(v, ok) for v, ok in cols]
        part, peer = (np.array(b) for b in R.boundaries(lists, npart, n))
    else:
        part, peer = R.np_boundaries(cols, npart)
    dpart, dpeer = gq.window_boundaries(
        [dev(v) for v, _ in cols], [dev_valid(ok) for _, ok in cols], npart, n=n)
    assert dpart.dtype == torch.int64 and dpart.numel() == (n + 63) // 64
    assert same_bits(dpart, R.bits_of(part).view(np.int64)), "part"
    assert same_bits(dpeer, R.bits_of(peer).view(np.int64)), "peer"


def test_boundaries_float_zero_and_nan_equality(gq):
    nan2 = np.array([0x7FF8000000000123], dtype=np.uint64).view(np.float64)[0]
    k = np.array([-0.0, 0.0, 1.0, NAN, nan2, -NAN, INF], dtype=np.float64)
    dpart, dpeer = gq.window_boundaries([dev(k)], None, 1)
    assert dpart.cpu().numpy().view(np.uint64)[0] == 0b1001101
    dpart, dpeer = gq.window_boundaries([dev(k)], None, 0)
    assert dpart.cpu().numpy().view(np.uint64)[0] == 1
    assert dpeer.cpu().numpy().view(np.uint64)[0] == 0b1001101


def test_boundaries_across_a_carry_step_size(gq):
    cols = key_columns(BIG)[:2]
    part, peer = R.np_boundaries(cols, 1)
    dpart, dpeer = gq.window_boundaries(
        [dev(v) for v, _ in cols], [dev_valid(ok) for _, ok in cols], 1)
    assert same_bits(dpart, R.bits_of(part).view(np.int64))
    assert same_bits(dpeer, R.bits_of(peer).view(np.int64))


# ---------------- shift ----------------

def check_shift(gq, name, n, offsets):
    part, _, ok = placement(name, n)
    xi, _, xs, _ = values(n)
    dpart, dok = dev_bits(part), dev_valid(ok)
    ws = gq.window_workspace(n)
    for vals, default in ((xi, -1), (xs, 2.5)):
        d = dev(vals)
        for offset in offsets:
            for dflt in (None, default):
                out, bits = gq.window_shift(d, offset, dpart, validity=dok,
                                            default=dflt, workspace=ws)
                want, wok = ref_shift(vals, ok, offset, part, dflt)
                assert same_bits(out, want), (name, n, offset, dflt)
                assert np.array_equal(host_bits(bits, n), wok), (name, n, offset, dflt)


@pytest.mark.parametrize("n", [1, 2, 64, 65, 257, T + 1])
def test_shift_sizes(gq, n):
    check_shift(gq, "random3", n, [-2, -1, 0, 1, 2])


@pytest.mark.parametrize("name", ["one", "one_no_bitmap", "edges", "far_end",
                                  "random3"])
def test_shift_offsets(gq, name):
    n = 3 * T + 1
    check_shift(gq, name, n, [-1, 1, -2, 2, -T, T, 0, -(n + 5), n + 5,
                              -(1 << 40), 1 << 40])


def test_shift_across_a_carry_step(gq):
    check_shift(gq, "random3", BIG, [-1, T])


# ---------------- argument errors ----------------

INVALID = 2


def _scan_rc(gq, n, op, frame, col, out_valid=True, ws_bytes=None):
    m = max(min(n, 64), 1)
    bits = torch.ones(1, dtype=torch.int64, device="cuda")
    out = torch.zeros(m, dtype=torch.int64, device="cuda")
    ov = torch.zeros(8, dtype=torch.uint8, device="cuda")
    ws = gq.window_workspace(min(n, 64))
    need = gq.lib().gpuq_window_workspace_bytes(min(n, 1 << 32))
    rc = gq.lib().gpuq_window_scan(
        0, n, op, frame, col, bits.data_ptr(), bits.data_ptr(), out.data_ptr(),
        ov.data_ptr() if out_valid else None, ws.data_ptr(),
        need if ws_bytes is None else ws_bytes)
    torch.cuda.synchronize()
    return rc


def test_scan_argument_errors(gq):
    x = torch.arange(64, dtype=torch.int64, device="cuda")
    v = torch.full((8,), 0xFF, dtype=torch.uint8, device="cuda")
    col = gq._Col(x.data_ptr(), None, gq.GPUQ_INT64)
    SUM, ROWS = gq.WIN_OP["sum"], gq.WIN_FRAME["rows"]
    assert _scan_rc(gq, 64, SUM, ROWS, col) == 0
    assert _scan_rc(gq, (1 << 32), SUM, ROWS, col) == INVALID
    assert b"nrows" in gq.lib().gpuq_last_error()
    assert _scan_rc(gq, -1, SUM, ROWS, col) == INVALID
    for op in (-1, 7):
        assert _scan_rc(gq, 64, op, ROWS, col) == INVALID
    for frame in (-1, 3):
        assert _scan_rc(gq, 64, SUM, frame, col) == INVALID
    for op in ("row_number", "rank", "dense_rank"):
        for frame in ("range", "partition"):
            assert _scan_rc(gq, 64, gq.WIN_OP[op], gq.WIN_FRAME[frame],
                            gq._Col(None, None, 0)) == INVALID
    bad = gq._Col(x.data_ptr(), None, gq.GPUQ_INT32)
    for op in ("count", "sum", "min", "max"):
        assert _scan_rc(gq, 64, gq.WIN_OP[op], ROWS, bad) == INVALID
    for op in ("sum", "min", "max"):
        assert _scan_rc(gq, 64, gq.WIN_OP[op], ROWS,
                        gq._Col(None, None, gq.GPUQ_INT64)) == INVALID
    assert _scan_rc(gq, 64, gq.WIN_OP["count"], ROWS,
                    gq._Col(None, None, gq.GPUQ_INT32)) == 0      # COUNT(*)
    need = gq.lib().gpuq_window_workspace_bytes(64)
    assert need > 0
    assert _scan_rc(gq, 64, SUM, ROWS, col, ws_bytes=need - 1) == INVALID
    nullable = gq._Col(x.data_ptr(), v.data_ptr(), gq.GPUQ_INT64)
    assert _scan_rc(gq, 64, SUM, ROWS, nullable, out_valid=False) == INVALID
    assert _scan_rc(gq, 64, SUM, ROWS, nullable) == 0
    assert _scan_rc(gq, 0, SUM, ROWS, col) == 0                   # nrows == 0


def test_boundaries_argument_errors(gq):
    x = torch.arange(64, dtype=torch.int64, device="cuda")
    out = torch.zeros(2, dtype=torch.int64, device="cuda")
    L = gq.lib()

    def rc(n, cols, nkeys, npart):
        arr = (gq._Col * max(len(cols), 1))(*cols)
        r = L.gpuq_window_boundaries(0, n, arr, nkeys, npart, out.data_ptr(),
                                     out.data_ptr() + 8)
        torch.cuda.synchronize()
        return r
    good = [gq._Col(x.data_ptr(), None, gq.GPUQ_INT64)] * 9
    assert rc(64, good, 8, 8) == 0
    assert rc(64, good, 9, 1) == INVALID
    assert rc(64, good, -1, 0) == INVALID
    assert rc(64, good, 2, 3) == INVALID
    assert rc(64, good, 2, -1) == INVALID
    assert rc(1 << 32, good, 1, 1) == INVALID
    assert rc(64, [gq._Col(x.data_ptr(), None, gq.GPUQ_INT32)], 1, 0) == INVALID
    assert rc(0, good, 1, 1) == 0


def test_shift_argument_errors(gq):
    x = torch.arange(64, dtype=torch.int64, device="cuda")
    out = torch.zeros(64, dtype=torch.int64, device="cuda")
    ov = torch.zeros(8, dtype=torch.uint8, device="cuda")
    bits = torch.ones(1, dtype=torch.int64, device="cuda")
    ws = gq.window_workspace(64)
    L = gq.lib()

    def rc(n, col, ws_bytes=ws.numel(), out_valid=ov.data_ptr()):
        r = L.gpuq_window_shift(0, n, col, 1, 0, 0.0, 0, bits.data_ptr(),
                                out.data_ptr(), out_valid, ws.data_ptr(), ws_bytes)
        torch.cuda.synchronize()
        return r
    col = gq._Col(x.data_ptr(), None, gq.GPUQ_INT64)
    assert rc(64, col) == 0
    assert rc(1 << 32, col, ws_bytes=L.gpuq_window_workspace_bytes(1 << 32)) == INVALID
    assert rc(64, gq._Col(x.data_ptr(), None, gq.GPUQ_INT32)) == INVALID
    assert rc(64, col, ws_bytes=ws.numel() - 1) == INVALID
    assert rc(64, gq._Col(None, None, gq.GPUQ_INT64)) == INVALID
    assert rc(64, col, out_valid=None) == INVALID
    assert rc(0, col) == 0


def test_wrapper_argument_checks(gq):
    x = torch.arange(10, dtype=torch.int64, device="cuda")
    part, peer = gq.window_boundaries([x], None, 1)
    with pytest.raises(ValueError, match="non-integral"):
        gq.window_shift(x, 1, part, default=0.5)
    with pytest.raises(ValueError, match="bitmap"):
        gq.window_shift(x, 1, torch.zeros(2, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError, match="unsupported dtype"):
        gq.window_scan("sum", "rows", part, peer, val=x.to(torch.int32))
    with pytest.raises(ValueError, match="rows frame"):
        gq.window_scan("rank", "range", part, peer, n=10)
    with pytest.raises(ValueError, match="needs a column"):
        gq.window_scan("sum", "rows", part, peer, n=10)
    with pytest.raises(ValueError, match="n is needed"):
        gq.window_scan("count", "rows", part, peer)
    with pytest.raises(ValueError, match="validity entries"):
        gq.window_boundaries([x], [None, None], 1)
    with pytest.raises(ValueError, match="npart"):
        gq.window_boundaries([x], None, 2)
    with pytest.raises(ValueError, match="rows"):
        gq.window_boundaries([x, x[:5].contiguous()], None, 1)
    empty = torch.empty(0, dtype=torch.float64, device="cuda")
    p0, q0 = gq.window_boundaries([empty], None, 1)
    out, bits = gq.window_scan("max", "range", p0, q0, val=empty)
    assert out.numel() == 0 and out.dtype == torch.float64 and bits is None


# ---------------- plan nodes ----------------

@functools.lru_cache(maxsize=None)
def node_table():
    """4000 unsorted rows in 3 batches: two partition keys (the second with
    NULLs), an order key with ties, value columns with bitmaps."""
    n = 4000
    rng = np.random.RandomState(99)
    cols = {
        "store": rng.randint(0, 12, size=n).astype(np.int64),
        "dept": rng.randint(0, 4, size=n).astype(np.int64),
        "day": rng.randint(0, 15, size=n).astype(np.float64),
        "sales": rng.randint(-20, 100, size=n).astype(np.float64),
        "units": rng.randint(-5, 50, size=n).astype(np.int64),
        "rowid": np.arange(n, dtype=np.int64),
    }
    ok = {"dept": rng.rand(n) > 0.15, "sales": rng.rand(n) > 0.3,
          "units": rng.rand(n) > 0.3}
    return cols, ok


def node_batches():
    from spark_amd import exec as gx
    cols, ok = node_table()
    cuts = [0, 1500, 1501, 4000]
    out = []
    for a, b in zip(cuts, cuts[1:]):
        out.append(gx.ColumnarBatch(
            {k: dev(v[a:b]) for k, v in cols.items()},
            validity={k: dev_valid(v[a:b]) for k, v in ok.items()}))
    return out


def collect(plan):
    """the plan's single output batch as host (values, ok-or-None) columns."""
    batches = list(plan.execute_columnar())
    assert len(batches) == 1
    b = batches[0]
    n = b.num_rows()
    return {k: (t.cpu().numpy(),
                None if b.validity(k) is None else host_bits(b.validity(k), n))
            for k, t in b.columns().items()}, n


def test_sort_then_window_node(gq):
    from spark_amd import exec as gx
    from spark_amd.exec import SortOrder, WindowExpr
    order = [SortOrder("day", descending=True)]
    exprs = [WindowExpr("row_number", None, "rn"), WindowExpr("rank", None, "rk"),
             WindowExpr("dense_rank", None, "drk"),
             WindowExpr("count", None, "cnt_star"),
             WindowExpr("count", "units", "cnt_units", frame="rows"),
             WindowExpr("sum", "units", "sum_units"),
             WindowExpr("sum", "sales", "sum_sales", frame="rows"),
             WindowExpr("min", "sales", "min_sales", frame="partition"),
             WindowExpr("max", "units", "max_units"),
             WindowExpr("avg", "sales", "avg_sales"),
             WindowExpr("avg", "sales", "avg_sales_rows", frame="rows"),
             WindowExpr("lag", "units", "lag_units"),
             WindowExpr("lead", "sales", "lead_sales", offset=2, default=-1.0)]
    win = gx.WindowExec(exprs, ["store", "dept"], order,
                        gx.SortExec([SortOrder("store"), SortOrder("dept")] + order,
                                    False, gx.InputBatches(node_batches())))
    assert win.children[0].output_ordering == win.required_child_ordering()
    plan = gx.GpuColumnarRule().pre_columnar_transitions(win)
    assert type(plan) is gx.GpuWindowExec and type(plan.children[0]) is gx.GpuSortExec
    output = plan.output         # before the run closes the input batches
    got, n = collect(plan)
    assert n == 4000 and list(got) == output

    # the sorted input, from the sort node alone
    srt, _ = collect(gx.GpuSortExec(win.children[0].sort_order, False,
                                    gx.InputBatches(node_batches())))
    for k, (v, ok) in srt.items():         # pass-through columns and bitmaps
        assert same_bits(got[k][0], v), k
        assert (ok is None and got[k][1] is None) or np.array_equal(got[k][1], ok), k

    part, peer = R.boundaries([R.to_list(*srt["store"]), R.to_list(*srt["dept"]),
                               R.to_list(*srt["day"])], 2, n)
    assert sum(part) > 12                  # the NULL dept groups are there
    for e in exprs:
        vals = R.to_list(*srt[e.col]) if e.col else None
        dt = "f64" if e.col == "sales" else "i64"
        frame = e.frame or "range"
        if e.fn in R.RANK_OPS:
            want = R.scan(e.fn, "rows", part, peer)
        elif e.fn == "avg":
            want = R.avg(frame, part, peer, vals)
        elif e.fn in ("lag", "lead"):
            want = R.shift(vals, -e.offset if e.fn == "lag" else e.offset, part,
                           e.default)
        else:
            want = R.scan(e.fn, frame, part, peer, vals, dt)
        wv, wok = R.from_list(want, got[e.name][0].dtype)
        gv, gok = got[e.name]
        if gok is None:
            assert wok.all(), e.name
        else:
            assert np.array_equal(gok, wok), e.name
            gv = np.where(gok, gv, 0)      # the value under a NULL is free
        assert same_bits(gv, wv), e.name


def test_top_n_per_group(gq):
    from spark_amd import exec as gx
    from spark_amd.exec import SortOrder, WindowExpr
    order = [SortOrder("sales", descending=True), SortOrder("rowid")]
    sort = gx.SortExec([SortOrder("store")] + order, False,
                       gx.InputBatches(node_batches()))
    plan = gx.GpuColumnarRule().pre_columnar_transitions(gx.FilterExec(
        "rn", "<=", 3,
        gx.WindowExec([WindowExpr("row_number", None, "rn")], "store", order, sort)))
    got, n = collect(plan)
    cols, ok = node_table()
    # reference: per store, the rows ordered by sales desc (NULLs last), rowid
    want = []
    for s in range(12):
        rows = [i for i in range(4000) if cols["store"][i] == s]
        rows.sort(key=lambda i: (not ok["sales"][i],
                                 -cols["sales"][i] if ok["sales"][i] else 0.0, i))
        want += [(s, i, r + 1) for r, i in enumerate(rows[:3])]
    assert n == len(want) == 36
    assert list(zip(got["store"][0].tolist(), got["rowid"][0].tolist(),
                    got["rn"][0].tolist())) == want
