"""GPU parity for sliding ROWS BETWEEN frames and first_value / last_value
(gpuq_window_slide, its wrapper and GpuWindowExec) against tests/slide_ref.py.

Exactness: everything is compared bit for bit (any NaN counts as NaN), the
float64 SUM of a two-sided bounded frame included: the kernel re-adds each
frame's rows in row order, which is the reference's arithmetic, so it is also
checked on doubles in [0, 1) whose sums round at every step. Frames from
UNBOUNDED PRECEDING run the ROWS scan, whose float64 SUM adds in tile order:
bit for bit on integer-valued doubles (every partial sum exact), and within
the scan's 1e-6 relative tolerance on the non-negative unit floats (input
recipe and bound of test_gpu_window.py::test_float_sum_tolerance).

Sizes up to 257 are compared with the row-by-row reference, longer ones with
its numpy twin (test_slide_ref.py checks the twin against the row-by-row
form).
"""
import functools
import zlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import slide_ref as S  # noqa: E402
import window_ref as R  # noqa: E402
from spark_amd import gpuq as G  # noqa: E402

T = G.WIN_TILE
CAP = G.WIN_SLIDE_MAX_SPAN
SIZES = [1, 2, 63, 64, 65, 257, T - 1, T, T + 1, 3 * T + 1]
BIG = G.WIN_CARRY_SPAN * T + T + 1
ROW_BY_ROW_MAX = 257
NAN, INF = float("nan"), float("inf")
FSPECIAL = np.array([NAN, INF, -INF, -0.0, 0.0, 1.5, -3.0, 7.0])
FRAMES = [(0, 0), (-1, 0), (0, 1), (-2, 2), (-3, -1), (2, 5), (-64, 63),
          (-CAP // 2, CAP // 2), (T + 7, T + 9), (-(2 * T + 5), -(2 * T + 3)),
          (None, -1), (None, 2), (None, None)]
LAYOUTS = ["one", "each", "random_edges"]


def frame_id(f):
    return "_".join("unb" if b is None else str(b) for b in f)


@pytest.fixture(scope="module")
def gq():
    assert torch.cuda.is_available()
    return G


def test_constants():
    assert CAP == 2048 and FRAMES[7] == (-1024, 1024)
    assert FRAMES[7][1] - FRAMES[7][0] == CAP
    assert BIG < 1 << 24        # the float-sum tolerance argument of the scan


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
    """bit-for-bit equality of two 8-byte columns; any NaN equals any NaN."""
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    assert got.dtype == want.dtype, (got.dtype, want.dtype)
    eq = got.view(np.uint64) == want.view(np.uint64)
    if got.dtype == np.float64:
        eq = eq | (np.isnan(got) & np.isnan(want))
    return bool(eq.all())


def ref(op, lo, hi, part, vals=None, ok=None):
    """(out, ok-or-None) from the row-by-row reference for short inputs, from
    the numpy twin otherwise; NULL rows hold 0, ok is None for count."""
    if len(part) > ROW_BY_ROW_MAX:
        return S.np_slide(op, lo, hi, part, vals, ok)
    dt = "f64" if vals is not None and vals.dtype == np.float64 else "i64"
    lst = None if vals is None else R.to_list(vals, ok)
    out = S.slide(op, lo, hi, part.tolist(), lst, dt)
    if op == "count":
        return np.array(out, dtype=np.int64), None
    return R.from_list(out, vals.dtype)


def can_be_empty(lo, hi):
    return (lo is not None and lo > 0) or (hi is not None and hi < 0)


def check(gq, op, lo, hi, part, dpart, vals, dvals, ok, dok, tag, rtol=None):
    """one call against the reference: values, validity, and when the
    wrapper returns a bitmap at all."""
    n = len(part)
    out, bits = gq.window_slide(op, lo, hi, dpart, val=dvals, validity=dok, n=n)
    want, wok = ref(op, lo, hi, part, vals, ok)
    if rtol is None:
        assert same_bits(out, want), tag
    else:
        np.testing.assert_allclose(out.cpu().numpy(), want, rtol=rtol, atol=0)
    expect_bits = op in ("first_value", "last_value") or (
        op != "count" and (ok is not None or can_be_empty(lo, hi)))
    assert (bits is not None) == expect_bits, tag
    if bits is None:
        assert wok is None or wok.all(), tag
    else:
        assert np.array_equal(host_bits(bits, n), wok), tag


# ---------------- layouts and values ----------------

def _groups(n, sizes):
    flags = np.zeros(n, dtype=bool)
    i = k = 0
    while i < n:
        flags[i] = True
        i += sizes[k % len(sizes)]
        k += 1
    return flags


@functools.lru_cache(maxsize=None)
def layout(name, n):
    """(part, ok): bool arrays; ok is the value columns' validity."""
    rng = np.random.RandomState(zlib.crc32(f"slide/{name}/{n}".encode()))
    ok = rng.rand(n) >= 0.3
    if name == "one":
        part = np.zeros(n, dtype=bool)
        part[0] = True
    elif name == "each":
        part = np.ones(n, dtype=bool)
    elif name == "random_edges":
        # random sizes, plus starts exactly on and beside the tile edges
        part = _groups(n, rng.choice([1, 2, 5, 40, 64, 300, 1000, 2500],
                                     size=64).tolist())
        for a in (T - 1, T, T + 1, 2 * T - 1, 2 * T + 1, 3 * T):
            if a < n:
                part[a] = True
    elif name == "null_run":
        # one partition with a NULL run longer than the widest frame, and a
        # second, all-NULL partition
        part = np.zeros(n, dtype=bool)
        part[[0, 2 * T + 400]] = True
        ok[100:100 + CAP + 150] = False
        ok[2 * T + 400:] = False
    else:
        raise KeyError(name)
    part.setflags(write=False)
    ok.setflags(write=False)
    return part, ok


@functools.lru_cache(maxsize=None)
def values(n):
    """int64 values, integer-valued doubles, doubles with NaN / inf / signed
    zeros, doubles in [0, 1)."""
    rng = np.random.RandomState(177 + n % 9973)
    xi = rng.randint(-(1 << 62), 1 << 62, size=n).astype(np.int64)
    xd = rng.randint(-50, 51, size=n).astype(np.float64)
    xs = FSPECIAL[rng.randint(0, len(FSPECIAL), size=n)]
    xu = rng.rand(n)
    for a in (xi, xd, xs, xu):
        a.setflags(write=False)
    return xi, xd, xs, xu


def check_frame(gq, name, n, lo, hi, with_bitmap=True):
    part, ok = layout(name, n)
    if not with_bitmap:
        ok = None
    xi, xd, xs, xu = values(n)
    dpart, dok = dev_bits(part), dev_valid(ok)
    tag = (name, n, lo, hi, with_bitmap)
    check(gq, "count", lo, hi, part, dpart, None, None, None, None, ("count*",) + tag)
    di, dd, ds, du = dev(xi), dev(xd), dev(xs), dev(xu)
    for op in S.OPS:
        check(gq, op, lo, hi, part, dpart, xi, di, ok, dok, (op, "i64") + tag)
    for op in ("min", "max", "first_value", "last_value", "count"):
        check(gq, op, lo, hi, part, dpart, xs, ds, ok, dok, (op, "special") + tag)
    check(gq, "sum", lo, hi, part, dpart, xd, dd, ok, dok, ("sum", "exact") + tag)
    if lo is not None:
        # row-order sums: inf + -inf, NaN, and sums that round at every add
        check(gq, "sum", lo, hi, part, dpart, xs, ds, ok, dok, ("sum", "special") + tag)
        check(gq, "sum", lo, hi, part, dpart, xu, du, ok, dok, ("sum", "unit") + tag)
    else:
        check(gq, "sum", lo, hi, part, dpart, xu, du, ok, dok, ("sum", "unit") + tag,
              rtol=1e-6)


# ---------------- the kernels ----------------

@pytest.mark.parametrize("frame", FRAMES, ids=frame_id)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", LAYOUTS)
def test_slide_sizes(gq, name, n, frame):
    check_frame(gq, name, n, *frame)


@pytest.mark.parametrize("frame", FRAMES, ids=frame_id)
@pytest.mark.parametrize("n", [65, 3 * T + 1])
def test_slide_without_a_bitmap(gq, n, frame):
    check_frame(gq, "random_edges", n, *frame, with_bitmap=False)


@pytest.mark.parametrize("frame", FRAMES, ids=frame_id)
def test_null_run_longer_than_the_frame(gq, frame):
    check_frame(gq, "null_run", 3 * T + 1, *frame)


@pytest.mark.parametrize("name", LAYOUTS)
def test_unbounded_frames_equal_the_scan(gq, name):
    n = 3 * T + 1
    part, ok = layout(name, n)
    xi, xd, xs, xu = values(n)
    dpart, dok = dev_bits(part), dev_valid(ok)
    for hi, frame in ((0, "rows"), (None, "partition")):
        a, _ = gq.window_slide("count", None, hi, dpart, n=n)
        b, _ = gq.window_scan("count", frame, dpart, dpart, n=n)
        assert torch.equal(a, b)
        for x in (xi, xd, xs, xu):
            d = dev(x)
            for op in ("count", "sum", "min", "max"):
                a, abits = gq.window_slide(op, None, hi, dpart, val=d, validity=dok)
                b, bbits = gq.window_scan(op, frame, dpart, dpart, val=d, validity=dok)
                assert same_bits(a, b.cpu().numpy()), (op, frame, name)
                assert (abits is None) == (bbits is None)
                if abits is not None:
                    assert torch.equal(abits, bbits), (op, frame, name)


def test_int64_sum_wraps_past_2_63(gq):
    n = 300
    part = np.zeros(n, dtype=bool)
    part[0] = True
    x = np.full(n, (1 << 62) + 12345, dtype=np.int64)
    want, _ = S.np_slide("sum", -2, 0, part, x)
    assert (want < 0).any() and (want > 0).any()
    assert want.tolist() == S.slide("sum", -2, 0, part.tolist(), x.tolist())
    out, bits = gq.window_slide("sum", -2, 0, dev_bits(part), val=dev(x))
    assert bits is None and same_bits(out, want)


@pytest.mark.parametrize("frame", [(-3, 3), (None, 2)], ids=frame_id)
def test_slide_across_a_carry_step(gq, frame):
    """the partition positions carried from tile to tile, past one step of
    the carry kernel, against the numpy twin."""
    lo, hi = frame
    n = BIG
    rng = np.random.RandomState(4242)
    part = _groups(n, rng.choice([1, 3, 700, 5000, 3 * T + 5], size=97).tolist())
    part[[T * G.WIN_CARRY_SPAN - 1, T * G.WIN_CARRY_SPAN + 1]] = True
    ok = rng.rand(n) >= 0.3
    xi = rng.randint(-(1 << 62), 1 << 62, size=n).astype(np.int64)
    xd = rng.randint(-50, 51, size=n).astype(np.float64)
    dpart, dok = dev_bits(part), dev_valid(ok)
    check(gq, "sum", lo, hi, part, dpart, xi, dev(xi), ok, dok, ("sum", "i64", frame))
    check(gq, "sum", lo, hi, part, dpart, xd, dev(xd), ok, dok, ("sum", "f64", frame))
    check(gq, "last_value", lo, hi, part, dpart, xi, dev(xi), ok, dok, ("last", frame))
    check(gq, "count", lo, hi, part, dpart, None, None, None, None, ("count*", frame))


def test_count_accepts_a_validity_buffer(gq):
    """the C entry point fills a bitmap given for COUNT, all valid."""
    n = 131
    part, ok = layout("random_edges", n)
    dpart = dev_bits(part)
    for lo, hi in ((2, 3), (None, -1)):
        clo = -(1 << 63) if lo is None else lo
        ws = gq.window_slide_workspace(n, lo, hi)
        out = torch.empty(n, dtype=torch.int64, device="cuda")
        bits = torch.zeros((n + 7) // 8, dtype=torch.uint8, device="cuda")
        rc = gq.lib().gpuq_window_slide(
            0, n, gq.WIN_OP["count"], gq._Col(None, None, 0), clo, hi,
            dpart.data_ptr(), out.data_ptr(), bits.data_ptr(), ws.data_ptr(),
            ws.numel())
        torch.cuda.synchronize()
        assert rc == 0 and host_bits(bits, n).all()
        assert same_bits(out, ref("count", lo, hi, part)[0])


def test_wrapper_errors(gq):
    x = torch.arange(10, dtype=torch.int64, device="cuda")
    part, _ = gq.window_boundaries([x], None, 0)
    with pytest.raises(ValueError, match="span"):
        gq.window_slide("sum", 0, CAP + 1, part, val=x)
    with pytest.raises(ValueError, match="span"):
        gq.window_slide("sum", -CAP - 1, 0, part, val=x)
    with pytest.raises(ValueError, match="unbounded hi"):
        gq.window_slide("sum", 1, None, part, val=x)
    with pytest.raises(ValueError, match="bad op"):
        gq.window_slide("rank", 0, 0, part, n=10)
    out, bits = gq.window_slide("sum", -CAP, 0, part, val=x)       # the cap itself
    assert bits is None and out.cpu().tolist() == np.cumsum(np.arange(10)).tolist()
    empty = torch.empty(0, dtype=torch.float64, device="cuda")
    p0, _ = gq.window_boundaries([empty], None, 1)
    out, bits = gq.window_slide("last_value", None, None, p0, val=empty)
    assert out.numel() == 0 and out.dtype == torch.float64 and bits.numel() == 0


# ---------------- plan nodes ----------------

@functools.lru_cache(maxsize=None)
def node_table():
    """4000 unsorted rows: a partition key, a unique order key, value columns
    with bitmaps."""
    n = 4000
    rng = np.random.RandomState(2024)
    cols = {
        "store": rng.randint(0, 12, size=n).astype(np.int64),
        "day": rng.permutation(n).astype(np.int64),
        "sales": (rng.rand(n) * 100).astype(np.float64),
        "units": rng.randint(-5, 50, size=n).astype(np.int64),
    }
    ok = {"sales": rng.rand(n) > 0.3, "units": rng.rand(n) > 0.3}
    return cols, ok


def node_batches():
    from spark_amd import exec as gx
    cols, ok = node_table()
    cuts = [0, 1500, 1501, 4000]
    return [gx.ColumnarBatch({k: dev(v[a:b]) for k, v in cols.items()},
                             validity={k: dev_valid(v[a:b]) for k, v in ok.items()})
            for a, b in zip(cuts, cuts[1:])]


def collect(plan):
    batches = list(plan.execute_columnar())
    assert len(batches) == 1
    b = batches[0]
    n = b.num_rows()
    return {k: (t.cpu().numpy(),
                None if b.validity(k) is None else host_bits(b.validity(k), n))
            for k, t in b.columns().items()}, n


def test_sort_then_sliding_window_node(gq):
    from spark_amd import exec as gx
    from spark_amd.exec import RowsBetween, SortOrder, WindowExpr
    order = [SortOrder("day")]
    exprs = [WindowExpr("avg", "sales", "ma3", frame=RowsBetween(-2, 0)),
             WindowExpr("min", "units", "cmin", frame=RowsBetween(-1, 1)),
             WindowExpr("count", "units", "ahead", frame=RowsBetween(1, 3)),
             WindowExpr("first_value", "sales", "fv"),
             WindowExpr("first_value", "units", "fv_prev", frame=RowsBetween(-2, -1)),
             WindowExpr("last_value", "sales", "lv", frame="partition"),
             WindowExpr("last_value", "units", "lv_rows", frame="rows"),
             WindowExpr("sum", "units", "running", frame=RowsBetween(None, 0)),
             WindowExpr("max", "sales", "whole", frame=RowsBetween(None, None))]
    win = gx.WindowExec(exprs, ["store"], order,
                        gx.SortExec([SortOrder("store")] + order, False,
                                    gx.InputBatches(node_batches())))
    plan = gx.GpuColumnarRule().pre_columnar_transitions(win)
    assert type(plan) is gx.GpuWindowExec and type(plan.children[0]) is gx.GpuSortExec
    assert plan.window_exprs == exprs
    output = plan.output
    got, n = collect(plan)
    assert n == 4000 and list(got) == output

    srt, _ = collect(gx.GpuSortExec(win.children[0].sort_order, False,
                                    gx.InputBatches(node_batches())))
    for k, (v, ok) in srt.items():         # pass-through columns and bitmaps
        assert same_bits(got[k][0], v), k
        assert (ok is None and got[k][1] is None) or np.array_equal(got[k][1], ok), k

    part, _ = R.boundaries([R.to_list(*srt["store"]), R.to_list(*srt["day"])], 1, n)
    assert sum(part) == 12
    frames = {"fv": (None, 0), "lv": (None, None), "lv_rows": (None, 0)}
    for e in exprs:
        vals = R.to_list(*srt[e.col])
        dt = "f64" if e.col == "sales" else "i64"
        lo, hi = frames.get(e.name) or (e.frame.lo, e.frame.hi)
        if e.fn == "avg":
            want = S.avg(lo, hi, part, vals)
        else:
            want = S.slide(e.fn, lo, hi, part, vals, dt)
        gv, gok = got[e.name]
        if e.fn == "count":
            wv, wok = np.array(want, dtype=np.int64), np.ones(n, dtype=bool)
        else:
            wv, wok = R.from_list(want, gv.dtype)
        if gok is None:
            assert wok.all(), e.name
        else:
            assert np.array_equal(gok, wok), e.name
            gv = np.where(gok, gv, 0)      # the value under a NULL is free
        if e.name == "running":
            # (None, 0) runs the scan; int64, so still exact
            assert gv.dtype == np.int64
        assert same_bits(gv, wv), e.name


def test_last_value_under_the_range_frame_is_refused(gq):
    from spark_amd import exec as gx
    from spark_amd.exec import SortOrder, WindowExpr
    order = [SortOrder("day")]
    for frame in (None, "range"):
        plan = gx.GpuWindowExec([WindowExpr("last_value", "sales", "lv", frame=frame)],
                                ["store"], order, gx.InputBatches(node_batches()))
        with pytest.raises(ValueError, match="RANGE frame"):
            list(plan.execute_columnar())
