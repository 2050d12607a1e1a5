"""Argument checks of gpuq_window_slide that need no GPU: the entry point
validates everything before any HIP call, so each refusal is driven here
through ctypes with fake, never dereferenced pointers. Also nrows == 0, the
workspace helper's arithmetic and the constants' mirrors."""
import os
import subprocess

import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x1000     # never dereferenced: every call here stops before a launch
INVALID = 2
UNB_LO, UNB_HI = -(1 << 63), (1 << 63) - 1
COUNT, SUM, MIN, MAX, FIRST, LAST = 3, 4, 5, 6, 7, 8


@pytest.fixture(scope="module")
def gpuq():
    # always through make: a library older than its source lacks the entry
    # point tested here
    subprocess.run(["make", "-C", os.path.join(ROOT, "spark_amd", "csrc"), "-s"],
                   check=True)
    from spark_amd import gpuq as g
    return g


def call(gpuq, n=64, op=SUM, lo=-1, hi=1, data=FAKE, validity=None, dtype=None,
         out_valid=FAKE, ws_bytes=None):
    L = gpuq.lib()
    col = gpuq._Col(data, validity, gpuq.GPUQ_INT64 if dtype is None else dtype)
    if ws_bytes is None:
        ws_bytes = 1 << 40          # fake and large: never the reason to refuse
    rc = L.gpuq_window_slide(None, n, op, col, lo, hi, FAKE, FAKE, out_valid,
                             FAKE, ws_bytes)
    return rc, L.gpuq_last_error().decode()


# name -> (keyword overrides, what the message must name)
BAD = {
    "nrows_negative": (dict(n=-1), "nrows"),
    "nrows_over_u32": (dict(n=0x100000000), "nrows"),
    "op_rank": (dict(op=2), "bad op"),
    "op_negative": (dict(op=-1), "bad op"),
    "op_high": (dict(op=9), "bad op"),
    "dtype_int32": (dict(dtype=2), "dtype"),
    "dtype_count_col": (dict(op=COUNT, dtype=2), "dtype"),
    "sum_without_column": (dict(data=None), "needs a value column"),
    "min_without_column": (dict(op=MIN, data=None), "needs a value column"),
    "first_without_column": (dict(op=FIRST, data=None), "needs a value column"),
    "lo_over_hi": (dict(lo=1, hi=0), "lo > hi"),
    "lo_outside_int32": (dict(lo=-(1 << 31) - 1, hi=0), "int32"),
    "hi_outside_int32": (dict(lo=UNB_LO, hi=1 << 31), "int32"),
    "lo_unbounded_following": (dict(lo=UNB_HI, hi=UNB_HI), "int32"),
    "hi_unbounded_preceding": (dict(lo=UNB_LO, hi=UNB_LO), "int32"),
    "span_over_cap": (dict(lo=-1024, hi=1025), "span"),
    "span_over_cap_far": (dict(lo=5000, hi=5000 + 2049), "span"),
    "finite_lo_unbounded_hi": (dict(lo=1, hi=UNB_HI), "UNBOUNDED FOLLOWING"),
    "current_row_unbounded_hi": (dict(lo=0, hi=UNB_HI), "UNBOUNDED FOLLOWING"),
    "first_without_bitmap": (dict(op=FIRST, out_valid=None), "output bitmap"),
    "last_without_bitmap": (dict(op=LAST, lo=UNB_LO, hi=UNB_HI, out_valid=None),
                            "output bitmap"),
    "nullable_sum_without_bitmap": (dict(validity=FAKE, out_valid=None),
                                    "output bitmap"),
    "following_frame_without_bitmap": (dict(lo=1, hi=2, out_valid=None),
                                       "output bitmap"),
    "preceding_frame_without_bitmap": (dict(op=MAX, lo=-2, hi=-1, out_valid=None),
                                       "output bitmap"),
    "unbounded_to_preceding_without_bitmap": (dict(lo=UNB_LO, hi=-1, out_valid=None),
                                              "output bitmap"),
    "short_workspace": (dict(ws_bytes=0), "workspace"),
    "short_workspace_by_one": (dict(lo=UNB_LO, hi=2, ws_bytes=-1), "workspace"),
}


@pytest.mark.parametrize("name", list(BAD))
def test_rejected_before_any_hip_call(gpuq, name):
    kw, needle = BAD[name]
    kw = dict(kw)
    if kw.get("ws_bytes") == -1:
        kw["ws_bytes"] = gpuq.lib().gpuq_window_slide_workspace_bytes(
            kw.get("n", 64), kw["lo"], kw["hi"]) - 1
        assert kw["ws_bytes"] >= 0
    rc, msg = call(gpuq, **kw)
    assert rc == INVALID, (name, rc, msg)
    assert msg.startswith("window_slide:") and needle in msg, (name, msg)


def test_zero_rows_launch_nothing(gpuq):
    # legal calls at nrows == 0 return GPUQ_OK without touching a pointer: a
    # NULL column, a NULL workspace of 0 bytes, every op and both shapes
    for op in (COUNT, SUM, MIN, MAX, FIRST, LAST):
        for lo, hi in ((-1, 1), (0, 0), (5000, 5002), (-1024, 1024),
                       (UNB_LO, 2), (UNB_LO, UNB_HI)):
            rc, msg = call(gpuq, n=0, op=op, lo=lo, hi=hi, data=None, ws_bytes=0)
            assert rc == 0, (op, lo, hi, msg)
    # refusals still come first
    assert call(gpuq, n=0, lo=1, hi=0)[0] == INVALID
    assert call(gpuq, n=0, op=9)[0] == INVALID
    # an empty bitmap's pointer may be NULL, like an empty column's
    assert call(gpuq, n=0, op=FIRST, data=None, out_valid=None)[0] == 0


def test_optional_bitmap_cases_pass_validation(gpuq):
    # the calls below are legal without an output bitmap; they are stopped by
    # a short workspace, the last check, so every earlier one has passed
    for kw in (dict(op=COUNT), dict(op=COUNT, data=None), dict(op=COUNT, lo=2, hi=3),
               dict(op=COUNT, validity=FAKE), dict(op=SUM, lo=-3, hi=0),
               dict(op=MIN, lo=0, hi=0), dict(op=MAX, lo=UNB_LO, hi=0),
               dict(op=SUM, lo=UNB_LO, hi=UNB_HI), dict(op=SUM, lo=-1024, hi=1024)):
        rc, msg = call(gpuq, out_valid=None, ws_bytes=0, **kw)
        assert rc == INVALID and "workspace" in msg, (kw, msg)


def test_workspace_arithmetic(gpuq):
    L = gpuq.lib()
    scan = L.gpuq_window_workspace_bytes
    slide = L.gpuq_window_slide_workspace_bytes

    def up(b):
        return (b + 255) // 256 * 256
    for n in (0, 1, 64, 2048, 2049, 1 << 20, 0xFFFFFFFF):
        # two finite bounds: the scan's per-tile summaries only
        assert slide(n, -1, 1) == slide(n, -1024, 1024) == slide(n, 7, 9) == scan(n)
        # from UNBOUNDED PRECEDING: plus nrows words and a bitmap
        extra = up(n * 8) + up((n + 7) // 8)
        assert slide(n, UNB_LO, 2) == slide(n, UNB_LO, UNB_HI) == scan(n) + extra
    assert scan(64) > 0
    # arguments the entry point refuses
    for n, lo, hi in ((-1, 0, 0), (0x100000000, 0, 0), (64, 1, 0), (64, 0, 2049),
                      (64, 1, UNB_HI), (64, -(1 << 31) - 1, 0), (64, UNB_LO, 1 << 31)):
        assert slide(n, lo, hi) == 0, (n, lo, hi)


def test_constants_mirror_the_header(gpuq):
    header = open(os.path.join(ROOT, "include", "gpuq.h")).read()

    def define(name):
        for line in header.splitlines():
            parts = line.split()
            if len(parts) >= 3 and parts[0] == "#define" and parts[1] == name:
                return parts[2]
        raise KeyError(name)

    assert int(define("GPUQ_WIN_SLIDE_MAX_SPAN")) == gpuq.WIN_SLIDE_MAX_SPAN == 2048
    assert int(define("GPUQ_WIN_FIRST_VALUE")) == gpuq.WIN_SLIDE_OP["first_value"] == 7
    assert int(define("GPUQ_WIN_LAST_VALUE")) == gpuq.WIN_SLIDE_OP["last_value"] == 8
    assert define("GPUQ_WIN_UNBOUNDED_PRECEDING") == "INT64_MIN"
    assert define("GPUQ_WIN_UNBOUNDED_FOLLOWING") == "INT64_MAX"
    # the scan's tables are left as they were
    assert gpuq.WIN_OP == {"row_number": 0, "rank": 1, "dense_rank": 2, "count": 3,
                           "sum": 4, "min": 5, "max": 6}
    assert gpuq.WIN_FRAME == {"rows": 0, "range": 1, "partition": 2}
    assert gpuq.WIN_TILE + gpuq.WIN_SLIDE_MAX_SPAN == 4096


def test_scan_still_refuses_the_new_ops(gpuq):
    L = gpuq.lib()
    for op in (FIRST, LAST):
        rc = L.gpuq_window_scan(None, 64, op, 0, gpuq._Col(FAKE, None, gpuq.GPUQ_INT64),
                                FAKE, FAKE, FAKE, FAKE, FAKE, 1 << 40)
        assert rc == INVALID and b"bad op" in L.gpuq_last_error()


def test_wrapper_refusals_need_no_gpu(gpuq):
    """window_slide's Python-side checks run before any tensor is touched."""
    part = torch.zeros(1, dtype=torch.int64)
    x = torch.zeros(64, dtype=torch.int64)
    cap = gpuq.WIN_SLIDE_MAX_SPAN
    for kw, match in (
            (dict(op="rank", lo=0, hi=0, n=64), "bad op"),
            (dict(op="sum", lo=1, hi=0, val=x), "lo 1 > hi 0"),
            (dict(op="sum", lo=0, hi=cap + 1, val=x), "span"),
            (dict(op="sum", lo=1, hi=None, val=x), "unbounded hi"),
            (dict(op="sum", lo=0, hi=None, val=x), "unbounded hi"),
            (dict(op="sum", lo=-(1 << 31) - 1, hi=0, val=x), "int32"),
            (dict(op="sum", lo=None, hi=1 << 31, val=x), "int32"),
            (dict(op="sum", lo=0.5, hi=1, val=x), "int or None"),
            (dict(op="sum", lo=0, hi=0, n=64), "needs a column"),
            (dict(op="first_value", lo=0, hi=0, n=64), "needs a column"),
            (dict(op="count", lo=0, hi=0), "n is needed"),
            (dict(op="count", lo=0, hi=0, n=64, validity=x), "validity without"),
            (dict(op="sum", lo=0, hi=0, val=x.to(torch.int32)), "unsupported dtype"),
            (dict(op="sum", lo=0, hi=0, val=x, n=63), "differs"),
            (dict(op="sum", lo=0, hi=0, val=torch.zeros(65, dtype=torch.int64)),
             "bitmap"),
            (dict(op="sum", lo=None, hi=0, val=x,
                  workspace=torch.zeros(8, dtype=torch.uint8)), "workspace")):
        kw = dict(kw)
        op, lo, hi = kw.pop("op"), kw.pop("lo"), kw.pop("hi")
        with pytest.raises(ValueError, match=match):
            gpuq.window_slide(op, lo, hi, part, **kw)
    with pytest.raises(ValueError, match="span"):
        gpuq.window_slide_workspace(64, 0, cap + 1)
    with pytest.raises(ValueError, match="unbounded hi"):
        gpuq.window_slide_workspace(64, 1, None)
