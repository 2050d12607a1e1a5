"""Sliding-frame window kernels (gpuq_window_slide) against the engine's own
streaming yardstick, gpuq_project_binop (column + literal: 8 B read + 8 B
written per row), and against the ROWS scan sum_rows (window_scan SUM), over
the same rows of device-generated columns in one process. There is no earlier
implementation to compare with, so nothing is gated on these numbers. Per
point the results are checked first (against closed forms of the generated
layout, computed with torch on the device), everything is warmed up, then
every case, sum_rows and the yardstick are timed with HIP events in 9
alternating repeats. A profiled call afterwards gives the per-tag kernel
times. Prints one JSON line per case.

  n in 2^AB_LOG2N (default 26)
  layouts  p1000   partitions of 1000 rows
           single  one partition over the whole input
  cases    sum_span{2,8,32,64,128,256,2048}  float64 SUM over ROWS BETWEEN span
                       PRECEDING AND CURRENT ROW (k_win_slide: span + 1 LDS
                       reads per row)
           sum_unb_2   SUM over UNBOUNDED PRECEDING .. 2 FOLLOWING (the ROWS
                       scan into the workspace, then k_win_pick)
           first_span32  FIRST_VALUE over 32 PRECEDING .. CURRENT ROW
           first_rows  FIRST_VALUE over UNBOUNDED PRECEDING .. CURRENT ROW
           sum_rows    window_scan SUM, ROWS frame (the second yardstick)

ratio = case median / yardstick median, ratio_sum_rows = case median /
sum_rows median."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from spark_amd import gpuq as gq

reps = int(os.environ.get("AB_REPS", 9))
log2ns = [int(x) for x in os.environ.get("AB_LOG2N", "26").split(",")]
TAGS = ("win_reduce", "win_carry", "win_apply", "win_slide", "win_pick")
PART_ROWS = 1000
SPANS = (2, 8, 32, 64, 128, 256, 2048)


def timed(fn):
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(ts):
    return {"median": round(statistics.median(ts), 3), "min": round(min(ts), 3),
            "max": round(max(ts), 3)}


def check(layout, n, x, part, ws_rows):
    """parity first: closed forms of the generated layout."""
    i = gq.range_i64(n)
    begin = (i // PART_ROWS) * PART_ROWS if layout == "p1000" else torch.zeros_like(i)
    end = (begin + PART_ROWS - 1).clamp(max=n - 1) if layout == "p1000" \
        else torch.full_like(i, n - 1)
    zero = torch.zeros_like(x)
    # span 2 bit for bit: ((0 + x[i-2]) + x[i-1]) + x[i] in that order
    out, bits = gq.window_slide("sum", -2, 0, part, val=x)
    want = (torch.where(i - 2 >= begin, x[(i - 2).clamp(min=0)], zero)
            + torch.where(i - 1 >= begin, x[(i - 1).clamp(min=0)], zero)) + x
    assert bits is None and torch.equal(out, want), "sum_span2"
    del want
    # wider spans against a difference of prefix sums, which is good enough
    # for a tolerance on non-negative unit floats
    c = torch.cumsum(x, 0)
    for span in SPANS[1:]:
        out, _ = gq.window_slide("sum", -span, 0, part, val=x)
        first = torch.maximum(begin, i - span)
        before = torch.where(first > 0, c[(first - 1).clamp(min=0)], zero)
        torch.testing.assert_close(out, c - before, rtol=1e-6, atol=1e-6)
        del first, before
    del c
    rows, _ = gq.window_scan("sum", "rows", part, part, val=x, workspace=ws_rows)
    out, bits = gq.window_slide("sum", None, 2, part, val=x)
    assert bits is None and torch.equal(out, rows[torch.minimum(i + 2, end)]), "sum_unb_2"
    del rows
    out, bits = gq.window_slide("first_value", -32, 0, part, val=x)
    assert torch.equal(out, x[torch.maximum(begin, i - 32)]), "first_span32"
    assert bool(gq.bits_to_u8(bits, n).bool().all()), "first_span32 validity"
    out, bits = gq.window_slide("first_value", None, 0, part, val=x)
    assert torch.equal(out, x[begin]), "first_rows"
    del out, bits


for log2n in log2ns:
    n = 1 << log2n
    for layout in ("p1000", "single"):
        i = gq.range_i64(n)
        p = gq.project_binop(i, "/", literal=PART_ROWS) if layout == "p1000" \
            else gq.project_binop(i, "*", literal=0)
        del i
        x = gq.gen_f64_unit(seed=91, n=n)
        part, _ = gq.window_boundaries([p], None, 1)
        del p
        ws_rows = gq.window_workspace(n)
        ws_a = gq.window_slide_workspace(n, -1, 0)
        ws_b = gq.window_slide_workspace(n, None, 2)
        check(layout, n, x, part, ws_rows)
        torch.cuda.empty_cache()

        def slide_sum(span):
            return lambda: gq.window_slide("sum", -span, 0, part, val=x, workspace=ws_a)
        cases = {f"sum_span{s}": slide_sum(s) for s in SPANS}
        cases.update({
            "sum_unb_2": lambda: gq.window_slide("sum", None, 2, part, val=x,
                                                 workspace=ws_b),
            "first_span32": lambda: gq.window_slide("first_value", -32, 0, part,
                                                    val=x, workspace=ws_a),
            "first_rows": lambda: gq.window_slide("first_value", None, 0, part,
                                                  val=x, workspace=ws_b),
            "sum_rows": lambda: gq.window_scan("sum", "rows", part, part, val=x,
                                               workspace=ws_rows),
        })
        yard = lambda: gq.project_binop(x, "+", literal=1.0)  # noqa: E731
        for fn in list(cases.values()) + [yard]:     # warm-up
            fn()
        torch.cuda.synchronize()
        times = {k: [] for k in cases}
        t_yard = []
        for _ in range(reps):                        # alternate all variants
            for k, fn in cases.items():
                times[k].append(timed(fn))
            t_yard.append(timed(yard))
        s_yard = stats(t_yard)
        s_rows = stats(times["sum_rows"])
        for k, fn in cases.items():
            gq.profiling(True)
            gq.kernel_stats_reset()
            fn()
            torch.cuda.synchronize()
            tags = {}
            for t in TAGS:
                ms, launches = gq.kernel_stats(t)
                if launches:
                    tags[t] = {"ms": round(ms, 3), "launches": launches}
            gq.profiling(False)
            gq.kernel_stats_reset()
            s = stats(times[k])
            print(json.dumps({
                "case": k, "layout": layout, "rows": n, "reps": reps, "ms": s,
                "yardstick_ms": s_yard, "sum_rows_ms": s_rows,
                "ratio": round(s["median"] / s_yard["median"], 2),
                "ratio_sum_rows": round(s["median"] / s_rows["median"], 2),
                "kernels": tags,
                "device": torch.cuda.get_device_name(0)}), flush=True)
        del x, part, ws_rows, ws_a, ws_b, cases, yard
        torch.cuda.empty_cache()
