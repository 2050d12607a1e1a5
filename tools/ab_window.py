"""Window kernels against the engine's own streaming yardstick,
gpuq_project_binop (column + literal: 8 B read + 8 B written per row), over the
same rows of device-generated columns. There is no earlier implementation to
compare with, so nothing is gated on these numbers. One process; per point
the results are checked first (against closed forms of the generated layout,
computed with torch on the device), everything is warmed up, then every case
and the yardstick are timed with HIP events in 9 alternating repeats. A
profiled call afterwards gives the per-tag kernel times. Prints one JSON line
per case.

  n in 2^AB_LOG2N (default 26,28)
  layouts  p1000   partitions of 1000 rows (p = i / 1000), peer groups of 4
                   rows (o = i / 4)
           single  one partition over the whole input, the same peer groups
  cases    bounds      window_boundaries over the 2 keys (p, o)
           sum_rows    window_scan SUM(float64), ROWS frame
           sum_range   the same under the RANGE frame (adds the spread pass)
           row_number  window_scan row_number
           shift       window_shift lag 1
           sort        the stable two-key sort that precedes a window node, on
                       unsorted keys of the same cardinalities: two sort_perm
                       passes and the gathers of the other two columns

model_bytes_per_row is the byte model of DESIGN.md "Window (segmented scan)";
ratio = case median / yardstick median, model_ratio = model bytes / 16."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from spark_amd import gpuq as gq

reps = int(os.environ.get("AB_REPS", 9))
log2ns = [int(x) for x in os.environ.get("AB_LOG2N", "26,28").split(",")]
TAGS = ("win_bounds", "win_reduce", "win_carry", "win_apply", "win_spread",
        "win_shift")
PART_ROWS, PEER_ROWS = 1000, 4
MODEL = {"bounds": 16.25, "sum_rows": 24.0, "sum_range": 40.0,
         "row_number": 8.5, "shift": 16.25, "sort": None}


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


def sort_two_keys(pk, ok_, x, ws):
    """what GpuSortExec does for ORDER BY (p, o): stable passes from the last
    key to the first, the other columns gathered through each permutation."""
    perm, o1 = gq.sort_perm(ok_, workspace=ws)
    p1, x1 = gq.gather(pk, perm), gq.gather(x, perm)
    perm, p2 = gq.sort_perm(p1, workspace=ws)
    return p2, gq.gather(o1, perm), gq.gather(x1, perm)


def check(layout, n, x, part, peer, ws):
    """parity first: closed forms of the generated layout."""
    i = gq.range_i64(n)
    begin = (i // PART_ROWS) * PART_ROWS if layout == "p1000" else torch.zeros_like(i)
    rn, _ = gq.window_scan("row_number", "rows", part, peer, n=n, workspace=ws)
    assert torch.equal(rn, i - begin + 1), "row_number"
    del rn
    rows, _ = gq.window_scan("sum", "rows", part, peer, val=x, workspace=ws)
    c = torch.cumsum(x, 0)
    before = torch.where(begin > 0, c[(begin - 1).clamp(min=0)], torch.zeros_like(c))
    torch.testing.assert_close(rows, c - before, rtol=1e-6, atol=1e-6)
    del c, before
    rng, _ = gq.window_scan("sum", "range", part, peer, val=x, workspace=ws)
    last_peer = (i | (PEER_ROWS - 1)).clamp(max=n - 1)    # 1000 % 4 == 0
    assert torch.equal(rng, rows[last_peer]), "sum_range"
    del rng, rows, last_peer
    lag, bits = gq.window_shift(x, -1, part, workspace=ws)
    inside = i > begin
    want = torch.where(inside, x[(i - 1).clamp(min=0)], torch.zeros_like(x))
    assert torch.equal(lag, want), "shift"
    assert torch.equal(gq.bits_to_u8(bits, n).bool(), inside), "shift validity"


for log2n in log2ns:
    n = 1 << log2n
    for layout in ("p1000", "single"):
        i = gq.range_i64(n)
        p = gq.project_binop(i, "/", literal=PART_ROWS) if layout == "p1000" \
            else gq.project_binop(i, "*", literal=0)
        o = gq.project_binop(i, "/", literal=PEER_ROWS)
        del i
        x = gq.gen_f64_unit(seed=91, n=n)
        nparts = max(n // PART_ROWS, 1) if layout == "p1000" else 1
        pk = gq.gen_i64(seed=92, n=n, range_=nparts)
        ok_ = gq.gen_i64(seed=93, n=n, range_=250)
        ws = gq.window_workspace(n)
        sort_ws = gq.sort_workspace(n)
        part, peer = gq.window_boundaries([p, o], None, 1)
        check(layout, n, x, part, peer, ws)
        torch.cuda.empty_cache()

        cases = {
            "bounds": lambda: gq.window_boundaries([p, o], None, 1),
            "sum_rows": lambda: gq.window_scan("sum", "rows", part, peer, val=x,
                                               workspace=ws),
            "sum_range": lambda: gq.window_scan("sum", "range", part, peer, val=x,
                                                workspace=ws),
            "row_number": lambda: gq.window_scan("row_number", "rows", part, peer,
                                                 n=n, workspace=ws),
            "shift": lambda: gq.window_shift(x, -1, part, workspace=ws),
            "sort": lambda: sort_two_keys(pk, ok_, x, sort_ws),
        }
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
                "yardstick_ms": s_yard,
                "ratio": round(s["median"] / s_yard["median"], 2),
                "model_bytes_per_row": MODEL[k],
                "model_ratio": None if MODEL[k] is None else round(MODEL[k] / 16, 2),
                "kernels": tags,
                "device": torch.cuda.get_device_name(0)}), flush=True)
        del p, o, x, pk, ok_, ws, sort_ws, part, peer, cases, yard
        torch.cuda.empty_cache()
