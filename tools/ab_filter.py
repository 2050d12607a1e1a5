"""A/B: the fused compound-predicate filter (gpuq_filter_expr) against the
single-comparison path (gpuq_filter_cmp) on device-generated columns. One
process; per point both variants are checked for identical output first
(faster and different is not faster), warmed up, then timed with HIP events
in 9 alternating repeats. A separate profiled call afterwards gives the
per-tag kernel times of the new path. Prints one JSON line per point.

  n in 2^AB_LOG2N (default 26,28)
  leaf   one int64 comparison, k < 500 over k in [0, 1000): filter_cmp against
         filter_expr, the permutation only
  q6x3   shipdate < d1 AND discount >= 0.05 AND quantity < 24, one comparison
         per column: three stacked GpuFilterExec nodes against one condition
         node, gathers of all three columns included
  q6     the whole Q6 filter (shipdate >= d0 AND shipdate < d1 AND discount
         BETWEEN 0.05 AND 0.07 AND quantity < 24): five stacked nodes against
         one condition node, gathers included

new_wins is the project's acceptance rule: the new median is below the old
median by more than the larger of the two max-min spreads."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from spark_amd import exec as gx
from spark_amd import gpuq as gq
from spark_amd.predicate import And, Between, Cmp

reps = int(os.environ.get("AB_REPS", 9))
log2ns = [int(x) for x in os.environ.get("AB_LOG2N", "26,28").split(",")]
TAGS = ("filter_expr_mask", "filter_expr_emit")
D0, D1 = 365, 730


def timed(fn):
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def stats(ts):
    return {"median": round(statistics.median(ts), 3), "min": round(min(ts), 3),
            "max": round(max(ts), 3)}


def report(case, n, old, new, same, **extra):
    o, w = old(), new()              # parity first; also the warm-up
    torch.cuda.synchronize()
    assert same(o, w), (case, n)
    del o, w
    t_old, t_new = [], []
    for _ in range(reps):            # alternate the variants
        t_old.append(timed(old)[0])
        t_new.append(timed(new)[0])
    gq.profiling(True)
    gq.kernel_stats_reset()
    new()
    torch.cuda.synchronize()
    tags = {t: dict(zip(("ms", "launches"),
                        (round(gq.kernel_stats(t)[0], 3), gq.kernel_stats(t)[1])))
            for t in TAGS}
    gq.profiling(False)
    gq.kernel_stats_reset()
    s_old, s_new = stats(t_old), stats(t_new)
    spread = max(s_old["max"] - s_old["min"], s_new["max"] - s_new["min"])
    print(json.dumps({
        "case": case, "rows": n, "reps": reps, "old_ms": s_old, "new_ms": s_new,
        "speedup": round(s_old["median"] / s_new["median"], 2),
        "new_wins": s_new["median"] < s_old["median"] - spread,
        "new_kernels": tags, **extra,
        "device": torch.cuda.get_device_name(0)}), flush=True)


def run_plan(make_plan, cols):
    """execute a filter plan over one batch of `cols`; the batch object is
    rebuilt per run (the filter closes its input), the tensors are shared"""
    plan = make_plan(gx.InputBatches([gx.ColumnarBatch(dict(cols))]))
    (out,) = gx.GpuColumnarRule().pre_columnar_transitions(plan).execute_columnar()
    return out


def same_batch(a, b):
    return a.num_rows() == b.num_rows() and all(
        torch.equal(a.column(k).view(torch.int64), b.column(k).view(torch.int64))
        for k in a.columns())


for log2n in log2ns:
    n = 1 << log2n

    # (a) single int64 leaf, permutation only; workspaces allocated once
    k = gq.gen_i64(seed=81, n=n, range_=1000)
    ws_old = torch.empty(gq.lib().gpuq_filter_workspace_bytes(n),
                         dtype=torch.uint8, device="cuda")
    ws_new = gq.filter_expr_workspace(n)
    report("leaf", n,
           lambda: gq.filter_cmp(k, "<", 500, workspace=ws_old),
           lambda: gq.filter_expr({"k": k}, Cmp("k", "<", 500), workspace=ws_new),
           lambda o, w: o[1] == w[1] and torch.equal(o[0], w[0]),
           selectivity=0.5)
    del k, ws_old, ws_new
    torch.cuda.empty_cache()

    # (b) Q6 shape over three columns, through the exec nodes
    cols = {
        "l_shipdate": gq.gen_i64(seed=82, n=n, range_=2556),
        "l_discount": gq.project_binop(gq.gen_f64_unit(seed=83, n=n), "*",
                                       literal=0.1),
        "l_quantity": gq.project_binop(gq.gen_f64_unit(seed=84, n=n), "*",
                                       literal=50.0),
    }
    report("q6x3", n,
           lambda: run_plan(lambda c: gx.FilterExec(
               "l_quantity", "<", 24.0, gx.FilterExec(
                   "l_discount", ">=", 0.05, gx.FilterExec(
                       "l_shipdate", "<", D1, c))), cols),
           lambda: run_plan(lambda c: gx.FilterExec(
               And(Cmp("l_shipdate", "<", D1), Cmp("l_discount", ">=", 0.05),
                   Cmp("l_quantity", "<", 24.0)), c), cols),
           same_batch, stacked_nodes=3)
    report("q6", n,
           lambda: run_plan(lambda c: gx.FilterExec(
               "l_quantity", "<", 24.0, gx.FilterExec(
                   "l_discount", "<=", 0.07, gx.FilterExec(
                       "l_discount", ">=", 0.05, gx.FilterExec(
                           "l_shipdate", "<", D1, gx.FilterExec(
                               "l_shipdate", ">=", D0, c))))), cols),
           lambda: run_plan(lambda c: gx.FilterExec(
               And(Cmp("l_shipdate", ">=", D0), Cmp("l_shipdate", "<", D1),
                   Between("l_discount", 0.05, 0.07),
                   Cmp("l_quantity", "<", 24.0)), c), cols),
           same_batch, stacked_nodes=5)
    del cols
    torch.cuda.empty_cache()
