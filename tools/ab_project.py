"""A/B: the fused expression projection (gpuq_project_expr) against the
one-operation-per-call path (gpuq_project_binop_nullable) on device-generated
columns. One process; per point both variants are checked for identical
output first (faster and different is not faster), warmed up, then timed with
HIP events in 9 alternating repeats. A separate profiled call afterwards gives
the kernel time of the new path. Prints one JSON line per point.

  n in 2^AB_LOG2N (default 26,28)
  leaf   one nullable int64 col * literal: project_binop_nullable against
         project_expr, 8 B/row and a bitmap in, the same out
  q1     TPC-H Q1's disc_price = ep * (100 - d) and charge = disc_price *
         (100 + t) with NULLs in t: the three stacked 5-tuple GpuProjectExec
         nodes of bench.py's plan against one node holding both expressions.
         Byte model: about 80 B/row through the four old kernels, 40 B/row
         (three columns in, two out) through the fused one

new_wins is the project's acceptance rule: the new median is below the old
median by more than the larger of the two max-min spreads. The baselines are
the existing kernels in the same process."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from spark_amd import exec as gx
from spark_amd import gpuq as gq
from spark_amd.expression import BinOp, Lit
from spark_amd.predicate import Col

reps = int(os.environ.get("AB_REPS", 9))
log2ns = [int(x) for x in os.environ.get("AB_LOG2N", "26,28").split(",")]
TAGS = ("project_expr",)


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


def same_pair(o, w):
    return torch.equal(o[0], w[0]) and torch.equal(o[1], w[1])


def run_plan(make_plan, cols, validity):
    """execute a project plan over one batch; the batch object is rebuilt per
    run (the node closes its input), the tensors are shared"""
    plan = make_plan(gx.InputBatches(
        [gx.ColumnarBatch(dict(cols), validity=dict(validity))]))
    (out,) = gx.GpuColumnarRule().pre_columnar_transitions(plan).execute_columnar()
    return out


def same_batch(a, b):
    def bits(batch, k):
        return batch.validity(k)

    return list(a.columns()) == list(b.columns()) and all(
        torch.equal(a.column(k), b.column(k))
        and (bits(a, k) is None) == (bits(b, k) is None)
        and (bits(a, k) is None or torch.equal(bits(a, k), bits(b, k)))
        for k in a.columns())


def stacked_q1(child):
    return gx.ProjectExec(
        ["disc_price", ("charge", "disc_price", "*", "__one_plus_tax", None)],
        gx.ProjectExec(
            ["__one_plus_tax",
             ("disc_price", "l_extendedprice", "*", "__one_minus_disc", None)],
            gx.ProjectExec(
                ["l_extendedprice",
                 ("__one_minus_disc", "l_discount", "rsub", None, 100),
                 ("__one_plus_tax", "l_tax", "+", None, 100)], child)))


def fused_q1(child):
    ep, d, t = Col("l_extendedprice"), Col("l_discount"), Col("l_tax")
    return gx.ProjectExec(
        [("disc_price", BinOp("*", ep, BinOp("-", Lit(100), d))),
         ("charge", BinOp("*", BinOp("*", ep, BinOp("-", Lit(100), d)),
                          BinOp("+", Lit(100), t)))], child)


for log2n in log2ns:
    n = 1 << log2n
    # about one NULL row in five, as a bitmap
    null_bits = gq.u8_to_bits((gq.gen_i64(seed=90, n=n, range_=5) != 0)
                              .to(torch.uint8))

    # (a) one nullable leaf
    a = gq.gen_i64(seed=91, n=n, range_=10000000)
    report("leaf", n,
           lambda: gq.project_binop_nullable(a, "*", literal=3,
                                             a_validity=null_bits),
           lambda: gq.project_expr({"a": a}, [("o", BinOp("*", Col("a"), 3))],
                                   validities={"a": null_bits})["o"],
           same_pair, bytes_per_row_old=16.25, bytes_per_row_new=16.25)
    del a
    torch.cuda.empty_cache()

    # (b) Q1's two products through the exec nodes
    cols = {"l_extendedprice": gq.gen_i64(seed=92, n=n, range_=10000000),
            "l_discount": gq.gen_i64(seed=93, n=n, range_=11),
            "l_tax": gq.gen_i64(seed=94, n=n, range_=9)}
    validity = {"l_tax": null_bits}
    report("q1", n,
           lambda: run_plan(stacked_q1, cols, validity),
           lambda: run_plan(fused_q1, cols, validity),
           same_batch, stacked_nodes=3, bytes_per_row_old=80, bytes_per_row_new=40)
    del cols, validity, null_bits
    torch.cuda.empty_cache()
