"""A/B: topk_perm (radix select + sort of the k candidates) against the way
the same answer was computed before it existed, sort_perm + head, on the same
device-generated key column. One process; per point both variants are checked
for bit-identical output first (faster and different is not faster), warmed
up, then timed with HIP events in 9 alternating repeats. A separate profiled
call afterwards gives the per-tag kernel times of the select. Prints one JSON
line per point.

  n in 2^AB_LOG2N (default 26,28); full-range int64 and unit-range float64;
  k in {10, 10^3, 2^16, n/64, n/8, n/2}.

select_wins is the acceptance rule of DESIGN.md "Top-K": the select's median
is below the sort's median by more than the larger of the two max-min
spreads."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from spark_amd import gpuq as gq

reps = int(os.environ.get("AB_REPS", 9))
log2ns = [int(x) for x in os.environ.get("AB_LOG2N", "26,28").split(",")]
TAGS = ("topk_hist", "topk_collect", "topk_emit")


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


for log2n in log2ns:
    n = 1 << log2n
    for label, gen in (("i64 full range", lambda: gq.gen_i64(seed=71, n=n)),
                       ("f64 unit range", lambda: gq.gen_f64_unit(seed=72, n=n))):
        keys = gen()
        # the sort's buffers are allocated once, as its large callers do
        ws = gq.sort_workspace(n)
        operm = torch.empty(n, dtype=torch.int32, device="cuda")
        okeys = torch.empty(n, dtype=keys.dtype, device="cuda")

        def by_sort(k):
            perm, skeys = gq.sort_perm(keys, workspace=ws, out_perm=operm,
                                       out_keys=okeys)
            return perm[:k], skeys[:k]

        for k in (10, 1000, 1 << 16, n // 64, n // 8, n // 2):
            def by_select():
                return gq.topk_perm(keys, k)

            # parity first; these two calls are also the warm-up
            ps, ks_ = by_sort(k)
            pt, kt = by_select()
            torch.cuda.synchronize()
            assert torch.equal(pt, ps), (label, n, k)
            assert torch.equal(kt.view(torch.int64), ks_.view(torch.int64)), (label, n, k)
            t_sort, t_sel = [], []
            for _ in range(reps):            # alternate the variants
                t_sort.append(timed(lambda: by_sort(k))[0])
                t_sel.append(timed(by_select)[0])
            gq.profiling(True)
            gq.kernel_stats_reset()
            by_select()
            torch.cuda.synchronize()
            tags = {t: dict(zip(("ms", "launches"),
                                (round(gq.kernel_stats(t)[0], 3), gq.kernel_stats(t)[1])))
                    for t in TAGS}
            gq.profiling(False)
            gq.kernel_stats_reset()
            s_sort, s_sel = stats(t_sort), stats(t_sel)
            spread = max(s_sort["max"] - s_sort["min"], s_sel["max"] - s_sel["min"])
            print(json.dumps({
                "keys": label, "rows": n, "k": k, "k_over_n": k / n, "reps": reps,
                "sort_head_ms": s_sort, "topk_perm_ms": s_sel,
                "speedup": round(s_sort["median"] / s_sel["median"], 2),
                "select_wins": s_sel["median"] < s_sort["median"] - spread,
                "select_kernels": tags,
                "device": torch.cuda.get_device_name(0)}), flush=True)
        del ws, operm, okeys, keys
        torch.cuda.empty_cache()
