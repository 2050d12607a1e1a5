"""A/B: cost of the exact 128-bit decimal SUM (spec ops 8/9, a returning
64-bit atomic plus a rare carry add) against the wrapping SUM(int64) (op 3,
one non-returning atomic) in k_aggm_build, on the same device-generated
rows. Two shapes: 4 groups (the Q1 shape, per-block LDS tables) and 1M
groups (the global table). Kernel time comes from the library's HIP-event
profiling (kernel_stats("aggm_build")); the two variants alternate inside
one process and each is warmed up first. Prints one JSON line per shape."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from spark_amd import gpuq as gq

n = int(os.environ.get("AB_ROWS", 1 << 26))
reps = int(os.environ.get("AB_REPS", 9))
vals = gq.gen_i64(seed=61, n=n)          # full-range int64: lo wraps often
gq.profiling(True)


def build_ms(keys, spec, cap, ws):
    gq.kernel_stats_reset()
    gq.hash_agg_multi(keys, [spec], cap, workspace=ws)
    torch.cuda.synchronize()
    ms, cnt = gq.kernel_stats("aggm_build")
    assert cnt == 1, cnt
    return ms


for label, groups, cap in (("4 groups (LDS)", 4, 1 << 10),
                           ("1M groups (global)", 1 << 20, 1 << 21)):
    keys = gq.gen_i64(seed=62, n=n, range_=groups)
    variants = {"sum_i64": ("sum", vals), "sum_dec128": ("sum_dec128", vals)}
    ws = gq.agg_multi_workspace(cap, 2)
    times = {k: [] for k in variants}
    for k, spec in variants.items():     # warm-up, not timed
        build_ms(keys, spec, cap, ws)
    for _ in range(reps):                # alternate the variants
        for k, spec in variants.items():
            times[k].append(build_ms(keys, spec, cap, ws))
    # parity: the low word of the 128-bit sum is the wrapping int64 sum
    k3, _, a3 = gq.hash_agg_multi(keys, [variants["sum_i64"]], cap, workspace=ws)
    k8, _, a8 = gq.hash_agg_multi(keys, [variants["sum_dec128"]], cap, workspace=ws)
    assert torch.equal(a3[0][torch.argsort(k3)], a8[0][torch.argsort(k8)])
    med = {k: statistics.median(v) for k, v in times.items()}
    print(json.dumps({
        "shape": label, "rows": n, "reps": reps,
        "sum_i64_ms": {"median": round(med["sum_i64"], 3),
                       "min": round(min(times["sum_i64"]), 3),
                       "max": round(max(times["sum_i64"]), 3)},
        "sum_dec128_ms": {"median": round(med["sum_dec128"], 3),
                          "min": round(min(times["sum_dec128"]), 3),
                          "max": round(max(times["sum_dec128"]), 3)},
        "ratio_dec128_over_i64": round(med["sum_dec128"] / med["sum_i64"], 3),
        "device": torch.cuda.get_device_name(0)}), flush=True)
    del keys, ws
