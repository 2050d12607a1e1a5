"""A/B: 2-key inner join through the composite-key table
(gpuq_join_build_keys / gpuq_join_probe_keys) versus what a user had before
it — pack the two keys with gpuq_pack2_i64 and run the single-key join —
over the SAME rows, on the same device, in the same run, alternating.

Kernel times are the engine's own HIP-event stats (gpuq_kernel_stats tags
join_keys_build / join_keys_probe vs join_build / join_probe, one sample per
repetition); call times are a host clock around calls that end in a device
synchronise (both probe entry points read the match count back). Both
variants are warmed first, and the pair multisets are compared at the timed
size before any number is reported. Needs a GPU: there is no fallback.

    python tools/bench_join_keys.py [--build-rows N] [--probe-rows N] [--reps R]

Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from spark_amd import gpuq as gq  # noqa: E402

A_BITS, B_BITS = 22, 10     # key column ranges; the packed key fits 32 bits


def make_rows(nb, npr):
    """build: random (a, b) tuples; probe: ~half drawn from the build rows
    (they match), ~half fresh random tuples (almost all miss)."""
    ba = gq.gen_i64(seed=71, n=nb, range_=1 << A_BITS)
    bb = gq.gen_i64(seed=72, n=nb, range_=1 << B_BITS)
    pick = gq.gen_i64(seed=73, n=npr, range_=2 * nb)
    hit = pick < nb
    src = torch.where(hit, pick, torch.zeros_like(pick))
    pa = torch.where(hit, ba[src], gq.gen_i64(seed=74, n=npr, range_=1 << A_BITS))
    pb = torch.where(hit, bb[src], gq.gen_i64(seed=75, n=npr, range_=1 << B_BITS))
    return ba, bb, pa.contiguous(), pb.contiguous()


def pair_codes(op, ob):
    p = op.to(torch.int64) & 0xFFFFFFFF
    b = ob.to(torch.int64) & 0xFFFFFFFF
    return torch.sort((p << 32) | b).values


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build-rows", type=int, default=1 << 21)
    ap.add_argument("--probe-rows", type=int, default=1 << 23)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_join_keys needs a GPU"
    nb, npr = args.build_rows, args.probe_rows
    cap = 1 << (2 * nb - 1).bit_length()
    ba, bb, pa, pb = make_rows(nb, npr)
    out_cap = 2 * npr + 64

    ws_k = torch.empty(gq.lib().gpuq_join_keys_workspace_bytes(nb, cap, 2),
                       dtype=torch.uint8, device="cuda")
    ws_1 = torch.empty(gq.lib().gpuq_join_build_workspace_bytes(nb, cap),
                       dtype=torch.uint8, device="cuda")

    def composite():
        t0 = time.perf_counter()
        gq.join_build_keys([ba, bb], cap, workspace=ws_k)
        op, ob, n = gq.join_probe_keys([pa, pb], ws_k, cap, nb, out_cap)
        return time.perf_counter() - t0, op, ob, n

    def packed():
        t0 = time.perf_counter()
        kb = gq.pack2_i64(ba, bb, 0, 0, B_BITS)
        kp = gq.pack2_i64(pa, pb, 0, 0, B_BITS)
        gq.join_build(kb, cap, workspace=ws_1)
        op, ob, n = gq.join_probe(kp, ws_1, cap, nb, out_cap)
        return time.perf_counter() - t0, op, ob, n

    # warm-up + parity at the timed size
    _, op_k, ob_k, n_k = composite()
    _, op_1, ob_1, n_1 = packed()
    assert op_k is not None and op_1 is not None, "out_cap too small"
    assert n_k == n_1, (n_k, n_1)
    assert torch.equal(pair_codes(op_k, ob_k), pair_codes(op_1, ob_1))
    del op_k, ob_k, op_1, ob_1

    tags = ["join_keys_build", "join_keys_probe", "join_build", "join_probe"]
    samples = {t: [] for t in tags}
    calls = {"composite": [], "packed": []}
    gq.profiling(True)
    for _ in range(args.reps):       # alternate the two variants
        for name, fn in (("composite", composite), ("packed", packed)):
            gq.kernel_stats_reset()
            dt, _, _, _ = fn()
            torch.cuda.synchronize()
            calls[name].append(dt * 1e3)
            for t in tags:
                ms, cnt = gq.kernel_stats(t)
                if cnt:
                    samples[t].append(ms / cnt)
    gq.profiling(False)

    def summary(xs):
        return {"median_ms": round(statistics.median(xs), 4),
                "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4)}

    res = {"device": torch.cuda.get_device_name(0), "build_rows": nb,
           "probe_rows": npr, "capacity": cap, "matches": n_k,
           "reps": args.reps,
           "kernels": {t: summary(samples[t]) for t in tags},
           "calls": {k: summary(v) for k, v in calls.items()}}
    med = lambda t: statistics.median(samples[t])
    res["probe_ratio_composite_over_packed"] = round(
        med("join_keys_probe") / med("join_probe"), 3)
    res["build_ratio_composite_over_packed"] = round(
        med("join_keys_build") / med("join_build"), 3)
    res["call_ratio_composite_over_packed"] = round(
        statistics.median(calls["composite"]) / statistics.median(calls["packed"]), 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
