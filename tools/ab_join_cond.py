"""A/B: the residual join condition evaluated inside the probe
(gpuq_join_probe_keys_cond) against what an INNER join could do before it —
probe every key-equal pair, gather the condition operands through the pair
list, filter, gather the surviving pairs. Inner is the only join type for
which that unfused baseline is correct at all.

tools/ab_filter.py's protocol: one process; per point both variants are
checked for the same pair multiset first (faster and different is not
faster), which is also the warm-up; then 9 alternating repeats timed with
HIP events; a separate profiled call afterwards gives the kernel time under
the join_keys_probe_cond tag. Prints one JSON line per point.

  2-key table over 2^AB_LOG2_BUILD (default 22) build rows, every tuple
  twice; probes of 2^AB_LOG2N (default 24,26) rows, about half of which hit
  a tuple, so a matched probe row has 2 candidates and the key-equal pair
  count is about the probe row count.
  condition probe.x < build.y, both uniform over 1000 values; the windows
  are shifted against each other for pass rates of about 10 %, 50 %, 90 %.

  new  join_probe_keys_cond
  old  join_probe_keys, gather x through op and y through ob, filter_expr,
       gather op and ob through the surviving permutation

uncond_ms is the unconditioned gpuq_join_probe_keys call alone over the same
table and probe rows (the existing path, for comparing two commits); with
AB_UNCOND_ONLY=1 nothing else is measured, which also runs on a checkout
from before the conditioned probe existed.

new_wins is the project's acceptance rule: the new median is below the old
median by more than the larger of the two max-min spreads."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from spark_amd import gpuq as gq  # noqa: E402
from spark_amd.predicate import Cmp, Col  # noqa: E402

reps = int(os.environ.get("AB_REPS", 9))
log2ns = [int(x) for x in os.environ.get("AB_LOG2N", "24,26").split(",")]
nb = 1 << int(os.environ.get("AB_LOG2_BUILD", 22))
uncond_only = os.environ.get("AB_UNCOND_ONLY", "") == "1"
# (x window start, y window start) over windows of 1000 values:
# P(x < y) = (1000 - s)^2 / 2e6 for x shifted up by s, and 1 - that for y
SHIFTS = {"10%": (553, 0), "50%": (0, 0), "90%": (0, 553)}
COND = Cmp("x", "<", Col("y"))


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


def pair_codes(op, ob):
    p = op.to(torch.int64) & 0xFFFFFFFF
    b = ob.to(torch.int64) & 0xFFFFFFFF
    return torch.sort((p << 32) | b).values


def tag_ms(tag):
    ms, cnt = gq.kernel_stats(tag)
    return {"ms": round(ms, 3), "launches": cnt}


assert torch.cuda.is_available(), "ab_join_cond needs a GPU"
cap = 1 << (2 * nb - 1).bit_length()
# every build tuple twice: rows 2t and 2t + 1 carry tuple (t, t mod 1024)
ba = torch.div(gq.range_i64(nb), 2, rounding_mode="floor").contiguous()
bb = (ba % 1024).contiguous()
ws = gq.join_build_keys([ba, bb], cap)

for log2n in log2ns:
    n = 1 << log2n
    # half the probe rows copy a build row's tuple, half miss (a >= nb)
    pick = gq.gen_i64(seed=91, n=n, range_=2 * nb)
    hit = pick < nb
    pa = torch.where(hit, ba[torch.where(hit, pick, torch.zeros_like(pick))],
                     pick).contiguous()
    pb = (pa % 1024).contiguous()
    del pick, hit
    out_cap = n + n // 4 + 64
    keys = [pa, pb]

    def uncond():
        return gq.join_probe_keys(keys, ws, cap, nb, out_cap)

    _, _, ncand = uncond()
    t_un = [timed(uncond)[0] for _ in range(reps)]
    gq.profiling(True)
    gq.kernel_stats_reset()
    uncond()
    torch.cuda.synchronize()
    un_kernel = tag_ms("join_keys_probe")
    gq.profiling(False)
    gq.kernel_stats_reset()
    base = {"rows": n, "build_rows": nb, "candidate_pairs": ncand,
            "reps": reps, "uncond_ms": stats(t_un),
            "uncond_kernel": un_kernel,
            "device": torch.cuda.get_device_name(0)}
    if uncond_only:
        print(json.dumps({"case": "uncond", **base}), flush=True)
        continue

    for rate, (xs, ys) in SHIFTS.items():
        x = (gq.gen_i64(seed=92, n=n, range_=1000) + xs).contiguous()
        y = (gq.gen_i64(seed=93, n=nb, range_=1000) + ys).contiguous()

        def new():
            op, ob, _ = gq.join_probe_keys_cond(keys, ws, cap, nb, out_cap,
                                                COND, {"x": x}, {"y": y})
            return op, ob

        def old():
            op, ob, _ = gq.join_probe_keys(keys, ws, cap, nb, out_cap)
            perm, _ = gq.filter_expr(
                {"x": gq.gather(x, op), "y": gq.gather(y, ob)}, COND)
            return gq.gather(op, perm), gq.gather(ob, perm)

        o, w = old(), new()          # parity first; also the warm-up
        torch.cuda.synchronize()
        npass = w[0].numel()
        assert o[0].numel() == npass, (rate, n)
        assert torch.equal(pair_codes(*o), pair_codes(*w)), (rate, n)
        del o, w
        t_old, t_new = [], []
        for _ in range(reps):        # alternate the variants
            t_old.append(timed(old)[0])
            t_new.append(timed(new)[0])
        gq.profiling(True)
        gq.kernel_stats_reset()
        new()
        torch.cuda.synchronize()
        new_kernel = tag_ms("join_keys_probe_cond")
        gq.profiling(False)
        gq.kernel_stats_reset()
        s_old, s_new = stats(t_old), stats(t_new)
        spread = max(s_old["max"] - s_old["min"], s_new["max"] - s_new["min"])
        print(json.dumps({
            "case": "inner x<y", "target_pass_rate": rate,
            "pass_rate": round(npass / ncand, 3), "passing_pairs": npass,
            "old_ms": s_old, "new_ms": s_new,
            "speedup": round(s_old["median"] / s_new["median"], 2),
            "new_wins": s_new["median"] < s_old["median"] - spread,
            "new_kernel": new_kernel, **base}), flush=True)
        del x, y
        torch.cuda.empty_cache()
    del pa, pb, keys
    torch.cuda.empty_cache()
