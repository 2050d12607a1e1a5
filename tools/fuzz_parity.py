"""Randomized GPU-vs-oracle parity fuzz: random shapes, ranges, descs,
validity patterns across sort/partition/agg/join and the filter/project
kernels (the latter against tests/expr_ref.py). Seeded per iteration and
bounded by FUZZ_SECONDS (default 240)."""
import os, sys, time
_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _ROOT)
sys.path.insert(0, os.path.join(_ROOT, "tests"))
import numpy as np
import torch
import oracle
import expr_ref
from spark_amd import gpuq as gq

BUDGET = float(os.environ.get("FUZZ_SECONDS", 240))
rng = np.random.default_rng(int(os.environ.get("FUZZ_SEED", 0)))
t_end = time.time() + BUDGET
it = 0
fails = 0

def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()

# filter/project sizes: the bitmap-byte, block, compaction-tile and grid-cap
# boundaries, or a random n <= 200 000 (the reference is row-by-row Python)
EXPR_SIZES = [0, 1, 7, 8, 9, 255, 256, 257, 5631, 5632, 5633, 11265,
              524288 + 257]
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1

def expr_n():
    if rng.integers(2):
        return int(rng.choice(EXPR_SIZES))
    return int(rng.integers(0, 200_001))

def expr_valid(n):
    """None, or a bool mask with a random NULL density"""
    if rng.integers(3) == 0:
        return None, None
    valid = rng.random(n) >= rng.random()
    return valid, torch.from_numpy(np.packbits(valid, bitorder="little")).cuda()

def unpack(bits, n):
    return np.unpackbits(bits.cpu().numpy(), bitorder="little")[:n].astype(bool)

def same_values(got, exp, valid):
    g, e = got[valid], exp[valid]
    if got.dtype == np.float64:
        return bool(((g.view(np.uint64) == e.view(np.uint64))
                     | (np.isnan(g) & np.isnan(e))).all())
    return bool((g == e).all())

while time.time() < t_end:
    it += 1
    op = rng.choice(["sort_i64", "sort_f64", "sort_nulls", "partition",
                     "agg", "join", "minmax_agg", "composite_agg",
                     "typed_join", "partition_multi",
                     "filter_i64", "filter_f64", "project"])
    n = int(rng.integers(1, 3_000_000))
    seed = int(rng.integers(0, 2**31))
    try:
        if op == "filter_i64":
            n = expr_n()
            r = int(rng.choice([3, 7, 1000]))
            vals = rng.integers(-r, r + 1, size=n, dtype=np.int64)
            if n and rng.integers(2):
                vals[:: max(1, n // 40)] = rng.choice([I64_MIN, I64_MAX])
            cmp_ = str(rng.choice(expr_ref.CMP_OPS))
            lit = [0, 1, -r, r, I64_MIN, I64_MAX, 0.5, -1.5, 2.0, 1e30,
                   float("inf"), float("-inf"), float("nan")][int(rng.integers(13))]
            valid, vb = expr_valid(n)
            if valid is not None and not isinstance(lit, float):
                vals[~valid] = lit
            perm, cnt = gq.filter_cmp(dev(vals), cmp_, lit, validity=vb)
            exp = expr_ref.ref_filter(vals, valid, cmp_, lit, "i64")
            assert cnt == len(exp)
            assert (perm.cpu().numpy().view(np.uint32) == exp).all()
        elif op == "filter_f64":
            n = expr_n()
            vals = rng.random(n) * 2 - 1
            if n:
                for sp in (0.0, -0.0, np.nan, np.inf, -np.inf, 0.5):
                    vals[int(rng.integers(n)):: int(rng.integers(5, 60))] = sp
            cmp_ = str(rng.choice(expr_ref.CMP_OPS))
            lit = [0.5, 0.0, -0.0, float("inf"), float("-inf"), float("nan"),
                   float(rng.random() * 2 - 1)][int(rng.integers(7))]
            valid, vb = expr_valid(n)
            perm, cnt = gq.filter_cmp(dev(vals), cmp_, lit, validity=vb)
            exp = expr_ref.ref_filter(vals, valid, cmp_, lit, "f64")
            assert cnt == len(exp)
            assert (perm.cpu().numpy().view(np.uint32) == exp).all()
        elif op == "project":
            n = expr_n()
            dt = str(rng.choice(["i64", "f64"]))
            bop = str(rng.choice(expr_ref.BIN_OPS))
            if dt == "i64":
                a = rng.integers(-100, 101, size=n, dtype=np.int64)
                b = rng.integers(-10, 11, size=n, dtype=np.int64)
                specials = [I64_MIN, I64_MAX, -1, 0, 2]
                lit = int(rng.choice([-1, 0, 3, 100])) if rng.integers(4) \
                    else [I64_MIN, I64_MAX][int(rng.integers(2))]
            else:
                a = rng.random(n) * 200 - 100
                b = rng.random(n) * 20 - 10
                specials = [0.0, -0.0, np.inf, -np.inf, np.nan, 5e-324]
                lit = [2.5, 0.0, -0.0, float("inf"), float("nan"),
                       5e-324][int(rng.integers(6))]
            if n:
                for sp in specials:
                    a[int(rng.integers(n)):: int(rng.integers(5, 60))] = sp
                    b[int(rng.integers(n)):: int(rng.integers(5, 60))] = sp
            av, avb = expr_valid(n)
            if av is not None:
                a[~av] = specials[0]
            if rng.integers(2):          # column-column
                bv, bvb = expr_valid(n)
                if bv is not None:
                    b[~bv] = 0
                out, bits = gq.project_binop_nullable(
                    dev(a), bop, b=dev(b), a_validity=avb, b_validity=bvb)
                ev, evalid = expr_ref.ref_binop(a, av, bop, b, bv, dt)
                nullable = av is not None or bv is not None or bop == "/"
            else:                        # column-literal
                out, bits = gq.project_binop_nullable(
                    dev(a), bop, literal=lit, a_validity=avb)
                ev, evalid = expr_ref.ref_binop(a, av, bop, lit, None, dt)
                nullable = av is not None or bop == "/"
            assert (bits is not None) == nullable
            if bits is not None:
                assert (unpack(bits, n) == evalid).all()
            else:
                assert evalid.all()
            assert same_values(out.cpu().numpy(), ev, evalid)
        elif op == "sort_i64":
            r = int(rng.choice([0, 1, 10, 1000, 10**6, 2**62]))
            keys = oracle.gen_i64(seed, n, range_=r)
            desc = bool(rng.integers(2))
            perm, skeys = gq.sort_perm(dev(keys), desc=desc)
            exp = oracle.sort_perm(keys, desc=desc)
            assert (perm.cpu().numpy().astype(np.uint32) == exp.astype(np.uint32)).all()
            assert (skeys.cpu().numpy() == keys[exp]).all()
        elif op == "sort_f64":
            keys = oracle.gen_f64_unit(seed, n)
            if n > 10:
                keys[:: max(1, n // 50)] = rng.choice([np.nan, np.inf, -np.inf, -0.0, 0.0])
            desc = bool(rng.integers(2))
            perm, _ = gq.sort_perm(dev(keys), desc=desc)
            exp = oracle.sort_perm(keys, desc=desc)
            assert (perm.cpu().numpy().astype(np.uint32) == exp.astype(np.uint32)).all()
        elif op == "sort_nulls":
            keys = oracle.gen_i64(seed, n, range_=max(1, n // 10))
            valid = rng.random(n) > rng.random() * 0.9
            vb = np.packbits(valid, bitorder="little")
            desc = bool(rng.integers(2))
            perm, _ = gq.sort_perm(dev(keys), desc=desc,
                                   key_validity=torch.from_numpy(vb).cuda())
            exp = oracle.sort_perm(keys, desc=desc, validity=vb)
            assert (perm.cpu().numpy().astype(np.uint32) == exp.astype(np.uint32)).all()
        elif op == "partition":
            nparts = int(rng.choice([1, 2, 7, 8, 200, 256, 1000, 65536]))
            keys = oracle.gen_i64(seed, n)
            perm, counts = gq.partition_perm(dev(keys), nparts)
            pids = oracle.partition_ids(keys, nparts)
            assert (counts.cpu().numpy() == np.bincount(pids, minlength=nparts)).all()
            assert (perm.cpu().numpy().astype(np.uint32)
                    == np.argsort(pids, kind="stable").astype(np.uint32)).all()
        elif op == "agg":
            groups = int(rng.integers(1, max(2, n // 2)))
            keys = oracle.gen_i64(seed, n, range_=groups)
            if rng.integers(4) == 0:
                keys[:: max(1, n // 17)] = -1
            vals = oracle.gen_f64_unit(seed + 1, n)
            cap = 1 << max(4, int(groups * 2 + 2).bit_length())
            gk, gkv, gs, gsv, gc = (t.cpu().numpy() for t in
                                    gq.hash_agg(dev(keys), dev(vals), cap))
            ok, okv, osum, osv, ocnt = oracle.hash_agg(keys, vals)
            g, o = np.lexsort((gk, gkv)), np.lexsort((ok, okv))
            assert (gk[g] == ok[o]).all() and (gc[g] == ocnt[o]).all()
            np.testing.assert_allclose(gs[g], osum[o], rtol=1e-6)
        elif op == "join":
            bn = int(rng.integers(1, max(2, n)))
            r = max(1, int(rng.integers(1, 2 * n)))
            bkeys = oracle.gen_i64(seed, bn, range_=r)
            pkeys = oracle.gen_i64(seed + 1, n, range_=r)
            cap = 1 << max(4, int(bn * 2 + 2).bit_length())
            ws = gq.join_build(dev(bkeys), cap)
            op_o, ob_o = oracle.join_inner(bkeys, pkeys)
            gp, gb, nm = gq.join_probe(dev(pkeys), ws, cap, bn, len(op_o) + 64)
            assert nm == len(op_o)
            g = np.lexsort((gb.cpu().numpy(), gp.cpu().numpy()))
            o = np.lexsort((ob_o, op_o))
            assert (gp.cpu().numpy()[g] == op_o[o]).all()
            assert (gb.cpu().numpy()[g] == ob_o[o]).all()
        elif op == "minmax_agg":
            groups = int(rng.integers(1, max(2, n // 2)))
            keys = oracle.gen_i64(seed, n, range_=groups)
            vals = oracle.gen_i64(seed + 1, n)
            valid = rng.random(n) > rng.random() * 0.8
            vb = torch.from_numpy(np.packbits(valid, bitorder="little")).cuda()
            cap = 1 << max(4, int(groups * 2 + 2).bit_length())
            ok_, okv_, accs = gq.hash_agg_multi(
                dev(keys), [("min", dev(vals), vb), ("max", dev(vals), vb),
                            ("count", dev(vals), vb)], cap)
            gk = ok_.cpu().numpy()
            gmin, gmax, gcnt = (t.cpu().numpy() for t in accs)
            ref = {}
            for i in range(n):
                ref.setdefault(int(keys[i]), []).append(i)
            assert len(gk) == len(ref)
            for j, k in enumerate(gk):
                vv = [vals[i] for i in ref[int(k)] if valid[i]]
                assert gcnt[j] == len(vv)
                if vv:
                    assert gmin[j] == min(vv) and gmax[j] == max(vv)
        elif op == "composite_agg":
            g1 = int(rng.integers(1, 100))
            g2 = int(rng.integers(1, 100))
            k1 = oracle.gen_i64(seed, n, range_=g1)
            k2 = oracle.gen_i64(seed + 1, n, range_=g2)
            vals = oracle.gen_f64_unit(seed + 2, n)
            cap = 1 << max(6, int(g1 * g2 * 2 + 2).bit_length())
            okeys, kmask, accs = gq.hash_agg_keys(
                [dev(k1), dev(k2)], [("sum", dev(vals), None), ("count*",)],
                cap)
            ref = {}
            for i in range(n):
                t_ = (int(k1[i]), int(k2[i]))
                ref.setdefault(t_, [0.0, 0])
                ref[t_][0] += vals[i]
                ref[t_][1] += 1
            a1, a2 = okeys[0].cpu().numpy(), okeys[1].cpu().numpy()
            gs_, gc_ = accs[0].cpu().numpy(), accs[1].cpu().numpy()
            assert len(a1) == len(ref)
            for j in range(len(a1)):
                s, c = ref[(int(a1[j]), int(a2[j]))]
                assert gc_[j] == c
                np.testing.assert_allclose(gs_[j], s, rtol=1e-6)
        elif op == "typed_join":
            jt = int(rng.choice([1, 2, 3]))
            bn = int(rng.integers(1, max(2, n)))
            r = max(1, int(rng.integers(1, 2 * n)))
            bkeys = oracle.gen_i64(seed, bn, range_=r)
            pkeys = oracle.gen_i64(seed + 1, n, range_=r)
            cap = 1 << max(4, int(bn * 2 + 2).bit_length())
            ws = gq.join_build(dev(bkeys), cap)
            bset = set(bkeys.tolist())
            from collections import Counter
            bc = Counter(bkeys.tolist())
            if jt == 1:       # outer: matches + 1 per unmatched probe row
                exp_n = sum(bc.get(int(k), 0) or 1 for k in pkeys)
            elif jt == 2:     # semi
                exp_n = sum(1 for k in pkeys if int(k) in bset)
            else:             # anti
                exp_n = sum(1 for k in pkeys if int(k) not in bset)
            if exp_n > 20_000_000:
                continue   # skip pathological cross products (alloc bound)
            gp, gb, nm = gq.join_probe(dev(pkeys), ws, cap, bn,
                                       exp_n + 64, join_type=jt)
            assert nm == exp_n
        else:  # partition_multi
            nparts = int(rng.choice([1, 2, 8, 200]))
            k1 = oracle.gen_i64(seed, n)
            k2 = oracle.gen_i64(seed + 1, n, range_=100)
            perm, counts = gq.partition_perm_multi([dev(k1), dev(k2)], nparts)
            ones = np.packbits(np.ones(n, dtype=bool), bitorder="little")
            pids = oracle.partition_ids_multi(
                [k1, k2], nparts, validity=np.stack([ones, ones]))
            assert (counts.cpu().numpy()
                    == np.bincount(pids, minlength=nparts)).all()
            assert (perm.cpu().numpy().astype(np.uint32)
                    == np.argsort(pids, kind="stable").astype(np.uint32)).all()
    except AssertionError:
        fails += 1
        print(f"FAIL it={it} op={op} n={n} seed={seed}", flush=True)
        if fails > 3:
            raise
print(f"fuzz done: {it} iterations, {fails} failures", flush=True)
assert fails == 0
