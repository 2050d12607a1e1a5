#!/usr/bin/env python3
"""bench.py — measures the GPU engine on BASELINE.json's workloads.

Primary line (N=1 default): config 2 — ORDER BY int64 key on 1B rows x 3 cols
(int64 key, int64, float64) on one MI355X, whole-operator rows/s with inputs
resident in HBM. A plain run does that and nothing else: set up, warm up,
time --steps steps, print one JSON line. --dump-outputs DIR also writes what
the last timed step produced (seeded sample, float64 .npy) so two builds can
be compared output for output.

--full adds, in the same JSON line, the sub-benchmarks — config 3 (GROUP BY
1B rows / 10M groups, SUM float64), config 4 scaled per GPU (shuffled hash
join, 0.5B rows/side/GPU; at N>1 the real RCCL all-to-all exchange runs) and
the config-5 Q1/Q3 plans — and the CPU baseline.

N>1 (launched by the driver via torch.distributed.run): sort and agg run as
independent per-rank batches (weak scaling — config 2/3 are single-partition
operators; the cross-GPU exchange lives in the join workload); the join
partitions + all-to-all exchanges + joins across all N ranks.

Roofline: per-kernel HIP events (gpuq_profiling) on the launching stream give
the dominant kernel's (radix_scatter) average launch time; achieved =
algorithmic bytes/launch / time. PMC traffic comes from rocprofv3 runs
committed under profiles/ (null here).

CPU baseline: the C oracle (kind "port", single thread) timed on this box's
host cores over a bounded sample of the same workload — a reported baseline,
not the target.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

PEAK_HBM_GBPS = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md)


def env_rank():
    return int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1")), \
        int(os.environ.get("LOCAL_RANK", "0"))


def dist_setup():
    rank, world, local = env_rank()
    if os.environ.get("GPUQ_FORCE_DEV0"):   # single-GPU multi-rank debug
        local = 0
    torch.cuda.set_device(local if world > 1 else 0)
    if world > 1:
        import torch.distributed as dist
        if not dist.is_initialized():
            # nccl backend IS RCCL on ROCm; device set first so the
            # communicator binds this rank's GPU
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    return rank, world, local


def barrier_sync(world):
    torch.cuda.synchronize()
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        torch.cuda.synchronize()


def max_over_ranks(x: float, world) -> float:
    if world == 1:
        return x
    import torch.distributed as dist
    t = torch.tensor([x], dtype=torch.float64, device="cuda")
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


# ---------------- workloads ----------------

class SortWorkload:
    """Config 2: ORDER BY int64 key, rows x (i64 key, i64, f64), 1 partition."""

    def __init__(self, gq, rows, rank):
        self.gq, self.rows = gq, rows
        seed_off = rank * 3
        self.keys = gq.gen_i64(seed=42 + seed_off, n=rows)          # full-range int64
        self.pay1 = gq.gen_i64(seed=43 + seed_off, n=rows)
        self.pay2 = gq.gen_f64_unit(seed=44 + seed_off, n=rows)
        self.ws = gq.sort_workspace(rows)
        self.out1 = torch.empty(rows, dtype=torch.int64, device="cuda")
        self.out2 = torch.empty(rows, dtype=torch.float64, device="cuda")
        self.perm = torch.empty(rows, dtype=torch.int32, device="cuda")
        self.skeys = torch.empty(rows, dtype=torch.int64, device="cuda")
        self.pair_scratch = torch.empty(rows * 2, dtype=torch.int64,
                                        device="cuda")

    def step(self):
        gq = self.gq
        # the payload interleave depends only on the input columns, not on
        # the sort — run it on a SIDE stream concurrently with the radix
        # passes (it is still inside the timed step; it just overlaps)
        if not hasattr(self, "_side"):
            self._side = torch.cuda.Stream()
        ev = torch.cuda.Event()
        # the scratch is read by the previous step's gather on the main
        # stream — order the side-stream rewrite after it
        self._side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(self._side):
            gq._check(gq.lib().gpuq_interleave2_i64(
                torch.cuda.current_stream().cuda_stream, self.rows,
                self.pay1.data_ptr(), self.pay2.data_ptr(),
                self.pair_scratch.data_ptr()))
            ev.record(self._side)
        perm, skeys = gq.sort_perm(self.keys, workspace=self.ws,
                                   out_perm=self.perm, out_keys=self.skeys)
        torch.cuda.current_stream().wait_event(ev)
        # interleaved-pair payload gather: one random b128 load per row
        # serves both payload columns
        gq._check(gq.lib().gpuq_gather2_pairs(
            gq._stream(), self.rows, self.pair_scratch.data_ptr(),
            perm.data_ptr(), self.out1.data_ptr(), self.out2.data_ptr()))

    def free(self):
        del self.keys, self.pay1, self.pay2, self.ws, self.out1, self.out2, \
            self.perm, self.skeys, self.pair_scratch


class AggWorkload:
    """Config 3: GROUP BY int64 key (10M distinct), SUM(float64)."""

    def __init__(self, gq, rows, groups, rank):
        self.gq, self.rows = gq, rows
        self.cap = 1 << max(4, (groups * 2 - 1).bit_length())
        seed_off = rank * 3
        self.keys = gq.gen_i64(seed=52 + seed_off, n=rows, range_=groups)
        self.vals = gq.gen_f64_unit(seed=53 + seed_off, n=rows)
        self.ws = gq.agg_workspace(self.cap)
        mg = groups + 2
        self.outs = [torch.empty(mg, dtype=d, device="cuda")
                     for d in (torch.int64, torch.uint8, torch.float64,
                               torch.uint8, torch.int64)]

    def step(self):
        import ctypes
        gq = self.gq
        ng = ctypes.c_int64(0)
        if os.environ.get("GPUQ_PART_AGG"):
            if not hasattr(self, "pws"):
                self.pws = torch.empty(
                    gq.lib().gpuq_hash_agg_part_workspace_bytes(self.rows, self.cap),
                    dtype=torch.uint8, device="cuda")
            rc = gq.lib().gpuq_hash_agg_partitioned(
                gq._stream(), self.rows, gq._col(self.keys), gq._col(self.vals),
                self.pws.data_ptr(), self.cap, 1,
                *[t.data_ptr() for t in self.outs], ctypes.byref(ng))
        else:
            rc = gq.lib().gpuq_hash_agg_i64_f64(
                gq._stream(), self.rows, gq._col(self.keys), gq._col(self.vals),
                self.ws.data_ptr(), self.cap, 1, 1, 1,  # ops=SUM (config 3 shape)
                *[t.data_ptr() for t in self.outs], ctypes.byref(ng))
        gq._check(rc)
        self.ngroups = ng.value

    def free(self):
        del self.keys, self.vals, self.ws, self.outs


class JoinWorkload:
    """Config 4 per-GPU slice: shuffled hash join of two tables,
    rows_per_gpu per side per rank, int64 keys uniform over world*rows space
    (~matching rate of the 4B x 4B config), one int64 payload each.
    At world>1: radix-partition by Pmod(Murmur3,world) + RCCL all-to-all,
    then local build+probe — the real exchange path."""

    def __init__(self, gq, rows, rank, world):
        self.gq, self.rows, self.world, self.rank = gq, rows, world, rank
        keyspace = rows * world
        self.bkeys = gq.gen_i64(seed=62, n=rows, range_=keyspace, start=rank * rows)
        self.bpay = gq.gen_i64(seed=63, n=rows, range_=0, start=rank * rows)
        self.pkeys = gq.gen_i64(seed=64, n=rows, range_=keyspace, start=rank * rows)
        self.ppay = gq.gen_i64(seed=65, n=rows, range_=0, start=rank * rows)
        self.part_ws = gq.partition_workspace(rows, world) if world > 1 else None
        # after exchange each rank holds ~rows per side (margin 1.25x)
        self.local_cap_rows = int(rows * 1.25) + 4096
        # ~0.6 max load factor: linear probing stays short, table stays small
        self.cap = 1 << max(4, int(self.local_cap_rows * 1.6 - 1).bit_length())
        self.join_ws = torch.empty(
            gq.lib().gpuq_join_build_workspace_bytes(self.local_cap_rows, self.cap),
            dtype=torch.uint8, device="cuda")
        self.probe_ws = None  # hash-order probe bucketing is opt-in (see gpuq.hip)
        self.out_cap = int(rows * 2.5) + 4096
        self.nmatches = 0

    def _exchange(self, keys, pay):
        """partition by murmur3 pmod(world) + all_to_all; returns local cols."""
        gq = self.gq
        if self.world == 1:
            return keys, pay
        import torch.distributed as dist
        perm, counts = gq.partition_perm(keys, self.world, workspace=self.part_ws)
        pk = gq.gather(keys, perm)
        pp = gq.gather(pay, perm)
        in_splits = counts.cpu().tolist()
        out_counts = torch.empty(self.world, dtype=torch.int64, device="cuda")
        dist.all_to_all_single(out_counts, counts)
        out_splits = out_counts.cpu().tolist()
        total = sum(out_splits)
        rk = torch.empty(total, dtype=torch.int64, device="cuda")
        rp = torch.empty(total, dtype=torch.int64, device="cuda")
        dist.all_to_all_single(rk, pk, out_splits, in_splits)
        dist.all_to_all_single(rp, pp, out_splits, in_splits)
        return rk, rp

    def _exchange_tiled(self, sides, ntiles=4):
        """Overlapped exchange (north star: the all-to-all rides a side HIP
        stream, overlapped with the partition kernel): each table side is
        split into tiles; tile i's RCCL all-to-all runs on the comm stream
        while tile i+1 is partitioned + gathered on the compute stream.
        Join semantics don't depend on row order, so per-tile arrival
        order is free concat fodder."""
        gq = self.gq
        import torch.distributed as dist
        if not hasattr(self, "_comm_stream"):
            self._comm_stream = torch.cuda.Stream()
        comm = self._comm_stream
        compute = torch.cuda.current_stream()
        recv = [[] for _ in sides]
        jobs = []
        for si, (keys, pay) in enumerate(sides):
            n = keys.numel()
            step = (n + ntiles - 1) // ntiles
            for t0 in range(0, n, step):
                jobs.append((si, keys[t0:t0 + step], pay[t0:t0 + step]))
        out_counts = torch.empty(self.world, dtype=torch.int64, device="cuda")
        for si, k, p in jobs:
            # compute stream: partition + gather THIS tile (overlaps the
            # previous tile's data all-to-all already queued on `comm`)
            perm, counts = gq.partition_perm(k, self.world)
            pk = gq.gather(k, perm)
            pp = gq.gather(p, perm)
            # these tensors are consumed by the comm stream after their
            # python refs drop next iteration — pin them in the caching
            # allocator against compute-stream reuse until comm is done
            pk.record_stream(comm)
            pp.record_stream(comm)
            counts.record_stream(comm)
            ev = torch.cuda.Event()
            ev.record(compute)
            in_splits = counts.cpu().tolist()
            with torch.cuda.stream(comm):
                comm.wait_event(ev)
                dist.all_to_all_single(out_counts, counts)
                out_splits = out_counts.cpu().tolist()
                total = sum(out_splits)
                rk = torch.empty(total, dtype=torch.int64, device="cuda")
                rp = torch.empty(total, dtype=torch.int64, device="cuda")
                dist.all_to_all_single(rk, pk, out_splits, in_splits)
                dist.all_to_all_single(rp, pp, out_splits, in_splits)
            recv[si].append((rk, rp))
        compute.wait_stream(comm)
        out = []
        for parts in recv:
            out.append((torch.cat([a for a, _ in parts]),
                        torch.cat([b for _, b in parts])))
        return out

    def step(self):
        gq = self.gq
        if self.world > 1 and not os.environ.get("GPUQ_NO_OVERLAP"):
            (bk, bp), (pk, pp) = self._exchange_tiled(
                [(self.bkeys, self.bpay), (self.pkeys, self.ppay)])
        else:
            bk, bp = self._exchange(self.bkeys, self.bpay)
            pk, pp = self._exchange(self.pkeys, self.ppay)
        bn = bk.numel()
        gq.lib().gpuq_join_build_i64(gq._stream(), bn, gq._col(bk),
                                     self.join_ws.data_ptr(), self.cap)
        op, ob, nm = gq.join_probe(pk, self.join_ws, self.cap, bn, self.out_cap,
                                   probe_ws=self.probe_ws)
        assert op is not None, f"join out_cap {self.out_cap} < {nm}"
        # materialize one payload column per side (what SHJ emits)
        gq.gather(bp, ob)
        gq.gather(pp, op)
        self.nmatches = nm

    def free(self):
        del self.bkeys, self.bpay, self.pkeys, self.ppay, self.part_ws, self.join_ws, self.probe_ws


class GlobalSortWorkload:
    """Config-2 extended to N GPUs: global ORDER BY via the range exchange
    (sampled bounds -> range partition -> RCCL all-to-all -> local sort);
    rank-major order is the global sort order. Only meaningful at world>1."""

    def __init__(self, gq, rows, rank, world):
        self.gq, self.rows, self.world = gq, rows, world
        self.keys = gq.gen_i64(seed=142, n=rows, start=rank * rows)
        self.pay = gq.gen_i64(seed=143, n=rows, start=rank * rows)
        self.nrows_local = 0

    def step(self):
        from spark_amd.exchange import range_exchange
        gq = self.gq
        k, payload, _ = range_exchange(self.keys, {"p": self.pay})
        perm, skeys = gq.sort_perm(k)
        gq.gather(payload["p"], perm)
        self.nrows_local = k.numel()

    def free(self):
        del self.keys, self.pay


class Q1Workload:
    """Config-5 single-GPU slice: the REAL TPC-H Q1 shape
    (resources/tpch/q1.sql) over a lineitem-shaped synthetic batch —
    decimal(12,2) columns as scaled int64 (Spark's compact-long Decimal),
    shipdate as int64 days, returnflag/linestatus as dictionary ids.
    Plan: filter (l_shipdate <= date'1998-12-01' - 90 days) -> projected
    decimal products (scale-4 disc_price, scale-6 charge, exact i64) ->
    GROUP BY (l_returnflag, l_linestatus) — the composite tuple rides the
    narrow-key pack rule into the LDS low-cardinality path — with
    sum_qty/sum_base_price/sum_disc_price/sum_charge (wrapping-exact i64),
    avg_disc (f64 of exact sums) and count_order, then ORDER BY the
    grouping keys. Driven through the exec-node layer (the same operator
    objects a ColumnarRule would produce)."""

    def __init__(self, gq, rows, rank):
        from spark_amd import exec as gx
        self.gx = gx
        off = rank * 7
        self.cols = dict(
            l_returnflag=gq.gen_i64(seed=71 + off, n=rows, range_=3),
            l_linestatus=gq.gen_i64(seed=76 + off, n=rows, range_=2),
            l_quantity=gq.gen_i64(seed=72 + off, n=rows, range_=5000),
            l_extendedprice=gq.gen_i64(seed=73 + off, n=rows,
                                       range_=10_000_000),
            l_discount=gq.gen_i64(seed=74 + off, n=rows, range_=11),
            l_tax=gq.gen_i64(seed=77 + off, n=rows, range_=9),
            # days offset into the 1992..1998 window (values 0..2555);
            # the Q1 cutoff (date '1998-12-01' - 90 days) sits at ~95%
            l_shipdate=gq.gen_i64(seed=75 + off, n=rows, range_=2556),
        )
        self.rows = rows
        self.ngroups = 0

    def step(self):
        gx = self.gx
        scan = gx.InputBatches([gx.ColumnarBatch(dict(self.cols))])
        passthru = ["l_returnflag", "l_linestatus", "l_quantity",
                    "l_extendedprice", "l_discount"]
        plan = gx.SortExec(
            [gx.SortOrder("l_returnflag"), gx.SortOrder("l_linestatus")],
            False,
            gx.HashAggregateExec(
                ("l_returnflag", "l_linestatus"),
                [("sum", "l_quantity"), ("sum", "l_extendedprice"),
                 ("sum", "disc_price"), ("sum", "charge"),
                 ("avg", "l_discount"), ("count*", None)],
                "complete",
                gx.ProjectExec(
                    passthru + ["disc_price",
                                ("charge", "disc_price", "*",
                                 "__one_plus_tax", None)],
                    gx.ProjectExec(
                        passthru + ["__one_plus_tax",
                                    ("disc_price", "l_extendedprice", "*",
                                     "__one_minus_disc", None)],
                        gx.ProjectExec(
                            passthru + [
                                ("__one_minus_disc", "l_discount", "rsub",
                                 None, 100),
                                ("__one_plus_tax", "l_tax", "+", None, 100)],
                            gx.FilterExec("l_shipdate", "<=", 2435,
                                          scan)))),
                capacity=64))
        plan = gx.GpuColumnarRule().pre_columnar_transitions(plan)
        out = next(plan.execute_columnar())
        self.ngroups = out.num_rows()
        out.close()

    def free(self):
        self.cols.clear()


def build_q3_plan(gx, lineitem, orders, customer, cut_date: int,
                  segment_id: int):
    """The TPC-H Q3 plan shape (resources/tpch/q3.sql) over device batches:
    customer filtered on mktsegment feeds a BROADCAST dimension join with
    date-filtered orders (BroadcastHashJoinExec, the §8(f).3 slot); the
    result is the build side of the fact join with shipdate-filtered
    lineitem; revenue = extendedprice*(100-discount) as exact scale-4
    int64; 3-key composite GROUP BY (l_orderkey, o_orderdate,
    o_shippriority); ORDER BY revenue DESC, o_orderdate. LIMIT is the
    host's slice of the sorted output (a CollectLimit concern, not the
    engine's)."""
    cust = gx.FilterExec("c_mktsegment", "==", segment_id,
                         gx.InputBatches([customer]))
    ord_f = gx.FilterExec("o_orderdate", "<", cut_date,
                          gx.InputBatches([orders]))
    # dimension join: broadcast the filtered customers, stream orders
    j1 = gx.BroadcastHashJoinExec("o_custkey", "c_custkey", "right",
                                  ord_f, gx.BroadcastExchangeExec(cust))
    j1p = gx.ProjectExec(["o_orderkey", "o_orderdate", "o_shippriority"], j1)
    li = gx.FilterExec("l_shipdate", ">", cut_date,
                       gx.InputBatches([lineitem]))
    j2 = gx.ShuffledHashJoinExec("l_orderkey", "o_orderkey", "right",
                                 li, j1p)
    rev = gx.ProjectExec(
        ["l_orderkey", "o_orderdate", "o_shippriority", "l_extendedprice",
         ("__omd", "l_discount", "rsub", None, 100)],
        j2)
    rev2 = gx.ProjectExec(
        ["l_orderkey", "o_orderdate", "o_shippriority",
         ("revenue", "l_extendedprice", "*", "__omd", None)],
        rev)
    agg = gx.HashAggregateExec(
        ("l_orderkey", "o_orderdate", "o_shippriority"),
        [("sum", "revenue")], "complete", rev2)
    return gx.SortExec([gx.SortOrder("sum(revenue)", descending=True),
                        gx.SortOrder("o_orderdate")], False, agg)


class Q3Workload:
    """Config-5 Q3 probe (single-GPU slice): two joins (broadcast dimension
    + shuffled fact), date filters, exact decimal revenue, 3-key composite
    grouping, multi-key ORDER BY with DESC over the aggregate output."""

    def __init__(self, gq, rows, rank):
        from spark_amd import exec as gx
        self.gx = gx
        orders_n = max(rows // 4, 1024)
        cust_n = max(rows // 20, 1024)
        off = rank * 11
        # persistent column tensors; fresh ColumnarBatch wrappers per step
        # (consumers close their input batches — the batch lifetime
        # contract)
        self.li = dict(
            l_orderkey=gq.gen_i64(seed=81 + off, n=rows, range_=orders_n),
            l_extendedprice=gq.gen_i64(seed=82 + off, n=rows,
                                       range_=10_000_000),
            l_discount=gq.gen_i64(seed=83 + off, n=rows, range_=11),
            l_shipdate=gq.gen_i64(seed=84 + off, n=rows, range_=2556),
        )
        self.od = dict(
            o_orderkey=gq.range_i64(orders_n),
            o_custkey=gq.gen_i64(seed=85 + off, n=orders_n, range_=cust_n),
            o_orderdate=gq.gen_i64(seed=86 + off, n=orders_n, range_=2556),
            o_shippriority=gq.gen_i64(seed=87 + off, n=orders_n, range_=2),
        )
        self.cu = dict(
            c_custkey=gq.range_i64(cust_n),
            c_mktsegment=gq.gen_i64(seed=88 + off, n=cust_n, range_=5),
        )
        self.rows = rows
        self.ngroups = 0

    def step(self):
        gx = self.gx
        plan = build_q3_plan(gx, gx.ColumnarBatch(dict(self.li)),
                             gx.ColumnarBatch(dict(self.od)),
                             gx.ColumnarBatch(dict(self.cu)),
                             cut_date=1169,   # ~1995-03-15 in day offsets
                             segment_id=1)
        plan = gx.GpuColumnarRule().pre_columnar_transitions(plan)
        out = next(plan.execute_columnar())
        self.ngroups = out.num_rows()
        # top-10 = the already-sorted head (CollectLimit host slice)
        out.close()

    def free(self):
        self.li.clear(), self.od.clear(), self.cu.clear()


def time_workload(w, steps, warmup, world):
    for _ in range(warmup):
        w.step()
    barrier_sync(world)
    t0 = time.perf_counter()
    for _ in range(steps):
        w.step()
    barrier_sync(world)
    dt = max_over_ranks(time.perf_counter() - t0, world)
    return dt / steps


DUMP_SAMPLE_ROWS = 1 << 20   # 6 float64 arrays x 8 MiB = 48 MiB <= the 64 MB cap
DUMP_SAMPLE_SEED = 20260


def _save_i64_split(path_stem, t):
    """int64 (full-range) does not fit float64's 53-bit mantissa: store the
    signed high and unsigned low 32-bit halves, each exact in float64
    (value = hi * 2**32 + lo)."""
    import numpy as np
    a = t.cpu().numpy()
    np.save(path_stem + "_hi.npy", (a >> 32).astype(np.float64))
    np.save(path_stem + "_lo.npy", (a & 0xFFFFFFFF).astype(np.float64))


def dump_sort_outputs(w, out_dir):
    """What the timed sort step handed back in its last step — the
    permutation, the sorted keys and both gathered payload columns — at a
    fixed seeded sample of output positions (all of them when the output is
    no larger than the sample), one float64 .npy per array."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    if w.rows <= DUMP_SAMPLE_ROWS:
        pos = np.arange(w.rows, dtype=np.int64)
    else:
        pos = np.sort(np.random.default_rng(DUMP_SAMPLE_SEED).integers(
            0, w.rows, DUMP_SAMPLE_ROWS, dtype=np.int64))
    torch.cuda.synchronize()
    idx = torch.from_numpy(pos).cuda()
    # row ids are u32 carried in an int32 tensor
    rid = w.perm[idx].to(torch.int64) & 0xFFFFFFFF
    np.save(os.path.join(out_dir, "sort_perm.npy"),
            rid.cpu().numpy().astype(np.float64))
    _save_i64_split(os.path.join(out_dir, "sort_keys"), w.skeys[idx])
    _save_i64_split(os.path.join(out_dir, "sort_payload_i64"), w.out1[idx])
    np.save(os.path.join(out_dir, "sort_payload_f64.npy"),
            w.out2[idx].cpu().numpy())


def cpu_baseline_sort(sample_rows):
    """Oracle (C restatement) on the same sort workload shape, OpenMP
    multithreaded (the substitute leg BASELINE.md specifies). The thread
    count is auto-tuned on a small probe — the per-thread histogram scan and
    memory contention make full oversubscription SLOWER on many-core hosts,
    and the baseline should be the best honest CPU number."""
    import oracle
    ncpu = os.cpu_count()
    probe = oracle.gen_i64(42, 4_000_000)
    best, best_t = 1, float("inf")
    for t in sorted({1, 4, 8, 16, min(32, ncpu), min(64, ncpu)}):
        t0 = time.perf_counter()
        oracle.sort_perm_mt(probe, nthreads=t)
        dt = time.perf_counter() - t0
        if dt < best_t:
            best, best_t = t, dt
    cores = best
    keys = oracle.gen_i64(42, sample_rows)
    pay1 = oracle.gen_i64(43, sample_rows)
    pay2 = oracle.gen_f64_unit(44, sample_rows)
    t0 = time.perf_counter()
    perm = oracle.sort_perm_mt(keys, nthreads=cores)
    _o1 = oracle.gather_i64_mt(pay1, perm)
    _o2 = oracle.gather_i64_mt(pay2.view("int64"), perm)
    dt = time.perf_counter() - t0
    return sample_rows / dt, dt, cores


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=10)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--rows", type=int, default=1_000_000_000)
    p.add_argument("--agg-rows", type=int, default=1_000_000_000)
    p.add_argument("--agg-groups", type=int, default=10_000_000)
    p.add_argument("--join-rows", type=int, default=500_000_000)
    p.add_argument("--quick", action="store_true", help="small sizes (CI/sanity)")
    p.add_argument("--no-cpu-baseline", action="store_true")
    p.add_argument("--cpu-sample-rows", type=int, default=40_000_000)
    p.add_argument("--full", action="store_true",
                   help="also run the sub-benchmarks (agg, join, q1, q3, and "
                        "gsort at N>1) and the CPU-oracle baseline; a plain "
                        "run times the headline sort workload only")
    p.add_argument("--workloads", default=None,
                   help="with --full: which workloads to run "
                        "(default sort,agg,join,q1,q3,gsort)")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="after the timed steps, write what the last sort step "
                        "produced as DIR/<name>.npy (float64, seeded sample)")
    args = p.parse_args()
    if args.full:
        args.workloads = args.workloads or "sort,agg,join,q1,q3,gsort"
    elif args.workloads is not None:
        p.error("--workloads needs --full")
    else:
        args.workloads = "sort"
        args.no_cpu_baseline = True
    if args.dump_outputs and "sort" not in args.workloads.split(","):
        p.error("--dump-outputs writes the sort workload's outputs")
    if args.quick:
        args.rows, args.agg_rows, args.agg_groups, args.join_rows = \
            20_000_000, 20_000_000, 200_000, 10_000_000
        args.cpu_sample_rows = 2_000_000

    rank, world, local = dist_setup()
    from spark_amd import gpuq as gq
    gq.profiling(True)
    wl = args.workloads.split(",")
    results = {}

    def guarded(name, fn):
        """One failing sub-workload must not sink the whole bench run (the
        driver's round-end N>1 runs) — record the error and continue.
        Collective-using workloads are not guarded at N>1 (a half-failed
        collective would wedge the other ranks)."""
        try:
            fn()
        except Exception as e:  # noqa: BLE001
            if world > 1:
                raise
            import traceback
            traceback.print_exc()
            results[name] = {"error": f"{type(e).__name__}: {e}"}

    def _run_sort():
            w = SortWorkload(gq, args.rows, rank)
            gq.kernel_stats_reset()
            sec = time_workload(w, args.steps, args.warmup, world)
            scat_ms, scat_n = gq.kernel_stats("radix_scatter")
            hist_ms, hist_n = gq.kernel_stats("radix_hist")
            if args.dump_outputs and rank == 0:
                dump_sort_outputs(w, args.dump_outputs)
            w.free()
            torch.cuda.empty_cache()
            results["sort"] = {
                "sec_per_step": sec,
                "rows_per_sec": args.rows * world / sec,
                "scatter_ms_avg": scat_ms / max(scat_n, 1),
                "scatter_launches": scat_n,
                "hist_ms_avg": hist_ms / max(hist_n, 1),
            }


    if "sort" in wl:
        guarded("sort", _run_sort)
    def _run_agg():
            w = AggWorkload(gq, args.agg_rows, args.agg_groups, rank)
            sec = time_workload(w, args.steps, args.warmup, world)
            ng = w.ngroups
            ab_ms, ab_n = gq.kernel_stats("agg_build")
            w.free()
            torch.cuda.empty_cache()
            results["agg"] = {"sec_per_step": sec,
                              "rows_per_sec": args.agg_rows * world / sec,
                              "agg_build_ms_avg": ab_ms / max(ab_n, 1),
                              "ngroups": ng}


    if "agg" in wl:
        guarded("agg", _run_agg)
    def _run_join():
            w = JoinWorkload(gq, args.join_rows, rank, world)
            gq.kernel_stats_reset()
            sec = time_workload(w, args.steps, args.warmup, world)
            nm = w.nmatches
            w.free()
            torch.cuda.empty_cache()
            jb_ms, jb_n = gq.kernel_stats("join_build")
            jp_ms, jp_n = gq.kernel_stats("join_probe")
            results["join"] = {
                "sec_per_step": sec,
                "build_ms_avg": jb_ms / max(jb_n, 1),
                "probe_ms_avg": jp_ms / max(jp_n, 1),
                # rows processed = both tables, all ranks (the config's rate basis)
                "rows_per_sec": 2 * args.join_rows * world / sec,
                "matches_local": nm,
                "exchange": "rccl_all_to_all" if world > 1 else "none (single GPU)",
            }


    if "join" in wl:
        guarded("join", _run_join)
    def _run_gsort():
            w = GlobalSortWorkload(gq, args.rows, rank, world)
            sec = time_workload(w, args.steps, args.warmup, world)
            w.free()
            torch.cuda.empty_cache()
            results["gsort"] = {"sec_per_step": sec,
                                "rows_per_sec": args.rows * world / sec,
                                "scaling": "weak, one range exchange",
                                "local_rows": w.nrows_local}


    if "gsort" in wl and world > 1:
        guarded("gsort", _run_gsort)
    def _run_q1():
            w = Q1Workload(gq, args.join_rows, rank)
            sec = time_workload(w, args.steps, args.warmup, world)
            ng = w.ngroups
            w.free()
            torch.cuda.empty_cache()
            results["q1"] = {"sec_per_step": sec,
                             "rows_per_sec": args.join_rows * world / sec,
                             "plan": "real Q1: filter(shipdate)->decimal "
                                     "projects->groupby(retflag,linestatus) "
                                     "4 sums+avg+count*->orderby",
                             "ngroups": ng}


    if "q1" in wl:
        guarded("q1", _run_q1)

    def _run_q3():
            w = Q3Workload(gq, args.join_rows, rank)
            sec = time_workload(w, args.steps, args.warmup, world)
            ng = w.ngroups
            w.free()
            torch.cuda.empty_cache()
            results["q3"] = {"sec_per_step": sec,
                             "rows_per_sec": args.join_rows * world / sec,
                             "plan": "Q3: cust-filter->broadcast dim join->"
                                     "fact join->revenue->3-key groupby->"
                                     "orderby(revenue desc, date)",
                             "ngroups": ng}


    if "q3" in wl:
        guarded("q3", _run_q3)
    if rank != 0:
        return

    ok_results = {k: v for k, v in results.items() if "rows_per_sec" in v}
    primary = ok_results.get("sort") or next(iter(ok_results.values()))
    # roofline of the dominant kernel (radix scatter): 12B read + 12B write
    # per row per pass ((u64 encoded key, u32 rowid) pairs), algorithmic.
    roofline = None
    if "sort" in results:
        r = results["sort"]
        alg_bytes_per_launch = 24.0 * args.rows
        ach = alg_bytes_per_launch / (r["scatter_ms_avg"] / 1e3) / 1e9 \
            if r["scatter_ms_avg"] > 0 else 0.0
        roofline = {"bound": "hbm", "achieved": round(ach, 1),
                    "peak": PEAK_HBM_GBPS, "unit": "GB/s",
                    "frac": round(ach / PEAK_HBM_GBPS, 4),
                    "traffic": None,
                    "kernel": "radix_scatter",
                    "alg_bytes_per_launch": alg_bytes_per_launch}

    cpu = None
    if not args.no_cpu_baseline and world == 1 and "sort" in results:
        rate, dt, cores = cpu_baseline_sort(args.cpu_sample_rows)
        cpu = {"value": round(rate, 1), "unit": "rows/s", "cores": cores,
               "kind": "port",
               "sample": f"oracle C sort+gather of {args.cpu_sample_rows} rows "
                         f"({dt:.1f}s, OpenMP x{cores} host cores)"}

    out = {
        "metric": "rows/sec (sort+hash-agg+join, 1B-row synth)",
        "value": round(primary["rows_per_sec"], 1),
        "unit": "rows/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(primary["sec_per_step"] * 1e3, 3),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "int64",
        "data": "synthetic",
        "config": {
            "workload": "orderby-1b-int64x3 (BASELINE configs[1]); value = sort rows/s",
            "rows": args.rows,
            "cols": "int64 key + int64 + float64 payload",
            "parallelism": ("independent per-GPU sorts (single-partition ORDER BY); "
                            "join sub-benchmark exchanges via RCCL all-to-all"
                            if world > 1 else "single GPU"),
        },
        "roofline": roofline,
        "cpu_baseline": cpu,
        "sub_benchmarks": results,
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
