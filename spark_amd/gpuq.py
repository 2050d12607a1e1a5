"""ctypes binding over libgpuq.so (include/gpuq.h) — the C-ABI boundary.

Device memory, streams and the process-per-GPU launch come from PyTorch-ROCm
(plumbing only); every compute kernel is hand-written HIP in
spark_amd/csrc/gpuq.hip. There is NO CPU fallback here: if the extension is
missing or a call fails, we raise — the product path must never silently run
on an eager/CPU substitute (GPU parity would be meaningless).
"""
import ctypes
import os

import torch

from . import expression, predicate
from .predicate import rewrite_i64_float_cmp

_DIR = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_DIR, "libgpuq.so")

GPUQ_INT64 = 0
GPUQ_FLOAT64 = 1
GPUQ_INT32 = 2

_DTYPE_MAP = {
    torch.int64: GPUQ_INT64,
    torch.float64: GPUQ_FLOAT64,
    torch.int32: GPUQ_INT32,
}


class GpuqError(RuntimeError):
    pass


class _Col(ctypes.Structure):
    _fields_ = [("data", ctypes.c_void_p),
                ("validity", ctypes.c_void_p),
                ("dtype", ctypes.c_int32)]


class _PredInsn(ctypes.Structure):
    _fields_ = [("opcode", ctypes.c_int32),
                ("cmp", ctypes.c_int32),
                ("col_a", ctypes.c_int32),
                ("col_b", ctypes.c_int32),
                ("lit_i64", ctypes.c_int64),
                ("lit_f64", ctypes.c_double)]


class _ExprInsn(ctypes.Structure):
    _fields_ = [("opcode", ctypes.c_int32),
                ("arg", ctypes.c_int32),
                ("dtype", ctypes.c_int32),
                ("pad", ctypes.c_int32),
                ("lit_i64", ctypes.c_int64),
                ("lit_f64", ctypes.c_double)]


_lib = None


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(_SO):
            raise GpuqError(
                f"libgpuq.so not found at {_SO}. Build it with "
                f"`make -C spark_amd/csrc` (or __graft_entry__.build()). "
                f"There is no CPU fallback.")
        L = ctypes.CDLL(_SO)
        i32, i64, u64 = ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64
        vp = ctypes.c_void_p
        L.gpuq_last_error.restype = ctypes.c_char_p
        L.gpuq_device_count.restype = i32
        L.gpuq_gen_i64_range.restype = i32
        L.gpuq_gen_i64_range.argtypes = [vp, u64, u64, i64, u64, vp]
        L.gpuq_gen_f64_unit.restype = i32
        L.gpuq_gen_f64_unit.argtypes = [vp, u64, u64, i64, vp]
        L.gpuq_sort_workspace_bytes.restype = i64
        L.gpuq_sort_workspace_bytes.argtypes = [i64]
        L.gpuq_sort_perm.restype = i32
        L.gpuq_sort_perm.argtypes = [vp, i64, _Col, i32, i32, vp, vp, vp, i64]
        L.gpuq_topk_workspace_bytes.restype = i64
        L.gpuq_topk_workspace_bytes.argtypes = [i64]
        L.gpuq_topk_candidates.restype = i32
        L.gpuq_topk_candidates.argtypes = [vp, i64, _Col, i32, i32, i64, i32,
                                           vp, i64, ctypes.POINTER(i64),
                                           vp, i64]
        L.gpuq_gather.restype = i32
        L.gpuq_gather.argtypes = [vp, i64, _Col, vp, vp]
        L.gpuq_gather2_i64.restype = i32
        L.gpuq_gather2_i64.argtypes = [vp, i64, vp, vp, vp, vp, vp]
        L.gpuq_gather2_i64_fast.restype = i32
        L.gpuq_gather2_i64_fast.argtypes = [vp, i64, vp, vp, vp, vp, vp, vp]
        L.gpuq_interleave2_i64.restype = i32
        L.gpuq_interleave2_i64.argtypes = [vp, i64, vp, vp, vp]
        L.gpuq_gather2_pairs.restype = i32
        L.gpuq_gather2_pairs.argtypes = [vp, i64, vp, vp, vp, vp]
        L.gpuq_hash_agg_workspace_bytes.restype = i64
        L.gpuq_hash_agg_workspace_bytes.argtypes = [i64]
        L.gpuq_hash_agg_i64_f64.restype = i32
        L.gpuq_hash_agg_i64_f64.argtypes = [vp, i64, _Col, _Col, vp, i64, i32, i32, i32,
                                            vp, vp, vp, vp, vp, ctypes.POINTER(i64)]
        L.gpuq_hash_agg_part_workspace_bytes.restype = i64
        L.gpuq_hash_agg_part_workspace_bytes.argtypes = [i64, i64]
        L.gpuq_hash_agg_partitioned.restype = i32
        L.gpuq_hash_agg_partitioned.argtypes = [vp, i64, _Col, _Col, vp, i64, i32,
                                                vp, vp, vp, vp, vp,
                                                ctypes.POINTER(i64)]
        L.gpuq_hash_agg_multi_workspace_bytes.restype = i64
        L.gpuq_hash_agg_multi_workspace_bytes.argtypes = [i64, i32]
        L.gpuq_hash_agg_multi.restype = i32
        L.gpuq_hash_agg_multi.argtypes = [vp, i64, _Col, vp, vp, vp, i32,
                                          vp, i64, i32, i32, vp, vp, vp,
                                          ctypes.POINTER(i64)]
        L.gpuq_partition_workspace_bytes.restype = i64
        L.gpuq_partition_workspace_bytes.argtypes = [i64, i32]
        L.gpuq_partition_perm.restype = i32
        L.gpuq_partition_perm.argtypes = [vp, i64, _Col, i32, vp, vp, vp, i64]
        L.gpuq_partition_perm_multi.restype = i32
        L.gpuq_partition_perm_multi.argtypes = [vp, i64, ctypes.POINTER(_Col), i32,
                                                i32, vp, vp, vp, i64]
        L.gpuq_hash_agg_keys_workspace_bytes.restype = i64
        L.gpuq_hash_agg_keys_workspace_bytes.argtypes = [i64, i32, i32]
        L.gpuq_hash_agg_keys.restype = i32
        L.gpuq_hash_agg_keys.argtypes = [vp, i64, ctypes.POINTER(_Col), i32,
                                         ctypes.POINTER(_Col), vp, vp, i32,
                                         vp, i64, i32, i32,
                                         vp, vp, vp, ctypes.POINTER(i64)]
        L.gpuq_gather_bits.restype = i32
        L.gpuq_gather_bits.argtypes = [vp, i64, vp, vp, vp]
        L.gpuq_bits_to_u8.restype = i32
        L.gpuq_bits_to_u8.argtypes = [vp, i64, vp, vp]
        L.gpuq_u8_to_bits.restype = i32
        L.gpuq_u8_to_bits.argtypes = [vp, i64, vp, vp]
        L.gpuq_nonzero_to_bits.restype = i32
        L.gpuq_nonzero_to_bits.argtypes = [vp, i64, vp, vp]
        L.gpuq_dec128_overflow_to_null.restype = i32
        L.gpuq_dec128_overflow_to_null.argtypes = [vp, i64, vp, vp, i32, vp]
        L.gpuq_maskbit_to_bits.restype = i32
        L.gpuq_maskbit_to_bits.argtypes = [vp, i64, vp, i32, vp]
        L.gpuq_minmax_i64.restype = i32
        L.gpuq_minmax_i64.argtypes = [vp, i64, _Col, vp]
        L.gpuq_pack2_i64.restype = i32
        L.gpuq_pack2_i64.argtypes = [vp, i64, vp, vp, i64, i64, i32, vp]
        L.gpuq_unpack2_i64.restype = i32
        L.gpuq_unpack2_i64.argtypes = [vp, i64, vp, i64, i64, i32, vp, vp]
        L.gpuq_range_partition_perm.restype = i32
        L.gpuq_range_partition_perm.argtypes = [vp, i64, _Col, i32, i32, vp, i32,
                                                vp, vp, vp, i64]
        L.gpuq_join_build_workspace_bytes.restype = i64
        L.gpuq_join_build_workspace_bytes.argtypes = [i64, i64]
        L.gpuq_join_probe_workspace_bytes.restype = i64
        L.gpuq_join_probe_workspace_bytes.argtypes = [i64]
        L.gpuq_join_build_i64.restype = i32
        L.gpuq_join_build_i64.argtypes = [vp, i64, _Col, vp, i64]
        L.gpuq_join_probe_i64.restype = i32
        L.gpuq_join_probe_i64.argtypes = [vp, i64, _Col, vp, i64, i64, vp, i64,
                                          vp, vp, i64, ctypes.POINTER(i64)]
        L.gpuq_join_probe_i64_typed.restype = i32
        L.gpuq_join_probe_i64_typed.argtypes = [vp, i64, _Col, vp, i64, i64, vp,
                                                i64, i32, vp, vp, i64,
                                                ctypes.POINTER(i64)]
        L.gpuq_join_keys_workspace_bytes.restype = i64
        L.gpuq_join_keys_workspace_bytes.argtypes = [i64, i64, i32]
        L.gpuq_join_build_keys.restype = i32
        L.gpuq_join_build_keys.argtypes = [vp, i64, ctypes.POINTER(_Col), i32,
                                           vp, i64]
        L.gpuq_join_probe_keys.restype = i32
        L.gpuq_join_probe_keys.argtypes = [vp, i64, ctypes.POINTER(_Col), i32,
                                           vp, i64, i64, i32, vp, vp, i64,
                                           ctypes.POINTER(i64)]
        L.gpuq_join_probe_keys_cond.restype = i32
        L.gpuq_join_probe_keys_cond.argtypes = [
            vp, i64, ctypes.POINTER(_Col), i32, vp, i64, i64, i32,
            ctypes.POINTER(_Col), ctypes.POINTER(i32), i32,
            ctypes.POINTER(_PredInsn), i32, vp, vp, i64, ctypes.POINTER(i64)]
        L.gpuq_join_keys_unmatched_build.restype = i32
        L.gpuq_join_keys_unmatched_build.argtypes = [vp, vp, i64, i64, i32,
                                                     vp, vp, i64,
                                                     ctypes.POINTER(i64)]
        L.gpuq_gather_nullable.restype = i32
        L.gpuq_gather_nullable.argtypes = [vp, i64, _Col, vp, vp, vp]
        L.gpuq_filter_workspace_bytes.restype = i64
        L.gpuq_filter_workspace_bytes.argtypes = [i64]
        L.gpuq_filter_cmp.restype = i32
        L.gpuq_filter_cmp.argtypes = [vp, i64, _Col, i32, ctypes.c_double, i64,
                                      vp, vp, vp, i64]
        L.gpuq_filter_expr_workspace_bytes.restype = i64
        L.gpuq_filter_expr_workspace_bytes.argtypes = [i64]
        L.gpuq_filter_expr.restype = i32
        L.gpuq_filter_expr.argtypes = [vp, i64, ctypes.POINTER(_Col), i32,
                                       ctypes.POINTER(_PredInsn), i32,
                                       vp, vp, vp, i64]
        L.gpuq_project_binop.restype = i32
        L.gpuq_project_binop.argtypes = [vp, i64, _Col, vp, ctypes.c_double, i64,
                                         i32, vp]
        L.gpuq_project_binop_nullable.restype = i32
        L.gpuq_project_binop_nullable.argtypes = [vp, i64, _Col, _Col,
                                                  ctypes.c_double, i64, i32,
                                                  vp, vp]
        L.gpuq_project_expr.restype = i32
        L.gpuq_project_expr.argtypes = [vp, i64, ctypes.POINTER(_Col), i32,
                                        ctypes.POINTER(_ExprInsn), i32,
                                        ctypes.POINTER(vp), ctypes.POINTER(vp),
                                        ctypes.POINTER(i32), i32]
        L.gpuq_range_i64.restype = i32
        L.gpuq_sort_last_plan.restype = None
        L.gpuq_sort_last_plan.argtypes = [ctypes.POINTER(ctypes.c_int)] * 3
        L.gpuq_range_i64.argtypes = [vp, i64, i64, i64, vp]
        L.gpuq_cast_i64_f64.restype = i32
        L.gpuq_cast_i64_f64.argtypes = [vp, i64, vp, vp]
        L.gpuq_window_boundaries.restype = i32
        L.gpuq_window_boundaries.argtypes = [vp, i64, ctypes.POINTER(_Col), i32,
                                             i32, vp, vp]
        L.gpuq_window_workspace_bytes.restype = i64
        L.gpuq_window_workspace_bytes.argtypes = [i64]
        L.gpuq_window_scan.restype = i32
        L.gpuq_window_scan.argtypes = [vp, i64, i32, i32, _Col, vp, vp, vp, vp,
                                       vp, i64]
        L.gpuq_window_shift.restype = i32
        L.gpuq_window_shift.argtypes = [vp, i64, _Col, i64, i32,
                                        ctypes.c_double, i64, vp, vp, vp,
                                        vp, i64]
        L.gpuq_window_slide_workspace_bytes.restype = i64
        L.gpuq_window_slide_workspace_bytes.argtypes = [i64, i64, i64]
        L.gpuq_window_slide.restype = i32
        L.gpuq_window_slide.argtypes = [vp, i64, i32, _Col, i64, i64, vp, vp, vp,
                                        vp, i64]
        L.gpuq_profiling.restype = None
        L.gpuq_profiling.argtypes = [i32]
        L.gpuq_kernel_stats_reset.restype = None
        L.gpuq_kernel_stats.restype = i32
        L.gpuq_kernel_stats.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_double),
                                        ctypes.POINTER(ctypes.c_longlong)]
        _lib = L
    return _lib


def profiling(enable: bool):
    lib().gpuq_profiling(1 if enable else 0)


def kernel_stats_reset():
    lib().gpuq_kernel_stats_reset()


def kernel_stats(name: str):
    ms = ctypes.c_double(0)
    cnt = ctypes.c_longlong(0)
    lib().gpuq_kernel_stats(name.encode(), ctypes.byref(ms), ctypes.byref(cnt))
    return ms.value, cnt.value


def _check(rc: int):
    if rc != 0:
        raise GpuqError(lib().gpuq_last_error().decode())


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _col(t: torch.Tensor, validity=None) -> _Col:
    assert t.is_cuda and t.is_contiguous()
    return _Col(t.data_ptr(), validity.data_ptr() if validity is not None else None,
                _DTYPE_MAP[t.dtype])


def _dp(t) -> int:
    return t.data_ptr() if t is not None else None


def device_count() -> int:
    return lib().gpuq_device_count()


def gen_i64(seed: int, n: int, range_: int = 0, start: int = 0,
            device="cuda") -> torch.Tensor:
    out = torch.empty(n, dtype=torch.int64, device=device)
    _check(lib().gpuq_gen_i64_range(_stream(), seed, start, n, range_, out.data_ptr()))
    return out


def gen_f64_unit(seed: int, n: int, start: int = 0, device="cuda") -> torch.Tensor:
    out = torch.empty(n, dtype=torch.float64, device=device)
    _check(lib().gpuq_gen_f64_unit(_stream(), seed, start, n, out.data_ptr()))
    return out


def sort_workspace(n: int, device="cuda") -> torch.Tensor:
    return torch.empty(lib().gpuq_sort_workspace_bytes(n), dtype=torch.uint8, device=device)


def sort_perm(keys: torch.Tensor, desc=False, nulls_first=None, workspace=None,
              out_keys=True, key_validity=None, out_perm=None):
    """out_keys: True (allocate), False/None (skip), or a preallocated tensor.
    out_perm: optional preallocated int32 tensor (large callers reuse buffers
    to avoid fresh multi-GB hipMallocs per call)."""
    n = keys.numel()
    if nulls_first is None:
        nulls_first = not desc
    if workspace is None:
        workspace = sort_workspace(n, keys.device)
    perm = out_perm if out_perm is not None else         torch.empty(n, dtype=torch.int32, device=keys.device)  # u32 bits
    if isinstance(out_keys, torch.Tensor):
        ok = out_keys
    else:
        ok = torch.empty(n, dtype=keys.dtype, device=keys.device) if out_keys else None
    _check(lib().gpuq_sort_perm(_stream(), n, _col(keys, key_validity), int(desc), int(nulls_first),
                                perm.data_ptr(), _dp(ok),
                                workspace.data_ptr(), workspace.numel()))
    return perm, ok


def sort_last_plan():
    """(window_passes, deferred_bytes, fell_back) of the last sort_perm on this
    thread; deferred_bytes == 0 means the classic all-active-bytes plan ran."""
    wp, db, fb = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    lib().gpuq_sort_last_plan(ctypes.byref(wp), ctypes.byref(db), ctypes.byref(fb))
    return wp.value, db.value, fb.value


# mirrors of the #defines in csrc/gpuq.hip: the bucket size below which the
# select copies the surviving keys to its workspace, and the emit kernels'
# rows per block
TOPK_COMPACT_MAX = 1 << 20
TOPK_EMIT_TILE = 2048


def topk_workspace(n: int, device="cuda") -> torch.Tensor:
    return torch.empty(lib().gpuq_topk_workspace_bytes(n), dtype=torch.uint8,
                       device=device)


def topk_candidates(keys: torch.Tensor, k: int, desc=False, nulls_first=None,
                    key_validity=None, keep_ties=False, workspace=None):
    """Rows of the first k positions of sort_perm(keys, desc, nulls_first)'s
    order, by radix select. Returns (rids, n_before, n_tie): rids (int32, u32
    bits) ascending, n_before rows sorting strictly before the tie group T
    that holds position min(k, n) - 1, n_tie = |T|. keep_ties=False takes the
    first min(k, n) - n_before rows of T in input order (len(rids) ==
    min(k, n)); keep_ties=True takes all of T."""
    n = keys.numel()
    dev = keys.device
    if nulls_first is None:
        nulls_first = not desc
    if workspace is None:
        workspace = topk_workspace(n, dev)
    kk = max(min(n, k), 0)
    cap = kk if not keep_ties else min(n, max(2 * kk, 1024))
    counts = (ctypes.c_int64 * 3)()
    for _ in range(2):
        rids = torch.empty(cap, dtype=torch.int32, device=dev)
        rc = lib().gpuq_topk_candidates(
            _stream(), n, _col(keys, key_validity), int(desc), int(nulls_first),
            k, int(keep_ties), rids.data_ptr(), cap, counts,
            workspace.data_ptr(), workspace.numel())
        if rc != 3:  # GPUQ_ERR_OVERFLOW: retry once at the reported n_cand
            break
        cap = counts[0]
    _check(rc)
    return rids[:counts[0]], counts[1], counts[2]


def topk_perm(keys: torch.Tensor, k: int, desc=False, nulls_first=None,
              key_validity=None):
    """(perm, sorted_keys), each of length min(k, n): bit-identical to the
    first k entries of sort_perm(keys, desc, nulls_first, key_validity).
    Select the candidate rows, then stable-sort only those: they come in
    input order, so ties resolve as in the full sort."""
    if nulls_first is None:
        nulls_first = not desc
    rids, _, _ = topk_candidates(keys, k, desc=desc, nulls_first=nulls_first,
                                 key_validity=key_validity, keep_ties=False)
    if rids.numel() == 0:
        return rids, torch.empty(0, dtype=keys.dtype, device=keys.device)
    small = gather(keys, rids)
    small_valid = gather_bits(key_validity, rids) \
        if key_validity is not None else None
    small_perm, skeys = sort_perm(small, desc=desc, nulls_first=nulls_first,
                                  key_validity=small_valid)
    return gather(rids, small_perm), skeys


def gather(col: torch.Tensor, perm: torch.Tensor) -> torch.Tensor:
    n = perm.numel()
    out = torch.empty(n, dtype=col.dtype, device=col.device)
    _check(lib().gpuq_gather(_stream(), n, _col(col), perm.data_ptr(), out.data_ptr()))
    return out


def agg_workspace(capacity: int, device="cuda") -> torch.Tensor:
    return torch.empty(lib().gpuq_hash_agg_workspace_bytes(capacity),
                       dtype=torch.uint8, device=device)


AGG_SUM = 1
AGG_COUNT = 2


def hash_agg(keys: torch.Tensor, vals: torch.Tensor, capacity: int,
             workspace=None, max_groups=None,
             key_validity=None, val_validity=None, ops=AGG_SUM | AGG_COUNT):
    """One-shot aggregate of a single batch. Returns (keys, key_valid, sums,
    sum_valid, counts) tensors sliced to ngroups.

    Mid-cardinality routing: when the capacity hint falls in the band where
    the direct table's atomic contention dominates (measured on MI355X at
    1B rows: 100K groups 60->40 ms, 1M groups 49->43 ms) and the batch is
    single-shot with non-null values, the bucket-partitioned kernel runs
    instead (identical results contract)."""
    n = keys.numel()
    dev = keys.device
    if (val_validity is None and (1 << 16) <= capacity <= (1 << 22)
            and n >= (1 << 24) and os.environ.get("GPUQ_NO_PART_AGG") is None):
        return hash_agg_partitioned(keys, vals, capacity,
                                    max_groups=max_groups,
                                    key_validity=key_validity, ops=ops)
    if workspace is None:
        workspace = agg_workspace(capacity, dev)
    mg = max_groups if max_groups is not None else min(n + 2, capacity + 2)
    ok = torch.empty(mg, dtype=torch.int64, device=dev)
    okv = torch.empty(mg, dtype=torch.uint8, device=dev)
    osum = torch.empty(mg, dtype=torch.float64, device=dev)
    osv = torch.empty(mg, dtype=torch.uint8, device=dev)
    ocnt = torch.empty(mg, dtype=torch.int64, device=dev)
    ng = ctypes.c_int64(0)
    _check(lib().gpuq_hash_agg_i64_f64(
        _stream(), n, _col(keys, key_validity), _col(vals, val_validity),
        workspace.data_ptr(), capacity, 1, 1, ops,
        ok.data_ptr(), okv.data_ptr(), osum.data_ptr(), osv.data_ptr(),
        ocnt.data_ptr(), ctypes.byref(ng)))
    g = ng.value
    return ok[:g], okv[:g], osum[:g], osv[:g], ocnt[:g]


def partition_workspace(n: int, nparts: int, device="cuda") -> torch.Tensor:
    return torch.empty(lib().gpuq_partition_workspace_bytes(n, nparts),
                       dtype=torch.uint8, device=device)


def partition_perm(keys: torch.Tensor, nparts: int, workspace=None, key_validity=None):
    """Stable group-by-partition permutation + per-partition counts."""
    n = keys.numel()
    dev = keys.device
    if workspace is None:
        workspace = partition_workspace(n, nparts, dev)
    perm = torch.empty(n, dtype=torch.int32, device=dev)
    counts = torch.empty(nparts, dtype=torch.int64, device=dev)
    _check(lib().gpuq_partition_perm(_stream(), n, _col(keys, key_validity), nparts,
                                     perm.data_ptr(), counts.data_ptr(),
                                     workspace.data_ptr(), workspace.numel()))
    return perm, counts


def join_build(build_keys: torch.Tensor, capacity: int, workspace=None,
               key_validity=None):
    bn = build_keys.numel()
    dev = build_keys.device
    if workspace is None:
        workspace = torch.empty(lib().gpuq_join_build_workspace_bytes(bn, capacity),
                                dtype=torch.uint8, device=dev)
    _check(lib().gpuq_join_build_i64(_stream(), bn, _col(build_keys, key_validity),
                                     workspace.data_ptr(), capacity))
    return workspace


def join_probe_workspace(probe_rows: int, device="cuda") -> torch.Tensor:
    """The probe needs no workspace of its own any more: 0 bytes. join_probe
    still takes probe_ws= and ignores it."""
    return torch.empty(lib().gpuq_join_probe_workspace_bytes(probe_rows),
                       dtype=torch.uint8, device=device)


JOIN_INNER, JOIN_OUTER, JOIN_SEMI, JOIN_ANTI, JOIN_FULL, JOIN_ANTI_NULLAWARE = 0, 1, 2, 3, 4, 5
JOIN_NIL = 0xFFFFFFFF


def join_probe(probe_keys: torch.Tensor, workspace: torch.Tensor, capacity: int,
               build_rows: int, out_cap: int, key_validity=None, probe_ws=None,
               join_type: int = JOIN_INNER):
    pn = probe_keys.numel()
    dev = probe_keys.device
    op = torch.empty(out_cap, dtype=torch.int32, device=dev)
    ob = torch.empty(out_cap, dtype=torch.int32, device=dev)
    nm = ctypes.c_int64(0)
    rc = lib().gpuq_join_probe_i64_typed(_stream(), pn, _col(probe_keys, key_validity),
                                   workspace.data_ptr(), capacity, build_rows,
                                   _dp(probe_ws),
                                   probe_ws.numel() if probe_ws is not None else 0,
                                   join_type,
                                   op.data_ptr(), ob.data_ptr(), out_cap,
                                   ctypes.byref(nm))
    if rc == 3:  # GPUQ_ERR_OVERFLOW: caller retries with nm.value capacity
        return None, None, nm.value
    _check(rc)
    return op[:nm.value], ob[:nm.value], nm.value


def _key_cols_arr(key_cols, key_validities):
    nkeys = len(key_cols)
    kv = key_validities or [None] * nkeys
    assert len(kv) == nkeys
    return (_Col * nkeys)(*[_col(k, v) for k, v in zip(key_cols, kv)])


def join_build_keys(key_cols, capacity: int, key_validities=None,
                    workspace=None):
    """Composite-key join build over (k1..kK), K <= 4 int64 columns.
    key_validities: optional list (same length) of validity bitmaps; a row
    with a NULL in any key column is not inserted. Returns the workspace."""
    nkeys = len(key_cols)
    bn = key_cols[0].numel()
    dev = key_cols[0].device
    keys_arr = _key_cols_arr(key_cols, key_validities)
    if workspace is None:
        workspace = torch.empty(
            lib().gpuq_join_keys_workspace_bytes(bn, capacity, nkeys),
            dtype=torch.uint8, device=dev)
    _check(lib().gpuq_join_build_keys(_stream(), bn, keys_arr, nkeys,
                                      workspace.data_ptr(), capacity))
    return workspace


def join_probe_keys(key_cols, workspace: torch.Tensor, capacity: int,
                    build_rows: int, out_cap: int, key_validities=None,
                    join_type: int = JOIN_INNER):
    """Probe one batch against a join_build_keys table. Returns (op, ob, n),
    or (None, None, n) on output overflow, like join_probe. JOIN_FULL sets
    matched bits only; the unmatched build rows come from
    join_keys_unmatched_build after the last batch."""
    nkeys = len(key_cols)
    pn = key_cols[0].numel()
    dev = key_cols[0].device
    keys_arr = _key_cols_arr(key_cols, key_validities)
    op = torch.empty(out_cap, dtype=torch.int32, device=dev)
    ob = torch.empty(out_cap, dtype=torch.int32, device=dev)
    nm = ctypes.c_int64(0)
    rc = lib().gpuq_join_probe_keys(_stream(), pn, keys_arr, nkeys,
                                    workspace.data_ptr(), capacity, build_rows,
                                    join_type, op.data_ptr(), ob.data_ptr(),
                                    out_cap, ctypes.byref(nm))
    if rc == 3:  # GPUQ_ERR_OVERFLOW: caller retries with nm.value capacity
        return None, None, nm.value
    _check(rc)
    return op[:nm.value], ob[:nm.value], nm.value


JOIN_SIDE_PROBE, JOIN_SIDE_BUILD = 0, 1


def lower_join_cond(cond, probe_columns: dict, build_columns: dict):
    """-> (names, sides, program): a residual join condition lowered by
    predicate.lower over the merged schema of the two sides, and for each
    column it reads the side it comes from. A column that both sides carry
    raises ValueError (ambiguous), one that neither carries too (unknown)."""
    for name in predicate.columns_of(cond):
        if name in probe_columns and name in build_columns:
            raise ValueError(f"join condition column {name!r} is ambiguous: "
                             f"both sides have it")
        if name not in probe_columns and name not in build_columns:
            raise ValueError(f"join condition reads unknown column {name!r}")
    schema = {k: t.dtype for k, t in build_columns.items()}
    schema.update({k: t.dtype for k, t in probe_columns.items()})
    names, prog = predicate.lower(cond, schema)
    sides = [JOIN_SIDE_PROBE if k in probe_columns else JOIN_SIDE_BUILD
             for k in names]
    return names, sides, prog


def join_probe_keys_cond(key_cols, workspace: torch.Tensor, capacity: int,
                         build_rows: int, out_cap: int, cond,
                         probe_columns: dict, build_columns: dict,
                         probe_validities: dict = None,
                         build_validities: dict = None, key_validities=None,
                         join_type: int = JOIN_INNER):
    """join_probe_keys with a residual join condition evaluated inside the
    probe: a key-equal (probe row, build row) pair counts as a match only if
    cond is TRUE for it (FALSE and NULL fail), which is what decides outer
    fills, semi / anti membership and full outer's matched bits.

    cond is a predicate.Pred over the columns of probe_columns (name ->
    tensor, one row per probe row) and build_columns (one row per build row
    of the table), or an already lowered (names, sides, program) triple from
    lower_join_cond. Returns (op, ob, n), or (None, None, n) on output
    overflow, like join_probe_keys."""
    probe_validities = probe_validities or {}
    build_validities = build_validities or {}
    if isinstance(cond, predicate.Pred):
        names, sides, prog = lower_join_cond(cond, probe_columns, build_columns)
    else:
        names, sides, prog = cond
    nkeys = len(key_cols)
    pn = key_cols[0].numel()
    dev = key_cols[0].device
    cols = []
    for name, side in zip(names, sides):
        src, val, rows = ((probe_columns, probe_validities, pn)
                          if side == JOIN_SIDE_PROBE
                          else (build_columns, build_validities, build_rows))
        if src[name].numel() != rows:
            raise ValueError(f"join_probe_keys_cond: column {name!r} has "
                             f"{src[name].numel()} rows, expected {rows}")
        cols.append(_col(src[name], val.get(name)))
    keys_arr = _key_cols_arr(key_cols, key_validities)
    cols_arr = (_Col * max(len(cols), 1))(*cols)
    sides_arr = (ctypes.c_int32 * max(len(sides), 1))(*sides)
    prog_arr = (_PredInsn * max(len(prog), 1))(
        *[_PredInsn(*insn) for insn in prog])
    op = torch.empty(out_cap, dtype=torch.int32, device=dev)
    ob = torch.empty(out_cap, dtype=torch.int32, device=dev)
    nm = ctypes.c_int64(0)
    rc = lib().gpuq_join_probe_keys_cond(
        _stream(), pn, keys_arr, nkeys, workspace.data_ptr(), capacity,
        build_rows, join_type, cols_arr, sides_arr, len(cols),
        prog_arr, len(prog), op.data_ptr(), ob.data_ptr(), out_cap,
        ctypes.byref(nm))
    if rc == 3:  # GPUQ_ERR_OVERFLOW: caller retries with nm.value capacity
        return None, None, nm.value
    _check(rc)
    return op[:nm.value], ob[:nm.value], nm.value


def join_keys_unmatched_build(workspace: torch.Tensor, capacity: int,
                              build_rows: int, nkeys: int):
    """(NIL, build_rid) pairs for the build rows no JOIN_FULL probe has
    matched so far. Returns (op, ob, n)."""
    dev = workspace.device
    out_cap = max(build_rows, 1)
    op = torch.empty(out_cap, dtype=torch.int32, device=dev)
    ob = torch.empty(out_cap, dtype=torch.int32, device=dev)
    nr = ctypes.c_int64(0)
    _check(lib().gpuq_join_keys_unmatched_build(
        _stream(), workspace.data_ptr(), capacity, build_rows, nkeys,
        op.data_ptr(), ob.data_ptr(), out_cap, ctypes.byref(nr)))
    return op[:nr.value], ob[:nr.value], nr.value


CMP = predicate.CMP
BINOP = {"+": 0, "-": 1, "*": 2, "/": 3, "rsub": 4}


def gather_nullable(col: torch.Tensor, perm: torch.Tensor, validity=None):
    """gather with NIL (0xFFFFFFFF) permutation entries producing NULL
    rows (outer-join build side). Returns (values, validity bitmap)."""
    n = perm.numel()
    out = torch.empty(n, dtype=col.dtype, device=col.device)
    bits = torch.empty(_bitmap_bytes(n), dtype=torch.uint8, device=col.device)
    _check(lib().gpuq_gather_nullable(_stream(), n, _col(col, validity),
                                      perm.data_ptr(),
                                      out.data_ptr(), bits.data_ptr()))
    return out, bits


def filter_cmp(col: torch.Tensor, op: str, literal, workspace=None, validity=None):
    """Stable filter: returns (perm[:count], count) — passing rows in input
    order (FilterExec replacement for col OP literal predicates).

    A NULL row never passes. float64 columns follow Spark's ordering
    (NaN == NaN, NaN greater than everything, -0.0 == 0.0); inf and NaN
    literals are passed through to the kernel.

    An int64 column compared against a float literal follows Spark's
    cast-to-double comparison semantics: the predicate is rewritten to an
    equivalent integer comparison (e.g. k < 0.5 == k <= 0), never truncated
    (k < 0.5 must keep k == 0). +/-inf and NaN literals become constant
    predicates (NaN is greater than every double a bigint casts to)."""
    n = col.numel()
    dev = col.device
    if col.dtype == torch.int64 and isinstance(literal, float):
        op, literal = rewrite_i64_float_cmp(op, literal)
    if col.dtype == torch.int64:
        lit_i = int(literal)
        lit_f = float(lit_i)
    else:
        lit_f = float(literal)   # inf / NaN included; the kernel orders them
        lit_i = 0
    if workspace is None:
        workspace = torch.empty(lib().gpuq_filter_workspace_bytes(n),
                                dtype=torch.uint8, device=dev)
    perm = torch.empty(n, dtype=torch.int32, device=dev)
    cnt = torch.zeros(1, dtype=torch.int64, device=dev)
    _check(lib().gpuq_filter_cmp(_stream(), n, _col(col, validity), CMP[op],
                                 lit_f, lit_i,
                                 perm.data_ptr(), cnt.data_ptr(),
                                 workspace.data_ptr(), workspace.numel()))
    c = int(cnt.item())
    return perm[:c], c


def filter_expr_workspace(n: int, device="cuda") -> torch.Tensor:
    return torch.empty(lib().gpuq_filter_expr_workspace_bytes(n),
                       dtype=torch.uint8, device=device)


def filter_expr(columns: dict, pred, validities: dict = None, workspace=None):
    """Stable filter on a compound predicate (spark_amd.predicate: And / Or /
    Not / In / Between / IsNull / IsNotNull / Cmp against a literal or another
    column), evaluated under SQL three-valued logic in one fused pass over the
    referenced columns. Returns (perm[:count], count): the rows for which the
    predicate is TRUE, in input order.

    columns maps name -> tensor (all of one length; only the columns the
    predicate names are read), validities name -> validity bitmap. pred may
    also be an already lowered (column_names, program) pair."""
    validities = validities or {}
    if isinstance(pred, predicate.Pred):
        names, prog = predicate.lower(
            pred, {k: t.dtype for k, t in columns.items()})
    else:
        names, prog = pred
    any_col = next(iter(columns.values()))
    n = any_col.numel()
    dev = any_col.device
    for name in names:
        if columns[name].numel() != n:
            raise ValueError(f"filter_expr: column {name!r} has "
                             f"{columns[name].numel()} rows, expected {n}")
    cols_arr = (_Col * max(len(names), 1))(
        *[_col(columns[k], validities.get(k)) for k in names])
    prog_arr = (_PredInsn * max(len(prog), 1))(
        *[_PredInsn(*insn) for insn in prog])
    if workspace is None:
        workspace = filter_expr_workspace(n, dev)
    perm = torch.empty(n, dtype=torch.int32, device=dev)
    cnt = torch.zeros(1, dtype=torch.int64, device=dev)
    _check(lib().gpuq_filter_expr(_stream(), n, cols_arr, len(names),
                                  prog_arr, len(prog),
                                  perm.data_ptr(), cnt.data_ptr(),
                                  workspace.data_ptr(), workspace.numel()))
    c = int(cnt.item())
    return perm[:c], c


def _binop_operands(a: torch.Tensor, b, literal):
    """(lit_f64, lit_i64) for a OP b after the operand type checks: a column
    b must have a's dtype, and an int64 column takes only integral literals
    (nothing is truncated or reinterpreted silently)."""
    if a.dtype not in (torch.int64, torch.float64):
        raise ValueError(f"project_binop: unsupported dtype {a.dtype}")
    if b is not None:
        if literal is not None:
            raise ValueError("project_binop: give b or literal, not both")
        if b.dtype != a.dtype:
            raise ValueError(f"project_binop: operand dtypes differ "
                             f"({a.dtype} vs {b.dtype})")
        if b.numel() != a.numel():
            raise ValueError("project_binop: operand lengths differ")
        return 0.0, 0
    if literal is None:
        raise ValueError("project_binop: needs b or literal")
    if a.dtype == torch.float64:
        return float(literal), 0
    import math
    if isinstance(literal, float) and (not math.isfinite(literal)
                                       or literal != int(literal)):
        raise ValueError(f"project_binop: non-integral literal {literal!r} "
                         f"on an int64 column")
    lit_i = int(literal)
    if not -(1 << 63) <= lit_i < (1 << 63):
        raise ValueError(f"project_binop: literal {literal!r} exceeds int64")
    return float(lit_i), lit_i


def project_binop(a: torch.Tensor, op: str, b=None, literal=None):
    """Elementwise a OP b (b: tensor or None with literal), no NULL tracking:
    the caller owns validity (AVG = sum / count derives it from the count).
    Projections over nullable inputs and any `/` whose zero divisors must
    come out NULL go through project_binop_nullable."""
    n = a.numel()
    lit_f, lit_i = _binop_operands(a, b, literal)
    out = torch.empty(n, dtype=a.dtype, device=a.device)
    _check(lib().gpuq_project_binop(_stream(), n, _col(a),
                                    b.data_ptr() if b is not None else None,
                                    lit_f, lit_i, BINOP[op], out.data_ptr()))
    return out


def project_binop_nullable(a: torch.Tensor, op: str, b=None, literal=None,
                           a_validity=None, b_validity=None):
    """NULL-aware a OP b -> (out, validity bitmap or None). A row is valid
    iff both inputs are valid and the op is not a division by zero (Spark
    non-ANSI: x / 0 is NULL; for float64 -0.0 is zero too). NULL rows hold 0.
    The bitmap is omitted only when nothing can be NULL: no input bitmap and
    op is not `/`."""
    n = a.numel()
    lit_f, lit_i = _binop_operands(a, b, literal)
    if b is None and b_validity is not None:
        raise ValueError("project_binop: a literal operand has no validity")
    out = torch.empty(n, dtype=a.dtype, device=a.device)
    bits = None
    if a_validity is not None or b_validity is not None or op == "/":
        bits = torch.empty(_bitmap_bytes(n), dtype=torch.uint8, device=a.device)
    bcol = _col(b, b_validity) if b is not None \
        else _Col(None, None, _DTYPE_MAP[a.dtype])
    _check(lib().gpuq_project_binop_nullable(
        _stream(), n, _col(a, a_validity), bcol, lit_f, lit_i, BINOP[op],
        out.data_ptr(), _dp(bits)))
    return out, bits


EXPR_TILE = 1024          # rows per block of k_expr_eval
EXPR_MAX_INSNS = expression.MAX_INSNS
EXPR_MAX_COLS = expression.MAX_COLS
EXPR_MAX_OUTS = expression.MAX_OUTS
EXPR_MAX_DEPTH = expression.MAX_DEPTH

_EXPR_TORCH = {"i64": torch.int64, "f64": torch.float64}


def project_expr_program(columns: dict, names, prog, out_names, out_dtypes,
                         out_nullable, validities: dict = None):
    """Run an already lowered program (the tuple expression.lower returns,
    plus the output names) in one gpuq_project_expr call. Returns
    {out_name: (tensor, bitmap or None)}; an output gets a bitmap only where
    out_nullable says it can hold a NULL."""
    validities = validities or {}
    if not columns:
        raise ValueError("project_expr: needs a column to take the row "
                         "count and device from")
    any_col = next(iter(columns.values()))
    n, dev = any_col.numel(), any_col.device
    for name in names:
        if columns[name].numel() != n:
            raise ValueError(f"project_expr: column {name!r} has "
                             f"{columns[name].numel()} rows, expected {n}")
    cols_arr = (_Col * max(len(names), 1))(
        *[_col(columns[k], validities.get(k)) for k in names])
    prog_arr = (_ExprInsn * max(len(prog), 1))(
        *[_ExprInsn(*insn) for insn in prog])
    nouts = len(out_names)
    outs = [torch.empty(n, dtype=_EXPR_TORCH[dt], device=dev)
            for dt in out_dtypes]
    bits = [torch.empty(_bitmap_bytes(n), dtype=torch.uint8, device=dev)
            if nl else None for nl in out_nullable]
    vp = ctypes.c_void_p
    outs_arr = (vp * max(nouts, 1))(*[t.data_ptr() for t in outs])
    bits_arr = (vp * max(nouts, 1))(*[_dp(b) for b in bits])
    dt_arr = (ctypes.c_int32 * max(nouts, 1))(
        *[expression.TYPE_CODE[dt] for dt in out_dtypes])
    _check(lib().gpuq_project_expr(_stream(), n, cols_arr, len(names),
                                   prog_arr, len(prog), outs_arr, bits_arr,
                                   dt_arr, nouts))
    return {name: (t, b) for name, t, b in zip(out_names, outs, bits)}


def project_expr(columns: dict, outputs, validities: dict = None):
    """Compound SELECT-list expressions (spark_amd.expression: arithmetic
    trees, Neg / Abs, Cast, comparisons as values, If / CaseWhen, Coalesce) in
    one fused pass: every referenced column is read once, up to EXPR_MAX_OUTS
    outputs are written. outputs is an ordered [(name, expr)] list; a later
    output that contains the whole tree of an earlier one reuses its value.
    Returns {name: (tensor, bitmap or None)}; the bitmap is None where nothing
    in the expression can be NULL.

    columns maps name -> tensor (all of one length; only the columns the
    expressions name are read), validities name -> validity bitmap."""
    validities = validities or {}
    outputs = list(outputs)
    names, prog, out_dtypes, out_nullable = expression.lower(
        outputs, {k: t.dtype for k, t in columns.items()},
        nullable=[k for k in columns if validities.get(k) is not None])
    return project_expr_program(columns, names, prog,
                                [name for name, _ in outputs], out_dtypes,
                                out_nullable, validities)


def cast_i64_f64(t: torch.Tensor) -> torch.Tensor:
    out = torch.empty(t.numel(), dtype=torch.float64, device=t.device)
    _check(lib().gpuq_cast_i64_f64(_stream(), t.numel(), t.data_ptr(), out.data_ptr()))
    return out


def range_i64(n: int, start: int = 0, step: int = 1, device="cuda") -> torch.Tensor:
    out = torch.empty(n, dtype=torch.int64, device=device)
    _check(lib().gpuq_range_i64(_stream(), n, start, step, out.data_ptr()))
    return out


def _build_agg_specs(specs, dev, mg, placeholder):
    """specs: list of (kind, col_tensor_or_None[, validity]) with kind in
    {"sum","count","count*","min","max"}. Op codes per gpuq.h:
    0=SUM_F64 1=COUNT(col) 2=COUNT(*) 3=SUM_I64 4=MIN_I64 5=MAX_I64
    6=MIN_F64 7=MAX_F64. Two kinds take a 128-bit (lo, hi) accumulator and
    expand to an op PAIR with TWO entries in outs (so indices into outs stay
    one per accumulator word; at most 12 words per call):
    ("sum_dec128", t, v) -> ops 8,9 over an int64 scaled-decimal column;
    ("merge_dec128", t_lo, v, t_hi) -> ops 10,9 over 128-bit partials.
    Returns (cols_arr, ops_arr, cid_arr, outs)."""
    cols, ops, colidx, outs = [], [], [], []
    for s in specs:
        kind = s[0]
        t = s[1] if len(s) > 1 else None
        v = s[2] if len(s) > 2 else None
        if kind in ("sum_dec128", "merge_dec128"):
            if t.dtype != torch.int64:
                raise ValueError(f"{kind} needs an int64 column")
            ops += [8 if kind == "sum_dec128" else 10, 9]
            colidx += [len(cols), len(cols)]
            cols.append(_col(t, v))
            if kind == "merge_dec128":
                if s[3].dtype != torch.int64:
                    raise ValueError("merge_dec128 needs an int64 hi column")
                colidx[-1] = len(cols)
                cols.append(_col(s[3]))
            outs += [torch.empty(mg, dtype=torch.int64, device=dev)
                     for _ in range(2)]
            continue
        if kind == "count*":
            ops.append(2); colidx.append(0)
            outs.append(torch.empty(mg, dtype=torch.int64, device=dev))
            continue
        if kind == "count":
            ops.append(1)
        elif kind == "sum":
            ops.append(3 if t.dtype == torch.int64 else 0)
        elif kind == "min":
            ops.append(4 if t.dtype == torch.int64 else 6)
        elif kind == "max":
            ops.append(5 if t.dtype == torch.int64 else 7)
        else:
            raise ValueError(f"bad agg spec kind {kind}")
        out_dtype = torch.float64 if ops[-1] in (0, 6, 7) else torch.int64
        outs.append(torch.empty(mg, dtype=out_dtype, device=dev))
        colidx.append(len(cols))
        cols.append(_col(t, v))
    if not cols:
        cols = [_col(placeholder)]  # placeholder, unused
    nspecs = len(ops)
    cols_arr = (_Col * len(cols))(*cols)
    ops_arr = (ctypes.c_int32 * nspecs)(*ops)
    cid_arr = (ctypes.c_int32 * nspecs)(*colidx)
    return cols_arr, ops_arr, cid_arr, outs


def agg_multi_workspace(capacity: int, nspecs: int, device="cuda"):
    return torch.empty(lib().gpuq_hash_agg_multi_workspace_bytes(capacity, nspecs),
                       dtype=torch.uint8, device=device)


def hash_agg_multi(keys: torch.Tensor, specs, capacity: int, key_validity=None,
                   max_groups=None, workspace=None, first_batch=True,
                   finalize=True):
    """Multi-accumulator GROUP BY (single int64 key). specs per
    _build_agg_specs. Multiple batches accumulate into the same workspace
    (first_batch=True resets it; finalize=True compacts) — the
    whole-partition aggregation contract. Returns (keys, key_valid,
    [acc_j...]) sliced to ngroups, or None before finalize."""
    n = keys.numel()
    dev = keys.device
    mg = max_groups or capacity + 2
    cols_arr, ops_arr, cid_arr, outs = _build_agg_specs(specs, dev, mg, keys)
    nspecs = len(outs)  # accumulator words (a dec128 spec is two)
    outp_arr = (ctypes.c_void_p * nspecs)(*[t.data_ptr() for t in outs])
    if workspace is None:
        workspace = agg_multi_workspace(capacity, nspecs, dev)
    ok = torch.empty(mg, dtype=torch.int64, device=dev)
    okv = torch.empty(mg, dtype=torch.uint8, device=dev)
    ng = ctypes.c_int64(0)
    _check(lib().gpuq_hash_agg_multi(
        _stream(), n, _col(keys, key_validity), cols_arr, ops_arr, cid_arr,
        nspecs, workspace.data_ptr(), capacity, int(first_batch),
        int(finalize), ok.data_ptr(), okv.data_ptr(),
        outp_arr, ctypes.byref(ng)))
    if not finalize:
        return None
    gn = ng.value
    return ok[:gn], okv[:gn], [t[:gn] for t in outs]


def hash_agg_keys(key_cols, specs, capacity: int, key_validities=None,
                  max_groups=None, workspace=None, first_batch=True,
                  finalize=True):
    """Composite-key GROUP BY (k1..kK), K <= 4 int64 columns.
    key_validities: optional list (same length) of validity bitmaps.
    Returns (key_out_cols list, kmask u8 tensor, [acc_j...]) sliced to
    ngroups; kmask bit c = key column c non-NULL in that group."""
    nkeys = len(key_cols)
    n = key_cols[0].numel()
    dev = key_cols[0].device
    kv = key_validities or [None] * nkeys
    mg = max_groups or capacity + 2
    cols_arr, ops_arr, cid_arr, outs = _build_agg_specs(specs, dev, mg, key_cols[0])
    nspecs = len(outs)
    outp_arr = (ctypes.c_void_p * nspecs)(*[t.data_ptr() for t in outs])
    keys_arr = (_Col * nkeys)(*[_col(k, v) for k, v in zip(key_cols, kv)])
    okeys = [torch.empty(mg, dtype=torch.int64, device=dev) for _ in range(nkeys)]
    okp_arr = (ctypes.c_void_p * nkeys)(*[t.data_ptr() for t in okeys])
    omask = torch.empty(mg, dtype=torch.uint8, device=dev)
    if workspace is None:
        workspace = torch.empty(
            lib().gpuq_hash_agg_keys_workspace_bytes(capacity, nkeys, nspecs),
            dtype=torch.uint8, device=dev)
    ng = ctypes.c_int64(0)
    _check(lib().gpuq_hash_agg_keys(
        _stream(), n, keys_arr, nkeys, cols_arr, ops_arr, cid_arr, nspecs,
        workspace.data_ptr(), capacity, int(first_batch), int(finalize),
        okp_arr, omask.data_ptr(), outp_arr, ctypes.byref(ng)))
    if not finalize:
        return None
    gn = ng.value
    return [t[:gn] for t in okeys], omask[:gn], [t[:gn] for t in outs]


def partition_perm_multi(key_cols, nparts: int, workspace=None,
                         key_validities=None):
    """Stable group-by-partition permutation over a composite key tuple
    (seed-chained Murmur3, hash.scala:849-860)."""
    nkeys = len(key_cols)
    n = key_cols[0].numel()
    dev = key_cols[0].device
    kv = key_validities or [None] * nkeys
    if workspace is None:
        workspace = partition_workspace(n, nparts, dev)
    keys_arr = (_Col * nkeys)(*[_col(k, v) for k, v in zip(key_cols, kv)])
    perm = torch.empty(n, dtype=torch.int32, device=dev)
    counts = torch.empty(nparts, dtype=torch.int64, device=dev)
    _check(lib().gpuq_partition_perm_multi(
        _stream(), n, keys_arr, nkeys, nparts, perm.data_ptr(),
        counts.data_ptr(), workspace.data_ptr(), workspace.numel()))
    return perm, counts


def _bitmap_bytes(n: int) -> int:
    return (n + 7) // 8


def gather_bits(bits: torch.Tensor, perm: torch.Tensor) -> torch.Tensor:
    """Permute a validity bitmap: out bit i = bits[perm[i]]."""
    n = perm.numel()
    out = torch.empty(_bitmap_bytes(n), dtype=torch.uint8, device=perm.device)
    _check(lib().gpuq_gather_bits(_stream(), n, bits.data_ptr(), perm.data_ptr(),
                                  out.data_ptr()))
    return out


def bits_to_u8(bits: torch.Tensor, n: int) -> torch.Tensor:
    out = torch.empty(n, dtype=torch.uint8, device=bits.device)
    _check(lib().gpuq_bits_to_u8(_stream(), n, bits.data_ptr(), out.data_ptr()))
    return out


def u8_to_bits(u8: torch.Tensor) -> torch.Tensor:
    n = u8.numel()
    out = torch.empty(_bitmap_bytes(n), dtype=torch.uint8, device=u8.device)
    _check(lib().gpuq_u8_to_bits(_stream(), n, u8.data_ptr(), out.data_ptr()))
    return out


def nonzero_to_bits(col: torch.Tensor) -> torch.Tensor:
    """bit i = (col[i] != 0) — NULL-ness of merged aggregates from a merged
    COUNT column (Sum.scala: NULL iff no non-null input)."""
    n = col.numel()
    out = torch.empty(_bitmap_bytes(n), dtype=torch.uint8, device=col.device)
    _check(lib().gpuq_nonzero_to_bits(_stream(), n, col.data_ptr(), out.data_ptr()))
    return out


def dec128_overflow_to_null(lo: torch.Tensor, hi: torch.Tensor,
                            result_precision: int, validity_bits=None):
    """Clear validity bit i where |(hi[i], lo[i])| >= 10**result_precision
    (Sum.scala: non-ANSI decimal overflow evaluates to NULL). Updates
    validity_bits in place (all-valid when None) and returns it."""
    n = lo.numel()
    if validity_bits is None:
        validity_bits = torch.full((_bitmap_bytes(n),), 0xFF, dtype=torch.uint8,
                                   device=lo.device)
    _check(lib().gpuq_dec128_overflow_to_null(
        _stream(), n, lo.data_ptr(), hi.data_ptr(), result_precision,
        validity_bits.data_ptr()))
    return validity_bits


def dec128_to_pyints(lo: torch.Tensor, hi: torch.Tensor):
    """(lo, hi) int64 word columns -> list of Python ints,
    (hi << 64) | (lo & (2**64-1)). Host-side helper (copies to the CPU)."""
    m = (1 << 64) - 1
    return [(h << 64) | (l & m)
            for l, h in zip(lo.cpu().tolist(), hi.cpu().tolist())]


def maskbit_to_bits(mask: torch.Tensor, bit: int) -> torch.Tensor:
    """Per-key-column validity bitmap from hash_agg_keys' kmask."""
    n = mask.numel()
    out = torch.empty(_bitmap_bytes(n), dtype=torch.uint8, device=mask.device)
    _check(lib().gpuq_maskbit_to_bits(_stream(), n, mask.data_ptr(), bit,
                                      out.data_ptr()))
    return out


def minmax_i64(col: torch.Tensor, validity=None):
    """(min, max, valid_count) of an int64 column; (None, None, 0) if no
    valid rows."""
    out = torch.empty(3, dtype=torch.int64, device=col.device)
    _check(lib().gpuq_minmax_i64(_stream(), col.numel(), _col(col, validity),
                                 out.data_ptr()))
    enc = out.cpu().tolist()
    sign = 1 << 63
    cnt = enc[2]
    if cnt == 0:
        return None, None, 0
    # decode_i64: e ^ SIGNBIT (two's complement)
    def dec(e):
        v = (e & 0xFFFFFFFFFFFFFFFF) ^ sign
        return v - (1 << 64) if v >= sign else v
    return dec(enc[0]), dec(enc[1]), cnt


def pack2_i64(a: torch.Tensor, b: torch.Tensor, a_bias: int, b_bias: int,
              shift: int) -> torch.Tensor:
    out = torch.empty(a.numel(), dtype=torch.int64, device=a.device)
    _check(lib().gpuq_pack2_i64(_stream(), a.numel(), a.data_ptr(), b.data_ptr(),
                                a_bias, b_bias, shift, out.data_ptr()))
    return out


def unpack2_i64(packed: torch.Tensor, a_bias: int, b_bias: int, shift: int):
    n = packed.numel()
    a = torch.empty(n, dtype=torch.int64, device=packed.device)
    b = torch.empty(n, dtype=torch.int64, device=packed.device)
    _check(lib().gpuq_unpack2_i64(_stream(), n, packed.data_ptr(), a_bias, b_bias,
                                  shift, a.data_ptr(), b.data_ptr()))
    return a, b


def range_partition_perm(keys: torch.Tensor, bounds: torch.Tensor, desc=False,
                         nulls_first=None, workspace=None, key_validity=None):
    """Stable range partition (RangePartitioning analog): returns
    (perm, counts[len(bounds)+1])."""
    n = keys.numel()
    dev = keys.device
    if nulls_first is None:
        nulls_first = not desc
    nparts = bounds.numel() + 1
    if workspace is None:
        workspace = partition_workspace(n, nparts, dev)
    perm = torch.empty(n, dtype=torch.int32, device=dev)
    counts = torch.empty(nparts, dtype=torch.int64, device=dev)
    _check(lib().gpuq_range_partition_perm(
        _stream(), n, _col(keys, key_validity), int(desc), int(nulls_first),
        bounds.data_ptr(), bounds.numel(), perm.data_ptr(), counts.data_ptr(),
        workspace.data_ptr(), workspace.numel()))
    return perm, counts


def hash_agg_partitioned(keys: torch.Tensor, vals: torch.Tensor, capacity: int,
                         workspace=None, max_groups=None, key_validity=None,
                         ops=AGG_SUM | AGG_COUNT):
    """Partitioned aggregation (bucket-ordered + LDS chunk tables); same
    results contract as hash_agg for non-null values."""
    n = keys.numel()
    dev = keys.device
    if workspace is None:
        workspace = torch.empty(lib().gpuq_hash_agg_part_workspace_bytes(n, capacity),
                                dtype=torch.uint8, device=dev)
    mg = max_groups if max_groups is not None else min(n + 2, capacity + 2)
    ok = torch.empty(mg, dtype=torch.int64, device=dev)
    okv = torch.empty(mg, dtype=torch.uint8, device=dev)
    osum = torch.empty(mg, dtype=torch.float64, device=dev)
    osv = torch.empty(mg, dtype=torch.uint8, device=dev)
    ocnt = torch.empty(mg, dtype=torch.int64, device=dev)
    ng = ctypes.c_int64(0)
    _check(lib().gpuq_hash_agg_partitioned(
        _stream(), n, _col(keys, key_validity), _col(vals),
        workspace.data_ptr(), capacity, ops,
        ok.data_ptr(), okv.data_ptr(), osum.data_ptr(), osv.data_ptr(),
        ocnt.data_ptr(), ctypes.byref(ng)))
    gn = ng.value
    return ok[:gn], okv[:gn], osum[:gn], osv[:gn], ocnt[:gn]


# ---------------- window functions (segmented scans) ----------------
# mirrors of the #defines in csrc/gpuq.hip: rows per block of the window
# kernels, and the number of tile summaries one step of the carry kernel
# covers
WIN_TILE = 2048
WIN_CARRY_SPAN = 2048

WIN_OP = {"row_number": 0, "rank": 1, "dense_rank": 2, "count": 3, "sum": 4,
          "min": 5, "max": 6}
WIN_FRAME = {"rows": 0, "range": 1, "partition": 2}


def _bitmap_words(n: int) -> int:
    return (n + 63) // 64


def window_boundaries(keys, validities, npart: int, n: int = None):
    """Partition-start and peer-group-start bitmaps of a batch sorted by
    (partition keys, order keys): keys[:npart] are the partition columns,
    keys[npart:] the order columns (int64 / float64), validities a list of
    the same length (entries may be None) or None. Returns (part_bits,
    peer_bits), int64 tensors of ceil(n / 64) words, LSB-first. n is taken
    from the keys; it must be given when there are none (one partition of
    one peer group)."""
    keys = list(keys)
    nkeys = len(keys)
    validities = list(validities) if validities is not None else [None] * nkeys
    if len(validities) != nkeys:
        raise ValueError(f"window_boundaries: {nkeys} keys but "
                         f"{len(validities)} validity entries")
    if not 0 <= npart <= nkeys:
        raise ValueError(f"window_boundaries: npart {npart} outside 0..{nkeys}")
    if nkeys == 0:
        if n is None:
            raise ValueError("window_boundaries: n is needed without keys")
        dev = "cuda"
    else:
        if n is None:
            n = keys[0].numel()
        dev = keys[0].device
    for k in keys:
        if k.dtype not in (torch.int64, torch.float64):
            raise ValueError(f"window_boundaries: unsupported dtype {k.dtype}")
        if k.numel() != n:
            raise ValueError(f"window_boundaries: key has {k.numel()} rows, "
                             f"expected {n}")
    part = torch.empty(_bitmap_words(n), dtype=torch.int64, device=dev)
    peer = torch.empty(_bitmap_words(n), dtype=torch.int64, device=dev)
    arr = (_Col * max(nkeys, 1))(*[_col(k, v) for k, v in zip(keys, validities)])
    _check(lib().gpuq_window_boundaries(_stream(), n, arr, nkeys, npart,
                                        part.data_ptr(), peer.data_ptr()))
    return part, peer


def window_workspace(n: int, device="cuda") -> torch.Tensor:
    return torch.empty(lib().gpuq_window_workspace_bytes(n), dtype=torch.uint8,
                       device=device)


def _check_bitmaps(who: str, n: int, *bitmaps):
    for b in bitmaps:
        if b.dtype != torch.int64 or b.numel() != _bitmap_words(n):
            raise ValueError(f"{who}: a boundary bitmap must be "
                             f"{_bitmap_words(n)} int64 words for {n} rows")


def window_scan(op: str, frame: str, part_bits, peer_bits, val=None,
                validity=None, n: int = None, workspace=None):
    """One window expression over the bitmaps of window_boundaries. op:
    row_number / rank / dense_rank (frame "rows", no val), count (val=None
    is COUNT(*)), sum / min / max; frame: "rows" | "range" | "partition"
    (every frame starts at UNBOUNDED PRECEDING). Returns (out,
    out_validity_or_None): the bitmap only for sum / min / max over a column
    that has one. n is taken from val and must be given without it."""
    if op not in WIN_OP:
        raise ValueError(f"window_scan: bad op {op!r}")
    if frame not in WIN_FRAME:
        raise ValueError(f"window_scan: bad frame {frame!r}")
    rank_op = WIN_OP[op] <= 2
    if rank_op and (val is not None or frame != "rows"):
        raise ValueError(f"window_scan: {op} takes no column and the rows frame")
    if val is None:
        if validity is not None:
            raise ValueError("window_scan: validity without a column")
        if op in ("sum", "min", "max"):
            raise ValueError(f"window_scan: {op} needs a column")
        if n is None:
            raise ValueError("window_scan: n is needed without a column")
    else:
        if val.dtype not in (torch.int64, torch.float64):
            raise ValueError(f"window_scan: unsupported dtype {val.dtype}")
        if n is not None and n != val.numel():
            raise ValueError("window_scan: n differs from the column length")
        n = val.numel()
    _check_bitmaps("window_scan", n, part_bits, peer_bits)
    dev = part_bits.device
    if workspace is None:
        workspace = window_workspace(n, dev)
    out_dtype = torch.float64 if (val is not None and val.dtype == torch.float64
                                  and op in ("sum", "min", "max")) else torch.int64
    out = torch.empty(n, dtype=out_dtype, device=dev)
    bits = None
    if validity is not None and op in ("sum", "min", "max"):
        bits = torch.empty(_bitmap_bytes(n), dtype=torch.uint8, device=dev)
    col = _col(val, validity) if val is not None else _Col(None, None, GPUQ_INT64)
    _check(lib().gpuq_window_scan(_stream(), n, WIN_OP[op], WIN_FRAME[frame], col,
                                  part_bits.data_ptr(), peer_bits.data_ptr(),
                                  out.data_ptr(), _dp(bits),
                                  workspace.data_ptr(), workspace.numel()))
    return out, bits


def window_shift(val, offset: int, part_bits, validity=None, default=None,
                 workspace=None):
    """lag (offset < 0) / lead (offset > 0) inside the partitions of
    part_bits: out[i] = val[i + offset] with its own NULL-ness, or `default`
    (NULL when None) where that row is outside i's partition. Returns (out,
    out_validity). An int64 column takes only an integral default."""
    if val.dtype not in (torch.int64, torch.float64):
        raise ValueError(f"window_shift: unsupported dtype {val.dtype}")
    n = val.numel()
    _check_bitmaps("window_shift", n, part_bits)
    lit_f, lit_i = 0.0, 0
    if default is not None:
        if val.dtype == torch.float64:
            lit_f = float(default)
        else:
            import math
            if isinstance(default, float) and (not math.isfinite(default)
                                               or default != int(default)):
                raise ValueError(f"window_shift: non-integral default "
                                 f"{default!r} on an int64 column")
            lit_i = int(default)
            if not -(1 << 63) <= lit_i < (1 << 63):
                raise ValueError(f"window_shift: default {default!r} exceeds int64")
    offset = int(offset)
    if not -(1 << 63) <= offset < (1 << 63):
        raise ValueError("window_shift: offset exceeds int64")
    dev = val.device
    if workspace is None:
        workspace = window_workspace(n, dev)
    out = torch.empty(n, dtype=val.dtype, device=dev)
    bits = torch.empty(_bitmap_bytes(n), dtype=torch.uint8, device=dev)
    _check(lib().gpuq_window_shift(_stream(), n, _col(val, validity), offset,
                                   int(default is not None), lit_f, lit_i,
                                   part_bits.data_ptr(), out.data_ptr(),
                                   bits.data_ptr(), workspace.data_ptr(),
                                   workspace.numel()))
    return out, bits


# ---------------- sliding ROWS BETWEEN frames, first_value / last_value ----
# the ops gpuq_window_slide takes on top of count / sum / min / max
WIN_SLIDE_OP = {"first_value": 7, "last_value": 8}
WIN_SLIDE_MAX_SPAN = 2048            # GPUQ_WIN_SLIDE_MAX_SPAN
_WIN_UNBOUNDED_PRECEDING = -(1 << 63)
_WIN_UNBOUNDED_FOLLOWING = (1 << 63) - 1


def _slide_ops():
    ops = {k: WIN_OP[k] for k in ("count", "sum", "min", "max")}
    ops.update(WIN_SLIDE_OP)
    return ops


def _slide_frame(who: str, lo, hi):
    """(lo, hi) as the C entry point takes them; None is unbounded."""
    for name, b in (("lo", lo), ("hi", hi)):
        if b is None:
            continue
        if isinstance(b, bool) or not isinstance(b, int):
            raise ValueError(f"{who}: {name} must be an int or None, got {b!r}")
        if not -(1 << 31) <= b < (1 << 31):
            raise ValueError(f"{who}: {name} {b} does not fit int32")
    if lo is not None and hi is None:
        raise ValueError(f"{who}: a finite lo ({lo}) with an unbounded hi is "
                         "not supported")
    if lo is not None:
        if lo > hi:
            raise ValueError(f"{who}: lo {lo} > hi {hi}")
        if hi - lo > WIN_SLIDE_MAX_SPAN:
            raise ValueError(f"{who}: span {hi - lo} exceeds "
                             f"{WIN_SLIDE_MAX_SPAN}")
    return (_WIN_UNBOUNDED_PRECEDING if lo is None else lo,
            _WIN_UNBOUNDED_FOLLOWING if hi is None else hi)


def window_slide_workspace(n: int, lo, hi, device="cuda") -> torch.Tensor:
    clo, chi = _slide_frame("window_slide_workspace", lo, hi)
    if not 0 <= n <= 0xFFFFFFFF:
        raise ValueError(f"window_slide_workspace: nrows {n} out of range")
    return torch.empty(lib().gpuq_window_slide_workspace_bytes(n, clo, chi),
                       dtype=torch.uint8, device=device)


def window_slide(op: str, lo, hi, part_bits, val=None, validity=None,
                 n: int = None, workspace=None):
    """One window expression over the frame ROWS BETWEEN lo AND hi: signed row
    offsets from the current row (negative PRECEDING, positive FOLLOWING),
    None for UNBOUNDED. Both finite with hi - lo <= WIN_SLIDE_MAX_SPAN, or lo
    None. op: count (val=None is COUNT(*)), sum / min / max, first_value /
    last_value. Returns (out, out_validity_or_None): no bitmap for count, and
    none for sum / min / max over a column without one under a frame that
    cannot be empty (lo <= 0 <= hi). n is taken from val and must be given
    without it."""
    ops = _slide_ops()
    if op not in ops:
        raise ValueError(f"window_slide: bad op {op!r}")
    clo, chi = _slide_frame("window_slide", lo, hi)
    if val is None:
        if validity is not None:
            raise ValueError("window_slide: validity without a column")
        if op != "count":
            raise ValueError(f"window_slide: {op} needs a column")
        if n is None:
            raise ValueError("window_slide: n is needed without a column")
    else:
        if val.dtype not in (torch.int64, torch.float64):
            raise ValueError(f"window_slide: unsupported dtype {val.dtype}")
        if n is not None and n != val.numel():
            raise ValueError("window_slide: n differs from the column length")
        n = val.numel()
    if not 0 <= n <= 0xFFFFFFFF:
        raise ValueError(f"window_slide: nrows {n} out of range")
    _check_bitmaps("window_slide", n, part_bits)
    dev = part_bits.device
    need = lib().gpuq_window_slide_workspace_bytes(n, clo, chi)
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    elif workspace.numel() < need:
        raise ValueError(f"window_slide: workspace {workspace.numel()} < {need}")
    out_dtype = torch.int64 if op == "count" else val.dtype
    out = torch.empty(n, dtype=out_dtype, device=dev)
    can_be_empty = (lo is not None and lo > 0) or (hi is not None and hi < 0)
    bits = None
    if op in WIN_SLIDE_OP or (op != "count" and (validity is not None
                                                 or can_be_empty)):
        bits = torch.empty(_bitmap_bytes(n), dtype=torch.uint8, device=dev)
    col = _col(val, validity) if val is not None else _Col(None, None, GPUQ_INT64)
    _check(lib().gpuq_window_slide(_stream(), n, ops[op], col, clo, chi,
                                   part_bits.data_ptr(), out.data_ptr(),
                                   _dp(bits), workspace.data_ptr(),
                                   workspace.numel()))
    return out, bits
