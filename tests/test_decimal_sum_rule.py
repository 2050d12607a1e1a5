"""CPU-side checks of the exact decimal SUM plumbing: the ColumnarRule
carries "sum_decimal" and decimal_precision onto the GPU node, the node's
output schema per mode, the (lo, hi) -> Python int helper, and the spec-op
pairing validation of the C ABI (which runs before any HIP call)."""
import ctypes
import os
import subprocess

import pytest

torch = pytest.importorskip("torch")

from spark_amd import exec as gx  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "spark_amd", "libgpuq.so")


def _leaf():
    return gx.InputBatches([gx.ColumnarBatch(
        {"k": torch.zeros(1, dtype=torch.int64),
         "v": torch.zeros(1, dtype=torch.int64)})])


def _gpu_node(mode, **kw):
    plan = gx.HashAggregateExec("k", [("sum_decimal", "v"), ("count*", None)],
                                mode, _leaf(), **kw)
    return gx.GpuColumnarRule().pre_columnar_transitions(plan)


def test_rule_preserves_sum_decimal_and_precision():
    node = _gpu_node("complete", decimal_precision={"v": 12})
    assert isinstance(node, gx.GpuHashAggregateExec)
    assert node.aggs == [("sum_decimal", "v"), ("count*", None)]
    assert node.decimal_precision == {"v": 12}
    assert node._result_precision("v") == 22
    # default input precision is 18 -> decimal(28, s)
    assert _gpu_node("complete").decimal_precision is None
    assert _gpu_node("complete")._result_precision("v") == 28


@pytest.mark.parametrize("mode", ["final", "complete"])
def test_output_final_and_complete(mode):
    assert _gpu_node(mode).output == [
        "k", "sum_decimal_lo(v)", "sum_decimal_hi(v)", "count(1)"]


def test_output_partial_lists_the_buffer_columns():
    assert _gpu_node("partial").output == [
        "k", "dsum_lo(v)", "dsum_hi(v)", "count(v)", "count(1)"]


def test_dec128_to_pyints_round_trip():
    from spark_amd import gpuq
    xs = [2**127 - 1, -(2**127 - 1), -1, 0, 2**64]
    m = (1 << 64) - 1

    def signed(w):
        return w - (1 << 64) if w >> 63 else w
    lo = torch.tensor([signed(x & m) for x in xs], dtype=torch.int64)
    hi = torch.tensor([signed((x >> 64) & m) for x in xs], dtype=torch.int64)
    assert gpuq.dec128_to_pyints(lo, hi) == xs


def test_spec_pairing_is_validated_before_any_hip_call():
    if not os.path.exists(SO):
        subprocess.run(["make", "-C", os.path.join(ROOT, "spark_amd", "csrc"),
                        "-s"], check=True)
    L = ctypes.CDLL(SO)
    L.gpuq_last_error.restype = ctypes.c_char_p
    i32, i64, vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p

    class Col(ctypes.Structure):
        _fields_ = [("data", vp), ("validity", vp), ("dtype", i32)]

    L.gpuq_hash_agg_multi.restype = i32
    L.gpuq_hash_agg_multi.argtypes = [vp, i64, Col, vp, vp, vp, i32, vp, i64,
                                      i32, i32, vp, vp, vp, vp]
    L.gpuq_hash_agg_keys.restype = i32
    L.gpuq_hash_agg_keys.argtypes = [vp, i64, vp, i32, vp, vp, vp, i32, vp,
                                     i64, i32, i32, vp, vp, vp, vp]
    cols = (Col * 2)(Col(None, None, 0), Col(None, None, 1))  # int64, float64
    key = (Col * 1)(Col(None, None, 0))
    for ops, cids, word in [([2, 8], [0, 0], b"followed by op 9"),
                            ([10], [0], b"followed by op 9"),
                            ([8, 3], [0, 0], b"followed by op 9"),
                            ([9], [0], b"must follow"),
                            ([2, 9], [0, 0], b"must follow"),
                            ([8, 9], [1, 1], b"int64"),
                            ([10, 9], [0, 1], b"int64")]:
        k = len(ops)
        a_ops, a_cids = (i32 * k)(*ops), (i32 * k)(*cids)
        rc = L.gpuq_hash_agg_multi(None, 8, key[0], cols, a_ops, a_cids, k,
                                   None, 1024, 1, 1, None, None, None, None)
        assert rc == 2 and word in L.gpuq_last_error(), (ops, "multi")
        rc = L.gpuq_hash_agg_keys(None, 8, key, 1, cols, a_ops, a_cids, k,
                                  None, 1024, 1, 1, None, None, None, None)
        assert rc == 2 and word in L.gpuq_last_error(), (ops, "keys")
    rc = L.gpuq_dec128_overflow_to_null(None, i64(8), None, None, 39, None)
    assert rc == 2 and b"precision" in L.gpuq_last_error()
