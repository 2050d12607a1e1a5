"""CPU tests of the composite-key join: tuple keys on the join plan nodes and
through the ColumnarRule, constructor contracts, and the C-ABI's argument
validation (which runs before any HIP call, so it is checkable without a
GPU). No GPU calls here."""
import ctypes
import os
import subprocess

import pytest

from spark_amd import exec as gx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "spark_amd", "libgpuq.so")


def leaf():
    scan = gx.InputBatches.__new__(gx.InputBatches)  # leaf without data
    gx.SparkPlan.__init__(scan)
    scan._batches = []
    return scan


def rule(plan, **kw):
    return gx.GpuColumnarRule(**kw).pre_columnar_transitions(plan)


# ---------------- tuple keys through the rule ----------------

@pytest.mark.parametrize("lk,rk", [(("a", "b"), ("c", "d")),
                                   (["a", "b", "e"], ["c", "d", "f"]),
                                   (("a", "b", "e", "g"), ("c", "d", "f", "h"))])
def test_shj_tuple_keys_through_rule(lk, rk):
    cpu = gx.ShuffledHashJoinExec(lk, rk, "right", leaf(), leaf(),
                                  join_type="left_outer")
    assert cpu.left_keys == tuple(lk) and cpu.right_keys == tuple(rk)
    plan = rule(cpu)
    assert type(plan) is gx.GpuShuffledHashJoinExec
    assert plan.left_key == lk and plan.right_key == rk   # kept as passed
    assert plan.left_keys == tuple(lk) and plan.right_keys == tuple(rk)
    assert plan.join_type == "left_outer" and plan.build_side == "right"
    dists = plan.required_child_distribution()
    assert [d.kind for d in dists] == ["clustered", "clustered"]
    assert dists[0].keys == tuple(lk) and dists[1].keys == tuple(rk)


def test_smj_tuple_keys_ordering_and_rule():
    smj = gx.SortMergeJoinExec(("a", "b"), ("c", "d"), leaf(), leaf())
    assert smj.left_keys == ("a", "b") and smj.right_keys == ("c", "d")
    assert [o.key for o in smj.output_ordering] == ["a", "b"]
    plan = rule(smj)
    assert isinstance(plan, gx.GpuSortExec)
    assert [o.key for o in plan.output_ordering] == ["a", "b"]
    join = plan.children[0]
    assert isinstance(join, gx.GpuShuffledHashJoinExec)
    assert join.left_keys == ("a", "b") and join.right_keys == ("c", "d")
    assert join.build_side == "right"
    dists = join.required_child_distribution()
    assert dists[0].keys == ("a", "b") and dists[1].keys == ("c", "d")

    ro = gx.SortMergeJoinExec(("a", "b"), ("c", "d"), leaf(), leaf(),
                              join_type="right_outer")
    assert [o.key for o in ro.output_ordering] == ["c", "d"]
    plan = rule(ro)
    assert isinstance(plan, gx.GpuSortExec)
    assert [o.key for o in plan.output_ordering] == ["c", "d"]
    assert plan.children[0].build_side == "left"

    fo = gx.SortMergeJoinExec(("a", "b"), ("c", "d"), leaf(), leaf(),
                              join_type="full_outer")
    assert fo.output_ordering == []
    assert isinstance(rule(fo), gx.GpuShuffledHashJoinExec)
    assert isinstance(rule(smj, preserve_smj_ordering=False),
                      gx.GpuShuffledHashJoinExec)


def test_bhj_tuple_keys_through_rule():
    bx = gx.BroadcastExchangeExec(leaf())
    bhj = gx.BroadcastHashJoinExec(("a", "b"), ("c", "d"), "right", leaf(), bx)
    assert bhj.left_keys == ("a", "b") and bhj.right_keys == ("c", "d")
    plan = rule(bhj)
    assert isinstance(plan, gx.GpuBroadcastHashJoinExec)
    assert plan.left_keys == ("a", "b") and plan.right_keys == ("c", "d")
    assert plan.join_type == "inner"
    dists = plan.required_child_distribution()
    assert dists[1].kind == "broadcast" and dists[0].kind == "unspecified"


def test_bhj_join_type_passes_through_rule():
    bx = gx.BroadcastExchangeExec(leaf())
    bhj = gx.BroadcastHashJoinExec(("a", "b"), ("c", "d"), "right", leaf(), bx,
                                   join_type="left_semi")
    plan = rule(bhj)
    assert isinstance(plan, gx.GpuBroadcastHashJoinExec)
    assert plan.join_type == "left_semi"


# ---------------- string keys: exactly as before ----------------

def test_string_keys_unchanged():
    shj = gx.ShuffledHashJoinExec("a", "b", "right", leaf(), leaf())
    assert shj.left_key == "a" and shj.right_key == "b"
    assert shj.left_keys == ("a",) and shj.right_keys == ("b",)
    plan = rule(shj)
    assert plan.left_key == "a" and plan.right_key == "b"
    assert plan.left_keys == ("a",) and plan.right_keys == ("b",)
    dists = plan.required_child_distribution()
    assert dists == [gx.Distribution("clustered", ("a",)),
                     gx.Distribution("clustered", ("b",))]
    smj = gx.SortMergeJoinExec("a", "b", leaf(), leaf())
    assert [o.key for o in smj.output_ordering] == ["a"]
    assert smj.left_keys == ("a",)
    bhj = gx.BroadcastHashJoinExec("a", "b", "left", leaf(), leaf())
    assert bhj.left_key == "a" and bhj.left_keys == ("a",)
    # a one-element sequence is a single key too
    one = rule(gx.ShuffledHashJoinExec(("a",), ("b",), "right", leaf(), leaf()))
    assert one.left_keys == ("a",) and one.left_key == ("a",)


# ---------------- constructor contracts ----------------

NODES = [
    lambda lk, rk: gx.ShuffledHashJoinExec(lk, rk, "right", leaf(), leaf()),
    lambda lk, rk: gx.SortMergeJoinExec(lk, rk, leaf(), leaf()),
    lambda lk, rk: gx.BroadcastHashJoinExec(lk, rk, "right", leaf(), leaf()),
    lambda lk, rk: gx.GpuShuffledHashJoinExec(lk, rk, "right", leaf(), leaf()),
    lambda lk, rk: gx.GpuBroadcastHashJoinExec(lk, rk, "right", leaf(), leaf()),
]


@pytest.mark.parametrize("make", NODES)
def test_constructor_rejects_bad_key_tuples(make):
    with pytest.raises(AssertionError):
        make(("a", "b"), ("c",))                       # unequal counts
    with pytest.raises(AssertionError):
        make("a", ("c", "d"))
    with pytest.raises(AssertionError):
        make(tuple("abcde"), tuple("fghij"))           # more than 4 keys
    with pytest.raises(AssertionError):
        make((), ())
    make(tuple("abcd"), tuple("efgh"))                 # 4 is allowed


def test_null_aware_anti_is_single_key_only():
    with pytest.raises(AssertionError):
        gx.GpuShuffledHashJoinExec(("a", "b"), ("c", "d"), "right", leaf(),
                                   leaf(), join_type="left_anti",
                                   null_aware_anti=True)
    with pytest.raises(AssertionError):
        gx.GpuBroadcastHashJoinExec(("a", "b"), ("c", "d"), "right", leaf(),
                                    leaf(), join_type="left_anti",
                                    null_aware_anti=True)
    gx.GpuShuffledHashJoinExec("a", "c", "right", leaf(), leaf(),
                               join_type="left_anti", null_aware_anti=True)
    gx.GpuShuffledHashJoinExec(("a",), ("c",), "right", leaf(), leaf(),
                               join_type="left_anti", null_aware_anti=True)


# ---------------- C-ABI validation without a GPU ----------------

GPUQ_ERR_INVALID = 2
GPUQ_INT64, GPUQ_FLOAT64 = 0, 1


class Col(ctypes.Structure):
    _fields_ = [("data", ctypes.c_void_p), ("validity", ctypes.c_void_p),
                ("dtype", ctypes.c_int32)]


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(SO):
        subprocess.run(["make", "-C", os.path.join(ROOT, "spark_amd", "csrc"),
                        "-s"], check=True)
    lib = ctypes.CDLL(SO)
    i32, i64, vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
    lib.gpuq_last_error.restype = ctypes.c_char_p
    lib.gpuq_join_keys_workspace_bytes.restype = i64
    lib.gpuq_join_keys_workspace_bytes.argtypes = [i64, i64, i32]
    lib.gpuq_join_build_keys.restype = i32
    lib.gpuq_join_build_keys.argtypes = [vp, i64, ctypes.POINTER(Col), i32,
                                         vp, i64]
    lib.gpuq_join_probe_keys.restype = i32
    lib.gpuq_join_probe_keys.argtypes = [vp, i64, ctypes.POINTER(Col), i32,
                                         vp, i64, i64, i32, vp, vp, i64,
                                         ctypes.POINTER(i64)]
    lib.gpuq_join_keys_unmatched_build.restype = i32
    lib.gpuq_join_keys_unmatched_build.argtypes = [vp, vp, i64, i64, i32,
                                                   vp, vp, i64,
                                                   ctypes.POINTER(i64)]
    return lib


def cols(*dtypes):
    return (Col * max(len(dtypes), 1))(*[Col(None, None, d) for d in dtypes])


def invalid(L, rc, *needles):
    msg = L.gpuq_last_error()
    assert rc == GPUQ_ERR_INVALID, (rc, msg)
    assert msg, "gpuq_last_error() is empty"
    for n in needles:
        assert n in msg, msg
    return True


def build(L, keys, nkeys, cap, rows=10):
    return L.gpuq_join_build_keys(None, rows, keys, nkeys, None, cap)


def probe(L, keys, nkeys, cap, jt, rows=10, brows=10):
    nm = ctypes.c_int64(-7)
    return L.gpuq_join_probe_keys(None, rows, keys, nkeys, None, cap, brows,
                                  jt, None, None, 0, ctypes.byref(nm))


def unmatched(L, nkeys, cap, brows=10):
    nr = ctypes.c_int64(-7)
    return L.gpuq_join_keys_unmatched_build(None, None, cap, brows, nkeys,
                                            None, None, 0, ctypes.byref(nr))


@pytest.mark.parametrize("nkeys", [0, 5, -1])
def test_cabi_rejects_bad_nkeys(L, nkeys):
    k = cols(*[GPUQ_INT64] * 5)
    assert invalid(L, build(L, k, nkeys, 16), b"nkeys")
    assert invalid(L, probe(L, k, nkeys, 16, 0), b"nkeys")
    assert invalid(L, unmatched(L, nkeys, 16), b"nkeys")
    assert L.gpuq_join_keys_workspace_bytes(10, 16, nkeys) == 0


@pytest.mark.parametrize("cap", [24, 0, -16])
def test_cabi_rejects_non_power_of_two_capacity(L, cap):
    k = cols(GPUQ_INT64, GPUQ_INT64)
    assert invalid(L, build(L, k, 2, cap), b"power of two")
    assert invalid(L, probe(L, k, 2, cap, 0), b"power of two")
    assert invalid(L, unmatched(L, 2, cap), b"power of two")


@pytest.mark.parametrize("nkeys,bad", [(1, 0), (2, 1), (4, 3), (3, 0)])
def test_cabi_rejects_non_int64_key(L, nkeys, bad):
    dts = [GPUQ_INT64] * nkeys
    dts[bad] = GPUQ_FLOAT64
    k = cols(*dts)
    assert invalid(L, build(L, k, nkeys, 16), b"int64")
    assert invalid(L, probe(L, k, nkeys, 16, 0), b"int64")


@pytest.mark.parametrize("jt", [5, 6, -1])
def test_cabi_rejects_bad_join_type(L, jt):
    k = cols(GPUQ_INT64, GPUQ_INT64)
    assert invalid(L, probe(L, k, 2, 16, jt))
    k1 = cols(GPUQ_INT64)
    assert invalid(L, probe(L, k1, 1, 16, jt))   # NAAJ: not through this ABI


def test_cabi_rejects_oversized_build(L):
    k = cols(GPUQ_INT64, GPUQ_INT64)
    assert invalid(L, build(L, k, 2, 1 << 33, rows=0x7FFFFFFF), b"31-bit")


def test_workspace_bytes_follows_the_slot_stride(L):
    """32 B slots for 1-2 keys, 64 B for 3-4: the table term doubles between
    2 and 3 keys and is flat within each pair. Pure arithmetic, no device."""
    ws = [L.gpuq_join_keys_workspace_bytes(1000, 2048, n) for n in (1, 2, 3, 4)]
    assert ws[0] == ws[1] and ws[2] == ws[3]
    assert ws[2] - ws[1] == 2048 * 32
    big = L.gpuq_join_keys_workspace_bytes(1000, 4096, 2)
    assert big - ws[1] == 2048 * 32
    assert ws[0] >= 2048 * 32 + 1000 * 4 + 1000 // 8


def test_new_symbols_declared_in_header_form():
    # tests/test_cabi.py derives its export list from declarations that
    # start a line as `int name(` / `int64_t name(`
    import re
    syms = [m.group(1) for line in open(os.path.join(ROOT, "include", "gpuq.h"))
            for m in [re.match(r"^(?:int|int64_t)\s+(gpuq_\w+)\(", line)] if m]
    for s in ["gpuq_join_keys_workspace_bytes", "gpuq_join_build_keys",
              "gpuq_join_probe_keys", "gpuq_join_keys_unmatched_build"]:
        assert s in syms
