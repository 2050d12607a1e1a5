"""Operand checks of the projection entry points that need no GPU: the
Python wrapper rejects mixed operand types before anything is launched, and
gpuq_project_binop_nullable validates its arguments before any HIP call."""
import ctypes
import math
import os
import subprocess

import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "spark_amd", "libgpuq.so")


@pytest.fixture(scope="module")
def gpuq():
    # always through make: a library older than its source (one built from
    # an earlier commit, say) lacks the entry point tested here
    subprocess.run(["make", "-C", os.path.join(ROOT, "spark_amd", "csrc"), "-s"],
                   check=True)
    from spark_amd import gpuq as g
    return g


def test_wrapper_operand_checks(gpuq):
    ai = torch.zeros(4, dtype=torch.int64)
    af = torch.zeros(4, dtype=torch.float64)
    ok = gpuq._binop_operands
    assert ok(ai, None, 3) == (3.0, 3)
    assert ok(ai, None, 2.0) == (2.0, 2)          # integral float literal
    assert ok(ai, None, -(1 << 63))[1] == -(1 << 63)
    assert ok(af, None, 3) == (3.0, 0)
    assert ok(af, None, math.inf)[0] == math.inf
    assert math.isnan(ok(af, None, math.nan)[0])
    assert ok(ai, ai, None) == (0.0, 0)
    for a, b, lit in [(ai, None, 0.5),            # would truncate to 0
                      (ai, None, math.nan), (ai, None, math.inf),
                      (ai, None, 1 << 63),        # beyond int64
                      (ai, af, None), (af, ai, None),   # bits reinterpreted
                      (ai, ai[:2], None),         # ragged
                      (ai, ai, 1), (ai, None, None),
                      (torch.zeros(4, dtype=torch.int32), None, 1)]:
        with pytest.raises(ValueError):
            ok(a, b, lit)


def test_c_entry_point_validates_before_launch(gpuq):
    L = gpuq.lib()
    Col = gpuq._Col
    I64, F64 = gpuq.GPUQ_INT64, gpuq.GPUQ_FLOAT64
    fake = 0x1000   # never dereferenced: every call below fails validation

    def call(n, a, b, op, bits):
        return L.gpuq_project_binop_nullable(None, n, a, b, 0.0, 0,
                                             gpuq.BINOP[op], fake, bits)

    a = Col(fake, None, I64)
    assert call(8, a, Col(fake, None, F64), "+", fake) == 2
    assert b"dtypes differ" in L.gpuq_last_error()
    assert call(8, a, Col(None, fake, I64), "+", fake) == 2
    assert b"literal" in L.gpuq_last_error()
    assert call(8, Col(fake, None, gpuq.GPUQ_INT32), Col(None, None, I64),
                "+", fake) == 2
    assert b"dtype" in L.gpuq_last_error()
    assert L.gpuq_project_binop_nullable(None, 8, a, Col(None, None, I64),
                                         0.0, 0, 7, fake, fake) == 2
    assert b"bad op" in L.gpuq_last_error()
    # without an output bitmap nothing may be able to produce a NULL
    for aa, bb, op in [(Col(fake, fake, I64), Col(None, None, I64), "+"),
                       (a, Col(fake, fake, I64), "*"),
                       (a, Col(None, None, I64), "/")]:
        assert call(8, aa, bb, op, None) == 2
        assert b"output bitmap" in L.gpuq_last_error()
    # the plain entry point refuses a nullable input outright
    assert L.gpuq_project_binop(None, 8, Col(fake, fake, I64), None, 0.0, 0,
                                0, fake) == 2
    assert b"nullable" in L.gpuq_last_error()
