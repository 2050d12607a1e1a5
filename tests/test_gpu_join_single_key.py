"""GPU parity for the single-key typed probe (gpuq_join_build_i64 /
gpuq_join_probe_i64_typed, join types 0-5) against a plain Python dict join,
at the points nothing else tests directly: the key -1 (the table's EMPTY
sentinel, kept on its own chain) under every join type, chains longer than
two on that chain, and an output buffer exactly as large as the result.
Join order is unspecified, so pairs compare as sorted lists."""
import collections

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

I64_MIN = -(1 << 63)
NIL = 0xFFFFFFFF
CAP = 1024
BUILD_ROWS = 600
PROBE_ROWS = 4096 + 300      # two probe blocks of 4096 rows, the last partial


@pytest.fixture(scope="module")
def gq():
    from spark_amd import gpuq
    assert torch.cuda.is_available()
    return gpuq


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def pack_validity(valid_bool):
    return torch.from_numpy(np.packbits(valid_bool, bitorder="little")).cuda()


def pair_list(op, ob):
    p = op.cpu().numpy().view(np.uint32).tolist()
    b = ob.cpu().numpy().view(np.uint32).tolist()
    return sorted(zip(p, b))


def make_build():
    rng = np.random.RandomState(1)
    # ~3 rows per key: chains of 1, 2, 3 and more all occur
    keys = rng.randint(0, 200, size=BUILD_ROWS).astype(np.int64)
    valid = rng.randint(0, 10, size=BUILD_ROWS) != 0          # ~10 % NULL
    keys[[5, 77, 130, 311, 599]] = -1                        # a chain of 5
    valid[[5, 77, 130, 311, 599]] = True
    keys[42] = I64_MIN
    valid[42] = True
    nulls = np.flatnonzero(~valid)
    keys[nulls[::3]] = -1          # NULL rows whose data word is -1
    return keys, valid


def make_probe():
    rng = np.random.RandomState(2)
    # build keys cover [0, 200): about half of [0, 400) misses
    keys = rng.randint(0, 400, size=PROBE_ROWS).astype(np.int64)
    valid = rng.randint(0, 10, size=PROBE_ROWS) != 0          # ~10 % NULL
    for i in (0, 63, 64, 1000, 4095, 4096, 4200, PROBE_ROWS - 1):
        keys[i] = -1
        valid[i] = True
    keys[[7, 4100]] = I64_MIN
    valid[[7, 4100]] = True
    nulls = np.flatnonzero(~valid)
    keys[nulls[::4]] = -1
    return keys, valid


def reference(bkeys, bvalid, pkeys, pvalid, jt):
    """sorted (probe row, build row) pairs of join type jt, NIL for 'none'"""
    rows = collections.defaultdict(list)
    for j, (k, ok) in enumerate(zip(bkeys.tolist(), bvalid.tolist())):
        if ok:
            rows[k].append(j)
    out, touched = [], set()
    for i, (k, ok) in enumerate(zip(pkeys.tolist(), pvalid.tolist())):
        hits = rows.get(k, []) if ok else []
        if jt in (0, 1, 4):
            out += [(i, b) for b in hits]
            touched.update(hits)
            if not hits and jt != 0:
                out.append((i, NIL))
        elif jt == 2:
            if hits:
                out.append((i, NIL))
        elif jt == 3:
            if not hits:
                out.append((i, NIL))
        else:   # 5: a NULL probe key counts as matched
            if ok and not hits:
                out.append((i, NIL))
    if jt == 4:   # never-matched build rows, NULL-key rows among them
        out += [(NIL, j) for j in range(len(bkeys)) if j not in touched]
    return sorted(out)


@pytest.fixture(scope="module")
def data(gq):
    bkeys, bvalid = make_build()
    pkeys, pvalid = make_probe()
    assert (bkeys[bvalid] == -1).sum() >= 3 and (bkeys[~bvalid] == -1).any()
    assert (pkeys[pvalid] == -1).sum() >= 3
    ws = gq.join_build(to_dev(bkeys), CAP, key_validity=pack_validity(bvalid))
    ref = {jt: reference(bkeys, bvalid, pkeys, pvalid, jt) for jt in range(6)}
    return dict(ws=ws, pkeys=to_dev(pkeys), pvalid=pack_validity(pvalid), ref=ref)


@pytest.mark.parametrize("jt", range(6))
def test_pairs_match_reference(gq, data, jt):
    exp = data["ref"][jt]
    assert exp, "reference is empty: the case checks nothing"
    # once with room to spare, once with a buffer exactly as large as the result
    for out_cap in (len(exp) + 1000, len(exp)):
        op, ob, n = gq.join_probe(data["pkeys"], data["ws"], CAP, BUILD_ROWS,
                                  out_cap, key_validity=data["pvalid"],
                                  join_type=jt)
        assert n == len(exp), (jt, out_cap)
        assert op is not None, (jt, out_cap)
        assert pair_list(op, ob) == exp, (jt, out_cap)


def test_inner_one_slot_short_reports_count(gq, data):
    exp = data["ref"][0]
    op, ob, n = gq.join_probe(data["pkeys"], data["ws"], CAP, BUILD_ROWS,
                              len(exp) - 1, key_validity=data["pvalid"],
                              join_type=0)
    assert (op, ob, n) == (None, None, len(exp))


@pytest.mark.parametrize("jt", [0, 1, 4])
@pytest.mark.parametrize("empty", ["build", "probe"])
def test_empty_side(gq, jt, empty):
    bkeys, bvalid = make_build()
    pkeys, pvalid = make_probe()
    if empty == "build":
        bkeys, bvalid = bkeys[:0], bvalid[:0]
    else:
        pkeys, pvalid = pkeys[:0], pvalid[:0]
    exp = reference(bkeys, bvalid, pkeys, pvalid, jt)
    ws = gq.join_build(to_dev(bkeys), CAP, key_validity=pack_validity(bvalid))
    op, ob, n = gq.join_probe(to_dev(pkeys), ws, CAP, len(bkeys), len(exp) + 8,
                              key_validity=pack_validity(pvalid), join_type=jt)
    assert n == len(exp)
    assert pair_list(op, ob) == exp
