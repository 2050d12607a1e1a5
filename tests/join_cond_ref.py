"""Nested-loop reference for equi-joins with a residual join condition
(gpuq_join_probe_keys_cond, the `condition` of the hash-join nodes).

It knows nothing about hashing: every probe row is compared with every build
row. Two rows are a CANDIDATE pair iff all key columns are non-NULL on both
sides and equal; a candidate PASSES iff pred_ref.eval_row on the merged row
(probe columns and build columns under their own names) is True — False and
None (SQL NULL) both fail. The join types follow HashJoin.scala with "match"
read as "passing pair":

  0 inner       every passing pair
  1 outer       every passing pair; a probe row without one pairs with NIL
  2 left semi   (i, NIL) iff some pair passes
  3 left anti   (i, NIL) iff no pair passes
  4 full outer  as 1, plus the build rows in no passing pair ("unmatched")

The outer loop is Python; the inner loop over the build rows is one numpy
comparison per key column, so the parity-sized tables stay quick.
tests/test_join_cond_ref.py pins this to a hand-written table.

Key columns are (values, valid) pairs, valid None or one bool per row;
condition columns map name -> (values, valid, dtype) as in pred_ref.
"""
import numpy as np

import pred_ref

NIL = 0xFFFFFFFF
INNER, OUTER, SEMI, ANTI, FULL = range(5)


def _valid(valid, n):
    return np.ones(n, bool) if valid is None else np.asarray(valid, bool)


def candidate_lists(probe_keys, build_keys):
    """-> for each probe row the ascending list of key-equal build rows."""
    assert len(probe_keys) == len(build_keys) and probe_keys
    pn, bn = len(probe_keys[0][0]), len(build_keys[0][0])
    bvals = [np.asarray(k) for k, _ in build_keys]
    bok = np.ones(bn, bool)
    for _, v in build_keys:
        bok &= _valid(v, bn)
    pvalid = [_valid(v, pn) for _, v in probe_keys]
    out = []
    for i in range(pn):
        if not all(v[i] for v in pvalid):
            out.append([])
            continue
        eq = bok.copy()
        for (pk, _), bk in zip(probe_keys, bvals):
            eq &= bk == pk[i]
        out.append(np.flatnonzero(eq).tolist())
    return out


def _rows(cols):
    """name -> (values, valid, dtype)  ->  name -> list of values / None"""
    return {k: pred_ref._pyrows(*c) for k, c in cols.items()}


def verdicts(cands, probe_cols, build_cols, pred):
    """-> for each probe row [(build row, True / False / None)], one entry
    per candidate, in candidate order."""
    assert not set(probe_cols) & set(build_cols)
    dtypes = {k: c[2] for k, c in {**probe_cols, **build_cols}.items()}
    prow, brow = _rows(probe_cols), _rows(build_cols)
    out = []
    for i, cs in enumerate(cands):
        row = {k: v[i] for k, v in prow.items()}
        res = []
        for j in cs:
            row.update({k: v[j] for k, v in brow.items()})
            res.append((j, pred_ref.eval_row(pred, row, dtypes)))
        out.append(res)
    return out


def join_pairs(verd, join_type, build_rows):
    """-> (sorted (probe_rid, build_rid) pairs with NIL for the fills,
    sorted unmatched build rows — empty unless join_type is FULL)."""
    pairs, matched = [], set()
    for i, res in enumerate(verd):
        passing = [j for j, t in res if t is True]
        matched.update(passing)
        if join_type == INNER:
            pairs += [(i, j) for j in passing]
        elif join_type in (OUTER, FULL):
            pairs += [(i, j) for j in passing] if passing else [(i, NIL)]
        elif join_type == SEMI:
            pairs += [(i, NIL)] if passing else []
        elif join_type == ANTI:
            pairs += [] if passing else [(i, NIL)]
        else:
            raise ValueError(join_type)
    unmatched = ([j for j in range(build_rows) if j not in matched]
                 if join_type == FULL else [])
    return sorted(pairs), unmatched


def join_cond_ref(probe_keys, build_keys, probe_cols, build_cols, pred,
                  join_type):
    """The whole reference in one call: -> (pairs, unmatched_build)."""
    cands = candidate_lists(probe_keys, build_keys)
    verd = verdicts(cands, probe_cols, build_cols, pred)
    return join_pairs(verd, join_type, len(build_keys[0][0]))
