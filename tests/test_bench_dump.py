"""bench.py --dump-outputs: the float64 encoding is exact for full-range
int64, and the dumped arrays are the sort step's real outputs."""
import numpy as np
import pytest

import oracle

torch = pytest.importorskip("torch")


def _join_halves(d, stem):
    hi = np.load(d / f"{stem}_hi.npy")
    lo = np.load(d / f"{stem}_lo.npy")
    assert hi.dtype == np.float64 and lo.dtype == np.float64
    return (hi.astype(np.int64) << 32) | lo.astype(np.int64)


def test_i64_split_is_exact(tmp_path):
    import bench
    i64 = np.iinfo(np.int64)
    a = np.array([i64.min, i64.min + 1, -(1 << 53) - 1, -1, 0, 1,
                  (1 << 32) - 1, 1 << 32, (1 << 53) + 1, i64.max - 1, i64.max],
                 dtype=np.int64)
    bench._save_i64_split(str(tmp_path / "x"), torch.from_numpy(a))
    assert (_join_halves(tmp_path, "x") == a).all()


def test_plain_run_rejects_workload_selection(monkeypatch, capsys):
    import bench
    monkeypatch.setattr("sys.argv", ["bench.py", "--workloads", "agg"])
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 2 and "--full" in capsys.readouterr().err


@pytest.mark.gpu
@pytest.mark.parametrize("rows", [100_003, (1 << 20) + 12_345])
def test_dump_matches_oracle_sort(tmp_path, rows):
    """rows <= 2^20 dumps every position; above it, the seeded sample."""
    import bench
    from spark_amd import gpuq as gq
    w = bench.SortWorkload(gq, rows, rank=0)
    w.step()
    w.step()
    bench.dump_sort_outputs(w, str(tmp_path))
    w.free()

    keys = oracle.gen_i64(seed=42, n=rows)
    pay1 = oracle.gen_i64(seed=43, n=rows)
    pay2 = oracle.gen_f64_unit(seed=44, n=rows)
    perm = oracle.sort_perm(keys).astype(np.uint32).astype(np.int64)
    if rows <= bench.DUMP_SAMPLE_ROWS:
        pos = np.arange(rows)
    else:
        pos = np.sort(np.random.default_rng(bench.DUMP_SAMPLE_SEED).integers(
            0, rows, bench.DUMP_SAMPLE_ROWS, dtype=np.int64))
    got_perm = np.load(tmp_path / "sort_perm.npy")
    assert got_perm.dtype == np.float64 and got_perm.shape == pos.shape
    assert (got_perm.astype(np.int64) == perm[pos]).all()
    assert (_join_halves(tmp_path, "sort_keys") == keys[perm[pos]]).all()
    assert (_join_halves(tmp_path, "sort_payload_i64") == pay1[perm[pos]]).all()
    got_f = np.load(tmp_path / "sort_payload_f64.npy")
    assert got_f.dtype == np.float64
    assert (got_f == pay2[perm[pos]]).all()
    total = sum(p.stat().st_size for p in tmp_path.iterdir())
    assert total <= 64_000_000
