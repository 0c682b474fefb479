"""bench.py --dump-outputs (host logic only): the files depend on the table's rows, not on their order."""
import numpy as np
import pytest

import bench
import mhm2_proxy_amd as m


class _Finished:
    """Stands where a finished KmerCounter stands: fetch() returns the table."""

    def __init__(self, table):
        self.table = table

    def fetch(self):
        return self.table


@pytest.mark.parametrize("k,n", [(21, 200_000), (63, 30_000), (21, 0)])
def test_dump_is_order_independent_and_exact(tmp_path, monkeypatch, k, n):
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 1 << 20)  # small enough that the sample is a part of the rows
    nl = k // 32 + 1
    rng = np.random.default_rng(k)
    keys = np.unique(rng.integers(0, 2 ** 63, size=(n, nl), dtype=np.uint64) * np.uint64(2) + np.uint64(1), axis=0)
    n = len(keys)
    t = m.KmerTable(k, keys, rng.integers(2, 65536, n).astype(np.uint16), rng.integers(65, 90, n).astype(np.uint8),
                    rng.integers(65, 90, n).astype(np.uint8))
    st = dict(n_out=n, distinct=3 * n, occurrences=40 * n, count_sum=int(t.counts.sum()))
    p = rng.permutation(n)
    t2 = m.KmerTable(k, keys[p], t.counts[p], t.left[p], t.right[p])
    a = bench.dump_outputs(_Finished(t), st, tmp_path / "a")
    b = bench.dump_outputs(_Finished(t2), st, tmp_path / "b", rank=2)
    assert a["sample_rows"] == b["sample_rows"] <= n and a["bytes"] <= 64 << 20
    if n:
        assert 0 < a["sample_rows"] < n
    got = {}
    for name in ("totals", "keys", "counts", "left", "right"):
        x, y = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}_rank2.npy")
        assert x.dtype in (np.float32, np.float64)
        assert x.shape == y.shape and (x == y).all(), name
        got[name] = x
    assert got["totals"][:5].tolist() == [n, 3 * n, 40 * n, st["count_sum"], st["count_sum"]]
    assert got["totals"][7:].tolist() == [int(keys[:, w].sum(dtype=np.uint64)) & ((1 << 48) - 1) for w in range(nl)]
    # the sampled rows are rows of the table, whole and in key order
    words = (got["keys"][:, 0::2].astype(np.uint64) << np.uint64(32)) | got["keys"][:, 1::2].astype(np.uint64)
    row_of = {tuple(r): i for i, r in enumerate(keys.tolist())}
    idx = np.array([row_of[tuple(r)] for r in words.tolist()], dtype=np.int64)
    assert (np.diff(idx) > 0).all()  # keys is sorted (np.unique), so key order is ascending row index
    assert (got["counts"] == t.counts[idx]).all() and (got["left"] == t.left[idx]).all()
    assert (got["right"] == t.right[idx]).all()
