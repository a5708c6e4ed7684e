"""bench.py --dump-outputs (dump_outputs) on CPU: the files depend on the exported state only, not on
the export's row order; every stored number is exact in float64; the sample stays inside its byte
budget and is the same set of cells whatever else the state holds."""
import os

import numpy as np

import bench
from corrosion_amd.engine import ROW_FIELDS


class _State:
    """Stands in for a MergeEngine: export() / db_versions() of a fixed state, rows in `order`."""

    def __init__(self, rows, order):
        self.rows = {k: v[order] for k, v in rows.items()}

    def export(self):
        return dict(self.rows, long_values={})

    def db_versions(self):
        return np.arange(7, dtype=np.int64)


def _rows(m, seed=1):
    rng = np.random.default_rng(seed)
    rows = {k: rng.integers(0, 1 << (8 * np.dtype(dt).itemsize - 1), size=m, dtype=np.int64).astype(dt)
            for k, dt in ROW_FIELDS.items()}
    rows["val0"] = rng.integers(-(1 << 63), (1 << 63) - 1, size=m, dtype=np.int64).view(np.uint64)
    rows["pk"] = np.arange(1, m + 1, dtype=np.uint64)
    return rows


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def _join(d, f):
    return (d[f"rows_{f}_hi"].astype(np.uint64) << np.uint64(32)) | d[f"rows_{f}_lo"].astype(np.uint64)


def test_dump_is_independent_of_export_order_and_exact(tmp_path):
    m = 5000
    rows = _rows(m)
    rng = np.random.default_rng(2)
    budget = 64 << 10
    bench.dump_outputs(_State(rows, np.arange(m)), str(tmp_path / "a"), budget=budget)
    bench.dump_outputs(_State(rows, rng.permutation(m)), str(tmp_path / "b"), budget=budget)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].dtype == np.float64 and np.array_equal(a[k], b[k]), k
    assert a["count"].tolist() == [m] and a["db_versions"].tolist() == list(range(7))
    # a sample, inside the budget, of whole rows of the state, sorted by (table_cid, pk)
    n = len(a["rows_pk_lo"])
    assert 0 < n < m and sum(v.nbytes for k, v in a.items() if k.startswith("rows_")) <= budget
    pk = _join(a, "pk")
    at = pk.astype(np.int64) - 1            # pk i + 1 is row i of `rows`
    for f, dt in ROW_FIELDS.items():
        got = _join(a, f) if np.dtype(dt).itemsize == 8 else a[f"rows_{f}"].astype(np.uint64)
        assert np.array_equal(got, rows[f][at].astype(np.uint64)), f
    key = list(zip(a["rows_table_cid"].tolist(), pk.tolist()))
    assert key == sorted(key)
    # the checksums are over every row, as (upper, lower) halves of the wrapping 64-bit sums
    for i, f in enumerate(ROW_FIELDS):
        s = int(rows[f].astype(np.uint64).sum(dtype=np.uint64))
        assert a["checksum"][i].tolist() == [s >> 32, s & 0xFFFFFFFF], f


def test_dump_samples_the_same_cells_of_a_larger_state(tmp_path):
    """The sample is chosen by a hash of (pk, table_cid) alone: rows that differ elsewhere are seen."""
    m = 5000
    rows = _rows(m)
    other = {k: v.copy() for k, v in rows.items()}
    other["val0"] = other["val0"] + np.uint64(1)
    budget = 64 << 10
    bench.dump_outputs(_State(rows, np.arange(m)), str(tmp_path / "a"), budget=budget)
    bench.dump_outputs(_State(other, np.arange(m)), str(tmp_path / "b"), budget=budget)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert np.array_equal(_join(a, "pk"), _join(b, "pk"))
    assert np.array_equal(a["rows_table_cid"], b["rows_table_cid"])
    assert np.array_equal(_join(a, "val0") + np.uint64(1), _join(b, "val0"))
    assert not np.array_equal(a["checksum"], b["checksum"])


def test_dump_of_a_small_state_keeps_every_row(tmp_path):
    m = 40
    bench.dump_outputs(_State(_rows(m), np.arange(m)), str(tmp_path / "a"))
    a = _load(tmp_path / "a")
    assert sorted(_join(a, "pk").tolist()) == list(range(1, m + 1))
