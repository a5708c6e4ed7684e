"""The query model (tests/query_model.py) against SQLite's own answers (tests/golden/query_kats.json) and its
pivot against the oracle's merged state. CPU only."""
import json
import os

import numpy as np
import pytest

from oracle import oracle as O
from tests import query_model as M

HERE = os.path.dirname(os.path.abspath(__file__))


def dec(v):
    if isinstance(v, dict):
        if "f" in v:
            return float.fromhex(v["f"])
        return v["t"] if "t" in v else bytes.fromhex(v["b"])
    return v


def cell_of(v):
    """a Python value as the stored cell the engine would hold (inline or long)"""
    if v is None:
        return M.NULL_CELL
    if isinstance(v, int):
        return (M.INTEGER, 0, v & M.M64, 0, None)
    if isinstance(v, float):
        return (M.REAL, 0, int.from_bytes(np.float64(v).tobytes(), "little"), 0, None)
    b = v.encode() if isinstance(v, str) else bytes(v)
    ty = M.TEXT if isinstance(v, str) else M.BLOB
    if len(b) > 16:
        return (ty, M.VAL_LONG, int.from_bytes(b[:8], "big"), 0, b)
    p = b + b"\0" * (16 - len(b))
    return (ty, len(b), int.from_bytes(p[:8], "big"), int.from_bytes(p[8:], "big"), None)


@pytest.fixture(scope="module")
def kats():
    with open(os.path.join(HERE, "golden", "query_kats.json")) as f:
        return json.load(f)


def same(a, b):
    """equal as SQLite values: the class too (5 is not 5.0), and -0.0 is not 0.0"""
    return type(a) is type(b) and (a.hex() == b.hex() if isinstance(a, float) else a == b)


def test_model_agrees_with_sqlite_on_every_fixture_case(kats):
    names = [c[0] for c in kats["columns"]]
    types = [c[1] for c in kats["columns"]]
    rows = {}
    for r in kats["rows"]:
        vals = [M.apply_affinity(dec(v), t, comparing=False) for v, t in zip(r[1:], types)]
        rows[r[0] & M.M64] = {"cl": 1, "cells": [cell_of(v) for v in vals]}
    assert len(kats["cases"]) > 900
    for n, case in enumerate(kats["cases"]):
        where = [[tuple([t[0], t[1]] + [dec(v) for v in t[2:]]) for t in g] for g in case["where"]]
        got = M.query(rows, where, case["columns"], col_names=names, decl_types=types)
        pks = [p - (1 << 64) if p >> 63 else p for p in got["pk"]]
        assert pks == case["pks"], (n, case["where"])
        for cells, want in zip(got["cells"], case["values"]):
            assert len(cells) == len(want)
            for c, w in zip(cells, want):
                assert same(M.py_value(c), dec(w)), (n, case["where"])


def test_keyed_form_statuses():
    rows = {1: {"cl": 1, "cells": [cell_of(5)]}, 2: {"cl": 3, "cells": [cell_of(None)]}}
    got = M.query(rows, [[("a", ">", 1)]], ["a"], keys=[2, 9, 1, 7, 1], col_names=["a"], dead={7: {}})
    assert got["key_status"] == [3, 0, 1, 2, 1] and got["key_index"] == [2, 4] and got["pk"] == [1, 1]


def batch(changes):
    """(table, pk, cid, col_version, db_version, cl, seq, site, INTEGER value)"""
    a = np.array(changes, dtype=np.int64).reshape(-1, 9)
    return {"pk": a[:, 1].astype(np.uint64), "table_cid": ((a[:, 0] << 16) | a[:, 2]).astype(np.uint32),
            "col_version": a[:, 3], "db_version": a[:, 4], "cl": a[:, 5].astype(np.uint32), "seq": a[:, 6].astype(np.uint32),
            "site": a[:, 7].astype(np.uint32), "val0": a[:, 8].astype(np.uint64)}


def test_materialise_follows_the_oracle_through_insert_delete_and_resurrect():
    schema = {"t0": ["a", "b"], "t1": ["a", "b"]}
    fold = O.Fold(np.arange(32, dtype=np.uint8).reshape(2, 16))
    fold.apply(batch([(0, 1, 1, 1, 1, 1, 0, 0, 10), (0, 1, 2, 1, 1, 1, 1, 0, 11),      # row 1: inserted
                      (0, 2, 1, 1, 1, 1, 2, 0, 20), (1, 1, 2, 1, 1, 1, 3, 0, 99),      # row 2; pk 1 in table 1, b only
                      (0, 3, 1, 1, 1, 1, 4, 0, 30)]))
    live, dead = M.materialise(fold.export(), schema)
    assert {pk: [M.py_value(c) for c in r["cells"]] for pk, r in live[0].items()} == {1: [10, 11], 2: [20, None], 3: [30, None]}
    assert [M.py_value(c) for c in live[1][1]["cells"]] == [None, 99]
    fold.apply(batch([(0, 2, 0, 2, 2, 2, 0, 1, 0)]))                                   # row 2 deleted
    live, dead = M.materialise(fold.export(), schema)
    assert sorted(live[0]) == [1, 3] and sorted(dead[0]) == [2] and dead[0][2]["cl"] == 2
    fold.apply(batch([(0, 2, 0, 3, 3, 3, 0, 1, 0), (0, 2, 2, 1, 3, 3, 1, 1, 77)]))      # resurrected: b alone written
    live, dead = M.materialise(fold.export(), schema)
    assert live[0][2]["cl"] == 3 and [M.py_value(c) for c in live[0][2]["cells"]] == [None, 77]
    assert not dead.get(0)
