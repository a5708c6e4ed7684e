"""The seeded state and the seeded random predicates of the row-query parity test (tests/test_gpu_query.py),
kept apart from it so that the generator can be checked where no GPU is (tests/test_query_gen.py): three
tables -- "ta" keyed by its INTEGER pk with declared column types, "tb" the same without any, "tc" interned --
about 2,000 rows with deletes, resurrections, sentinel-only rows, rows without a sentinel and long values.
"""
import numpy as np

from tests import query_model as M

SCHEMA = {"ta": ["i", "r", "s", "n", "b"], "tb": ["x", "y", "z"], "tc": ["u", "v"]}
TYPES = {"ta": ["INTEGER", "REAL", "TEXT", "NUMERIC", "BLOB"], "tb": None, "tc": None}
INTERNED = ("tc",)
N_ROWS = {"ta": 800, "tb": 700, "tc": 500}
LONG_T = ["long-text-value-%04d-tail" % k for k in range(12)] + ["long-tex" + "q" * 12, "long-text-value-"]
LONG_B = [b"\x00long-blob-value-" + bytes([k, 255 - k]) * 3 for k in range(8)]
POOL = ([None] * 3 + list(range(0, 40)) + [-5, -1, 2**53 + 1, 2**63 - 1, -2**63] + [k + 0.5 for k in range(20)] + [3.0, 1e20, -7.25]
        + ["a", "ab", "abc", "b", "", "12", " 7 ", "3.5", "1e3", "x1", "abcdefgh", "abcdefghi", "abcdefghijklmnop"] + LONG_T
        + [b"", b"\x00", b"ab", b"abc", b"\xff" * 16] + LONG_B)
OPS = ("=", "!=", "<", "<=", ">", ">=")


def pk_of(table, k):
    """the k-th row's key: ta's run through the negatives, tb's overlap them, tc's are the interned ids 0.."""
    return {"ta": (k - 300) & M.M64, "tb": k + 1, "tc": k}[table]


def history(seed=7):
    """(batches, rows): the batches as lists of (table index, pk, cid, col_version, db_version, cl, seq, site,
    Python value), and per table {pk: ("live" | "dead", [the raw value written per column or None])}."""
    rng = np.random.default_rng(seed)
    names = list(SCHEMA)
    b1, b2, b3, rows = [], [], [], {t: {} for t in names}
    for ti, t in enumerate(names):
        nc = len(SCHEMA[t])
        for k in range(N_ROWS[t]):
            pk = pk_of(t, k)
            if k % 10 == 9:                                      # a sentinel and no cell
                b1.append((ti, pk, 0, 1, 1, 1, len(b1), 0, None))
                rows[t][pk] = ["live", [None] * nc]
                continue
            vals = [POOL[int(rng.integers(len(POOL)))] for _ in range(nc)]
            for c, v in enumerate(vals):                         # cells and no sentinel
                b1.append((ti, pk, c + 1, 1, 1, 1, len(b1), 0, v))
            rows[t][pk] = ["live", vals]
            if k % 7 == 3:                                       # deleted
                b2.append((ti, pk, 0, 2, 2, 2, len(b2), 0, None))
                rows[t][pk] = ["dead", [None] * nc]
                if k % 21 == 3:                                  # and resurrected with its first column alone
                    v = POOL[int(rng.integers(len(POOL)))]
                    b3.append((ti, pk, 0, 3, 3, 3, len(b3), 0, None))
                    b3.append((ti, pk, 1, 1, 3, 3, len(b3), 0, v))
                    rows[t][pk] = ["live", [v] + [None] * (nc - 1)]
    return [b1, b2, b3], rows


def expected_live(rows):
    """the live rows as the model takes them, each value as its column's declared type stores it (the
    model's own apply_affinity: good enough to judge a generator, not a reference)"""
    from tests.test_query_model import cell_of
    out = {}
    for t, tab in rows.items():
        types = TYPES[t] or [""] * len(SCHEMA[t])
        out[t] = {pk: {"cl": 1, "cells": [cell_of(M.apply_affinity(v, ty, comparing=False)) for v, ty in zip(vals, types)]}
                  for pk, (state, vals) in tab.items() if state == "live"}
    return out


def predicates(rows, n, seed, keyed=False):
    """n seeded queries: (table, where, columns, keys or None). Constants come from the values the column
    holds (three in four) or from the whole pool; the keyed form draws live, deleted, absent and repeated keys."""
    rng = np.random.default_rng(seed)
    names = list(SCHEMA)
    out = []
    for _ in range(n):
        t = names[int(rng.integers(len(names)))]
        cols = SCHEMA[t]
        tab = rows[t]
        held = {c: [v[j] for _s, v in tab.values() if v[j] is not None] for j, c in enumerate(cols)}
        where = []
        for _g in range(int(rng.integers(1, 4))):
            g = []
            for _k in range(int(rng.integers(1, 3))):
                c = cols[int(rng.integers(len(cols)))] if t == "tc" or rng.random() < 0.85 else "pk"
                u = rng.random()
                if u < 0.08:
                    g.append((c, "is null" if rng.random() < 0.5 else "is not null"))
                    continue
                if c == "pk":
                    v = int(rng.integers(-320, 520))
                elif u < 0.8 and held[c]:
                    v = held[c][int(rng.integers(len(held[c])))]
                else:
                    v = POOL[int(rng.integers(len(POOL)))]
                g.append((c, OPS[int(rng.integers(len(OPS)))], v))
            where.append(g)
        columns = [(["pk"] + cols)[int(rng.integers(len(cols) + 1))] for _ in range(int(rng.integers(0, 5)))]
        keys = None
        if keyed:
            pks = list(tab)
            keys = [pks[int(rng.integers(len(pks)))] if rng.random() < 0.8 else int(rng.integers(10**6, 10**6 + 50))
                    for _ in range(int(rng.integers(0, 70)))]
            keys += keys[:3]                                     # repeated keys
        out.append((t, where, columns, keys))
    return out


def interesting_share(rows, queries):
    """the share of the queries whose model answer over expected_live is neither empty nor everything asked"""
    live = expected_live(rows)
    hit = 0
    for t, where, columns, keys in queries:
        tab = live[t]
        got = M.query(tab, where, columns, keys=keys, col_names=SCHEMA[t], decl_types=TYPES[t], int_pk=t not in INTERNED)
        total = len(tab) if keys is None else sum(1 for k in keys if k in tab)
        hit += 0 < len(got["pk"]) < total
    return hit / max(len(queries), 1)
