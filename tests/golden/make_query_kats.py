"""Regenerate tests/golden/query_kats.json: the edges of SQL's comparison, answered by SQLite itself.

    python tests/golden/make_query_kats.py

The tables are built in the standard library's sqlite3 with declared column types, every WHERE is run with
its constants bound as parameters (a parameter has no affinity, so `column op ?` applies the column's
affinity to it exactly as to a literal), and the schema, the rows, the query, the selected pks and the
projected values are recorded. Values: null, an int, {"f": float.hex()}, {"t": text} or {"b": hex}.
"""
import json
import os
import sqlite3

HERE = os.path.dirname(os.path.abspath(__file__))
I64_MAX, I64_MIN = 2**63 - 1, -2**63
L16 = "abcdefghijklmnop"
OPS = ("=", "!=", "<", "<=", ">", ">=")

COLUMNS = [("i", "INTEGER"), ("r", "REAL"), ("s", "TEXT"), ("b", "BLOB")]
ROWS = [
    (1, 5, 5.0, "a", b"\x00"),
    (2, None, None, None, None),
    (3, 2**53 + 1, 9007199254740992.0, "ab", b""),
    (4, I64_MAX, 9.223372036854775807e18, "abc", b"ab"),
    (5, I64_MIN, -9.223372036854775807e18, "", None),
    (6, 0, -0.0, "5", "5"),
    (7, 2**53, 0.0, L16, L16.encode()),
    (8, 100, 100.0, L16 + "q", (L16 + "q").encode()),
    (9, 6, 5.5, "abcdefghXijklmnopqrstu", b"abcdefghXijklmnopqrstu"),
    (10, 4, 4.5, "abcdefghYijklmnopqrstu", b"abcdefghYijklmnopqrstu"),
    (11, -5, -5.0, L16 + "qrstA", "text in a blob column, long"),
    (12, -6, -5.5, L16 + "qrstB", 5),
    (13, "abc", "xyz", 12, 5.5),
    (14, -1, -1.5, "-1", b"\xff"),
    (15, 7, 0.5, None, L16),
    (-3, 1, 1.0, "neg", None),
    (I64_MAX, 2, 2.0, "max", None),
    (I64_MIN, 3, 3.0, "min", None),
]
CONSTANTS = [
    None, 5, 5.0, 5.5, 0, -0.0, 2**53, 2**53 + 1, 9007199254740992.0, I64_MAX, I64_MIN, 9.223372036854775807e18,
    -9.223372036854775807e18, "a", "ab", "abc", "", b"", b"\x00", "5", "5.0", "1e2", " 5 ", "5x", L16, L16 + "q",
    "abcdefghXijklmnopqrstu", "abcdefghYijklmnopqrstu", L16 + "qrstA", L16 + "qrstB", L16.encode(),
    (L16 + "q").encode(), b"abcdefghXijklmnopqrstu", "text in a blob column, long", "text in a blob column, lonh",
]


def enc(v):
    if v is None or isinstance(v, int):
        return v
    if isinstance(v, float):
        return {"f": v.hex()}
    if isinstance(v, str):
        return {"t": v}
    return {"b": bytes(v).hex()}


def sql_of(where):
    groups, params = [], []
    for g in where:
        terms = []
        for col, op, *val in g:
            name = "id" if col == "pk" else col
            if op in ("is null", "is not null"):
                terms.append(f"{name} {op}")
            else:
                terms.append(f"{name} {op} ?")
                params.append(val[0])
        groups.append("(" + " AND ".join(terms) + ")")
    return (" WHERE " + " OR ".join(groups) if groups else ""), params


# the SQLite whose conversions the engine's "sqlite-3.37.2" affinity policy emulates: the recorded policy
# and the recorded version go together
POLICY_OF_VERSION = {"3.37.2": "sqlite-3.37.2"}


def main():
    if sqlite3.sqlite_version not in POLICY_OF_VERSION:
        raise SystemExit(f"SQLite {sqlite3.sqlite_version}: no affinity policy of the engine emulates this version")
    db = sqlite3.connect(":memory:")
    db.execute("CREATE TABLE t (id INTEGER PRIMARY KEY, " + ", ".join(f"{n} {t}" for n, t in COLUMNS) + ")")
    db.executemany("INSERT INTO t VALUES (?, ?, ?, ?, ?)", ROWS)
    queries = []
    for col, _t in COLUMNS:
        for c in CONSTANTS:
            for op in OPS:
                queries.append(([[(col, op, c)]], ["pk"]))
        queries.append(([[(col, "is null")]], [col]))
        queries.append(([[(col, "is not null")]], [col]))
    for c in (5, 5.5, "5", "abc", -3, -3.0, I64_MIN, I64_MAX, 9.223372036854775807e18, None):
        for op in OPS:
            queries.append(([[("pk", op, c)]], ["pk", "i"]))
    queries += [
        ([], ["i", "r", "s", "b"]),                                               # the empty predicate
        ([], []),
        ([[("i", ">", 4), ("r", "<", 6.0)], [("s", "=", "neg")]], ["s", "pk", "s"]),  # OR of ANDs, a column twice
        ([[("i", "is null")], [("b", "is null"), ("s", ">=", "m")]], ["pk", "b"]),
        ([[("pk", ">", 0), ("pk", "<=", 9)], [("pk", "<", 0)]], ["pk"]),
        ([[("s", ">", L16), ("s", "<", L16 + "qrstB")]], ["s"]),
        ([[("i", "=", 5)], [("i", "=", 5)]], ["i"]),                               # a row two groups accept comes once
    ]
    cases = []
    for where, cols in queries:
        clause, params = sql_of(where)
        sel = ", ".join(["id"] + [("id" if c == "pk" else c) for c in cols])
        got = db.execute(f"SELECT {sel} FROM t{clause} ORDER BY id", params).fetchall()
        cases.append({"where": [[[t[0], t[1]] + [enc(v) for v in t[2:]] for t in g] for g in where], "columns": cols,
                      "pks": [r[0] for r in got], "values": [[enc(v) for v in r[1:]] for r in got]})
    out = {"sqlite_version": sqlite3.sqlite_version, "affinity_policy": POLICY_OF_VERSION[sqlite3.sqlite_version], "table": "t",
           "columns": [list(c) for c in COLUMNS], "rows": [[enc(v) for v in r] for r in ROWS], "cases": cases}
    with open(os.path.join(HERE, "query_kats.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print(len(cases), "cases")


if __name__ == "__main__":
    main()
