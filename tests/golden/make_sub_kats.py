"""Regenerate tests/golden/sub_kats.json: a subscription's materialised result set advanced by candidate keys,
answered by SQLite itself.

    python tests/golden/make_sub_kats.py

The result set is a `query` table with an AUTOINCREMENT rowid and a unique index on the row key. A round puts
the candidate keys into `cand` and their fresh rows (the rows the subscription's query selects among them now)
into `fresh`, then runs two statements: an upsert from `fresh EXCEPT current` and a delete from `current
EXCEPT fresh` over the candidates, both RETURNING the rowids. Which of the upserted rows existed before tells
an Insert from an Update; change ids count the returned rows, the upsert's first. The columns carry no declared
type, so a value is stored as it is given. Every sequence records its initial rows (entered through the same
upsert: rowids 1..n in ascending key), and per round the keys, the fresh rows, the events and the whole set
afterwards in rowid order. Values: null, an int, {"f": float.hex()}, {"t": text} or {"b": hex}.
"""
import json
import os
import sqlite3

HERE = os.path.dirname(os.path.abspath(__file__))
L16 = "abcdefghijklmnop"
LONG = "a long value, more than sixteen bytes"

SEQUENCES = [
    # every row of the transition table: 1 stays, 2 changes, 3 leaves, 4 enters, 5 is nowhere
    {"name": "transitions", "ncols": 2,
     "initial": [(1, "one", 10), (2, "two", 20), (3, "three", 30)],
     "rounds": [([1, 2, 3, 4, 5], [(1, "one", 10), (2, "two", 21), (4, "four", 40)]),
                ([], []),
                ([5, 5], [])]},
    # cell equality under IS, one row per case
    {"name": "equality", "ncols": 1,
     "initial": [(1, None), (2, 1), (3, 2**53 + 1), (4, 0.0), (5, "abc"), (6, b"abc"), (7, LONG), (8, L16), (9, LONG + "x"),
                 (10, None), (11, 2**53), (12, b""), (13, LONG.encode()), (14, 5.5)],
     "rounds": [([1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14],
                 [(1, None), (2, 1.0), (3, float(2**53)), (4, -0.0), (5, b"abc"), (6, b"abd"), (7, LONG), (8, L16 + "q"),
                  (9, LONG + "y"), (10, 0), (11, float(2**53)), (12, ""), (13, LONG), (14, 5.5)]),
                # the stored cells of the rows that made no event are the old ones: they leave as they were
                ([2, 4, 11, 7], [])]},
    # AUTOINCREMENT under upsert: Insert, Update, Insert, Update, Insert over rowids 1..3 gives 4, 6, 8
    {"name": "rowids", "ncols": 1,
     "initial": [(10, "a"), (20, "b"), (30, "c")],
     "rounds": [([5, 10, 15, 20, 25], [(5, "n5"), (10, "a2"), (15, "n15"), (20, "b2"), (25, "n25")]),
                ([35], [(35, "n35")]),
                ([20], []),                              # a Delete does not move the counter
                ([20], [(20, "again")]),                 # deleted, then selected again: a fresh rowid
                ([40, 30], [(40, "n40"), (30, "c2")]),   # the call ends with an Update ...
                ([50], [(50, "n50")]),                   # ... and the next Insert shows where the counter went
                ([30, 10], [(30, "c3"), (10, "a3")]),    # Updates alone
                ([60], [(60, "n60")])]},
    # the two event orders, with negative keys and duplicates
    {"name": "orders", "ncols": 1,
     "initial": [(3, "p3"), (-1, "m1"), (7, "p7"), (-5, "m5")],
     "rounds": [([7, -5, 2, -1, -10, 7, 2], [(2, "p2"), (-1, "m1b"), (-10, "m10")]),
                ([-10, 3], []),                          # rowid order (3, then -10) is not key order
                ([-2**63, 2**63 - 1, -1], [(-2**63, "min"), (2**63 - 1, "max")])]},
]


def enc(v):
    if v is None or isinstance(v, int):
        return v
    if isinstance(v, float):
        return {"f": v.hex()}
    if isinstance(v, str):
        return {"t": v}
    return {"b": bytes(v).hex()}


def advance(db, cols, keys, fresh, change_id):
    """One round: the events as [type, rowid, change id, key, values] and the last change id."""
    names = ", ".join(cols)
    db.execute("DELETE FROM cand")
    db.execute("DELETE FROM fresh")
    db.executemany("INSERT OR IGNORE INTO cand VALUES (?)", [(k,) for k in keys])
    db.executemany(f"INSERT INTO fresh VALUES (?{', ?' * len(cols)})", fresh)
    before = {k for (k,) in db.execute("SELECT k FROM query")}
    sets = ", ".join(f"{c} = excluded.{c}" for c in cols)
    up = db.execute(
        f"INSERT INTO query (k, {names}) SELECT k, {names} FROM (SELECT k, {names} FROM fresh EXCEPT SELECT k, {names} FROM query)"
        f" WHERE true ORDER BY k ON CONFLICT (k) DO UPDATE SET {sets} RETURNING __rowid, k, {names}").fetchall()
    gone = db.execute(
        f"DELETE FROM query WHERE k IN (SELECT k FROM (SELECT k, {names} FROM query WHERE k IN (SELECT k FROM cand)"
        f" EXCEPT SELECT k, {names} FROM fresh)) RETURNING __rowid, k, {names}").fetchall()
    if [r[0] for r in gone] != sorted(r[0] for r in gone):
        raise SystemExit("the delete did not return its rows in rowid order")
    if [r[1] for r in up] != sorted(r[1] for r in up):
        raise SystemExit("the upsert did not return its rows in key order")
    events = []
    for r in up:
        change_id += 1
        events.append(["Update" if r[1] in before else "Insert", r[0], change_id, r[1], [enc(v) for v in r[2:]]])
    for r in gone:
        change_id += 1
        events.append(["Delete", r[0], change_id, r[1], [enc(v) for v in r[2:]]])
    return events, change_id


def run(seq):
    cols = [f"c{j}" for j in range(seq["ncols"])]
    names = ", ".join(cols)
    db = sqlite3.connect(":memory:")
    db.execute(f"CREATE TABLE query (__rowid INTEGER PRIMARY KEY AUTOINCREMENT, k INTEGER NOT NULL, {names})")
    db.execute("CREATE UNIQUE INDEX query_k ON query (k)")
    db.execute(f"CREATE TABLE fresh (k INTEGER PRIMARY KEY, {names})")
    db.execute("CREATE TABLE cand (k INTEGER PRIMARY KEY)")

    def rows():
        return [[r[0], r[1], [enc(v) for v in r[2:]]] for r in db.execute(f"SELECT __rowid, k, {names} FROM query ORDER BY __rowid")]

    advance(db, cols, [r[0] for r in seq["initial"]], seq["initial"], 0)
    out = {"name": seq["name"], "columns": cols, "initial": [[enc(v) for v in r] for r in seq["initial"]], "rows": rows(),
           "rounds": []}
    change_id = 0
    for keys, fresh in seq["rounds"]:
        events, change_id = advance(db, cols, keys, fresh, change_id)
        out["rounds"].append({"keys": keys, "fresh": [[enc(v) for v in r] for r in fresh], "events": events, "rows": rows()})
    return out


def main():
    out = {"sqlite_version": sqlite3.sqlite_version, "sequences": [run(s) for s in SEQUENCES]}
    with open(os.path.join(HERE, "sub_kats.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print(sum(len(s["rounds"]) for s in out["sequences"]), "rounds")


if __name__ == "__main__":
    main()
