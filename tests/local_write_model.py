"""A plain-Python model of corro_local_write (include/corro_hip.h): one local transaction of row statements
-> the crsql_changes rows cr-sqlite 0.17.0's CRR triggers leave, and the fixtures' notation
(tests/golden/local_write_kats.json, written by tests/golden/make_local_writes.py) that the CPU and GPU
tests share. Column affinity is SQLite's own: a value is converted by storing it in a column of the declared
type of an in-memory table."""
import hashlib
import json
import os
import sqlite3
import struct

HERE = os.path.dirname(os.path.abspath(__file__))
KATS = os.path.join(HERE, "golden", "local_write_kats.json")
INSERT, UPDATE, UPSERT, DELETE = 0, 1, 2, 3
KIND_NAMES = ("insert", "update", "upsert", "delete")


class ConstraintError(Exception):
    def __init__(self, op):
        super().__init__("INSERT of a live row (op %d)" % op)
        self.op = op


def load_kats():
    with open(KATS) as f:
        return json.load(f)


def dec(v):
    """A pool value -> the Python value (None, int, float, str, bytes)."""
    if isinstance(v, dict):
        if "r" in v:
            return struct.unpack("<d", struct.pack("<Q", int(v["r"], 16)))[0]
        if "t" in v:
            return v["t"]
        return bytes.fromhex(v["b"])
    return v


def enc(v):
    if v is None or isinstance(v, int):
        return v
    if isinstance(v, float):
        return {"r": "%016x" % struct.unpack("<Q", struct.pack("<d", v))[0]}
    if isinstance(v, str):
        return {"t": v}
    return {"b": bytes(v).hex()}


def same(a, b):
    """Equal by storage class and bytes."""
    if type(a) is not type(b):
        return False
    if isinstance(a, float):
        return struct.pack("<d", a) == struct.pack("<d", b)
    return a == b


def statements(flat):
    """A "tx" list -> [(kind, table, pk, [(cid, value index)])]."""
    out, i = [], 0
    while i < len(flat):
        kind, t, pk, n = flat[i:i + 4]
        out.append((kind, t, pk, [(flat[i + 4 + 2 * k], flat[i + 5 + 2 * k]) for k in range(n)]))
        i += 4 + 2 * n
    return out


def chunks(flat, w):
    return [tuple(flat[i:i + w]) for i in range(0, len(flat), w)]


def digest(state, dbv):
    return hashlib.sha256(json.dumps([state, dbv], separators=(",", ":")).encode()).hexdigest()[:6]


class Affinity:
    """SQLite's column affinity by declared type."""

    def __init__(self):
        self.con = sqlite3.connect(":memory:")
        self.made = {}

    def convert(self, decl, v):
        if not decl or v is None or isinstance(v, bytes):
            return v
        if decl not in self.made:
            self.made[decl] = "x%d" % len(self.made)
            self.con.execute("create table %s (c %s)" % (self.made[decl], decl))
        t = self.made[decl]
        self.con.execute("delete from " + t)
        self.con.execute("insert into %s values (?)" % t, (v,))
        return self.con.execute("select c from " + t).fetchone()[0]


class Model:
    """The clock state of one node and its local writes. Rows are keyed (table index, pk); a row is
    {"L": causal length, "sent": None | [cv, dbv, site, seq], "cells": {cid: [value, cv, dbv, site, seq]}}."""

    def __init__(self, tables, nsites=4):
        self.tables = tables
        self.rows = {}
        self.dbv = [None] * nsites
        self.aff = Affinity()

    def ncols(self, t):
        return len(self.tables[t]["cols"])

    # ---- state in the fixtures' notation (values as Python values) ----
    def replace_rows(self, rows, keys=None):
        """Rows (table, pk, cid, value, cv, dbv, site, cl, seq) become the complete clock sets of their keys;
        `keys` lists the keys that are replaced (None: the whole state)."""
        if keys is None:
            self.rows = {}
        else:
            for k in keys:
                self.rows.pop(k, None)
        for t, pk, cid, val, cv, dbv, site, cl, seq in rows:
            r = self.rows.setdefault((t, pk), {"L": cl, "sent": None, "cells": {}})
            r["L"] = cl
            if cid == 0:
                r["sent"] = [cv, dbv, site, seq]
            else:
                r["cells"][cid] = [val, cv, dbv, site, seq]

    def export(self):
        out = []
        for (t, pk), r in self.rows.items():
            if r["sent"]:
                cv, dbv, site, seq = r["sent"]
                out.append((t, pk, 0, None, cv, dbv, site, r["L"], seq))
            for cid, (val, cv, dbv, site, seq) in r["cells"].items():
                out.append((t, pk, cid, val, cv, dbv, site, r["L"], seq))
        return out

    # ---- one local transaction ----
    def local_write(self, stmts, site=0):
        """stmts: [(kind, table, pk, [(cid, value)])] -> (db_version, last_seq, rows, op_result) with rows =
        [(table, pk, cid, value, col_version, cl, seq)] in seq order; (0, 0, [], ...) and no change of state
        when no clock was written. Raises ConstraintError, the state untouched, for an INSERT of a live row."""
        work = {}                      # the rows the transaction addresses, copied
        writes = {}                    # (t, pk, cid) -> (value, cv, cl, seq): the surviving clock writes
        seq = 0
        result = []

        def row_of(key):
            if key not in work:
                r = self.rows.get(key)
                work[key] = {"L": r["L"], "sent": r["sent"], "cells": {c: list(x) for c, x in r["cells"].items()}} if r \
                    else {"L": 0, "sent": None, "cells": {}}
            return work[key]

        for op, (kind, t, pk, cells) in enumerate(stmts):
            key = (t, pk)
            r = row_of(key)
            live = r["L"] % 2 == 1
            decl = [ty for _, ty in self.tables[t]["cols"]]
            conv = {cid: self.aff.convert(decl[cid - 1], v) for cid, v in cells}
            wrote = False
            if kind == DELETE:
                if live:
                    r["L"] += 1
                    for c in list(writes):
                        if c[:2] == key:
                            del writes[c]
                    r["cells"] = {}
                    r["sent"] = [r["L"], None, site, seq]
                    writes[key + (0,)] = (None, r["L"], r["L"], seq)
                    seq += 1
                    wrote = True
            elif kind == INSERT and live:
                raise ConstraintError(op)
            elif not live and kind in (INSERT, UPSERT):
                n = self.ncols(t)
                if r["L"] > 0 or n == 0:
                    r["L"] += 1
                    r["sent"] = [r["L"], None, site, seq]
                    writes[key + (0,)] = (None, r["L"], r["L"], seq)
                    seq += 1
                else:
                    r["L"] = 1
                for cid in range(1, n + 1):
                    v = conv.get(cid)
                    r["cells"][cid] = [v, 1, None, site, seq]
                    writes[key + (cid,)] = (v, 1, r["L"], seq)
                    seq += 1
                wrote = True
            elif live:                  # UPDATE, or UPSERT of a live row: the listed cells by ascending cid
                for cid in sorted(conv):
                    cur = r["cells"].get(cid)
                    if same(conv[cid], cur[0] if cur else None):
                        continue
                    cv = (cur[1] if cur else 0) + 1
                    r["cells"][cid] = [conv[cid], cv, None, site, seq]
                    writes[key + (cid,)] = (conv[cid], cv, r["L"], seq)
                    seq += 1
                    wrote = True
            result.append(1 if wrote else 0)
        if seq == 0:
            return 0, 0, [], result
        v = (self.dbv[site] or 0) + 1
        self.dbv[site] = v
        for key, r in work.items():
            if r["sent"] and r["sent"][1] is None:
                r["sent"][1] = v
            for x in r["cells"].values():
                if x[2] is None:
                    x[2] = v
            if r["L"]:
                self.rows[key] = r
        rows = sorted(((t, pk, cid) + w for (t, pk, cid), w in writes.items()), key=lambda x: x[6])
        return v, seq - 1, rows, result


def bound(tables, stmts):
    """corro_local_bound: inserts and upserts count ncols + 1, updates their cells, deletes 1."""
    n = 0
    for kind, t, pk, cells in stmts:
        n += len(tables[t]["cols"]) + 1 if kind in (INSERT, UPSERT) else len(cells) if kind == UPDATE else 1
    return n
