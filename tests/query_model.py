"""A plain-Python model of a query over one table's live rows of the merged state (SELECT <projection> FROM
<table> WHERE <predicate>): the pivot from clock records to rows, SQLite's comparison, the OR-of-ANDs
predicate, the two row sources (the whole table, or a list of keys) and the per-key status. The engine has no
such call yet; this is the reference a device implementation is to be checked against, and
tests/test_query_model.py pins it against SQLite's own answers (tests/golden/query_kats.json).

A cell is (val_type, val_len, val0, val1, bytes or None): the stored encoding, a long value by its bytes.
"""
import re
import struct

INTEGER, REAL, TEXT, BLOB, NULL = 1, 2, 3, 4, 5
VAL_LONG = 255
NULL_CELL = (NULL, 0, 0, 0, None)
M64 = (1 << 64) - 1


def py_value(cell):
    """The Python value of a cell: None, int, float, str or bytes."""
    ty, ln, w0, w1, raw = cell
    if ty == NULL:
        return None
    if ty == INTEGER:
        return w0 - (1 << 64) if w0 >> 63 else w0
    if ty == REAL:
        return struct.unpack("<d", struct.pack("<Q", w0))[0]
    b = raw if ln == VAL_LONG else (w0.to_bytes(8, "big") + w1.to_bytes(8, "big"))[:ln]
    return b.decode() if ty == TEXT else bytes(b)


def materialise(export_rows, schema):
    """An export (MergeEngine.export() or the oracle's: the crsql_changes columns and "long_values") as the
    pair (live, dead), each {table index: {pk: {"cl": causal length, "cells": [one cell per column]}}}. A row
    is live when its causal length (the sentinel's col_version, 1 without a sentinel) is odd, and a column
    without a clock record is NULL. An export holds every table, so the rows are keyed by table first; the
    deleted rows are returned too because the keyed form tells a deleted key (status 2) from an absent one."""
    ncols = [len(cols) for _name, cols in (schema.items() if isinstance(schema, dict) else schema)]
    long_values = export_rows.get("long_values", {})
    rows = {}
    n = len(export_rows["pk"])
    for k in range(n):
        tc = int(export_rows["table_cid"][k])
        t, c = tc >> 16, tc & 0xFFFF
        r = rows.setdefault(t, {}).setdefault(int(export_rows["pk"][k]) & M64, {"cl": 1, "cells": [NULL_CELL] * ncols[t]})
        if c == 0:
            r["cl"] = int(export_rows["col_version"][k])
        else:
            ln = int(export_rows["val_len"][k])
            r["cells"][c - 1] = (int(export_rows["val_type"][k]), ln, int(export_rows["val0"][k]) & M64,
                                 int(export_rows["val1"][k]) & M64 if ln != VAL_LONG else 0,
                                 long_values[k] if ln == VAL_LONG else None)
    dead = {t: {pk: r for pk, r in tab.items() if r["cl"] % 2 == 0} for t, tab in rows.items()}
    live = {t: {pk: r for pk, r in tab.items() if r["cl"] % 2} for t, tab in rows.items()}
    return live, dead


# ---- SQLite's comparison ----

def _class(v):
    return 1 if isinstance(v, str) else 2 if isinstance(v, (bytes, bytearray)) else 0


def sql_cmp(a, b):
    """The order of two non-NULL values: numbers (compared exactly: Python compares an int with a float
    without rounding the int) below TEXT below BLOB; TEXT and BLOB by their bytes, the shorter first."""
    ca, cb = _class(a), _class(b)
    if ca != cb:
        return -1 if ca < cb else 1
    if ca == 1:
        a, b = a.encode(), b.encode()
    return -1 if a < b else 1 if a > b else 0


_NUM = re.compile(r"^[+-]?(\d+\.?\d*([eE][+-]?\d+)?|\.\d+([eE][+-]?\d+)?)$")


def apply_affinity(v, decl_type, comparing=True):
    """v as a column of the declared type stores it (the cases the fixture holds, not all of SQLite's
    applyAffinity). comparing: an int is not made a float for a REAL column, as in a comparison. This is a
    convenience of the model and no authority: the fixture's recorded answers are, and a device query is
    to be compared with those directly."""
    t = (decl_type or "").upper()
    aff = ("INTEGER" if "INT" in t else "TEXT" if any(x in t for x in ("CHAR", "CLOB", "TEXT"))
           else "BLOB" if "BLOB" in t or not t else "REAL" if any(x in t for x in ("REAL", "FLOA", "DOUB")) else "NUMERIC")
    if v is None or isinstance(v, (bytes, bytearray)) or aff == "BLOB":
        return v
    if aff == "TEXT":
        if isinstance(v, int):
            return str(v)
        if isinstance(v, float):
            if v == 0:
                return "0.0"                            # (SQLite 3.37.2 renders -0.0 so)
            s = "%.15g" % v
            if "e" in s:
                m, e = s.split("e")
                return (m if "." in m else m + ".0") + "e" + e[0] + e[1:].lstrip("0").rjust(2, "0")
            return s if "." in s else s + ".0"
        return v
    if isinstance(v, str):
        s = v.strip(" \t\n\r\f\v")
        if not _NUM.match(s):
            return v
        try:
            v = int(s)
        except ValueError:
            v = float(s)
        if isinstance(v, int) and not -2**63 <= v < 2**63:
            v = float(v)
    if isinstance(v, float) and v == int(v) and -2**63 < v < 2**63:
        # (a REAL column stores the integer and reads it back as a float: -0.0 comes back 0.0)
        return int(v) if aff != "REAL" or comparing else float(int(v))
    if isinstance(v, int) and aff == "REAL" and not comparing:
        return float(v)
    return v


def term_true(value, op, const):
    if op == "is null":
        return value is None
    if op == "is not null":
        return value is not None
    if value is None or const is None:
        return False
    c = sql_cmp(value, const)
    return {"=": c == 0, "==": c == 0, "!=": c != 0, "<>": c != 0, "<": c < 0, "<=": c <= 0, ">": c > 0, ">=": c >= 0}[op]


def query(rows, where=(), columns=(), keys=None, col_names=(), decl_types=None, dead=(), int_pk=True):
    """The query over one table's live rows: rows = materialise(...)[0][table index], dead = its deleted rows
    (keyed form only). The model has no engine behind it, so what an engine would know of the table comes as
    arguments: col_names (its columns), decl_types (their declared types; None: no affinity) and int_pk
    (False: an interned table, ordered by id). where: a list of groups, each a list of (column name or "pk",
    op, Python value), a row matching when every term of some group is true; columns: the projected names,
    "pk" for the key. Returns {"pk", "cl", "cells" (one list per match, in projection order)} and, for the
    keyed form, "key_status" and "key_index". Table form: ascending pk, signed for an INTEGER pk."""
    col_names = list(col_names)

    def value_of(pk, r, col):
        if col == "pk":
            return pk - (1 << 64) if pk >> 63 else pk
        return py_value(r["cells"][col_names.index(col)])

    def const_of(col, v):
        if col == "pk":
            return apply_affinity(v, "INTEGER")
        return apply_affinity(v, decl_types[col_names.index(col)]) if decl_types else v

    prepared = [[(t[0], " ".join(t[1].lower().split()), const_of(t[0], t[2]) if len(t) > 2 else None) for t in g] for g in where]

    def matches(pk, r):
        if not prepared:
            return True
        return any(all(term_true(value_of(pk, r, col), op, c) for col, op, c in g) for g in prepared)

    out = {"pk": [], "cl": [], "cells": []}

    def emit(pk, r):
        out["pk"].append(pk)
        out["cl"].append(r["cl"])
        out["cells"].append([(INTEGER, 0, pk, 0, None) if c == "pk" else r["cells"][col_names.index(c)] for c in columns])

    if keys is None:
        order = sorted(rows, key=(lambda p: p - (1 << 64) if p >> 63 else p) if int_pk else None)
        for pk in order:
            if matches(pk, rows[pk]):
                emit(pk, rows[pk])
        return out
    out["key_status"], out["key_index"] = [], []
    for i, pk in enumerate(keys):
        pk = int(pk) & M64
        if pk in rows:
            ok = matches(pk, rows[pk])
            out["key_status"].append(1 if ok else 3)
            if ok:
                emit(pk, rows[pk])
                out["key_index"].append(i)
        else:
            out["key_status"].append(2 if pk in dead else 0)
    return out
