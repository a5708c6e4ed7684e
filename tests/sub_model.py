"""A plain-Python model of a subscription's materialised result set (corro_sub_create / _update / _rows): the
set keyed by row key with its AUTOINCREMENT rowids, the transition of every candidate key, cell equality under
SQLite's IS, the two event orders and the change ids. tests/test_sub_model.py pins it against SQLite's own
answers (tests/golden/sub_kats.json); the device implementation is compared with it exactly.

Cells are Python values (None, int, float, str, bytes), as tests/query_model.py's py_value gives them.
"""
import json
import math
import os

try:
    from tests import query_model as Q
except ImportError:                                     # (tests/ itself on the path)
    import query_model as Q

INSERT, UPDATE, DELETE = "Insert", "Update", "Delete"
TYPES = (INSERT, UPDATE, DELETE)                        # by corro_sub_events.type
HERE = os.path.dirname(os.path.abspath(__file__))


def load_kats():
    with open(os.path.join(HERE, "golden", "sub_kats.json")) as f:
        return json.load(f)


def dec(v):
    """A fixture value as the Python value."""
    if isinstance(v, dict):
        return float.fromhex(v["f"]) if "f" in v else v["t"] if "t" in v else bytes.fromhex(v["b"])
    return v


def _number(v):
    return isinstance(v, (int, float)) and not isinstance(v, bool)


def cell_is(a, b):
    """a IS b: NULL is NULL, numbers compare exactly across INTEGER and REAL (Python compares an int with a
    float without rounding the int; -0.0 == 0.0), TEXT and BLOB by type and bytes."""
    if a is None or b is None:
        return a is None and b is None
    if _number(a) or _number(b):
        return _number(a) and _number(b) and a == b
    return type(a) is type(b) and a == b


def identical(a, b):
    """The strict comparison of a test: the same storage class and the same bits (1 is not 1.0, 0.0 not -0.0)."""
    if type(a) is not type(b):
        return False
    if isinstance(a, float):
        return a == b and math.copysign(1, a) == math.copysign(1, b)
    return a == b


def signed(k):
    k = int(k) & Q.M64
    return k - (1 << 64) if k >> 63 else k


class SubModel:
    """The set: {row key (unsigned): [rowid, cells]}, the rowid counter and the last change id."""

    def __init__(self, initial=(), int_pk=True):
        """initial: the (row key, cells) the query selects now, in any order: they take rowids 1..n in
        ascending key (signed for an INTEGER pk, by id for an interned table) and make no event."""
        self.int_pk = int_pk
        self.set = {}
        for n, (k, cells) in enumerate(sorted(((int(k) & Q.M64, c) for k, c in initial), key=lambda r: self._order(r[0]))):
            self.set[k] = [n + 1, list(cells)]
        self.counter = len(self.set)
        self.change_id = 0

    def _order(self, k):
        return signed(k) if self.int_pk else k

    def update(self, keys, fresh):
        """keys: the candidate row keys; fresh: {row key: cells} of the candidates the query selects now.
        Returns the events [(type, rowid, change id, row key (unsigned), cells)] in emission order."""
        fresh = {int(k) & Q.M64: list(c) for k, c in fresh.items()}
        distinct = sorted({int(k) & Q.M64 for k in keys}, key=self._order)
        events, gone = [], []
        for k in distinct:
            old, new = self.set.get(k), fresh.get(k)
            if new is not None and old is None:
                self.counter += 1
                self.set[k] = [self.counter, new]
                events.append([INSERT, self.counter, k, new])
            elif new is not None and not all(cell_is(a, b) for a, b in zip(old[1], new)):
                self.counter += 1                       # (the value the upsert advanced past is never used)
                old[1] = new
                events.append([UPDATE, old[0], k, new])
            elif new is None and old is not None:
                gone.append(k)
        for k in sorted(gone, key=lambda k: self.set[k][0]):
            rowid, cells = self.set.pop(k)
            events.append([DELETE, rowid, k, cells])
        out = []
        for ty, rowid, k, cells in events:
            self.change_id += 1
            out.append((ty, rowid, self.change_id, k, list(cells)))
        return out

    def rows(self):
        """The set in ascending rowid: [(rowid, row key (unsigned), cells)]."""
        return sorted(((r, k, list(c)) for k, (r, c) in self.set.items()))


def fresh_of(rows, keys, where=(), columns=(), col_names=(), decl_types=None, dead=(), int_pk=True):
    """{row key: cells as Python values} of the candidate keys the query selects: tests/query_model.py's keyed
    form over rows = materialise(...)[0][table index]."""
    keys = [int(k) & Q.M64 for k in keys]
    got = Q.query(rows, where, columns, keys=keys, col_names=col_names, decl_types=decl_types, dead=dead, int_pk=int_pk)
    return {pk: [Q.py_value(c) for c in cells] for pk, cells in zip(got["pk"], got["cells"])}


def selected(rows, where=(), columns=(), col_names=(), decl_types=None, int_pk=True):
    """[(row key, cells as Python values)] of every row the query selects (the initial fill)."""
    got = Q.query(rows, where, columns, col_names=col_names, decl_types=decl_types, int_pk=int_pk)
    return [(pk, [Q.py_value(c) for c in cells]) for pk, cells in zip(got["pk"], got["cells"])]
