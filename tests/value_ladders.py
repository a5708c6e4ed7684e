"""Value ladders and a plain model of the merge's order, for the directed value-order tests
(test_gpu_value_order.py on the GPU, test_value_order_oracle.py on the CPU oracle).

The model is a third statement of SURVEY App. A.2 / A.4 next to the HIP kernels and the oracle's
value_cmp (oracle/crsql_fold.c): Python's own int, float and bytes comparison under the class order
NULL < BLOB < TEXT < REAL < INTEGER. It imports no GPU code and nothing of the oracle.

A ladder is a list of values of one storage class, sorted by `key` here (never by hand), whose
neighbours differ exactly where a packed or split comparison key can go wrong: at every bit of an
INTEGER (the bit-15/16 and bit-47/48 seams of the packed keys, bit 62 against bit 63), at the sign,
the zeros, the denormals and the infinities of a REAL, at bytes >= 0x80, embedded NULs and the
8- and 16-byte word boundaries of a TEXT / BLOB, and at the inline / long boundary (17 bytes).

Changes are plain tuples (Change); `model_fold` folds cl = 1 column changes in application order and
returns the winning change of every cell, the per-change impact flags and the per-site db_versions."""
import random
from collections import namedtuple

import numpy as np

from tests._util import LONG, encode_values

INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
DBL_MAX, DBL_MIN, DENORM_MIN = 1.7976931348623157e308, 2.2250738585072014e-308, 5e-324
ULP1 = 2.220446049250313e-16  # 1 + ULP1 is the double after 1.0


# ---------------------------------------------------------------------------------------------
# the order
def key(v):
    """Total order of a SqliteValue (None | int | float | bytes | str): the class rank, then
    Python's own comparison within the class (bytes: memcmp over the common length, then the longer
    value is greater; float: -0.0 == 0.0)."""
    if v is None:
        return (0,)
    if isinstance(v, (bytes, bytearray)):
        return (1, bytes(v))
    if isinstance(v, str):
        return (2, v.encode())
    if isinstance(v, float):
        assert v == v, "NaN has no place in the order (k_validate rejects it)"
        return (3, v)
    assert isinstance(v, int) and not isinstance(v, bool)
    assert INT64_MIN <= v <= INT64_MAX
    return (4, v)


def _ladder(values):
    out = []
    for v in sorted(values, key=key):
        if not out or key(out[-1]) != key(v):
            out.append(v)
    return out


def _clip(v):
    return min(max(v, INT64_MIN), INT64_MAX)


INTEGER = _ladder([_clip(s * (1 << k) + d) for k in range(63) for s in (1, -1) for d in (-1, 0, 1)] +
                  [INT64_MIN, INT64_MIN + 1, -(1 << 62) - 1, 1 << 62, INT64_MAX])

REAL = _ladder([float("-inf"), -DBL_MAX, -2.25, -1.5, -(1.0 + ULP1), -1.0, -DBL_MIN, -DENORM_MIN, 0.0, DENORM_MIN,
                DBL_MIN, 1.0, 1.0 + ULP1, 1.5, float(1 << 53), 1e308, float("inf")])

LONG_40 = b"a" * 17 + bytes(range(0x80, 0x80 + 23))  # shares its first 17 bytes with b"a" * 17
BLOB = _ladder([b""] + [b"\0" * n for n in (1, 2, 8, 9, 16, 17)] + [b"\0" * 16 + b"\1"] +
               [b"a", b"a\0"] + [b"a" * n for n in (7, 8, 9, 15, 16, 17)] + [b"a" * 8 + b"\0", b"a" * 16 + b"\0"] +
               [b"a" * 15 + b"\x7f", b"a" * 15 + b"\x80", b"a" * 7 + b"\x80"] +
               [b"\x7f", b"\x80", b"\xff", b"\xff" * 16, b"\xff" * 17] + [LONG_40])

TEXT = _ladder(["", "a"] + ["a" * n for n in (8, 9, 16, 17)] + ["b", "é", "é" * 8, chr(0xFFFF)])

# the greatest BLOB below the smallest TEXT, and so on up the classes
CROSS = _ladder([None, b"\xff" * 17, "", float("inf"), INT64_MIN])

# the same climb with an inline BLOB: a long value sends its bucket to the general body, so this is
# the form in which NULL / BLOB / TEXT meet inside the mixed-class fast bodies
CROSS_INLINE = _ladder([None, b"\xff" * 16, "", float("inf"), INT64_MIN])

LADDERS = {"integer": INTEGER, "real": REAL, "blob": BLOB, "text": TEXT, "cross": CROSS, "cross_inline": CROSS_INLINE}
LADDER_LEN = {"integer": 374, "real": 17, "blob": 27, "text": 10, "cross": 5, "cross_inline": 5}


def is_long(v):
    """a TEXT / BLOB value of more than 16 bytes (held in the value arena, not inline)"""
    return isinstance(v, (str, bytes, bytearray)) and len(v.encode() if isinstance(v, str) else v) > 16


def pairs_of(ladder):
    """adjacent (lo, hi) pairs of a ladder"""
    return list(zip(ladder[:-1], ladder[1:]))


# ---------------------------------------------------------------------------------------------
# changes, batches, site tables
Change = namedtuple("Change", "pk cid value cv dbv site cl seq")


def batch_of(changes, table=0):
    """Changes in application order -> the SoA batch MergeEngine.apply and oracle.Fold.apply take."""
    n = len(changes)
    b = {"pk": np.array([c.pk for c in changes], np.uint64),
         "table_cid": np.array([(table << 16) | c.cid for c in changes], np.uint32),
         "col_version": np.array([c.cv for c in changes], np.int64),
         "db_version": np.array([c.dbv for c in changes], np.int64),
         "cl": np.array([c.cl for c in changes], np.uint32),
         "seq": np.array([c.seq for c in changes], np.uint32),
         "site": np.array([c.site for c in changes], np.uint32),
         "ts": np.array([1000 + c.dbv for c in changes], np.uint64)}
    assert len(b["pk"]) == n
    b.update(encode_values([c.value for c in changes]))
    return b


def shuffled_sites(n, seed):
    """n distinct 16-byte site ids registered in shuffled id order, so ordinal != rank. Returns
    (ids [n, 16] uint8 by ordinal, rank[ordinal], ordinal[rank]); rank = position of the id in
    memcmp order. The first four bytes are the big-endian rank, the rest is noise."""
    rng = np.random.default_rng(seed)
    ordinal_of_rank = rng.permutation(n)
    while n > 1 and np.array_equal(ordinal_of_rank, np.arange(n)):
        ordinal_of_rank = rng.permutation(n)
    ids = rng.integers(0, 256, size=(n, 16), dtype=np.uint8)
    rank_of_ordinal = np.empty(n, np.int64)
    rank_of_ordinal[ordinal_of_rank] = np.arange(n)
    ids[:, :4] = rank_of_ordinal.astype(">u4").view(np.uint8).reshape(n, 4)
    # (the model's own check of the ranks: Python's bytes order of the ids)
    by_bytes = sorted(range(n), key=lambda o: ids[o].tobytes()) if n <= 4096 else None
    assert by_bytes is None or by_bytes == [int(o) for o in ordinal_of_rank]
    return ids, rank_of_ordinal, ordinal_of_rank


class Case:
    """Changes in application order with the apply each belongs to in the two-apply form (phase 0
    or 1) and a label per cell for assertion messages."""

    def __init__(self):
        self.changes, self.phase, self.label = [], [], {}

    def add(self, phase, pk, cid, value, cv, site, cl=1, dbv=None):
        i = len(self.changes)
        self.changes.append(Change(pk, cid, value, cv, i + 1 if dbv is None else dbv, site, cl, i))
        self.phase.append(phase)

    def __len__(self):
        return len(self.changes)


def contest_batch(contests, pk0=1, cid=1):
    """contests: [(first, second, label)], each member (value, col_version, site ordinal). Every
    contest is one cell on its own pk, `first` applied before `second`; in the two-apply form
    `first` goes in apply 1 and `second` in apply 2. Every change has its own db_version (its
    1-based position), so the exported row shows which change won."""
    c = Case()
    for k, (first, second, label) in enumerate(contests):
        pk = pk0 + k
        c.add(0, pk, cid, first[0], first[1], first[2])
        c.add(1, pk, cid, second[0], second[1], second[2])
        c.label[(pk, cid)] = label
    return c


def duel_batch(pairs, lo_site, hi_site, cv=1, pk0=1):
    """For each (lo, hi), key(lo) < key(hi), two cells on their own pks in the orders lo, hi and
    hi, lo, same col_version, cl = 1. lo_site must be the site of HIGHER rank: a compare that
    wrongly reports "equal" then hands the cell to lo."""
    contests = []
    for lo, hi in pairs:
        assert key(lo) < key(hi)
        a, b = (lo, cv, lo_site), (hi, cv, hi_site)
        contests.append((a, b, f"lo={lo!r} hi={hi!r} order=lo,hi"))
        contests.append((b, a, f"lo={lo!r} hi={hi!r} order=hi,lo"))
    return contest_batch(contests, pk0)


def melee_batch(ladder, seed, nsites, pk0=1, cell_size=None, cv=1, into=None):
    """The whole ladder in one cell, in shuffled order, written by random sites (cell_size: cut it
    into consecutive slices of at most that many values, one cell on its own pk each, for the bodies
    that hold a bounded row, and so that other values than the ladder's top win a cell). Every value
    appears twice, so that equal values meet with different sites. In the two-apply form the first
    half of the shuffled order is apply 1. `into`: a Case to extend (its pks must differ)."""
    rnd = random.Random(seed)
    vals = list(ladder)
    step = cell_size or len(vals)
    c = into or Case()
    for k, at in enumerate(range(0, len(vals), step)):
        members = vals[at:at + step] * 2
        rnd.shuffle(members)
        pk = pk0 + k
        for j, v in enumerate(members):
            c.add(0 if j < len(members) // 2 else 1, pk, 1, v, cv, rnd.randrange(nsites))
        c.label[(pk, 1)] = f"melee seed={seed} slice={k} ({len(members)} changes)"
    return c


def equal_batch(values, site_a, site_b, pk0=1):
    """Equal values at equal col_version: per value, written by two sites in both orders (the higher
    rank wins regardless of order), and twice by one site (the earlier change keeps the cell)."""
    contests = []
    for v in values:
        w = v[1] if isinstance(v, tuple) else v
        v = v[0] if isinstance(v, tuple) else v
        assert key(v) == key(w)
        contests.append(((v, 1, site_a), (w, 1, site_b), f"equal {v!r} / {w!r} sites a,b"))
        contests.append(((v, 1, site_b), (w, 1, site_a), f"equal {v!r} / {w!r} sites b,a"))
        contests.append(((w, 1, site_a), (v, 1, site_b), f"equal {w!r} / {v!r} sites a,b"))
        contests.append(((v, 1, site_a), (w, 1, site_a), f"equal {v!r} / {w!r} same site"))
    return contest_batch(contests, pk0)


CV_PAIRS = [((1 << 15) - 2, (1 << 15) - 1), ((1 << 15) - 1, 1 << 15), ((1 << 31) - 1, 1 << 31),
            ((1 << 32) - 1, 1 << 32), (1 << 62, (1 << 63) - 1)]


def col_version_batch(cv_pairs, high_rank_site, low_rank_site, pk0=1, values=(-(1 << 40) - 1, 1 << 40)):
    """Duels on col_version with everything else reversed: the lower col_version carries the greater
    value and the higher site rank, so only the col_version compare can give the right winner. Both
    orders of each pair, each cell on its own pk."""
    small, great = values
    assert key(small) < key(great)
    contests = []
    for lo, hi in cv_pairs:
        assert lo < hi
        a, b = (great, lo, high_rank_site), (small, hi, low_rank_site)
        contests.append((a, b, f"col_version lo={lo} hi={hi} order=lo,hi"))
        contests.append((b, a, f"col_version lo={lo} hi={hi} order=hi,lo"))
    return contest_batch(contests, pk0)


EQUAL_INTEGER = [-(1 << 47), (1 << 16) - 1]
EQUAL_WIDE = EQUAL_INTEGER + [(-0.0, 0.0), "é" * 8, LONG_40, b"a\0"]


# ---------------------------------------------------------------------------------------------
# the model
def model_fold(changes, rank):
    """Fold cl = 1 column changes (cid > 0) in application order. A change takes its cell when
    (col_version, key(value), site rank) is strictly greater than the holder's (an
    equal triple leaves the earlier change in place). Sentinel changes (cid 0) are outside the
    model: they must sit on rows of their own, their impact is None and they leave no model row.
    Returns (winner Change per (pk, cid), impact flag per change, db_version per site ordinal)."""
    held, best, impact = {}, {}, []
    dbv = {}
    sentinel_pks = {c.pk for c in changes if c.cid == 0}
    for c in changes:
        dbv[c.site] = max(dbv.get(c.site, -1), c.dbv)
        if c.cid == 0:
            impact.append(None)
            continue
        assert c.cl == 1 and c.pk not in sentinel_pks
        k = (c.cv, key(c.value), int(rank[c.site]))
        cell = (c.pk, c.cid)
        if cell not in held or k > best[cell]:
            held[cell], best[cell] = c, k
            impact.append(1)
        else:
            impact.append(0)
    return held, impact, dbv


def row_tuple(c, table=0, with_ts=False):
    """The winning change of a cell as tests._util.rows_to_tuples shows its exported row."""
    e = encode_values([c.value])
    t, ln = int(e["val_type"][0]), int(e["val_len"][0])
    v1 = 0
    if t in (3, 4):
        v1 = (c.value.encode() if isinstance(c.value, str) else bytes(c.value)) if ln == LONG else int(e["val1"][0])
    tup = (table, c.pk, c.cid, t, int(e["val0"][0]) if t != 5 else 0, v1, ln if t in (3, 4) else 0, c.cv, c.dbv,
           c.site, c.cl, c.seq)
    return tup + (1000 + c.dbv,) if with_ts else tup


def model_rows(held, with_ts=False):
    return sorted(row_tuple(c, with_ts=with_ts) for c in held.values())
