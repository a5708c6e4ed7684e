"""Frames for the wire decoder's edge tests, built on the host with corrosion_amd/wire.py's encoder:
shared by tests/test_wire_model.py (the model alone) and tests/test_gpu_wire_edges.py (the decoder
against the model)."""
import struct

import numpy as np

from corrosion_amd import wire
from corrosion_amd.agent import Change, ChangeV1, Empty, EmptySet
from tests import wire_model as M

SCHEMA = {"users": ["name", "age", "blob"], "t2": ["x"], "kv": ["v"], "wide": ["a", "b"]}
INTERNED = ("kv", "wide")
ACT = [bytes([i] * 16) for i in range(1, 6)]
KINDS = (wire.PAYLOAD_SYNC, wire.PAYLOAD_UNI)


class Raw:
    """an encoded SqliteValue given as its bytes (tags and bit patterns encode_value cannot produce)"""
    def __init__(self, b):
        self.b = bytes(b)


def real_bits(bits):
    return Raw(b"\x02" + struct.pack("<Q", bits))


def change_bytes(ch):
    """wire.encode_change, with Raw values passed through"""
    if not isinstance(ch.val, Raw):
        return wire.encode_change(ch)
    zero = wire.encode_change(Change(ch.table, ch.pk, ch.cid, None, ch.col_version, ch.db_version, ch.seq,
                                     ch.site_id, ch.cl))
    return zero[:-49] + ch.val.b + zero[-48:]      # (a NULL is its one tag byte before the 48 fixed bytes)


def prefix(kind):
    return struct.pack("<II", 0, 1) if kind == wire.PAYLOAD_SYNC else struct.pack("<III", 0, 0, 0)


def suffix(kind, cluster_id=7):
    return b"" if kind == wire.PAYLOAD_SYNC else struct.pack("<H", cluster_id)


def full(kind, actor, version, changes, ts=9, count=None, seqs=None, last_seq=None):
    n = len(changes)
    seqs = (0, max(n - 1, 0)) if seqs is None else seqs
    return (prefix(kind) + actor + struct.pack("<IQI", 1, version, n if count is None else count) +
            b"".join(change_bytes(c) for c in changes) +
            struct.pack("<QQQQ", seqs[0], seqs[1], max(n - 1, 0) if last_seq is None else last_seq, ts) + suffix(kind))


def message(kind, cv):
    return wire.encode_sync_changeset(cv) if kind == wire.PAYLOAD_SYNC else wire.encode_uni_change(cv, 7)


def pk_int_n(v, n):
    """one INTEGER column packed in exactly n bytes (canonical or not)"""
    return bytes([1, (n << 3) | 1]) + (v & ((1 << (8 * n)) - 1)).to_bytes(n, "big")


KV_PK = bytes([1, (1 << 3) | 3, 2]) + b"k1"                              # kv: one TEXT column
WIDE_PK = bytes([2, (1 << 3) | 1, 5, (1 << 3) | 3, 1]) + b"z"            # wide: INTEGER, TEXT
KV_PK_LOOSE = bytes([1, (2 << 3) | 3, 0, 2]) + b"k1" + b"\xEE"           # a 2-byte length, a trailing byte
KV_PK_BAD = bytes([1, (4 << 3) | 4, 0, 0, 0, 9, 1])                      # a BLOB of 9 bytes with 1 present


def mixed_changes(actor=ACT[0], version=3):
    """6 changes, about 570 bytes encoded: mixed tables (plain, interned, unknown), every value tag, one
    17-byte TEXT"""
    return [Change("users", 5, "name", "q" * 17, 1, version, 0, actor, 1),
            Change("t2", -300, "x", -(1 << 63), 2, version, 1, ACT[1], 1),
            Change("kv", KV_PK, "v", 2.5, 3, version, 2, actor, 2),
            Change("users", 1 << 60, "blob", bytes(range(16)), 4, version, 3, ACT[2], 1),
            Change("nope", 7, "zz", None, 5, version, 4, actor, 3),
            Change("wide", WIDE_PK, "-1", None, 6, version, 5, actor, 1)]


def good_frames(kind):
    """the known-good neighbours every test interleaves"""
    return [full(kind, ACT[0], 11, mixed_changes(ACT[0], 11), ts=77),
            message(kind, ChangeV1(ACT[1], Empty((4, 9), ts=12345))),
            message(kind, ChangeV1(ACT[2], EmptySet([(1, 2), (5, 9)], ts=99))),
            full(kind, ACT[3], 12, [Change("users", k - 2, "age", k, 1, 12, k, ACT[3], 1) for k in range(5)], ts=78)]


def interleave(items, kind, every=5):
    """items with a good frame after every `every` of them -> (payloads, indices of the good ones)"""
    good = good_frames(kind)
    out, idx = [], []
    for i, x in enumerate(items):
        out.append(x)
        if i % every == every - 1 or i == len(items) - 1:
            idx.append(len(out))
            out.append(good[len(idx) % len(good)])
    return out, idx


def one(kind, ch, **kw):
    return full(kind, ACT[0], 21, [Change("users", 1, "age", 1, 1, 21, 0, ACT[0], 1), ch,
                                   Change("users", 3, "age", 3, 1, 21, 2, ACT[0], 1)], **kw)


def directed(kind):
    """[(name, payload, the status the layout and the kernel's documented screens give)]"""
    P, S = prefix(kind), suffix(kind)
    A = ACT[0]

    def chg(pk=2, table="users", cid="age", val=2, cv=1, dbv=21, seq=1, cl=1):
        return Change(table, pk, cid, val, cv, dbv, seq, A, cl)

    body = A + struct.pack("<IQQB", 0, 1, 2, 0)
    cases = []
    if kind == wire.PAYLOAD_SYNC:
        cases += [("first tag nonzero", struct.pack("<II", 1, 1) + body, 1),
                  ("second tag Clock", struct.pack("<IIQ", 0, 2, 42), 1),
                  ("second tag Request", struct.pack("<II", 0, 4) + body, 1)]
    else:
        cases += [("first tag nonzero", struct.pack("<III", 1, 0, 0) + body + S, 1),
                  ("second tag nonzero", struct.pack("<III", 0, 1, 0) + body + S, 1),
                  ("third tag nonzero", struct.pack("<III", 0, 0, 2) + body + S, 1)]
    set3 = struct.pack("<II", 2, 3) + struct.pack("<QQQQQQ", 1, 2, 4, 5, 7, 9)
    huge = P + A + struct.pack("<II", 2, 0x10000000)
    cases += [
        ("changeset variant 3", P + A + struct.pack("<IQQB", 3, 1, 2, 0) + S, -1),
        ("Empty option byte 2", P + A + struct.pack("<IQQB", 0, 1, 2, 2) + struct.pack("<Q", 5) + S, -1),
        ("Empty option byte 0", P + A + struct.pack("<IQQB", 0, 1, 2, 0) + S, 0),
        ("Empty ends after versions", P + A + struct.pack("<IQQ", 0, 1, 2), 0),
        ("Empty lone option byte 1", P + A + struct.pack("<IQQB", 0, 1, 2, 1), -1),
        ("EmptySet count 2^28 in 60 bytes", huge + bytes(60 - len(huge)), -1),
        ("EmptySet exact count, ts missing", P + A + set3, -1),
        ("EmptySet exact count, ts present", P + A + set3 + struct.pack("<Q", 6) + S, 0),
        ("EmptySet of no ranges", P + A + struct.pack("<IIQ", 2, 0, 6) + S, 0),
        ("Full count 0", full(kind, A, 5, []), 0),
        ("Full count one more than present", full(kind, A, 5, [chg(), chg(3)], count=3, seqs=(0, 5)), -1),
        ("Full count one fewer than present", full(kind, A, 5, [chg(), chg(3)], count=1), 0),
        ("value tag 5", one(kind, chg(val=Raw(b"\x05"))), -1),
        ("value tag 255", one(kind, chg(val=Raw(b"\xFF" + bytes(8)))), -1),
        ("NaN quiet", one(kind, chg(val=real_bits(0x7FF8000000000000))), 0),
        ("NaN signalling", one(kind, chg(val=real_bits(0x7FF0000000000001))), 0),
        ("NaN quiet, sign set", one(kind, chg(val=real_bits(0xFFF8000000000000))), 0),
        ("NaN signalling, sign set", one(kind, chg(val=real_bits(0xFFF0000000000001))), 0),
        ("NaN all ones", one(kind, chg(val=real_bits(0xFFFFFFFFFFFFFFFF))), 0),
        ("+inf", one(kind, chg(val=real_bits(0x7FF0000000000000))), 0),
        ("-inf", one(kind, chg(val=real_bits(0xFFF0000000000000))), 0),
        ("-0.0", one(kind, chg(val=real_bits(0x8000000000000000))), 0),
        ("largest finite", one(kind, chg(val=real_bits(0x7FEFFFFFFFFFFFFF))), 0),
        ("seq 2^32 - 1", one(kind, chg(seq=(1 << 32) - 1)), 0),
        ("seq 2^32", one(kind, chg(seq=1 << 32)), -6),
        ("cl -1", one(kind, chg(cl=-1)), -6),
        ("cl 2^32 - 1", one(kind, chg(cl=(1 << 32) - 1)), 0),
        ("cl 2^32", one(kind, chg(cl=1 << 32)), -6),
        ("db_version 2^63 - 1", one(kind, chg(dbv=(1 << 63) - 1)), 0),
        ("db_version 2^63", one(kind, chg(dbv=1 << 63)), -6),
        ("pk type byte TEXT", one(kind, chg(pk=bytes([1, (1 << 3) | 3, 1, 97]))), -6),
        ("pk of 9 bytes", one(kind, chg(pk=pk_int_n(1, 9))), -6),
        ("pk of 8 bytes", one(kind, chg(pk=pk_int_n(-2, 8))), 0),
        ("pk shorter than its type byte says", one(kind, chg(pk=bytes([1, (2 << 3) | 1, 5]))), -6),
        ("pk longer than its type byte says", one(kind, chg(pk=bytes([1, (1 << 3) | 1, 5, 6]))), -6),
        ("pk of one byte", one(kind, chg(pk=b"\x01")), -6),
        ("pk empty", one(kind, chg(pk=b"")), -6),
        ("two-column pk, plain table", one(kind, chg(pk=bytes([2, 9, 1, 9, 2]))), -6),
        ("pk not canonical, plain table", one(kind, chg(pk=pk_int_n(5, 3))), 0),
        ("interned pk malformed", one(kind, chg(pk=KV_PK_BAD, table="kv", cid="v")), -1),
        ("interned pk empty", one(kind, chg(pk=b"", table="kv", cid="v")), -1),
        ("interned pk not canonical", one(kind, chg(pk=KV_PK_LOOSE, table="kv", cid="v")), 0),
        ("E_RANGE change and malformed interned pk",
         full(kind, A, 22, [chg(seq=1 << 32), chg(pk=KV_PK_BAD, table="kv", cid="v")]), -6),
        ("malformed interned pk and E_RANGE change",
         full(kind, A, 22, [chg(pk=KV_PK_BAD, table="kv", cid="v"), chg(cl=-1)]), -6),
        ("unknown table, malformed pk", one(kind, chg(pk=bytes([2, 9, 1, 9, 2]), table="nope")), 0),
        ("unknown column, malformed pk", one(kind, chg(pk=b"\x07", cid="zz")), 0),
        ("unknown column of an interned table, malformed pk", one(kind, chg(pk=KV_PK_BAD, table="kv", cid="zz")), 0),
        ("table name not UTF-8", one(kind, chg()).replace(b"\x05\x00\x00\x00users", b"\x05\x00\x00\x00\xff\xfeers", 1), 0),
        ("TEXT not UTF-8", one(kind, chg(val=Raw(b"\x03" + struct.pack("<I", 3) + b"\xff\xc0\x80"))), 0),
    ]
    return cases


def fuzz_bases():
    """about 20 well-formed Full frames of 300 to 800 bytes, both payload kinds, plain / interned /
    unknown tables, and one above 16 KB"""
    rng = np.random.default_rng(77)
    bases = []
    for i in range(20):
        kind = KINDS[i % 2]
        a = ACT[i % 4]
        ch = []
        for k in range(int(rng.integers(4, 9))):
            t = ["users", "t2", "kv", "wide", "nope"][int(rng.choice(5, p=[0.4, 0.2, 0.15, 0.15, 0.1]))]
            cols = SCHEMA.get(t, ["zz"])
            cid = "-1" if rng.random() < 0.1 else cols[int(rng.integers(len(cols)))]
            r = rng.random()
            val = (None if cid == "-1" or r < 0.15 else int(rng.integers(-(1 << 62), 1 << 62)) if r < 0.4 else
                   float(rng.choice([0.0, -2.5, 1e300, float("inf")])) if r < 0.55 else
                   "".join(chr(97 + int(x)) for x in rng.integers(0, 26, int(rng.integers(0, 30)))) if r < 0.8 else
                   bytes(rng.integers(0, 256, int(rng.integers(0, 30))).astype(np.uint8)))
            pk = (KV_PK[:-1] + bytes([97 + k]) if t == "kv" else bytes([2, 9, k, (1 << 3) | 3, 1, 98]) if t == "wide" else
                  int(rng.choice([k, -k - 1, int(rng.integers(-(1 << 40), 1 << 40)), 1 << 60])))
            ch.append(Change(t, pk, cid, val, int(rng.integers(1, 9)), i + 1, k, ACT[int(rng.integers(5))] if
                             rng.random() < 0.3 else a, int(rng.choice([1, 1, 2, 3]))))
        bases.append((full(kind, a, i + 1, ch, ts=1000 + i), kind))
        assert 300 <= len(bases[-1][0]) <= 800, len(bases[-1][0])
    big = [Change("users", 1, "blob", bytes(range(256)) * 66, 1, 30, 0, ACT[0], 1)] + \
          [Change("users", k, "age", k, 1, 30, k, ACT[0], 1) for k in range(1, 6)]
    bases.append((full(wire.PAYLOAD_SYNC, ACT[0], 30, big), wire.PAYLOAD_SYNC))
    return bases


FUZZ_N, FUZZ_SEED = 2000, 20261


def fuzz_frames():
    return M.mutate(fuzz_bases(), FUZZ_N, FUZZ_SEED)
