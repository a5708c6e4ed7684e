"""tests/wire_model.py, the plain host decoder the GPU wire decoder is pinned against
(tests/test_gpu_wire_edges.py): it decodes what corrosion_amd/wire.py encodes back to the same objects,
rejects each directed malformed frame with the documented code, and accepts / rejects enough of
the seeded mutation set that the differential over it is not vacuous."""
import pytest

from corrosion_amd import wire
from corrosion_amd.agent import Change, ChangeV1, Empty, EmptySet, Full, encode_value
from tests import wire_cases as W
from tests import wire_model as M

BOUNDS = sorted({s * v for n in range(1, 9) for v in ((1 << (8 * n - 1)) - 1, 1 << (8 * n - 1), (1 << (8 * n)) - 1,
                                                      1 << (8 * n)) for s in (1, -1)
                 if -(1 << 63) <= s * v < (1 << 63)} | {0, 1, -1, -(1 << 63), (1 << 63) - 1})
VALUES = [None, 0, -1, (1 << 63) - 1, -(1 << 63), 0.0, -0.0, 1.5, float("inf"), float("-inf"), float("nan"), 5e-324,
          "", "a" * 16, "b" * 17, "é" * 8, b"", bytes(range(16)), bytes(range(17)), b"\x00" * 40]


def expect_change(ch, ts):
    vt, v0, v1, ln = encode_value(ch.val)
    try:
        t = list(W.SCHEMA).index(ch.table)
        tcid = t << 16 if ch.cid == "-1" else (t << 16) | (W.SCHEMA[ch.table].index(ch.cid) + 1)
    except ValueError:
        tcid = M.TCID_UNKNOWN
    if tcid != M.TCID_UNKNOWN and ch.table in W.INTERNED:
        pk = bytes(ch.pk)                                   # (the cases here pack canonically)
    else:
        pk = wire.unpack_int_pk(wire.pack_int_pk(ch.pk)) & 0xFFFFFFFFFFFFFFFF
    return {"pk": pk, "table_cid": tcid, "col_version": ch.col_version, "db_version": ch.db_version, "cl": ch.cl,
            "seq": ch.seq, "site": ch.site_id, "val_type": vt, "val0": v0, "val1": v1, "val_len": ln, "ts": ts}


@pytest.mark.parametrize("kind", W.KINDS)
def test_roundtrip_changesets(kind):
    ch = [Change("users", 5, "name", v, k + 1, 40, k, W.ACT[k % 5], 1 + k % 3) for k, v in enumerate(VALUES)]
    ch += [Change("t2", pk, "x", k, 1, 40, len(VALUES) + k, W.ACT[0], 1) for k, pk in enumerate(BOUNDS)]
    ch += W.mixed_changes(W.ACT[0], 40)
    msgs = [ChangeV1(W.ACT[0], Full(40, ch, (3, len(ch) + 2), len(ch) + 9, ts=(1 << 63) + 5)),
            ChangeV1(W.ACT[1], Full(41, [], (0, 0), 0, ts=0)),
            ChangeV1(W.ACT[2], Empty((4, 9), ts=None)), ChangeV1(W.ACT[2], Empty((0, (1 << 64) - 1), ts=12345)),
            ChangeV1(W.ACT[3], EmptySet([], ts=7)), ChangeV1(W.ACT[3], EmptySet([(1, 2), (5, 5), (9, 1 << 40)], ts=8))]
    for m in msgs:
        payload = W.message(kind, m)
        st, hdr, got = M.decode(payload, kind, W.SCHEMA, W.INTERNED)
        assert st == 0 and hdr["actor"] == m.actor_id
        x = m.changeset
        if isinstance(x, Full):
            assert (hdr["kind"], hdr["versions"], hdr["seqs"], hdr["last_seq"], hdr["ts"], hdr["nchanges"]) == \
                   ("full", (x.version, x.version), x.seqs, x.last_seq, x.ts, len(x.changes))
            for c, g in zip(x.changes, got):
                long_ = g.pop("long")
                assert g == expect_change(c, x.ts), c
                raw = c.val.encode() if isinstance(c.val, str) else c.val
                if isinstance(raw, bytes) and len(raw) > 16:
                    assert payload[long_[0]:long_[0] + long_[1]] == raw
                else:
                    assert long_ is None
        elif isinstance(x, Empty):
            assert (hdr["kind"], hdr["versions"], hdr["ts"], got) == ("empty", x.versions, x.ts or 0, [])
        else:
            assert (hdr["kind"], hdr["versions"], hdr["ts"], got) == ("empty_set", x.versions, x.ts, [])


def test_pk_boundaries_roundtrip():
    """every byte-count boundary of pack_columns' INTEGER: the model's get_int gives what
    wire.unpack_int_pk gives, and packs canonically what wire.pack_int_pk packs"""
    assert {0, 127, -127, 128, -128, 255, -255, 256, -256, -(1 << 63), (1 << 63) - 1} <= set(BOUNDS)
    for v in BOUNDS:
        b = wire.pack_int_pk(v)
        (typ, got), = M.unpack_pk(b)
        assert typ == M.T_INTEGER and got == wire.unpack_int_pk(b)
        assert M.pack_pk([(typ, v)]) == b
    assert M.pack_pk(M.unpack_pk(W.KV_PK_LOOSE)) == W.KV_PK and M.pack_pk(M.unpack_pk(W.WIDE_PK)) == W.WIDE_PK
    with pytest.raises(M.Malformed):
        M.unpack_pk(W.KV_PK_BAD)


@pytest.mark.parametrize("kind", W.KINDS)
def test_directed_cases(kind):
    for name, payload, want in W.directed(kind):
        assert M.decode(payload, kind, W.SCHEMA, W.INTERNED)[0] == want, name
    for g in W.good_frames(kind):
        assert M.decode(g, kind, W.SCHEMA, W.INTERNED)[0] == 0


def test_directed_values():
    """what the accepted directed cases decode to: NaN of every kind is NULL, +-inf and -0.0 stay REAL
    bit for bit, an unscreened malformed pk is 0, a loose interned pk is its canonical bytes"""
    got = {}
    for name, payload, _want in W.directed(wire.PAYLOAD_SYNC):
        st, _hdr, ch = M.decode(payload, wire.PAYLOAD_SYNC, W.SCHEMA, W.INTERNED)
        if st == 0 and ch and len(ch) == 3:
            got[name] = ch[1]
    for name, c in got.items():
        if name.startswith("NaN"):
            assert (c["val_type"], c["val0"], c["val1"], c["val_len"]) == (M.T_NULL, 0, 0, 0), name
    for name, bits in (("+inf", 0x7FF0 << 48), ("-inf", 0xFFF0 << 48), ("-0.0", 1 << 63)):
        assert (got[name]["val_type"], got[name]["val0"]) == (M.T_REAL, bits)
    assert got["unknown table, malformed pk"]["pk"] == 0 and got["unknown column, malformed pk"]["pk"] == 0
    assert got["unknown column of an interned table, malformed pk"]["table_cid"] == M.TCID_UNKNOWN
    assert got["interned pk not canonical"]["pk"] == W.KV_PK
    assert got["pk of 8 bytes"]["pk"] == (1 << 64) - 2 and got["pk not canonical, plain table"]["pk"] == 5
    bad_name = dict((n, p) for n, p, _w in W.directed(wire.PAYLOAD_SYNC))["table name not UTF-8"]
    assert [c["table_cid"] for c in M.decode(bad_name, 0, W.SCHEMA, W.INTERNED)[2]] == [M.TCID_UNKNOWN, 2, 2]
    assert (got["TEXT not UTF-8"]["val_type"], got["TEXT not UTF-8"]["val_len"]) == (M.T_TEXT, 3)


@pytest.mark.parametrize("kind", W.KINDS)
def test_truncations(kind):
    """every cut of a Full frame is rejected, except (uni) a cut inside the trailing cluster_id; an
    Empty that ends right after `versions` is accepted with ts 0"""
    p = W.good_frames(kind)[0]
    tail = 2 if kind == wire.PAYLOAD_UNI else 0
    ntag = 8 if kind == wire.PAYLOAD_SYNC else 12
    for n in range(len(p)):
        st = M.decode(p[:n], kind, W.SCHEMA, W.INTERNED)[0]
        assert st == (0 if n >= len(p) - tail else -1), n
    e = W.good_frames(kind)[1]
    for n in range(len(e)):
        st, hdr, _ = M.decode(e[:n], kind, W.SCHEMA, W.INTERNED)
        if n == ntag + 16 + 4 + 16:
            assert st == 0 and hdr["ts"] == 0 and hdr["versions"] == (4, 9)
        else:
            assert st == (0 if n >= len(e) - tail else -1), n


def test_fuzz_mix():
    """the mutation set of the GPU differential, through the model alone: at least one fifth accepted
    and at least one fifth rejected as malformed, so neither side of the comparison is idle"""
    frames = W.fuzz_frames()
    assert len(frames) == W.FUZZ_N
    st = [M.decode(p, kind, W.SCHEMA, W.INTERNED)[0] for p, kind, _b in frames]
    acc, rej, rng_ = st.count(0), st.count(-1), st.count(-6)
    print(f"fuzz mix: {acc} accepted, {rej} malformed, {rng_} out of range, {st.count(1)} not changesets")
    assert acc + rej + rng_ + st.count(1) == W.FUZZ_N
    assert acc * 5 >= W.FUZZ_N and rej * 5 >= W.FUZZ_N
    assert sum(1 for p, _k, b in frames if b == 20) > 20          # the base above 16 KB is in the mix
    assert W.fuzz_frames() == frames                              # seeded: the same set every run
