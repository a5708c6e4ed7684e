"""A plain host decoder of changeset frames: the inverse of corrosion_amd/wire.py's changeset encoder
and the independent statement of what corro_decode_frames (csrc/wire.hip) must give, malformed
input included. One cursor, `take(n)` that fails on a short read, no speculation, no clamping.
Nothing here comes from the GPU path.

Layout (wire.py's docstring; the reference files it cites): speedy 0.8.7, little endian, u32 enum
tags and length prefixes; `SyncMessage::V1(Changeset(ChangeV1))` = u32 0, u32 1 (sync.rs:19-30);
`UniPayload::V1 { Broadcast(Change(ChangeV1)), cluster_id }` = u32 0, u32 0, u32 0, ..., u16
(default_on_eof) (broadcast.rs:41-52, 93-96); `ChangeV1 { actor_id: 16 bytes, changeset }` and
`Changeset::{Empty 0, Full 1, EmptySet 2}` (broadcast.rs:114-148); `Change` (change.rs:19-30);
`SqliteValue` (corro-api-types lib.rs:615-641); packed pks: unpack_columns (pubsub.rs:2396-2451).

decode(payload, kind, schema, interned) -> (status, header, changes):
  status   1   the message tags were read in full and do not say "changeset"
          -1   the sequential parse fails anywhere (a short read -- inside the tags too --, a changeset
               variant >= 3, an Option byte other than 0 / 1, a value tag >= 5, fewer than 32 tail
               bytes), or a change of an interned table carries a packed pk unpack_columns rejects
          -6   the parse succeeds and a change fails one of k_wire_decode's CORRO_E_RANGE screens
               (each restated below with the kernel line it restates); -6 wins over a malformed
               interned pk, as the host loop's min(st, CORRO_E_INVALID) leaves it
           0   otherwise
  header   {"kind": "empty" | "full" | "empty_set", "actor": 16 bytes, "versions": (start, end) or, for
            an EmptySet, the list of ranges, "seqs": (start, end), "last_seq", "ts", "nchanges"}
  changes  one dict per change: "pk" (u64 after get_int sign extension; for a known column of an
           interned table the canonical packed bytes, which name its row), "table_cid", "col_version",
           "db_version", "cl", "seq", "site" (16 bytes), "val_type", "val0", "val1", "val_len", "ts" and
           "long" (None, or (offset in the payload, size) of a TEXT / BLOB over 16 bytes).
header and changes are None unless status is 0.

Rules that are not the layout itself:
  * trailing bytes after a changeset are accepted (speedy's read_from_buffer reads a prefix; the uni
    payload's cluster_id lies there, and its own default_on_eof accepts a cut inside it);
  * TEXT is not UTF-8 validated: the reference reads it with from_utf8_unchecked (lib.rs:625-631);
  * Empty's ts is Option<Timestamp> with default_on_eof: a frame that ends right after `versions`
    gives None (0 here); an option byte that is present is read as an Option (1 needs its 8 bytes);
  * NaN is bound as NULL by SQLite: (NULL, 0, 0, 0);
  * a change whose (table, cid) is not in the schema has table_cid 0xFFFFFFFF and is rolled back with
    its version by the caller, so its pk is not screened: a single packed INTEGER decodes, anything
    else gives pk 0.
"""
import struct

SYNC, UNI = 0, 1
T_INTEGER, T_REAL, T_TEXT, T_BLOB, T_NULL = 1, 2, 3, 4, 5   # ColumnType / the engine's val_type
VAL_LONG = 255
TCID_UNKNOWN = 0xFFFFFFFF
OK, NOT_CHANGESET, INVALID, RANGE = 0, 1, -1, -6


class Malformed(Exception):
    pass


class Cursor:
    def __init__(self, b):
        self.b, self.pos = bytes(b), 0

    def take(self, n):
        if n > len(self.b) - self.pos:
            raise Malformed(f"short read of {n} at {self.pos}")
        out = self.b[self.pos:self.pos + n]
        self.pos += n
        return out

    def u8(self):
        return self.take(1)[0]

    def u32(self):
        return struct.unpack("<I", self.take(4))[0]

    def u64(self):
        return struct.unpack("<Q", self.take(8))[0]

    def i64(self):
        return struct.unpack("<q", self.take(8))[0]

    def eof(self):
        return self.pos == len(self.b)


def _nbytes_i32(v):
    """num_bytes_needed_i32 (pubsub.rs:2376-2388) on the low 32 bits."""
    v &= 0xFFFFFFFF
    if v & 0xFF000000:
        return 4
    if v & 0x00FF0000:
        return 3
    if v & 0x0000FF00:
        return 2
    return 1 if (v * 0xFF) & 0xFFFFFFFF else 0


def _nbytes_i64(v):
    """num_bytes_needed_i64 (pubsub.rs:2363-2374)."""
    v &= 0xFFFFFFFFFFFFFFFF
    for n in (8, 7, 6, 5):
        if v & (0xFF << (8 * (n - 1))):
            return n
    return _nbytes_i32(v)


def _get_int(c, n):
    """bytes::Buf::get_int(n): n big-endian bytes, sign-extended; more than 8 cannot be an i64."""
    if n > 8:
        raise Malformed("integer of more than 8 bytes")
    return int.from_bytes(c.take(n), "big", signed=True) if n else 0


def unpack_pk(b):
    """unpack_columns (pubsub.rs:2396-2451) -> [(type, value)]; Malformed where it returns an error
    (or would read past the buffer). Bytes after the last column are ignored, as there."""
    c = Cursor(b)
    cols = []
    for _ in range(c.u8()):
        tb = c.u8()
        typ, intlen = tb & 7, tb >> 3
        if typ == T_INTEGER:
            cols.append((typ, _get_int(c, intlen)))
        elif typ == T_REAL:
            cols.append((typ, c.take(8)))
        elif typ in (T_TEXT, T_BLOB):
            n = _get_int(c, intlen)
            if n < 0:
                raise Malformed("negative length")
            cols.append((typ, c.take(n)))
        elif typ == T_NULL:
            cols.append((typ, None))
        else:
            raise Malformed("unknown column type")
    return cols


def pack_pk(cols):
    """pack_columns (pubsub.rs:2304-2358) of unpack_pk's result: the canonical bytes of a pk (-0.0 is
    stored as 0.0: one key in SQLite)."""
    out = bytearray([len(cols)])
    for typ, v in cols:
        if typ == T_INTEGER:
            n = _nbytes_i64(v)
            out.append((n << 3) | typ)
            out += (v & ((1 << (8 * n)) - 1)).to_bytes(n, "big")
        elif typ == T_REAL:
            out.append(typ)
            out += bytes(8) if v == b"\x80" + bytes(7) else v
        elif typ in (T_TEXT, T_BLOB):
            n = _nbytes_i32(len(v))
            out.append((n << 3) | typ)
            out += len(v).to_bytes(n, "big") + v
        else:
            out.append(typ)
    return bytes(out)


def _value(c):
    """SqliteValue (lib.rs:620-634) -> (val_type, val0, val1, val_len, long)."""
    tag = c.u8()
    if tag == 0:
        return T_NULL, 0, 0, 0, None
    if tag == 1:
        return T_INTEGER, c.u64(), 0, 0, None
    if tag == 2:
        bits = c.u64()
        if (bits >> 52) & 0x7FF == 0x7FF and bits & ((1 << 52) - 1):
            return T_NULL, 0, 0, 0, None
        return T_REAL, bits, 0, 0, None
    if tag in (3, 4):
        n = c.u32()
        at = c.pos
        b = c.take(n)
        if n > 16:
            return tag, int.from_bytes(b[:8], "big"), 0, VAL_LONG, (at, n)
        p = b + bytes(16 - n)
        return tag, int.from_bytes(p[:8], "big"), int.from_bytes(p[8:], "big"), n, None
    raise Malformed(f"unknown SqliteValue variant {tag}")


def _table_cid(schema, table, cid):
    for t, (name, cols) in enumerate(schema.items()):
        if name.encode() != table:
            continue
        if cid == b"-1":
            return t << 16
        for k, col in enumerate(cols):
            if col.encode() == cid:
                return (t << 16) | (k + 1)
        break
    return TCID_UNKNOWN


def decode(payload, kind, schema, interned=(), trace=None):
    """See the module docstring. `trace`, when a dict, receives the positions the mutation generator
    needs: "count" (the Full change count's offset) and "changes", per change a dict of its "start",
    "end" and the offsets of its "table" / "pk" / "cid" length prefixes, its value "tag" and its
    value length prefix "vlen" (None for a fixed-width value)."""
    payload = bytes(payload)
    c = Cursor(payload)
    try:
        for want in ((0, 1) if kind == SYNC else (0, 0, 0)):
            if c.u32() != want:
                return NOT_CHANGESET, None, None
        hdr = {"actor": c.take(16), "versions": None, "seqs": (0, 0), "last_seq": 0, "ts": 0, "nchanges": 0}
        raw = []
        variant = c.u32()
        if variant == 0:
            hdr["kind"] = "empty"
            hdr["versions"] = (c.u64(), c.u64())
            if not c.eof():                       # default_on_eof
                some = c.u8()
                if some == 1:
                    hdr["ts"] = c.u64()
                elif some != 0:
                    raise Malformed("Option byte")
        elif variant == 1:
            hdr["kind"] = "full"
            v = c.u64()
            hdr["versions"] = (v, v)
            if trace is not None:
                trace["count"], trace["changes"] = c.pos, []
            n = hdr["nchanges"] = c.u32()
            for _ in range(n):
                m = {"start": c.pos, "table": c.pos}
                table = c.take(c.u32())
                m["pk"] = c.pos
                pk = c.take(c.u32())
                m["cid"] = c.pos
                cid = c.take(c.u32())
                m["tag"] = c.pos
                m["vlen"] = c.pos + 1 if payload[c.pos:c.pos + 1] in (b"\x03", b"\x04") else None
                val = _value(c)
                raw.append((table, pk, cid, val, c.i64(), c.u64(), c.u64(), c.take(16), c.i64()))
                m["end"] = c.pos
                if trace is not None:
                    trace["changes"].append(m)
            hdr["seqs"] = (c.u64(), c.u64())
            hdr["last_seq"] = c.u64()
            hdr["ts"] = c.u64()
        elif variant == 2:
            hdr["kind"] = "empty_set"
            hdr["versions"] = [(c.u64(), c.u64()) for _ in range(c.u32())]
            hdr["ts"] = c.u64()
        else:
            raise Malformed("unknown Changeset variant")
    except Malformed:
        return INVALID, None, None

    status = OK
    changes = []
    tables = list(schema)
    for table, pk, cid, (vt, v0, v1, vl, long_), cv, dbv, seq, site, cl in raw:
        tcid = _table_cid(schema, table, cid)
        known = tcid != TCID_UNKNOWN
        if known and tables[tcid >> 16] in interned:
            # the host loop after the kernel: a pk corro_pk_keys rejects fails its frame,
            # st[f] = min(st[f], CORRO_E_INVALID)
            try:
                key = pack_pk(unpack_pk(pk))
            except Malformed:
                key = None
                status = min(status, INVALID)
        else:
            # k_wire_decode, "lp < 2 || p[pp] != 1 || (p[pp + 1] & 7) != 1 || (p[pp + 1] >> 3) + 2 != lp
            # || (p[pp + 1] >> 3) > 8": anything but exactly one packed INTEGER column...
            one_int = (len(pk) >= 2 and pk[0] == 1 and pk[1] & 7 == T_INTEGER and (pk[1] >> 3) + 2 == len(pk)
                       and pk[1] >> 3 <= 8)
            key = _get_int(Cursor(pk[2:]), pk[1] >> 3) & 0xFFFFFFFFFFFFFFFF if one_int else 0
            if not one_int and known:   # ... "if (known) err = CORRO_E_RANGE"
                status = min(status, RANGE)
        # k_wire_decode, "l >= (1u << 24)": a TEXT / BLOB of 16 MiB or more
        if long_ is not None and long_[1] >= 1 << 24:
            status = min(status, RANGE)
        # k_wire_decode, "seq > 0xFFFFFFFFULL || cl < 0 || cl > 0xFFFFFFFFLL || dbv > (uint64_t)INT64_MAX"
        if seq > 0xFFFFFFFF or cl < 0 or cl > 0xFFFFFFFF or dbv > (1 << 63) - 1:
            status = min(status, RANGE)
        changes.append({"pk": key, "table_cid": tcid, "col_version": cv, "db_version": dbv, "cl": cl, "seq": seq,
                        "site": site, "val_type": vt, "val0": v0, "val1": v1, "val_len": vl, "ts": hdr["ts"],
                        "long": long_})
    if status != OK:
        return status, None, None
    return OK, hdr, changes


# ---- the seeded mutation generator (tests/test_wire_model.py runs it through the model alone,
# tests/test_gpu_wire_edges.py through the decoder) -------------------------------------------------

def mutate(bases, n, seed):
    """n frames derived from `bases` = [(payload, kind), ...] (each a well-formed Full changeset the
    model accepts): 1 to 3 mutations each, drawn from: a length prefix overwritten with one of
    {0, 1, true - 1, true + 1, remaining, remaining + 1, 2^31, 2^32 - 1}; a value tag overwritten; one
    random byte flipped; the change count +-1; two changes' bytes swapped. Prefix and tag positions
    come from the model's parse of the frame being mutated (of the base frame once a mutation has
    made it unparseable). Returns [(payload, kind, base index)]."""
    import numpy as np
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        bi = int(rng.integers(len(bases)))
        base, kind = bases[bi]
        b = bytearray(base)
        tr = {}
        st, _h, _c = decode(base, kind, {}, (), tr)
        assert st == OK and tr["changes"], "a base frame must be a well-formed Full changeset"
        for _ in range(int(rng.integers(1, 4))):
            t2 = {}
            if decode(bytes(b), kind, {}, (), t2)[0] == OK and t2.get("changes"):
                tr = t2
            ch = tr["changes"]
            r = rng.random()
            if r < 0.25:                                    # a length prefix
                m = ch[int(rng.integers(len(ch)))]
                at = [m["table"], m["pk"], m["cid"]] + ([m["vlen"]] if m["vlen"] is not None else [])
                p = at[int(rng.integers(len(at)))]
                if p + 4 > len(b):
                    continue
                true = struct.unpack_from("<I", b, p)[0]
                rem = len(b) - (p + 4)
                v = [0, 1, true - 1, true + 1, rem, rem + 1, 1 << 31, (1 << 32) - 1][int(rng.integers(8))]
                struct.pack_into("<I", b, p, v & 0xFFFFFFFF)
            elif r < 0.35:                                  # a value tag
                m = ch[int(rng.integers(len(ch)))]
                if m["tag"] < len(b):
                    b[m["tag"]] = int(rng.choice([0, 1, 2, 3, 4, 5, 6, 255]))
            elif r < 0.75:                                  # one random byte
                p = int(rng.integers(len(b)))
                b[p] ^= 1 << int(rng.integers(8))
            elif r < 0.82:                                  # the change count
                cnt = struct.unpack_from("<I", b, tr["count"])[0]
                struct.pack_into("<I", b, tr["count"], (cnt + int(rng.choice([-1, 1]))) & 0xFFFFFFFF)
            elif len(ch) >= 2:                              # two changes swapped
                x, y = sorted(int(k) for k in rng.choice(len(ch), 2, replace=False))
                mx, my = ch[x], ch[y]
                if my["end"] <= len(b):
                    b = (b[:mx["start"]] + b[my["start"]:my["end"]] + b[mx["end"]:my["start"]] +
                         b[mx["start"]:mx["end"]] + b[my["end"]:])
        out.append((bytes(b), kind, bi))
    return out
