"""Wire format of the changesets corrosion gossips and syncs (host side, and the test encoder).

Restates the speedy 0.8.7 encoding (`corro-speedy` in Cargo.lock; not vendored in the reference)
of the types on the apply path, as derived for them in the reference:
  * little-endian integers; `Vec<T>` / `String` / `&str` / `[u8]` = u32 length + elements;
    `Option<T>` = u8 0/1 + value; derived enums = u32 variant index + fields in declaration order;
    `RangeInclusive<T>` = start, end; fixed arrays raw;
  * `ChangeV1 { actor_id: ActorId (16 raw bytes, actor.rs:91-104), changeset }` and
    `Changeset::{Empty{versions, ts: Option<Timestamp> (default_on_eof)}, Full{version, changes,
    seqs, last_seq, ts}, EmptySet{versions, ts}}` (broadcast.rs:114-148); `Timestamp` = u64
    (broadcast.rs:384-411); `CrsqlDbVersion`/`CrsqlSeq` = u64 (corro-base-types lib.rs:78-175);
  * `Change { table, pk, cid, val, col_version, db_version, seq, site_id, cl }` (change.rs:19-30)
    with `TableName`/`ColumnName` as str (corro-api-types lib.rs:781-850) and the hand-written
    `SqliteValue` encoding: u8 tag 0 Null | 1 i64 | 2 f64 | 3 u32 len + utf8 | 4 u32 len + bytes
    (lib.rs:615-680);
  * frames: tokio `LengthDelimitedCodec` defaults, u32 big-endian length + payload
    (peer/mod.rs:917-929, sync.rs:366-376);
  * `SyncMessage::V1(SyncMessageV1::Changeset(ChangeV1))` = u32 0, u32 1, ChangeV1 (sync.rs:19-30);
    `UniPayload::V1 { data: UniPayloadV1::Broadcast(BroadcastV1::Change(ChangeV1)), cluster_id }`
    = u32 0, u32 0, u32 0, ChangeV1, u16 cluster id (default_on_eof) (broadcast.rs:41-52, 93-96);
  * primary keys: `pack_columns` (pubsub.rs:2304-2384) / `unpack_columns` (:2396-2451).
The GPU decoder (csrc/wire.hip, corro_decode_frames) reads exactly this layout.
"""
import struct

from .agent import Change, ChangeV1, Empty, EmptySet, Full

PAYLOAD_SYNC, PAYLOAD_UNI = 0, 1


def _u32(x):
    return struct.pack("<I", x)


def _u64(x):
    return struct.pack("<Q", x & 0xFFFFFFFFFFFFFFFF)


def _i64(x):
    return struct.pack("<q", x)


def _bytes(b):
    return _u32(len(b)) + bytes(b)


def _num_bytes_i64(val):
    from .serve import num_bytes_needed_i64
    return num_bytes_needed_i64(val)


def pack_int_pk(v):
    """pack_columns([Integer(v)]): count 1, type byte (nbytes << 3 | 1), low nbytes big-endian."""
    n = _num_bytes_i64(v)
    return bytes([1, (n << 3) | 1]) + (v & ((1 << (8 * n)) - 1)).to_bytes(n, "big") if n else bytes([1, 1])


def unpack_int_pk(b):
    """unpack_columns for one INTEGER column: bytes::Buf::get_int(n) sign-extends n big-endian
    bytes (so pack/unpack round-trips only values whose top packed bit matches their sign)."""
    if len(b) < 2 or b[0] != 1 or (b[1] & 7) != 1:
        raise ValueError("not a single INTEGER packed pk")
    n = b[1] >> 3
    if n == 0:
        return 0
    v = int.from_bytes(b[2:2 + n], "big")
    if v >= 1 << (8 * n - 1):
        v -= 1 << (8 * n)
    return v


def encode_value(v):
    if v is None:
        return b"\x00"
    if isinstance(v, bool) or isinstance(v, int):
        return b"\x01" + _i64(v)
    if isinstance(v, float):
        return b"\x02" + struct.pack("<d", v)
    if isinstance(v, str):
        return b"\x03" + _bytes(v.encode())
    return b"\x04" + _bytes(bytes(v))


def encode_change(ch):
    pk = ch.pk if isinstance(ch.pk, (bytes, bytearray)) else pack_int_pk(ch.pk)
    return (_bytes(ch.table.encode()) + _bytes(pk) + _bytes(ch.cid.encode()) + encode_value(ch.val) +
            _i64(ch.col_version) + _u64(ch.db_version) + _u64(ch.seq) + bytes(ch.site_id) + _i64(ch.cl))


def encode_changeset(cs):
    if isinstance(cs, Empty):
        ts = b"\x00" if cs.ts is None else b"\x01" + _u64(cs.ts)
        return _u32(0) + _u64(cs.versions[0]) + _u64(cs.versions[1]) + ts
    if isinstance(cs, Full):
        return (_u32(1) + _u64(cs.version) + _u32(len(cs.changes)) + b"".join(encode_change(c) for c in cs.changes) +
                _u64(cs.seqs[0]) + _u64(cs.seqs[1]) + _u64(cs.last_seq) + _u64(cs.ts or 0))
    if isinstance(cs, EmptySet):
        return _u32(2) + _u32(len(cs.versions)) + b"".join(_u64(s) + _u64(e) for s, e in cs.versions) + _u64(cs.ts or 0)
    raise TypeError(cs)


def encode_changev1(cv):
    return bytes(cv.actor_id) + encode_changeset(cv.changeset)


def encode_sync_changeset(cv):
    """SyncMessage::V1(SyncMessageV1::Changeset(cv))"""
    return _u32(0) + _u32(1) + encode_changev1(cv)


def encode_uni_change(cv, cluster_id=0):
    """UniPayload::V1 { data: UniPayloadV1::Broadcast(BroadcastV1::Change(cv)), cluster_id }"""
    return _u32(0) + _u32(0) + _u32(0) + encode_changev1(cv) + struct.pack("<H", cluster_id)


def encode_sync_request(actor_id, needs):
    """SyncMessage::V1(SyncMessageV1::Request(vec![(actor_id, needs)])) (sync.rs:19-30, SyncRequestV1 =
    Vec<(ActorId, Vec<SyncNeedV1>)>): u32 0, u32 4, u32 1, the 16 id bytes, u32 count, then per need
    Full = u32 0 + versions start, end; Partial = u32 1 + version + Vec of seq ranges (sync.rs:252-264).
    `needs` holds sync.Full / sync.Partial; SyncNeedV1::Empty is never requested."""
    from . import sync as S
    if len(actor_id) != 16:
        raise ValueError("an actor id is 16 bytes")
    out = [_u32(0), _u32(4), _u32(1), bytes(actor_id), _u32(len(needs))]
    for nd in needs:
        if isinstance(nd, S.Full):
            out.append(_u32(0) + _u64(nd.start) + _u64(nd.end))
        elif isinstance(nd, S.Partial):
            out.append(_u32(1) + _u64(nd.version) + _u32(len(nd.seqs)) + b"".join(_u64(s) + _u64(e) for s, e in nd.seqs))
        else:
            raise TypeError(nd)
    return b"".join(out)


def decode_sync_request(payload):
    """The inverse of encode_sync_request for a Request of any number of (actor, needs) pairs: a list
    of (actor_id, [sync.Full | sync.Partial, ...]). Raises ValueError for anything else."""
    from . import sync as S
    pos = 0

    def take(fmt, size):
        nonlocal pos
        if pos + size > len(payload):
            raise ValueError("truncated sync request")
        v = struct.unpack_from(fmt, payload, pos)[0]
        pos += size
        return v

    if take("<I", 4) != 0 or take("<I", 4) != 4:
        raise ValueError("not a SyncMessage::V1 Request")
    out = []
    for _ in range(take("<I", 4)):
        if pos + 16 > len(payload):
            raise ValueError("truncated sync request")
        actor = bytes(payload[pos:pos + 16])
        pos += 16
        needs = []
        for _ in range(take("<I", 4)):
            tag = take("<I", 4)
            if tag == 0:
                s = take("<Q", 8)
                needs.append(S.Full(s, take("<Q", 8)))
            elif tag == 1:
                v = take("<Q", 8)
                seqs = []
                for _ in range(take("<I", 4)):
                    s = take("<Q", 8)
                    seqs.append((s, take("<Q", 8)))
                needs.append(S.Partial(v, tuple(seqs)))
            else:
                raise ValueError(f"SyncNeedV1 variant {tag} is not a request")
        out.append((actor, needs))
    if pos != len(payload):
        raise ValueError("trailing bytes after the sync request")
    return out


def encode_sync_state(state):
    """SyncMessage::V1(SyncMessageV1::State(state)) for a sync.SyncStateV1 (sync.rs:19-30, :79-87): u32 0,
    u32 0, the 16 id bytes, heads = u32 n + (actor, u64 head)*, need = u32 n + (actor, Vec of (start, end))*,
    partial_need = u32 n + (actor, u32 m + (version, Vec of (start, end))*)*, last_cleared_ts = u8 0 | u8 1 +
    u64. A HashMap goes on the wire in iteration order: the dicts' order is kept."""
    if len(state.actor_id) != 16:
        raise ValueError("an actor id is 16 bytes")
    ranges = lambda rs: _u32(len(rs)) + b"".join(_u64(s) + _u64(e) for s, e in rs)
    out = [_u32(0), _u32(0), bytes(state.actor_id), _u32(len(state.heads))]
    out += [bytes(a) + _u64(h) for a, h in state.heads.items()]
    out.append(_u32(len(state.need)))
    out += [bytes(a) + ranges(rs) for a, rs in state.need.items()]
    out.append(_u32(len(state.partial_need)))
    for a, part in state.partial_need.items():
        out.append(bytes(a) + _u32(len(part)) + b"".join(_u64(v) + ranges(rs) for v, rs in part.items()))
    out.append(b"\x00" if state.last_cleared_ts is None else b"\x01" + _u64(state.last_cleared_ts))
    if any(len(a) != 16 for m in (state.heads, state.need, state.partial_need) for a in m):
        raise ValueError("an actor id is 16 bytes")
    return b"".join(out)


def decode_sync_state(payload):
    """The inverse of encode_sync_state: a sync.SyncStateV1 with need ranges as lists of (start, end) and
    the dicts in wire order (a repeated key: the last one wins, as HashMap::insert). last_cleared_ts is
    default_on_eof: a payload that ends after partial_need decodes to None. Raises ValueError for
    anything that is not exactly one state."""
    from . import sync as S
    pos = 0

    def take(fmt, size):
        nonlocal pos
        if pos + size > len(payload):
            raise ValueError("truncated sync state")
        v = struct.unpack_from(fmt, payload, pos)[0]
        pos += size
        return v

    def actor():
        return bytes(take("16s", 16))

    def ranges():
        out = []
        for _ in range(take("<I", 4)):
            s = take("<Q", 8)
            out.append((s, take("<Q", 8)))
        return out

    if take("<I", 4) != 0 or take("<I", 4) != 0:
        raise ValueError("not a SyncMessage::V1 State")
    st = S.SyncStateV1(actor_id=actor())
    for _ in range(take("<I", 4)):
        a = actor()
        st.heads[a] = take("<Q", 8)
    for _ in range(take("<I", 4)):
        a = actor()
        st.need[a] = ranges()
    for _ in range(take("<I", 4)):
        a = actor()
        part = {}
        for _ in range(take("<I", 4)):
            v = take("<Q", 8)
            part[v] = ranges()
        st.partial_need[a] = part
    if pos != len(payload):
        opt = take("B", 1)
        if opt > 1:
            raise ValueError(f"Option tag {opt}")
        if opt:
            st.last_cleared_ts = take("<Q", 8)
    if pos != len(payload):
        raise ValueError("trailing bytes after the sync state")
    return st


def frame(payload):
    """LengthDelimitedCodec frame: u32 big-endian length + payload."""
    return struct.pack(">I", len(payload)) + payload


def frames(changes, kind=PAYLOAD_SYNC):
    enc = encode_sync_changeset if kind == PAYLOAD_SYNC else encode_uni_change
    return b"".join(frame(enc(cv)) for cv in changes)
