"""Mirror of corrosion's apply entry points over the device engine.

Types mirror corro-types: `Change` (change.rs:19-30), `ChangeV1` / `Changeset::{Full, Empty,
EmptySet}` (broadcast.rs:114-148); functions mirror corro-agent/src/agent/util.rs:
`process_multiple_changes` (:691), `process_fully_buffered_changes` (:541) and corro-types
`generate_sync` (sync.rs:284). All logic runs in libcorro_hip.so (csrc/agent.cpp + the HIP merge);
this module converts the Python objects to the C ABI structs and back.
"""
import ctypes as C
import struct
from dataclasses import dataclass, field

import numpy as np

from . import _lib as L
from .engine import MergeEngine
from .sync import SyncStateV1
from ._twopass import Mem


@dataclass
class Change:
    table: str
    pk: object              # INTEGER pk value, or pack_columns bytes (interned tables: any pk)
    cid: str                # column name, "-1" = row sentinel
    val: object             # None | int | float | str | bytes  (SqliteValue)
    col_version: int
    db_version: int
    seq: int
    site_id: bytes          # 16 bytes
    cl: int


@dataclass
class Full:
    version: int
    changes: list
    seqs: tuple             # (start, end) inclusive
    last_seq: int
    ts: int = 0


@dataclass
class Empty:
    versions: tuple         # (start, end) inclusive
    ts: int = None


@dataclass
class EmptySet:
    versions: list
    ts: int = 0


@dataclass
class ChangeV1:
    actor_id: bytes
    changeset: object


def value_bytes(v):
    """The bytes of a TEXT/BLOB SqliteValue (None for other classes)."""
    if v is None or isinstance(v, (bool, int, float)):
        return None
    return v.encode() if isinstance(v, str) else bytes(v)


def encode_value(v):
    """SqliteValue -> (type, val0, val1, len) of the engine's fixed-width value encoding. A TEXT/BLOB
    longer than 16 bytes gives len = CORRO_VAL_LONG and its first 8 bytes in val0: its bytes travel in
    the batch's val_data (value_bytes)."""
    if v is None:
        return L_NULL, 0, 0, 0
    if isinstance(v, bool) or isinstance(v, int):
        return 1, int(v) & 0xFFFFFFFFFFFFFFFF, 0, 0
    if isinstance(v, float):
        if v != v:
            return L_NULL, 0, 0, 0  # SQLite binds NaN as NULL
        return 2, struct.unpack("<Q", struct.pack("<d", v))[0], 0, 0
    b = v.encode() if isinstance(v, str) else bytes(v)
    if len(b) > 16:
        if len(b) >= 1 << 24:
            raise L.CorroError(-6, "TEXT/BLOB values of 16 MiB or more are outside the engine encoding")
        return (3 if isinstance(v, str) else 4), int.from_bytes(b[:8], "big"), 0, L.CORRO_VAL_LONG
    p = b + b"\0" * (16 - len(b))
    return (3 if isinstance(v, str) else 4), int.from_bytes(p[:8], "big"), int.from_bytes(p[8:], "big"), len(b)


L_NULL = 5


@dataclass
class Processed:
    known: list                               # per ChangeV1: "skipped" | "current" | "cleared" | "partial" | error code
    impactful: list = field(default_factory=list)  # per ChangeV1: impactful Change list (Full only)
    ready: list = field(default_factory=list)      # (actor, version) now fully buffered


class Bookie:
    def __init__(self):
        h = C.c_void_p()
        L.check(L.lib().corro_bookie_new(C.byref(h)))
        self._h = h

    def __del__(self):
        if getattr(self, "_h", None):
            L.lib().corro_bookie_free(self._h)
            self._h = None

    def last(self, actor):
        v = C.c_int64()
        L.check(L.lib().corro_bookie_last(self._h, actor, C.byref(v)))
        return None if v.value < 0 else v.value

    def needed(self, actor):
        c = C.c_uint64()
        L.check(L.lib().corro_bookie_needed(self._h, actor, None, None, 0, C.byref(c)))
        s = np.zeros(max(1, c.value), np.uint64)
        e = np.zeros(max(1, c.value), np.uint64)
        L.check(L.lib().corro_bookie_needed(self._h, actor, s.ctypes.data, e.ctypes.data, c.value, C.byref(c)))
        return [(int(s[i]), int(e[i])) for i in range(c.value)]

    def contains_all(self, actor, versions, seqs=None):
        r = C.c_int()
        L.check(L.lib().corro_bookie_contains_all(self._h, actor, versions[0], versions[1], 1 if seqs else 0,
                                                   seqs[0] if seqs else 0, seqs[1] if seqs else 0, C.byref(r)))
        return bool(r.value)

    def partial(self, actor, version):
        """(seq ranges, last_seq) of a partially received version, or None."""
        c, last = C.c_uint64(), C.c_int64()
        # sizing call first (cap 0), then the ranges: a version may hold any number of seq ranges
        L.check(L.lib().corro_bookie_partial(self._h, actor, version, None, None, 0, C.byref(c), C.byref(last)))
        if last.value < 0:
            return None
        n = int(c.value)
        s = np.zeros(max(n, 1), np.uint64)
        e = np.zeros(max(n, 1), np.uint64)
        L.check(L.lib().corro_bookie_partial(self._h, actor, version, s.ctypes.data, e.ctypes.data, n,
                                             C.byref(c), C.byref(last)))
        return [(int(s[i]), int(e[i])) for i in range(n)], int(last.value)

    def sync_book(self):
        """The bookie as one sync book (corro_bookie_sync_book): what generate_sync reads, one row per actor
        in generate_sync's order, as numpy arrays keyed like corro_sync_book -- "actor" (nrows x 16), "max"
        (int64, -1 = None), the needed gaps ("gap_off", "gap_start", "gap_end") and every partial
        ("part_off", "part_version", "part_last_seq") with the seq ranges it holds ("psr_off", "psr_start",
        "psr_end"). sync.state_frames_from_books takes it."""
        lib = L.lib()
        bk = L.SyncBook()
        L.check(lib.corro_bookie_sync_book(self._h, C.byref(bk), 0))
        nr, ng, npt, ns = bk.nrows, bk.ngaps, bk.nparts, bk.npsr
        sizes = {"actor": 16 * nr, "max": nr, "gap_off": nr + 1, "gap_start": ng, "gap_end": ng, "part_off": nr + 1,
                 "part_version": npt, "part_last_seq": npt, "psr_off": npt + 1, "psr_start": ns, "psr_end": ns}
        dts = {"actor": np.uint8, "max": np.int64}
        bufs = {k: np.zeros(max(1, n), dts.get(k, np.uint64)) for k, n in sizes.items()}
        for k, a in bufs.items():
            setattr(bk, k, a.ctypes.data)
        L.check(lib.corro_bookie_sync_book(self._h, C.byref(bk), 1))
        book = {k: bufs[k][:n] for k, n in sizes.items()}
        book["actor"] = book["actor"].reshape(nr, 16)
        return book


    def save(self, engine=None, device=False):
        """The bookie's image (corro_bookie_save): the three bookkeeping tables and the per-actor max as
        numpy arrays keyed like corro_bookie_image, "rows" = the __corro_buffered_changes rows sorted by
        (site, db_version, seq) -- numpy arrays, or with device=True CUDA tensors gathered from the device
        row pool without visiting the host. engine: the MergeEngine whose context holds the rows (None: a
        bookie without pool rows)."""
        from ._twopass import Mem, save_image
        mem = Mem("cuda:%d" % engine.device) if device else Mem()
        return save_image(L.lib().corro_bookie_save, engine._h if engine is not None else None, self._h, mem)

    def load(self, image, engine=None):
        """Load an image into this (empty) bookie (corro_bookie_load): from_conn per actor, the rows sorted
        and cut into pool segments on the device. Without rows no engine is needed and no device is
        touched. The fully buffered versions found are listed by take_ready."""
        from ._twopass import load_image
        load_image(L.lib().corro_bookie_load, engine._h if engine is not None else None, self._h, image)

    def take_ready(self):
        c = C.c_uint64()
        L.check(L.lib().corro_bookie_take_ready(self._h, None, None, 0, C.byref(c)))
        if c.value == 0:
            return []
        a = np.zeros((c.value, 16), np.uint8)
        v = np.zeros(c.value, np.uint64)
        L.check(L.lib().corro_bookie_take_ready(self._h, a.ctypes.data, v.ctypes.data, c.value, C.byref(c)))
        return [(bytes(a[k]), int(v[k])) for k in range(c.value)]

    def process_ready(self, engine, pairs):
        """process_fully_buffered_changes of the (actor, version) pairs in list order as one batch
        (corro_process_fully_buffered_batch): the rows gathered out of the device row pool, one apply.
        Returns the per-pair results: 0 not applied, 1 applied with no row impacted, 2 applied with
        rows impacted, negative = the pair's own gap bookkeeping refused it. engine: the MergeEngine the
        rows are merged into (None: a list that brings no row)."""
        n = len(pairs)
        if n == 0:
            return []
        a = np.frombuffer(b"".join(bytes(p[0]) for p in pairs), np.uint8)
        v = np.array([p[1] for p in pairs], np.uint64)
        res = np.zeros(n, np.int32)
        L.check(L.lib().corro_process_fully_buffered_batch(engine._h if engine is not None else None, self._h,
                                                           a.ctypes.data, v.ctypes.data, n, res.ctypes.data))
        return [int(r) for r in res]


class Agent:
    """One node's writer: the device merge engine + its Bookie (agent.rs:480-482 single writer)."""

    def __init__(self, schema, capacity_hint=1 << 20, device=0, actor_id=b"\0" * 16, interned=()):
        self.engine = MergeEngine(schema, capacity_hint=capacity_hint, device=device, interned=interned)
        self.bookie = Bookie()
        self.actor_id = actor_id
        self.site_ids = {}      # ordinal -> 16-byte site id (crsql_site_id)
        self.last_match = None  # the last match_changes result (update_subscription's default input)

    def row_keys(self, changes, find_only=False):
        """Row keys of the changes' primary keys: an INTEGER pk is its own key; an interned table's
        pk (pack_columns bytes, or an int packed as one INTEGER column) goes through corro_pk_keys, or with
        find_only through corro_pk_find (CORRO_PK_ABSENT for a key the table does not hold; nothing interned)."""
        from .wire import pack_int_pk, unpack_int_pk
        keys = np.zeros(len(changes), np.uint64)
        by_table = {}
        for j, ch in enumerate(changes):
            if ch.table in self.engine.interned:
                packed = bytes(ch.pk) if isinstance(ch.pk, (bytes, bytearray)) else pack_int_pk(ch.pk)
                by_table.setdefault(ch.table, ([], []))
                by_table[ch.table][0].append(j)
                by_table[ch.table][1].append(packed)
            elif isinstance(ch.pk, (bytes, bytearray)):
                keys[j] = unpack_int_pk(bytes(ch.pk)) & 0xFFFFFFFFFFFFFFFF
            else:
                keys[j] = ch.pk & 0xFFFFFFFFFFFFFFFF
        for table, (idx, packed) in by_table.items():
            keys[idx] = self.engine.pk_find(table, packed) if find_only else self.engine.pk_keys(table, packed)
        return keys

    def site(self, site_id):
        o = int(self.engine.register_sites(np.frombuffer(bytes(site_id), np.uint8).reshape(1, 16))[0])
        self.site_ids[o] = bytes(site_id)
        return o

    def change_queue(self, **kw):
        """handle_changes' batching loop in front of this agent (queue.ChangeQueue): apply each batch
        it returns with process_multiple_changes, then report it with job_done()."""
        from .queue import ChangeQueue
        return ChangeQueue(self.actor_id, self.bookie.contains_all, **kw)

    def handle_needs(self, needs, max_buf_size=None):
        """Answer (actor_id, SyncNeedV1) needs from this node's state (serve.handle_needs)."""
        from . import serve
        return serve.handle_needs(self, needs, max_buf_size or serve.MAX_CHANGES_BYTES_PER_MESSAGE)

    def handle_needs_frames(self, needs, max_buf_size=None, payload=0, cluster_id=0):
        """The same answers as wire frames, chunked and encoded on the device (serve.handle_needs_frames)."""
        from . import serve
        return serve.handle_needs_frames(self, needs, max_buf_size or serve.MAX_CHANGES_BYTES_PER_MESSAGE, payload,
                                         cluster_id)

    def handle_request_frames(self, buf, frame_off, max_buf_size=None, payload=0, cluster_id=0):
        """Answer a peer's SyncMessageV1::Request frames, request bytes to response bytes on the device
        (serve.handle_request_frames)."""
        from . import serve
        return serve.handle_request_frames(self, buf, frame_off, max_buf_size or serve.MAX_CHANGES_BYTES_PER_MESSAGE,
                                           payload, cluster_id)

    def handle_request_frames_buffered(self, buf, frame_off, max_buf_size=None, payload=0, cluster_id=0, timings=None):
        """The same answers with the buffered (partial) versions served from the device row pool, where
        process_frames left them, and the per-frame join on the device
        (serve.handle_request_frames_buffered)."""
        from . import serve
        return serve.handle_request_frames_buffered(self, buf, frame_off,
                                                    max_buf_size or serve.MAX_CHANGES_BYTES_PER_MESSAGE, payload,
                                                    cluster_id, timings)

    def process_multiple_changes(self, changes):
        """changes: list of ChangeV1 (or (ChangeV1, source, instant) tuples) in arrival order."""
        changes = [c[0] if isinstance(c, tuple) else c for c in changes]
        ncs = len(changes)
        rows = []
        descs = (L.Changeset * max(1, ncs))()
        actor_bufs = []
        for i, cv1 in enumerate(changes):
            cs = cv1.changeset
            d = descs[i]
            ab = C.create_string_buffer(bytes(cv1.actor_id), 16)
            actor_bufs.append(ab)
            d.actor_id = C.addressof(ab)
            d.site = self.site(cv1.actor_id)
            d.change_off = len(rows)
            if isinstance(cs, Full):
                d.kind = L.CORRO_CS_FULL
                d.version_start = d.version_end = cs.version
                d.seq_start, d.seq_end = cs.seqs
                d.last_seq = cs.last_seq
                d.ts = cs.ts or 0
                d.change_count = len(cs.changes)
                rows.extend(cs.changes)
            elif isinstance(cs, Empty):
                d.kind = L.CORRO_CS_EMPTY
                d.version_start, d.version_end = cs.versions
                d.ts = cs.ts or 0
            else:
                d.kind = L.CORRO_CS_EMPTY_SET
                d.ts = cs.ts or 0
        n = len(rows)
        arr = {k: np.zeros(max(1, n), dt) for k, dt in (
            ("pk", np.uint64), ("table_cid", np.uint32), ("col_version", np.int64), ("db_version", np.int64),
            ("cl", np.uint32), ("seq", np.uint32), ("site", np.uint32), ("val0", np.uint64),
            ("val1", np.uint64), ("val_type", np.uint8), ("val_len", np.uint8))}
        arr["pk"][:n] = self.row_keys(rows)
        voff, vsz, data = np.zeros(max(1, n), np.uint64), np.zeros(max(1, n), np.uint32), []
        dlen = 0
        for j, ch in enumerate(rows):
            try:
                tc = self.engine.lookup(ch.table, ch.cid)
            except L.CorroError:
                tc = L.CORRO_TCID_UNKNOWN
            t, v0, v1, ln = encode_value(ch.val)
            arr["table_cid"][j] = tc
            arr["col_version"][j] = ch.col_version
            arr["db_version"][j] = ch.db_version
            arr["cl"][j] = ch.cl
            arr["seq"][j] = ch.seq
            arr["site"][j] = self.site(ch.site_id)
            arr["val0"][j], arr["val1"][j], arr["val_type"][j], arr["val_len"][j] = v0, v1, t, ln
            if ln == L.CORRO_VAL_LONG:
                b = value_bytes(ch.val)
                voff[j], vsz[j] = dlen, len(b)
                data.append(b)
                dlen += len(b)
        s = L.Changes()
        s.n = n
        for k, a in arr.items():
            setattr(s, k, a.ctypes.data)
        s.ts = None
        if data:
            blob = np.frombuffer(b"".join(data), np.uint8)
            s.val_off, s.val_size, s.val_data, s.val_data_len = voff.ctypes.data, vsz.ctypes.data, blob.ctypes.data, dlen
        known = np.zeros(max(1, ncs), np.int32)
        imp = np.zeros(max(1, n), np.uint8)
        out = L.ProcessOut()
        out.known = known.ctypes.data
        out.impactful = imp.ctypes.data
        L.check(L.lib().corro_process_multiple_changes(self.engine._h, self.bookie._h, descs, ncs, C.byref(s),
                                                       L.CORRO_MEM_HOST, C.byref(out)))
        res = Processed(known=[L.KNOWN.get(int(k), int(k)) for k in known[:ncs]])
        for i, cv1 in enumerate(changes):
            cs = cv1.changeset
            if isinstance(cs, Full):
                off = descs[i].change_off
                res.impactful.append([c for k, c in enumerate(cs.changes) if imp[off + k]])
            else:
                res.impactful.append([])
        res.ready = self.take_ready()
        return res

    def process_frames(self, buf, payload=0):
        """Wire bytes -> merge without leaving the GPU: decode length-delimited changeset frames
        on the device (corro_decode_frames, CORRO_MEM_DEVICE, with the kept frames' headers built on
        the device too) and hand the decoded batch and headers to process_multiple_changes where
        they lie (CORRO_MEM_DEVICE_HEADERS: no change or header crosses PCIe again; the known
        outcomes come back once). Frames with a non-zero decode status are not applied. Returns
        (Processed over the applied frames, with .impact = per-change impactful flags as a CUDA
        uint8 tensor and .dec = the decode they index (what match_changes takes), per-frame decode
        status)."""
        import torch
        dec = self.engine.decode_frames(buf, payload, device=True, device_headers=True)
        nk = dec["n_dev"]
        self.site_ids = dict(enumerate(self.engine.site_ids()))   # the decoder may have registered sites
        ch = dec["changes"]
        n = int(ch["pk"].shape[0])
        s = L.Changes()
        s.n = n
        for k, a in ch.items():
            if k == "val_data":
                s.val_data, s.val_data_len = a.data_ptr(), int(a.numel())
            else:
                setattr(s, k, a.data_ptr() if n else None)
        known = torch.zeros(max(1, nk), dtype=torch.int32, device="cuda")
        imp = torch.zeros(max(1, n), dtype=torch.uint8, device="cuda")
        out = L.ProcessOut()
        out.known = known.data_ptr()
        out.impactful = imp.data_ptr()
        torch.cuda.current_stream().synchronize()
        L.check(L.lib().corro_process_multiple_changes(self.engine._h, self.bookie._h, C.c_void_p(dec["cs_dev"].data_ptr()),
                                                       nk, C.byref(s), L.CORRO_MEM_DEVICE_HEADERS, C.byref(out)))
        res = Processed(known=[L.KNOWN.get(int(k), int(k)) for k in known[:nk].cpu().tolist()])
        res.impact = imp[:n]
        res.dec = dec
        res.ready = self.take_ready()
        return res, dec["status"]

    def match_changes(self, processed, dec, filters):
        """match_changes for the subscription and update filters (updates.MatchFilters) behind
        process_frames, on the device: `processed` is its Processed (with .impact), `dec` the decode it ran
        on (processed.dec). The batch columns, the kept
        frames' headers and the impact flags are read where they lie (util.rs:1026-1030). Returns
        updates.match_changes' result; cand_cs indexes the kept frames (dec["cs_dev"])."""
        from . import updates
        self.last_match = updates.match_changes(self.engine, dec["changes"], processed.impact, dec["cs_dev"], filters,
                                                device=True, ncs=dec["n_dev"])
        return self.last_match

    def update_subscription(self, sub, cls, result=None):
        """The stage behind match_changes: advance the subscription `sub` (updates.Subscription) by filter
        class `cls`'s candidates of the last match_changes result (or `result`), on the device. Returns the
        subscription's events (Subscription.update) as CUDA tensors."""
        if result is None:
            result = self.last_match
            if result is None:
                raise ValueError("update_subscription needs a match result: call match_changes first or pass result=")
        return sub.handle_candidates(result, cls)

    def read_matched(self, processed, dec, filters, values=True):
        """match_changes, then the candidates' current rows (updates.read_candidates) where they lie: returns
        (match result, read_rows result), candidate j of the first owning rows [row_off[j], row_off[j + 1])
        of the second."""
        from . import updates
        res = self.match_changes(processed, dec, filters)
        return res, updates.read_candidates(self.engine, res, values=values)

    def local_write(self, statements, ts=0, device=False):
        """One local transaction (corro_local_write): statements = ("insert" | "update" | "upsert" | "delete",
        table, pk, {column: value}) tuples in execution order, names and pks resolved like row_keys. The
        changes are computed and merged on the device and the version is booked for self.actor_id. Returns
        (db_version, last_seq, changes): the version's surviving Change list in seq order, (0, 0, []) when
        the transaction wrote no clock. The raw result (what broadcast_frames takes) is kept in
        self.last_local; device=True passes the statements as CUDA tensors and keeps that result on the GPU.
        Interned tables: the pks of inserts and upserts are interned before the call (a new row needs its
        key), so a transaction that then fails has still grown the intern table by those keys, as a rolled
        back transaction leaves no trace in cr-sqlite's __crsql_pks but here leaves unused ids; the pks of
        updates and deletes are only looked up (an unknown one names an absent row) and never intern."""
        kinds = {"insert": L.CORRO_OP_INSERT, "update": L.CORRO_OP_UPDATE, "upsert": L.CORRO_OP_UPSERT,
                 "delete": L.CORRO_OP_DELETE}
        n = len(statements)
        site = self.site(self.actor_id)
        tix = {name: i for i, (name, _c) in enumerate(self.engine.schema)}
        ops = {"kind": np.zeros(n, np.uint8), "table": np.zeros(n, np.uint32), "cell_off": np.zeros(n + 1, np.uint64)}
        keyed = [Change(st[1], st[2], "-1", None, 0, 0, 0, self.actor_id, 0) for st in statements]
        cid, v0, v1, vt, vl, voff, vsz, data, dlen = [], [], [], [], [], [], [], [], 0
        for i, st in enumerate(statements):
            kind, table, _pk = st[0], st[1], st[2]
            cells = st[3] if len(st) > 3 and st[3] else {}
            ops["kind"][i] = kinds[kind]
            ops["table"][i] = tix[table]
            for col, val in cells.items():
                cid.append(self.engine.lookup(table, col) & 0xFFFF)
                t, a, b, ln = encode_value(val)
                v0.append(a), v1.append(b), vt.append(t), vl.append(ln)
                raw = value_bytes(val) if ln == L.CORRO_VAL_LONG else b""
                voff.append(dlen), vsz.append(len(raw))
                data.append(raw)
                dlen += len(raw)
            ops["cell_off"][i + 1] = len(cid)
        creates = [i for i, st in enumerate(statements) if st[0] in ("insert", "upsert")]
        others = [i for i, st in enumerate(statements) if st[0] not in ("insert", "upsert")]
        ops["pk"] = np.zeros(n, np.uint64)
        ops["pk"][creates] = self.row_keys([keyed[i] for i in creates])
        ops["pk"][others] = self.row_keys([keyed[i] for i in others], find_only=True)
        ops.update(cid=np.array(cid, np.uint32), val0=np.array(v0, np.uint64), val1=np.array(v1, np.uint64),
                   val_type=np.array(vt, np.uint8), val_len=np.array(vl, np.uint8))
        if dlen:
            ops.update(val_off=np.array(voff, np.uint64), val_size=np.array(vsz, np.uint32),
                       val_data=np.frombuffer(b"".join(data), np.uint8))
        self.last_local_ops = {k: ops[k] for k in ("kind", "table", "cell_off")}    # (host copies: local_bound's input)
        if device:
            import torch
            sgn = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}
            ops = {k: torch.from_numpy(a.view(sgn.get(a.dtype, a.dtype)).copy()).cuda() for k, a in ops.items()}
        res = self.engine.local_write(ops, ts, site, bookie=self.bookie, actor_id=self.actor_id)
        self.last_local = dict(res, ts_call=int(ts), site_ord=site)
        host = {k: (a.cpu().numpy() if device else a) for k, a in res.items() if hasattr(a, "shape")}
        return res["version"], res["last_seq"], self._changes_of(host)

    def _changes_of(self, rows):
        """crsql_changes columns (host arrays, with val_off / val_size / val_data) -> Change list."""
        out = []
        raw = rows["val_data"].tobytes() if "val_data" in rows else b""
        for k in range(len(rows["pk"])):
            tc = int(rows["table_cid"][k])
            table, cols = self.engine.schema[tc >> 16]
            c = tc & 0xFFFF
            ty, ln = int(rows["val_type"][k]), int(rows["val_len"][k])
            m64 = 0xFFFFFFFFFFFFFFFF                 # (a device result's columns come back as signed tensors)
            w0, w1 = int(rows["val0"][k]) & m64, int(rows["val1"][k]) & m64
            if ty == L_NULL:
                val = None
            elif ty == 1:
                val = w0 - (1 << 64) if w0 >> 63 else w0
            elif ty == 2:
                val = struct.unpack("<d", struct.pack("<Q", w0))[0]
            else:
                if ln == L.CORRO_VAL_LONG:
                    o = int(rows["val_off"][k])
                    b = raw[o:o + int(rows["val_size"][k])]
                else:
                    b = (w0.to_bytes(8, "big") + w1.to_bytes(8, "big"))[:ln]
                val = b.decode() if ty == 3 else b
            pk = int(rows["pk"][k]) & m64
            if table in self.engine.interned:
                pk = self.engine.pk_bytes(table, np.array([pk], np.uint64))[0]
            out.append(Change(table, pk, "-1" if c == 0 else cols[c - 1], val, int(rows["col_version"][k]),
                              int(rows["db_version"][k]), int(rows["seq"][k]), self.site_ids[int(rows["site"][k])],
                              int(rows["cl"][k])))
        return out

    def broadcast_frames(self, result=None, max_buf_size=None, cluster_id=0):
        """The broadcast of one local write (broadcast_changes, broadcast.rs:511-579): its rows as one span
        0..=last_seq through corro_encode_changesets with CORRO_PAYLOAD_UNI, where they lie. result: a raw
        engine.local_write result (None: the last local_write's). Returns encode_changesets' result ("buf"
        holds the frames), or None for a transaction that wrote nothing."""
        from . import serve
        res = self.last_local if result is None else result
        if not res["version"]:
            return None
        mem = Mem.of(res["pk"])
        one = lambda v, dt: (mem._torch.tensor([v], dtype=mem._tdt[dt], device=mem.dev) if mem.on_dev
                             else np.array([v], dt))
        spans = {"site": one(res["site_ord"], np.uint32), "version": one(res["version"], np.int64),
                 "last_seq": one(res["last_seq"], np.uint64), "ts": one(res["ts_call"], np.uint64),
                 "seq_start": one(0, np.uint64), "seq_end": one(res["last_seq"], np.uint64),
                 "row_off": one(0, np.uint64), "row_count": one(res["nrows"], np.uint64)}
        return self.engine.encode_changesets(spans, res, max_buf_size or serve.MAX_CHANGES_BYTES_PER_MESSAGE,
                                             L.CORRO_PAYLOAD_UNI, cluster_id)

    def take_ready(self):
        return self.bookie.take_ready()

    def save_bookie(self, device=False):
        """The bookie's image (Bookie.save): what a restart needs besides the exported state."""
        return self.bookie.save(self.engine, device=device)

    def load_bookie(self, image):
        """Load a saved image into this agent's empty bookie (Bookie.load). The image's site ordinals must
        be registered here to the same ids (register the sites and re-seed the state first); the fully
        buffered versions found are listed by take_ready."""
        self.bookie.load(image, self.engine)
        self.site_ids = dict(enumerate(self.engine.site_ids()))

    def process_fully_buffered_changes(self, actor, version):
        r = C.c_int()
        L.check(L.lib().corro_process_fully_buffered(self.engine._h, self.bookie._h, actor, version, C.byref(r)))
        return bool(r.value)

    def process_ready(self, pairs=None):
        """Every ready version applied in one batch (Bookie.process_ready): `pairs` in list order, or what
        take_ready() lists. Returns [(actor, version, result)]: result 0 not applied, 1 applied with no
        row impacted, 2 applied with rows impacted (the versions to match, updates.match_extracted),
        negative = refused by its own gap bookkeeping."""
        pairs = self.take_ready() if pairs is None else list(pairs)
        res = self.bookie.process_ready(self.engine, pairs)
        return [(bytes(a), int(v), r) for (a, v), r in zip(pairs, res)]

    def sync_book(self):
        """The bookie as one sync book (Bookie.sync_book): what generate_sync reads, one row per actor in
        generate_sync's order. sync.state_frames_from_books takes it."""
        return self.bookie.sync_book()

    def generate_sync_frame(self, last_cleared_ts=None, device=False):
        """This node's SyncMessageV1::State as one length-delimited frame, generated and encoded on the
        device from the sync book (corro_encode_states): the bytes wire.frame(wire.encode_sync_state(
        self.generate_sync())) gives. Returns bytes, or with device=True the CUDA uint8 tensor."""
        from .sync import state_frames_from_books
        res = state_frames_from_books(self.engine, [self.sync_book()], [self.actor_id], ts=[last_cleared_ts], device=device)
        st = int(res["state_status"][0])
        if st != 0:
            raise L.CorroError(st, "the bookie's sync book does not encode (not canonical, or larger than a frame)")
        return res["buf"] if device else res["buf"].tobytes()

    def generate_sync(self):
        lib = L.lib()
        st = L.SyncState()
        L.check(lib.corro_generate_sync(self.bookie._h, self.actor_id, C.byref(st), 0))
        na, nn, npr, ns = st.n_actors, st.n_need, st.n_partials, st.n_pseqs
        bufs = {"actor_ids": np.zeros(max(1, 16 * na), np.uint8), "heads": np.zeros(max(1, na), np.uint64),
                "need_off": np.zeros(na + 1, np.uint64), "need_start": np.zeros(max(1, nn), np.uint64),
                "need_end": np.zeros(max(1, nn), np.uint64), "partial_off": np.zeros(na + 1, np.uint64),
                "partial_ver": np.zeros(max(1, npr), np.uint64), "pseq_off": np.zeros(npr + 1, np.uint64),
                "pseq_start": np.zeros(max(1, ns), np.uint64), "pseq_end": np.zeros(max(1, ns), np.uint64)}
        for k, a in bufs.items():
            setattr(st, k, a.ctypes.data)
        L.check(lib.corro_generate_sync(self.bookie._h, self.actor_id, C.byref(st), 1))
        state = SyncStateV1(actor_id=self.actor_id)
        for i in range(na):
            a = bytes(bufs["actor_ids"][16 * i:16 * i + 16])
            state.heads[a] = int(bufs["heads"][i])
            need = [(int(bufs["need_start"][k]), int(bufs["need_end"][k]))
                    for k in range(int(bufs["need_off"][i]), int(bufs["need_off"][i + 1]))]
            if need:
                state.need[a] = need
            for p in range(int(bufs["partial_off"][i]), int(bufs["partial_off"][i + 1])):
                seqs = [(int(bufs["pseq_start"][k]), int(bufs["pseq_end"][k]))
                        for k in range(int(bufs["pseq_off"][p]), int(bufs["pseq_off"][p + 1]))]
                state.partial_need.setdefault(a, {})[int(bufs["partial_ver"][p])] = seqs
        return state
