"""Server side of sync: answering a peer's SyncNeedV1 with changesets from the device state.

Mirrors corro-agent/src/api/peer/mod.rs `handle_need` (:371-727) and `send_change_chunks`
(:729-789), and corro-types/src/change.rs `Change::estimated_byte_size` (:34-49) and
`ChunkedChanges` (:66-178). The row lookups — the GROUP BY db_version query (:385-394) and the
per-version / per-seq-range row queries (:423-431, :603-611) — run on the GPU through
corro_extract_changes (csrc/extract.hip), batched over every need of the call. Buffered (partial)
versions and the gap bookkeeping come from the host Bookie (csrc/agent.cpp), as they come from
__corro_buffered_changes / __corro_seq_bookkeeping / __corro_bookkeeping_gaps in the reference.
"""
import ctypes as C
import struct

import numpy as np

from . import _lib as L
from ._twopass import Mem, TwoPass
from .agent import Change, ChangeV1, Empty, Full
from .engine import SPAN_KEYS
from .sync import Full as NeedFull, Partial as NeedPartial

MAX_CHANGES_BYTES_PER_MESSAGE = 8 * 1024   # peer/mod.rs:365
SEQ_ALL = (0, 0xFFFFFFFF)


# ---- change.rs / pubsub.rs size arithmetic --------------------------------------------------

def num_bytes_needed_i32(val):
    """pubsub.rs num_bytes_needed_i32 — including its `val * 0xFF != 0` test for the last byte,
    which is non-zero for every non-zero val (255 is odd, so the wrapping product is 0 only at 0)."""
    v = val & 0xFFFFFFFF
    if v & 0xFF000000:
        return 4
    if v & 0x00FF0000:
        return 3
    if v & 0x0000FF00:
        return 2
    return 1 if v != 0 else 0


def num_bytes_needed_i64(val):
    v = val & 0xFFFFFFFFFFFFFFFF
    if v & 0xFF00000000000000:
        return 8
    if v & 0x00FF000000000000:
        return 7
    if v & 0x0000FF0000000000:
        return 6
    if v & 0x000000FF00000000:
        return 5
    return num_bytes_needed_i32(v & 0xFFFFFFFF)


def packed_pk_len(pk):
    """len(pack_columns([Integer(pk)])) (pubsub.rs:2304-2358): count byte + type byte + int bytes."""
    return 2 + num_bytes_needed_i64(pk)


def value_size(val):
    """SqliteValue::estimated_byte_size (corro-api-types/src/lib.rs:524-532)."""
    if val is None:
        return 1 + 1
    if isinstance(val, (bool, int, float)):
        return 1 + 8
    b = val.encode() if isinstance(val, str) else bytes(val)
    return 1 + 4 + len(b)


def estimated_byte_size(ch):
    """Change::estimated_byte_size (change.rs:34-49)."""
    pk_len = len(ch.pk) if isinstance(ch.pk, (bytes, bytearray)) else packed_pk_len(ch.pk)
    return len(ch.table) + pk_len + len(ch.cid) + value_size(ch.val) + 8 + 8 + 8 + 16 + 8 + 8


class ChunkedChanges:
    """change.rs:66-178: yields (changes, (start_seq, end_seq)) chunks of at most ~max_buf_size
    estimated bytes; the last chunk always ends at last_seq (even when empty)."""

    def __init__(self, it, start_seq, last_seq, max_buf_size, size=estimated_byte_size):
        self._it = iter(it)
        self._peek = []
        self.last_pushed_seq = 0
        self.last_start_seq = start_seq
        self.last_seq = last_seq
        self.max_buf_size = max_buf_size
        self.done = False
        self._size = size

    def _next_item(self):
        if self._peek:
            return self._peek.pop()
        return next(self._it, None)

    def _has_next(self):
        if not self._peek:
            x = next(self._it, None)
            if x is None:
                return False
            self._peek.append(x)
        return True

    def __iter__(self):
        return self

    def __next__(self):
        if self.done:
            raise StopIteration
        changes, buffered = [], 0
        while True:
            ch = self._next_item()
            if ch is None:
                break
            self.last_pushed_seq = ch.seq
            buffered += self._size(ch)
            changes.append(ch)
            if self.last_pushed_seq == self.last_seq:
                break
            if buffered >= self.max_buf_size:
                start = self.last_start_seq
                if not self._has_next():
                    break
                self.last_start_seq = self.last_pushed_seq + 1
                return changes, (start, self.last_pushed_seq)
        self.done = True
        return changes, (self.last_start_seq, self.last_seq)


def send_change_chunks(out, chunked, actor_id, version, last_seq, ts):
    """peer/mod.rs:729-789 without the channel: append Changeset::Full messages to `out`
    (an empty first-and-only chunk covering 0..=last_seq is dropped, :746-748)."""
    for changes, seqs in chunked:
        if not changes and seqs[0] == 0 and seqs[1] == last_seq:
            return
        out.append(ChangeV1(actor_id, Full(version=version, changes=changes, seqs=seqs, last_seq=last_seq, ts=ts)))


# ---- rows -> Change objects -------------------------------------------------------------------

def _decode_value(vt, v0, v1, ln, long_bytes=None):
    vt = int(vt)
    if vt in (3, 4) and int(ln) == L.CORRO_VAL_LONG:  # a long value: its bytes from the arena / bookie
        b = long_bytes()
        return b.decode() if vt == 3 else b
    if vt == 1:
        return struct.unpack("<q", struct.pack("<Q", int(v0)))[0]
    if vt == 2:
        return struct.unpack("<d", struct.pack("<Q", int(v0)))[0]
    if vt in (3, 4):
        b = (int(v0).to_bytes(8, "big") + int(v1).to_bytes(8, "big"))[: int(ln)]
        return b.decode() if vt == 3 else b
    return None


def rows_to_changes(engine, site_ids, rows, lo, hi, long_bytes=None):
    """crsql_changes rows [lo, hi) -> Change objects (table / cid names from the engine schema).
    long_bytes(k): the bytes of row k's long value (default: its val1 handle in the engine's arena)."""
    out = []
    if long_bytes is None:
        def long_bytes(k):
            return engine.value_bytes([int(rows["val1"][k])])[0]
    for k in range(lo, hi):
        tc = int(rows["table_cid"][k])
        t, cid = tc >> 16, tc & 0xFFFF
        name, cols = engine.schema[t]
        pk = int(rows["pk"][k])
        if name in engine.interned:  # the canonical packed pk of the row (cr-sqlite's t__crsql_pks)
            pk = engine.pk_bytes(t, [pk])[0]
        out.append(Change(table=name, pk=pk, cid="-1" if cid == 0 else cols[cid - 1],
                          val=_decode_value(rows["val_type"][k], rows["val0"][k], rows["val1"][k], rows["val_len"][k],
                                            lambda: long_bytes(k)),
                          col_version=int(rows["col_version"][k]), db_version=int(rows["db_version"][k]),
                          seq=int(rows["seq"][k]), site_id=site_ids[int(rows["site"][k])], cl=int(rows["cl"][k])))
    return out


# ---- bookie probes ------------------------------------------------------------------------------

def _buffered_versions(bookie, actor, s, e):
    c = C.c_uint64()
    L.check(L.lib().corro_bookie_buffered_versions(bookie._h, actor, s, e, None, 0, C.byref(c)))
    if not c.value:
        return []
    v = np.zeros(c.value, np.uint64)
    L.check(L.lib().corro_bookie_buffered_versions(bookie._h, actor, s, e, v.ctypes.data, c.value, C.byref(c)))
    return [int(x) for x in v]


def _seq_bookkeeping(bookie, actor, version):
    c, last, ts = C.c_uint64(), C.c_int64(), C.c_uint64()
    L.check(L.lib().corro_bookie_seq_bookkeeping(bookie._h, actor, version, None, None, 0, C.byref(c),
                                                 C.byref(last), C.byref(ts)))
    if last.value < 0 or not c.value:
        return []
    s = np.zeros(c.value, np.uint64)
    e = np.zeros(c.value, np.uint64)
    L.check(L.lib().corro_bookie_seq_bookkeeping(bookie._h, actor, version, s.ctypes.data, e.ctypes.data, c.value,
                                                 C.byref(c), C.byref(last), C.byref(ts)))
    return [((int(s[i]), int(e[i])), int(last.value), int(ts.value)) for i in range(c.value)]


def _buffered_rows(bookie, actor, version, s, e):
    c = C.c_uint64()
    L.check(L.lib().corro_bookie_buffered(bookie._h, actor, version, s, e, None, 0, C.byref(c)))
    from .engine import ROW_FIELDS
    rows = {k: np.zeros(max(1, c.value), dt) for k, dt in ROW_FIELDS.items()}
    r = L.Rows()
    for k, a in rows.items():
        setattr(r, k, a.ctypes.data)
    L.check(L.lib().corro_bookie_buffered(bookie._h, actor, version, s, e, C.byref(r), c.value, C.byref(c)))
    return rows, c.value


def _buffered_long(bookie, actor, version, rows):
    """long_bytes for rows_to_changes over buffered rows: the bookie keeps their bytes."""
    def get(k):
        n = C.c_uint64()
        seq = int(rows["seq"][k])
        L.check(L.lib().corro_bookie_buffered_value(bookie._h, actor, version, seq, None, 0, C.byref(n)))
        buf = C.create_string_buffer(max(1, n.value))
        L.check(L.lib().corro_bookie_buffered_value(bookie._h, actor, version, seq, buf, n.value, C.byref(n)))
        return buf.raw[:n.value]
    return get


def _in_ranges(ranges, v):
    return any(s <= v <= e for s, e in ranges)


def _subtract(ranges, holes):
    """[(s, e)] - [(s, e)] over integers, ascending, coalesced (RangeInclusiveSet::remove)."""
    out = []
    for s, e in ranges:
        cur = [(s, e)]
        for hs, he in holes:
            nxt = []
            for a, b in cur:
                if he < a or hs > b:
                    nxt.append((a, b))
                    continue
                if a < hs:
                    nxt.append((a, hs - 1))
                if he < b:
                    nxt.append((he + 1, b))
            cur = nxt
        out.extend(cur)
    out.sort()
    merged = []
    for a, b in out:
        if merged and a <= merged[-1][1] + 1:
            merged[-1] = (merged[-1][0], max(merged[-1][1], b))
        else:
            merged.append((a, b))
    return merged


# ---- handle_need ----------------------------------------------------------------------------

def handle_needs(agent, needs, max_buf_size=MAX_CHANGES_BYTES_PER_MESSAGE):
    """handle_need (peer/mod.rs:371-727) for a list of (actor_id, SyncNeedV1) at once.

    Change.site_id comes from the engine's site table (ordinal -> 16 bytes). Returns, per need,
    the list of ChangeV1 messages in the order the reference sends them. The crsql_changes
    queries of every need run as ONE batched device extraction."""
    eng = agent.engine
    site_ids = dict(enumerate(eng.site_ids()))
    # one extraction entry per crsql_changes query
    ent_site, ent_s, ent_e, ent_ss, ent_se, owner = [], [], [], [], [], []
    plan = []
    for i, (actor, need) in enumerate(needs):
        site = agent.site(actor)
        if isinstance(need, NeedFull):
            plan.append(("full", len(ent_site)))
            ent_site.append(site); ent_s.append(need.start); ent_e.append(need.end)
            ent_ss.append(SEQ_ALL[0]); ent_se.append(SEQ_ALL[1]); owner.append(i)
        elif isinstance(need, NeedPartial):
            first = len(ent_site)
            for s, e in [SEQ_ALL] + [tuple(r) for r in need.seqs]:
                ent_site.append(site); ent_s.append(need.version); ent_e.append(need.version)
                ent_ss.append(max(0, min(s, 0xFFFFFFFF))); ent_se.append(max(0, min(e, 0xFFFFFFFF))); owner.append(i)
            plan.append(("partial", first))
        else:
            plan.append(("none", -1))
    res = None
    if ent_site:
        res = eng.extract_changes({"site": np.array(ent_site, np.uint32), "start": np.array(ent_s, np.uint64),
                                   "end": np.array(ent_e, np.uint64), "seq_start": np.array(ent_ss, np.uint32),
                                   "seq_end": np.array(ent_se, np.uint32)})

    def groups(k):
        g0, g1 = int(res["grp_off"][k]), int(res["grp_off"][k + 1])
        return [(int(res["version"][g]), int(res["last_seq"][g]), int(res["ts"][g]), int(res["grp_row_off"][g]),
                 int(res["grp_rows"][g])) for g in range(g0, g1)]

    out_all = []
    for (actor, need), (kind, k) in zip(needs, plan):
        out, empties = [], []
        if kind == "full":
            found = set()
            for version, last_seq, ts, ro, rn in groups(k):    # db_version DESC (:385-394)
                found.add(version)
                chunks = ChunkedChanges(rows_to_changes(eng, site_ids, res["rows"], ro, ro + rn), 0, last_seq,
                                        max_buf_size)
                send_change_chunks(out, chunks, actor, version, last_seq, ts)
            unprocessed = _subtract([(need.start, need.end)], [(v, v) for v in sorted(found)])
            gaps = agent.bookie.needed(actor)
            for s, e in unprocessed:                           # :458-542
                buffered = _buffered_versions(agent.bookie, actor, s, e)
                for v in buffered:
                    for (rs, re_), last_seq, ts in _seq_bookkeeping(agent.bookie, actor, v):
                        rows, m = _buffered_rows(agent.bookie, actor, v, rs, re_)
                        chg = rows_to_changes(eng, site_ids, rows, 0, m, _buffered_long(agent.bookie, actor, v, rows))
                        send_change_chunks(out, ChunkedChanges(chg, rs, re_, max_buf_size), actor, v, last_seq, ts)
                empties += _subtract([(s, e)], gaps + [(v, v) for v in buffered])
        elif kind == "partial":
            g = groups(k)
            if g:                                              # :554-597
                version, last_seq, ts, _, _ = g[0]
                for j, (s, e) in enumerate(need.seqs):
                    _, _, _, ro, rn = groups(k + 1 + j)[0]
                    chunks = ChunkedChanges(rows_to_changes(eng, site_ids, res["rows"], ro, ro + rn), s, e, max_buf_size)
                    send_change_chunks(out, chunks, actor, version, last_seq, ts)
            else:                                              # :598-712
                v = need.version
                in_gaps = _in_ranges(agent.bookie.needed(actor), v)
                buffered = bool(_buffered_versions(agent.bookie, actor, v, v))
                if not buffered and not in_gaps:
                    empties.append((v, v))
                if buffered:
                    for qs, qe in need.seqs:
                        for (rs, re_), last_seq, ts in _seq_bookkeeping(agent.bookie, actor, v):
                            hit = (qs <= rs <= qe) or (rs <= qs and re_ >= qe) or (rs <= qe and re_ >= qe) or \
                                  (qs <= re_ <= qe)
                            if not hit:
                                continue
                            s, e = max(rs, qs), min(re_, qe)
                            rows, m = _buffered_rows(agent.bookie, actor, v, s, e)
                            chg = rows_to_changes(eng, site_ids, rows, 0, m,
                                                  _buffered_long(agent.bookie, actor, v, rows))
                            send_change_chunks(out, ChunkedChanges(chg, s, e, max_buf_size), actor, v, last_seq, ts)
        for s, e in _subtract(empties, []):                    # :715-724
            out.append(ChangeV1(actor, Empty(versions=(s, e), ts=None)))
        out_all.append(out)
    return out_all


def handle_need(agent, actor_id, need, max_buf_size=MAX_CHANGES_BYTES_PER_MESSAGE):
    return handle_needs(agent, [(actor_id, need)], max_buf_size)[0]


# ---- handle_need, rows to frames on the device --------------------------------------------------

def _bookie_messages(agent, actor, need, found, in_state, site_ids, max_buf_size):
    """What the host bookie adds to one need's answer after the state's versions (the same walk as in
    handle_needs): buffered versions' chunks, then the Empty ranges. found: the versions a Full need
    got from the state; in_state: a Partial need's version is in the state."""
    eng = agent.engine
    out, empties = [], []
    if isinstance(need, NeedFull):
        unprocessed = _subtract([(need.start, need.end)], [(v, v) for v in sorted(found)])
        gaps = agent.bookie.needed(actor)
        for s, e in unprocessed:                               # :458-542
            buffered = _buffered_versions(agent.bookie, actor, s, e)
            for v in buffered:
                for (rs, re_), last_seq, ts in _seq_bookkeeping(agent.bookie, actor, v):
                    rows, m = _buffered_rows(agent.bookie, actor, v, rs, re_)
                    chg = rows_to_changes(eng, site_ids, rows, 0, m, _buffered_long(agent.bookie, actor, v, rows))
                    send_change_chunks(out, ChunkedChanges(chg, rs, re_, max_buf_size), actor, v, last_seq, ts)
            empties += _subtract([(s, e)], gaps + [(v, v) for v in buffered])
    elif isinstance(need, NeedPartial) and not in_state:       # :598-712
        v = need.version
        in_gaps = _in_ranges(agent.bookie.needed(actor), v)
        buffered = bool(_buffered_versions(agent.bookie, actor, v, v))
        if not buffered and not in_gaps:
            empties.append((v, v))
        if buffered:
            for qs, qe in need.seqs:
                for (rs, re_), last_seq, ts in _seq_bookkeeping(agent.bookie, actor, v):
                    hit = (qs <= rs <= qe) or (rs <= qs and re_ >= qe) or (rs <= qe and re_ >= qe) or (qs <= re_ <= qe)
                    if not hit:
                        continue
                    s, e = max(rs, qs), min(re_, qe)
                    rows, m = _buffered_rows(agent.bookie, actor, v, s, e)
                    chg = rows_to_changes(eng, site_ids, rows, 0, m, _buffered_long(agent.bookie, actor, v, rows))
                    send_change_chunks(out, ChunkedChanges(chg, s, e, max_buf_size), actor, v, last_seq, ts)
    for s, e in _subtract(empties, []):                        # :715-724
        out.append(ChangeV1(actor, Empty(versions=(s, e), ts=None)))
    return out


def device_book(agent, dev):
    """The bookie as corro_decode_requests screens against it: per registered site ordinal, known (the
    bookie holds a version of the actor), max (BookedVersions::last, -1 = None) and the needed() gaps
    as a CSR, CUDA tensors on dev."""
    import torch
    ids = agent.engine.site_ids()
    known, mx, gap_off, gs, ge = [], [], [0], [], []
    for a in ids:
        last = agent.bookie.last(a)
        gaps = agent.bookie.needed(a)
        known.append(1 if last is not None or gaps else 0)
        mx.append(-1 if last is None else last)
        gs += [s for s, _ in gaps]
        ge += [e for _, e in gaps]
        gap_off.append(len(gs))

    def up(a, dt):
        a = np.asarray(a, dt)
        return torch.from_numpy(a.view(np.int64) if a.itemsize == 8 else a).to(dev)
    return {"known": up(known, np.uint8), "max": up(mx, np.int64), "gap_off": up(gap_off, np.uint64),
            "gap_start": up(gs, np.uint64), "gap_end": up(ge, np.uint64)}


def device_buffered(agent, dev):
    """The bookie's buffered (partial) versions as corro_need_tails reads them: per registered site
    ordinal, the versions that hold buffered rows, ascending, as a CSR ("buf_off", "buf_version"), CUDA
    tensors on dev."""
    import torch
    buf_off, bv = [0], []
    for a in agent.engine.site_ids():
        bv += _buffered_versions(agent.bookie, a, 0, 0xFFFFFFFFFFFFFFFF)
        buf_off.append(len(bv))

    def up(a):
        return torch.from_numpy(np.asarray(a, np.uint64).view(np.int64)).to(dev)
    return {"buf_off": up(buf_off), "buf_version": up(bv)}


_BUFIDX_FIELDS = (("ver_off", np.uint64, "nsites", 1, 1), ("version", np.uint64, "nver"), ("last_seq", np.int64, "nver"),
                  ("ts", np.uint64, "nver"), ("on_device", np.uint8, "nver"), ("sr_off", np.uint64, "nver", 1, 1),
                  ("sr_start", np.uint64, "nsr"), ("sr_end", np.uint64, "nsr"), ("seg_off", np.uint64, "nver", 1, 1),
                  ("seg_pool_off", np.uint64, "nseg"), ("seg_seq0", np.uint32, "nseg"), ("seg_n", np.uint32, "nseg"),
                  ("tail_gap_off", np.uint64, "nsites", 1, 1), ("tail_gap_start", np.uint64, "ntail_gap"),
                  ("tail_gap_end", np.uint64, "ntail_gap"), ("host_buf_off", np.uint64, "nsites", 1, 1),
                  ("host_buf_version", np.uint64, "nhost_buf"))


def buffered_index(agent):
    """corro_bookie_buffered_index over the engine's registered sites, as numpy arrays: one call in
    place of device_buffered's probe per site. Nothing is materialised: pool keys stay in the pool.
    Per site ordinal a CSR ("ver_off") over its buffered versions ("version", ascending) with
    "last_seq" (-1 = no seq bookkeeping), "ts", their seq ranges ("sr_off", "sr_start", "sr_end"),
    "on_device" and the on_device versions' pool segments ("seg_off", "seg_pool_off", "seg_seq0",
    "seg_n"); and the books need_tails takes with it: "tail_gap_off" / "_start" / "_end" (needed()
    united with the on_device versions) and "host_buf_off" / "host_buf_version" (the others). The pool
    offsets hold until the bookie's next process_multiple_changes / process_fully_buffered_changes."""
    ids = agent.engine.site_ids()
    S = len(ids)
    raw = np.frombuffer(b"".join(ids), np.uint8).copy() if S else np.zeros(1, np.uint8)
    tp = TwoPass(L.lib().corro_bookie_buffered_index, (agent.bookie._h, raw.ctypes.data, S), Mem(), L.BufferedIndex())
    tp.run(0)
    tp.run(1, _BUFIDX_FIELDS, {**tp.totals(("nver", "nsr", "nseg", "ntail_gap", "nhost_buf")), "nsites": S})
    return tp.result()


def device_buffered_index(agent, dev):
    """buffered_index for the device path: {"host": the numpy arrays, "dev": the version / seq range /
    segment arrays as CUDA tensors on dev (what MergeEngine.buffered_spans reads), "book": the derived
    books in need_tails' names ("gap_off", "gap_start", "gap_end", "buf_off", "buf_version"), CUDA
    tensors}. All of it goes up in one copy."""
    import torch
    h = buffered_index(agent)
    names = [f[0] for f in _BUFIDX_FIELDS]
    off, total = {}, 0
    for k in names:                                            # one staging buffer, 8-byte aligned slices
        off[k] = total
        total += (h[k].nbytes + 7) // 8 * 8
    stage = np.zeros(max(total, 8), np.uint8)
    for k in names:
        stage[off[k]:off[k] + h[k].nbytes] = h[k].view(np.uint8)
    d = torch.from_numpy(stage).to(dev)
    tdt = {1: torch.uint8, 4: torch.int32, 8: torch.int64}
    t = {k: d[off[k]:off[k] + h[k].nbytes].view(tdt[h[k].itemsize]) for k in names}
    book = {"gap_off": t["tail_gap_off"], "gap_start": t["tail_gap_start"], "gap_end": t["tail_gap_end"],
            "buf_off": t["host_buf_off"], "buf_version": t["host_buf_version"]}
    return {"host": h, "dev": {k: t[k] for k in names[:12]}, "book": book}


# ---- serving request frames: one pipeline, three ways to finish it ------------------------------

# decode_requests' arrays the host walk of a need reads
_NEED_KEYS = ("frame_pair_off", "pair_need_off", "pair_actor", "kind", "start", "end", "sr_off", "sr_n", "s_start",
              "s_end", "need_keep", "need_ent_off")


def _frame_messages(msgs, payload, cluster_id):
    """ChangeV1 messages as the length-delimited frames of a payload kind, back to back."""
    from . import wire
    if payload == wire.PAYLOAD_SYNC:
        return wire.frames(msgs, wire.PAYLOAD_SYNC)
    return b"".join(wire.frame(wire.encode_uni_change(cv, cluster_id)) for cv in msgs)


def _to_host(*parts):
    """Read back the named arrays of each (result dict, keys), in the order given, into one dict."""
    return {k: src[k].cpu().numpy() for src, keys in parts for k in keys}


def _host_need_frames(agent, h, t, actor, site_ids, max_buf_size, payload, cluster_id):
    """What the host bookie answers to decoded need t, framed: h holds the host copies of _NEED_KEYS,
    of need_spans' "in_state" and of the extraction's "grp_off" / "version" (the versions a Full need
    found in the state)."""
    k = int(h["need_ent_off"][t])
    if h["kind"][t] == 0:
        need = NeedFull(int(h["start"][t]), int(h["end"][t]))
        found = {int(v) for v in h["version"][int(h["grp_off"][k]):int(h["grp_off"][k + 1])]}
    else:
        q0 = int(h["sr_off"][t])
        need = NeedPartial(int(h["start"][t]), tuple((int(h["s_start"][q]), int(h["s_end"][q]))
                                                     for q in range(q0, q0 + int(h["sr_n"][t]))))
        found = set()
    msgs = _bookie_messages(agent, actor, need, found, bool(h["in_state"][t]), site_ids, max_buf_size)
    return _frame_messages(msgs, payload, cluster_id)


def _request_front(agent, buf, frame_off, max_buf_size, payload, cluster_id, timings):
    """The stages every request path starts with: the book, decode + screen, and unless no need is
    left the extraction, the spans and their encoding. Returns the stage results: lap (the stage timer:
    lap(name) adds the seconds since the last lap to timings[name], with the device idle), dev, book,
    dec, status, answers (b"" per frame) and ext, sp, enc -- ext is None when nothing is left to serve."""
    import time
    from types import SimpleNamespace

    import torch
    eng = agent.engine
    dev = torch.device("cuda", eng.device)
    t0 = time.perf_counter()

    def lap(name):
        nonlocal t0
        if timings is not None:
            torch.cuda.synchronize(dev)
            t1 = time.perf_counter()
            timings[name] = timings.get(name, 0.0) + (t1 - t0)
            t0 = t1

    if not torch.is_tensor(buf):
        buf = torch.from_numpy(np.frombuffer(bytes(buf), np.uint8).copy()).to(dev)
    if not torch.is_tensor(frame_off):
        frame_off = torch.from_numpy(np.ascontiguousarray(frame_off, np.uint64).view(np.int64)).to(dev)
    book = device_book(agent, dev)
    lap("book")
    dec = eng.decode_requests(buf, frame_off, book)
    lap("decode")
    st = SimpleNamespace(lap=lap, dev=dev, book=book, dec=dec, status=dec["frame_status"].cpu().numpy(),
                         answers=[b""] * dec["nframes"], ext=None)
    if dec["nneeds"] == 0 or dec["nents"] == 0:
        return st
    st.ext = eng.extract_changes({"site": dec["ent_site"], "start": dec["ent_start"], "end": dec["ent_end"],
                                  "seq_start": dec["ent_seq_start"], "seq_end": dec["ent_seq_end"]})
    lap("extract")
    st.sp = eng.need_spans(dec, st.ext)
    lap("spans")
    st.enc = eng.encode_changesets({k: st.sp[k] for k in SPAN_KEYS}, st.ext["rows"], max_buf_size, payload, cluster_id)
    lap("encode")
    return st


def _join_assembled(agent, st, tl, asm, max_buf_size, payload, cluster_id):
    """The answers from assemble_answers' buffer: one copy into a pinned staging tensor and one slice per
    frame. Only when a frame holds a host need (frame_host) are the need arrays read back: that frame's
    needs are walked, sliced by need_ans_off, and the host bookie's frames go in after each host need's
    encoded piece."""
    import torch
    eng = agent.engine
    fao, fhost = asm["frame_ans_off"].cpu().numpy(), asm["frame_host"].cpu().numpy()
    pinned = getattr(eng, "_answer_staging", None)             # pinned, kept with the engine and grown
    if pinned is None or pinned.numel() < asm["nbytes"]:
        pinned = eng._answer_staging = torch.empty(max(asm["nbytes"], 1), dtype=torch.uint8, pin_memory=True)
    pinned[:asm["nbytes"]].copy_(asm["buf"])
    out = memoryview(pinned.numpy())[:asm["nbytes"]]
    hosted = np.flatnonzero(fhost)
    if len(hosted):                                            # what the host bookie's walk needs
        h = _to_host((st.dec, _NEED_KEYS), (st.sp, ("in_state",)), (tl, ("need_host",)),
                     (st.ext, ("grp_off", "version")), (asm, ("need_ans_off",)))
        nao = h["need_ans_off"]
    st.lap("readback")
    for f in np.flatnonzero(fhost == 0):
        a, b = int(fao[f]), int(fao[f + 1])
        if b > a:
            st.answers[f] = bytes(out[a:b])
    if len(hosted):
        site_ids = dict(enumerate(eng.site_ids()))
        actors = h["pair_actor"].tobytes()
    for f in hosted:
        parts = []
        for p in range(int(h["frame_pair_off"][f]), int(h["frame_pair_off"][f + 1])):
            actor = actors[16 * p:16 * p + 16]
            t0n, t1n = int(h["pair_need_off"][p]), int(h["pair_need_off"][p + 1])
            lo = int(nao[t0n])                                 # the device bytes not yet taken
            for t in range(t0n, t1n):
                if not h["need_keep"][t] or not h["need_host"][t]:
                    continue
                parts.append(bytes(out[lo:int(nao[t + 1])]))   # up to and with this need's encoded piece
                lo = int(nao[t + 1])
                parts.append(_host_need_frames(agent, h, t, actor, site_ids, max_buf_size, payload, cluster_id))
            parts.append(bytes(out[lo:int(nao[t1n])]))
        st.answers[f] = b"".join(parts)
    st.lap("bookie")
    return st.status, st.answers


def handle_request_frames_buffered(agent, buf, frame_off, max_buf_size=MAX_CHANGES_BYTES_PER_MESSAGE, payload=0,
                                   cluster_id=0, timings=None):
    """handle_request_frames_assembled with the buffered (partial) versions served from the device row
    pool: the same arguments, the same (frame_status, answers), byte for byte.

    A need whose buffered versions all lie in the bookie's pool (what process_frames buffers from
    canonical partial changesets) no longer goes back to the host walk, which would read the
    version's rows out of the pool for good. Stages: decode -> extract -> spans -> encode -> tails
    against device_buffered_index's derived books (the pool versions count as gaps there, so only a
    need that touches a host-row version keeps need_host) -> buffered_spans (the buffered chunks as
    spans, their rows gathered from the pool) -> a second encode -> assemble_answers_buffered (per
    need: state frames, buffered frames, Empty frames). The request screen keeps the real gaps. A need
    still flagged need_host takes _bookie_messages, spliced in at need_ans_off[t + 1] as in
    handle_request_frames_assembled. timings: that function's keys plus "buffered" (buffered_spans
    and the second encode; the index call counts under "tails")."""
    eng = agent.engine
    st = _request_front(agent, buf, frame_off, max_buf_size, payload, cluster_id, timings)
    if st.ext is None:
        return st.status, st.answers
    idx = device_buffered_index(agent, st.dev)
    tl = eng.need_tails(st.dec, st.ext, st.sp, idx["book"], payload, cluster_id)
    st.lap("tails")
    bsp = eng.buffered_spans(agent.bookie, st.dec, st.ext, st.sp, tl, idx["dev"])
    benc = None
    if bsp["nspans"]:
        benc = eng.encode_changesets({k: bsp[k] for k in SPAN_KEYS}, bsp["rows"], max_buf_size, payload, cluster_id)
    st.lap("buffered")
    asm = eng.assemble_answers_buffered(st.dec, st.sp, st.enc, bsp, benc, tl, payload)
    st.lap("assemble")
    return _join_assembled(agent, st, tl, asm, max_buf_size, payload, cluster_id)


def handle_request_frames(agent, buf, frame_off, max_buf_size=MAX_CHANGES_BYTES_PER_MESSAGE, payload=0, cluster_id=0,
                          timings=None):
    """process_sync + handle_need from the request bytes to the response bytes (peer/mod.rs:791-905,
    :371-789): `buf` holds SyncMessageV1::Request frames back to back and frame_off their nframes + 1
    byte offsets (bytes / numpy, or CUDA tensors: what a peer's plan_requests_device returns). Returns
    (frame_status, answers): the int32 status per frame (corro_decode_requests: 0 ok, 1 not a request,
    2 holds an Empty need, negative = malformed) and, per frame, the response bytes -- per kept need in
    wire order, the need's device frames and then the host bookie's messages, as handle_needs_frames
    orders them; b"" for a frame with another status or with every need screened out.

    The path is decode + screen (corro_decode_requests, against device_book) -> extract_changes in
    device mode -> need_spans -> encode_changesets -> need_tails (the Empty frames that end a need's
    answer, against device_book's gaps and device_buffered). The host reads the totals, frame_status,
    the kept needs' offsets and the finished bytes, and joins them per frame; no state row becomes a
    Change. Only a need that touches a buffered version (need_tails' need_host) still takes the host
    bookie's walk, _bookie_messages, with its fields, the versions found and in_state. timings (optional
    dict) receives the seconds per stage ("tails": device_buffered and need_tails; "bookie": the join
    and what the host bookie still answers)."""
    from . import wire
    eng = agent.engine
    st = _request_front(agent, buf, frame_off, max_buf_size, payload, cluster_id, timings)
    if st.ext is None:
        return st.status, st.answers
    tl = eng.need_tails(st.dec, st.ext, st.sp, {**st.book, **device_buffered(agent, st.dev)}, payload, cluster_id)
    st.lap("tails")
    # what the host bookie's walk needs: the kept needs, the versions a Full need found, in_state
    h = _to_host((st.dec, _NEED_KEYS), (st.sp, ("need_span_off", "in_state")), (st.ext, ("grp_off", "version")))
    nso = h["need_span_off"]
    out = st.enc["buf"].cpu().numpy().tobytes()
    fo, sfo = st.enc["frame_off"].cpu().numpy(), st.enc["span_frame_off"].cpu().numpy()
    nto, need_host = tl["need_tail_off"].cpu().numpy(), tl["need_host"].cpu().numpy()
    tail, tfs = tl["buf"].cpu().numpy().tobytes(), 49 if payload == wire.PAYLOAD_SYNC else 55
    st.lap("readback")
    site_ids = dict(enumerate(eng.site_ids()))
    actors = h["pair_actor"].tobytes()
    for f in range(len(st.answers)):
        parts = []
        for p in range(int(h["frame_pair_off"][f]), int(h["frame_pair_off"][f + 1])):
            actor = actors[16 * p:16 * p + 16]
            for t in range(int(h["pair_need_off"][p]), int(h["pair_need_off"][p + 1])):
                if not h["need_keep"][t]:
                    continue
                parts.append(out[int(fo[int(sfo[int(nso[t])])]):int(fo[int(sfo[int(nso[t + 1])])])])
                if not need_host[t]:                            # its Empty frames, from the device
                    parts.append(tail[tfs * int(nto[t]):tfs * int(nto[t + 1])])
                    continue
                parts.append(_host_need_frames(agent, h, t, actor, site_ids, max_buf_size, payload, cluster_id))
        st.answers[f] = b"".join(parts)
    st.lap("bookie")
    return st.status, st.answers


def handle_request_frames_assembled(agent, buf, frame_off, max_buf_size=MAX_CHANGES_BYTES_PER_MESSAGE, payload=0,
                                    cluster_id=0, timings=None):
    """handle_request_frames with the per-frame join on the device: the same arguments, the same
    (frame_status, answers), byte for byte.

    The five stages of handle_request_frames run unchanged; then assemble_answers
    (corro_assemble_answers) lays every frame's answer out in one buffer. The host reads back
    frame_status, frame_ans_off, frame_host and that buffer (one copy into a pinned staging tensor), and
    a frame takes one slice. Only when a frame holds a need that touches a buffered version
    (frame_host) are the need arrays read back too: that frame's needs are walked, sliced by
    need_ans_off, and _bookie_messages' frames go in after each host need's encoded piece. timings: the
    keys of handle_request_frames plus "assemble"; the read-backs count under "readback" and the
    remaining join under "bookie"."""
    eng = agent.engine
    st = _request_front(agent, buf, frame_off, max_buf_size, payload, cluster_id, timings)
    if st.ext is None:
        return st.status, st.answers
    tl = eng.need_tails(st.dec, st.ext, st.sp, {**st.book, **device_buffered(agent, st.dev)}, payload, cluster_id)
    st.lap("tails")
    asm = eng.assemble_answers(st.dec, st.sp, st.enc, tl, payload)
    st.lap("assemble")
    return _join_assembled(agent, st, tl, asm, max_buf_size, payload, cluster_id)


def handle_needs_frames(agent, needs, max_buf_size=MAX_CHANGES_BYTES_PER_MESSAGE, payload=0, cluster_id=0):
    """handle_needs down to the bytes on the wire: per need, the length-delimited frames the reference
    would send, in order (equal to wire.frames(handle_needs(...)[i], payload)).

    The state's versions never become Change objects: the extraction runs in device mode, the
    spans (one per ChunkedChanges of handle_need: a Full need's versions, a Partial need's seq
    ranges) are gathered from its groups on the device, and corro_encode_changesets chunks and
    encodes them there; the host reads the group ranges per need, the versions found and the
    finished bytes. The host bookie's messages (buffered versions, Empty ranges) are a handful per
    need: they take the host encoder and follow the need's device frames, as handle_needs orders them."""
    import torch
    eng = agent.engine
    ent_site, ent_s, ent_e, ent_ss, ent_se = [], [], [], [], []
    plan = []
    for actor, need in needs:                                  # one extraction entry per crsql_changes query
        site = agent.site(actor)
        if isinstance(need, NeedFull):
            plan.append(("full", len(ent_site), site))
            ent_site.append(site); ent_s.append(need.start); ent_e.append(need.end)
            ent_ss.append(SEQ_ALL[0]); ent_se.append(SEQ_ALL[1])
        elif isinstance(need, NeedPartial):
            plan.append(("partial", len(ent_site), site))
            for s, e in [SEQ_ALL] + [tuple(r) for r in need.seqs]:
                ent_site.append(site); ent_s.append(need.version); ent_e.append(need.version)
                ent_ss.append(max(0, min(s, 0xFFFFFFFF))); ent_se.append(max(0, min(e, 0xFFFFFFFF)))
        else:
            plan.append(("none", -1, site))
    site_ids = dict(enumerate(eng.site_ids()))
    dev = torch.device("cuda", eng.device)

    def up(a, dt):
        a = np.asarray(a, dt)
        return torch.from_numpy(a.view(np.int64 if a.itemsize == 8 else np.int32)).to(dev)

    # spans: (site, group that gives version / last_seq / ts, group that gives the rows or -1, seq
    # range or None = 0 ..= last_seq), in need order
    sp_site, sp_meta, sp_rows, sp_s, sp_e, sp_full = [], [], [], [], [], []
    span_range, found, in_state = [], [], []
    if ent_site:
        res = eng.extract_changes({"site": up(ent_site, np.uint32), "start": up(ent_s, np.uint64),
                                   "end": up(ent_e, np.uint64), "seq_start": up(ent_ss, np.uint32),
                                   "seq_end": up(ent_se, np.uint32)})
        grp_off = res["grp_off"].cpu().numpy()
        versions = res["version"].cpu().numpy()
    for (actor, need), (kind, k, site) in zip(needs, plan):
        first = len(sp_site)
        fnd, ins = set(), False
        if kind == "full":
            for g in range(int(grp_off[k]), int(grp_off[k + 1])):      # db_version DESC (:385-394)
                fnd.add(int(versions[g]))
                sp_site.append(site); sp_meta.append(g); sp_rows.append(g)
                sp_s.append(0); sp_e.append(0); sp_full.append(True)
        elif kind == "partial" and grp_off[k + 1] > grp_off[k]:       # :554-597
            ins = True
            for j, (s, e) in enumerate(need.seqs):
                g0, g1 = int(grp_off[k + 1 + j]), int(grp_off[k + 2 + j])
                sp_site.append(site); sp_meta.append(int(grp_off[k])); sp_rows.append(g0 if g1 > g0 else -1)
                sp_s.append(s); sp_e.append(e); sp_full.append(False)
        span_range.append((first, len(sp_site)))
        found.append(fnd)
        in_state.append(ins)
    dev_bytes = [b""] * len(needs)
    if sp_site:
        meta, rws = up(sp_meta, np.int64), up(sp_rows, np.int64)
        has_rows, full = rws >= 0, torch.from_numpy(np.asarray(sp_full)).to(dev)
        rws = rws.clamp(min=0)
        last = res["last_seq"][meta]
        spans = {"site": up(sp_site, np.uint32), "version": res["version"][meta].contiguous(), "last_seq": last.contiguous(),
                 "ts": res["ts"][meta].contiguous(), "seq_start": up(sp_s, np.uint64),
                 "seq_end": torch.where(full, last, up(sp_e, np.uint64)).contiguous(),
                 "row_off": res["grp_row_off"][rws].contiguous(),
                 "row_count": torch.where(has_rows, res["grp_rows"][rws], torch.zeros_like(rws)).contiguous()}
        enc = eng.encode_changesets(spans, res["rows"], max_buf_size, payload, cluster_id)
        buf = enc["buf"].cpu().numpy().tobytes()
        fo, sfo = enc["frame_off"].cpu().numpy(), enc["span_frame_off"].cpu().numpy()
        dev_bytes = [buf[int(fo[int(sfo[a])]):int(fo[int(sfo[b])])] for a, b in span_range]
    out_all = []
    for i, (actor, need) in enumerate(needs):
        msgs = _bookie_messages(agent, actor, need, found[i], in_state[i], site_ids, max_buf_size)
        out_all.append(dev_bytes[i] + _frame_messages(msgs, payload, cluster_id))
    return out_all
