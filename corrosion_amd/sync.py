"""SyncStateV1 / SyncNeedV1 mirror and the batched need diff on the GPU.

Mirrors /root/reference/crates/corro-types/src/sync.rs:
  SyncStateV1 (:79-87), need_len (:90-109), need_len_for_actor (:111-125),
  compute_available_needs (:127-249), SyncNeedV1 (:252-264).
The arithmetic runs in the HIP kernel `k_needs` (csrc/sync_needs.hip) through corro_compute_needs;
this module only flattens HashMaps into CSR entries and rebuilds the HashMap result.
"""
import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import _lib as L
from ._twopass import Mem, TwoPass, two_pass


@dataclass(frozen=True)
class Full:
    """SyncNeedV1::Full { versions: start..=end }"""
    start: int
    end: int

    def count(self):
        return self.end - self.start + 1


@dataclass(frozen=True)
class Partial:
    """SyncNeedV1::Partial { version, seqs }"""
    version: int
    seqs: tuple

    def count(self):
        return 1


@dataclass
class SyncStateV1:
    actor_id: bytes = b"\0" * 16
    heads: dict = field(default_factory=dict)          # actor -> head
    need: dict = field(default_factory=dict)           # actor -> [(start, end), ...]
    partial_need: dict = field(default_factory=dict)   # actor -> {version: [(s, e), ...]}
    last_cleared_ts: int = None

    def need_len(self):
        full = sum(e - s + 1 for v in self.need.values() for s, e in v)
        part = sum(e - s + 1 for p in self.partial_need.values() for rs in p.values() for s, e in rs)
        return full + part // 50  # sync.rs:106 quirk

    def need_len_for_actor(self, actor):
        return sum(e - s + 1 for s, e in self.need.get(actor, [])) + len(self.partial_need.get(actor, {}))

    def compute_available_needs(self, other, engine):
        """HashMap<ActorId, Vec<SyncNeedV1>>; partials in ascending version order."""
        return batch_compute_available_needs(engine, [(self, other)])[0]


def entries_from_states(pairs):
    """Flatten (ours, theirs) SyncStateV1 pairs into CSR entries. Returns (entries, index) with
    index[e] = (pair number, actor)."""
    E = {k: [] for k in ("their_head", "our_head", "tn_start", "tn_end", "tp_ver", "tps_start",
                         "tps_end", "on_start", "on_end", "op_ver", "ops_start", "ops_end")}
    offs = {k: [0] for k in ("tn_off", "tp_off", "tps_off", "on_off", "op_off", "ops_off")}
    index = []
    for p, (ours, theirs) in enumerate(pairs):
        for actor, head in theirs.heads.items():
            if actor == ours.actor_id or head == 0:  # sync.rs:133-140
                continue
            index.append((p, actor))
            E["their_head"].append(head)
            E["our_head"].append(ours.heads.get(actor, -1))
            for s, e in theirs.need.get(actor, []):
                E["tn_start"].append(s)
                E["tn_end"].append(e)
            offs["tn_off"].append(len(E["tn_start"]))
            tp = theirs.partial_need.get(actor, {})
            for v in sorted(tp):
                E["tp_ver"].append(v)
                for s, e in tp[v]:
                    E["tps_start"].append(s)
                    E["tps_end"].append(e)
                offs["tps_off"].append(len(E["tps_start"]))
            offs["tp_off"].append(len(E["tp_ver"]))
            for s, e in ours.need.get(actor, []):
                E["on_start"].append(s)
                E["on_end"].append(e)
            offs["on_off"].append(len(E["on_start"]))
            op = ours.partial_need.get(actor, {})
            for v in sorted(op):
                E["op_ver"].append(v)
                for s, e in op[v]:
                    E["ops_start"].append(s)
                    E["ops_end"].append(e)
                offs["ops_off"].append(len(E["ops_start"]))
            offs["op_off"].append(len(E["op_ver"]))
    out = {k: np.array(v, dtype=np.int64 if k == "our_head" else np.uint64) for k, v in E.items()}
    for k, v in offs.items():
        out[k] = np.array(v, dtype=np.uint64)
    return out, index


def _needs_host(engine, ent):
    """Run corro_compute_needs on host CSR arrays (two passes). Returns the CSR result dict."""
    lib = L.lib()
    n = len(ent["their_head"])
    keep = []
    s = L.SyncEntries()
    s.n = n
    for k, _ in L.SyncEntries._fields_[1:]:
        a = np.ascontiguousarray(ent[k], dtype=np.int64 if k == "our_head" else np.uint64)
        keep.append(a)
        setattr(s, k, a.ctypes.data if a.size else None)
    o = L.NeedsOut()
    nc = np.zeros(max(n, 1), np.uint64)
    sc = np.zeros(max(n, 1), np.uint64)
    o.need_count, o.seq_count = nc.ctypes.data, sc.ctypes.data
    if n:
        L.check(lib.corro_compute_needs(engine._h, C.byref(s), L.CORRO_MEM_HOST, C.byref(o), 0))
    need_off = np.zeros(n + 1, np.uint64)
    seq_off = np.zeros(n + 1, np.uint64)
    need_off[1:] = np.cumsum(nc[:n])
    seq_off[1:] = np.cumsum(sc[:n])
    T, Ts = int(need_off[-1]), int(seq_off[-1])
    res = {"need_off": need_off, "seq_off": seq_off, "kind": np.zeros(max(T, 1), np.uint8),
           "start": np.zeros(max(T, 1), np.uint64), "end": np.zeros(max(T, 1), np.uint64),
           "sr_off": np.zeros(max(T, 1), np.uint64), "sr_n": np.zeros(max(T, 1), np.uint64),
           "s_start": np.zeros(max(Ts, 1), np.uint64), "s_end": np.zeros(max(Ts, 1), np.uint64)}
    for k in ("need_off", "seq_off", "kind", "start", "end", "sr_off", "sr_n", "s_start", "s_end"):
        setattr(o, k, res[k].ctypes.data)
    if n:
        L.check(lib.corro_compute_needs(engine._h, C.byref(s), L.CORRO_MEM_HOST, C.byref(o), 1))
    for k in ("kind", "start", "end", "sr_off", "sr_n"):
        res[k] = res[k][:T]
    for k in ("s_start", "s_end"):
        res[k] = res[k][:Ts]
    return res


def _needs_device(engine, ent):
    """corro_compute_needs on device-resident CSR entries (dict of CUDA int64 tensors).
    Returns the CSR result as CUDA tensors (two passes, offsets scanned on the device)."""
    import torch
    lib = L.lib()
    n = int(ent["their_head"].shape[0])
    dev = ent["their_head"].device
    s = L.SyncEntries()
    s.n = n
    for k, _ in L.SyncEntries._fields_[1:]:
        a = ent[k]
        setattr(s, k, a.data_ptr() if a.numel() else None)
    nc = torch.empty(max(n, 1), dtype=torch.int64, device=dev)  # pass 0 writes every entry
    sc = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
    o = L.NeedsOut()
    o.need_count, o.seq_count = nc.data_ptr(), sc.data_ptr()
    torch.cuda.current_stream().synchronize()
    L.check(lib.corro_compute_needs(engine._h, C.byref(s), L.CORRO_MEM_DEVICE, C.byref(o), 0))
    need_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    seq_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    L.check(lib.corro_scan_offsets(engine._h, nc.data_ptr(), need_off.data_ptr(), n))
    L.check(lib.corro_scan_offsets(engine._h, sc.data_ptr(), seq_off.data_ptr(), n))
    T, Ts = int(need_off[-1].item()), int(seq_off[-1].item())
    # pass 1 writes every output element: no fill needed
    res = {"need_off": need_off, "seq_off": seq_off,
           "kind": torch.empty(max(T, 1), dtype=torch.uint8, device=dev)}
    for k in ("start", "end", "sr_off", "sr_n"):
        res[k] = torch.empty(max(T, 1), dtype=torch.int64, device=dev)
    for k in ("s_start", "s_end"):
        res[k] = torch.empty(max(Ts, 1), dtype=torch.int64, device=dev)
    for k in ("need_off", "seq_off", "kind", "start", "end", "sr_off", "sr_n", "s_start", "s_end"):
        setattr(o, k, res[k].data_ptr())
    torch.cuda.current_stream().synchronize()
    L.check(lib.corro_compute_needs(engine._h, C.byref(s), L.CORRO_MEM_DEVICE, C.byref(o), 1))
    for k in ("kind", "start", "end", "sr_off", "sr_n"):
        res[k] = res[k][:T]
    for k in ("s_start", "s_end"):
        res[k] = res[k][:Ts]
    return res


def _needs_device_1pass(engine, ent):
    """corro_compute_needs_onepass on device-resident CSR entries: one kernel, every input read once
    (outputs sized by corro_needs_bound; re-run at the exact totals in the never-expected case of
    overlapping need ranges exceeding it). Returns the same CSR dict as _needs_device."""
    import torch
    lib = L.lib()
    n = int(ent["their_head"].shape[0])
    dev = ent["their_head"].device
    s = L.SyncEntries()
    s.n = n
    for k, _ in L.SyncEntries._fields_[1:]:
        a = ent[k]
        setattr(s, k, a.data_ptr() if a.numel() else None)
    torch.cuda.current_stream().synchronize()
    ncap, scap = C.c_uint64(), C.c_uint64()
    L.check(lib.corro_needs_bound(engine._h, C.byref(s), L.CORRO_MEM_DEVICE, C.byref(ncap), C.byref(scap)))
    caps = [ncap.value, scap.value]
    while True:
        res = {"need_off": torch.empty(n + 1, dtype=torch.int64, device=dev),
               "seq_off": torch.empty(n + 1, dtype=torch.int64, device=dev),
               "kind": torch.empty(max(caps[0], 1), dtype=torch.uint8, device=dev)}
        for k in ("start", "end", "sr_off", "sr_n"):
            res[k] = torch.empty(max(caps[0], 1), dtype=torch.int64, device=dev)
        for k in ("s_start", "s_end"):
            res[k] = torch.empty(max(caps[1], 1), dtype=torch.int64, device=dev)
        o = L.NeedsOut()
        for k in ("need_off", "seq_off", "kind", "start", "end", "sr_off", "sr_n", "s_start", "s_end"):
            setattr(o, k, res[k].data_ptr())
        tot = (C.c_uint64 * 2)()
        rc = lib.corro_compute_needs_onepass(engine._h, C.byref(s), C.byref(o), caps[0], caps[1], tot)
        if rc == -6 and (tot[0] > caps[0] or tot[1] > caps[1]):
            caps = [tot[0], tot[1]]
            continue
        L.check(rc)
        break
    if n == 0:
        res["need_off"].zero_()
        res["seq_off"].zero_()
    T, Ts = tot[0], tot[1]
    for k in ("kind", "start", "end", "sr_off", "sr_n"):
        res[k] = res[k][:T]
    for k in ("s_start", "s_end"):
        res[k] = res[k][:Ts]
    return res


def _needs_device_packed(engine, ent):
    """corro_compute_needs_packed on device-resident CSR entries: one kernel, no count pass; outputs
    in the workgroup-padded packed layout (slots sized by corro_needs_bound). Returns CUDA tensors
    need_off, need_count, range (2 per slot), kind, s_start, s_end."""
    import torch
    lib = L.lib()
    n = int(ent["their_head"].shape[0])
    dev = ent["their_head"].device
    s = L.SyncEntries()
    s.n = n
    for k, _ in L.SyncEntries._fields_[1:]:
        a = ent[k]
        setattr(s, k, a.data_ptr() if a.numel() else None)
    torch.cuda.current_stream().synchronize()
    ncap, scap = C.c_uint64(), C.c_uint64()
    L.check(lib.corro_needs_bound(engine._h, C.byref(s), L.CORRO_MEM_DEVICE, C.byref(ncap), C.byref(scap)))
    res = {"need_off": torch.empty(max(n, 1), dtype=torch.int64, device=dev),
           "need_count": torch.empty(max(n, 1), dtype=torch.int32, device=dev),
           "range": torch.empty(2 * max(ncap.value, 1), dtype=torch.int64, device=dev),
           "kind": torch.empty(max(ncap.value, 1), dtype=torch.uint8, device=dev),
           "s_start": torch.empty(max(scap.value, 1), dtype=torch.int64, device=dev),
           "s_end": torch.empty(max(scap.value, 1), dtype=torch.int64, device=dev)}
    o = L.NeedsPackedOut()
    for k in ("need_off", "need_count", "range", "kind", "s_start", "s_end"):
        setattr(o, k, res[k].data_ptr())
    L.check(lib.corro_compute_needs_packed(engine._h, C.byref(s), C.byref(o), ncap.value, scap.value))
    res["need_off"], res["need_count"] = res["need_off"][:n], res["need_count"][:n]
    return res


def packed_to_csr(res):
    """The packed layout as the CSR dict of corro_compute_needs (numpy, host): need_off / seq_off
    (n+1), kind, start, end, sr_off, sr_n, s_start, s_end."""
    import numpy as np
    g = {k: (v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)) for k, v in res.items()}
    cnt = g["need_count"].astype(np.int64)
    n = len(cnt)
    need_off = np.zeros(n + 1, np.int64)
    need_off[1:] = np.cumsum(cnt)
    T = int(need_off[-1])
    slot = np.repeat(g["need_off"].astype(np.int64) - need_off[:-1], cnt) + np.arange(T)
    rng = g["range"].view(np.uint64).reshape(-1, 2)[slot]
    kind = g["kind"][slot]
    part = kind == 1
    first = (rng[:, 1] >> np.uint64(24)).astype(np.int64)
    sr_n = np.where(part, (rng[:, 1] & np.uint64(0xFFFFFF)).astype(np.int64), 0)
    ent_of = np.repeat(np.arange(n), cnt)
    seq_cnt = np.bincount(ent_of, weights=sr_n, minlength=n).astype(np.int64) if T else np.zeros(n, np.int64)
    seq_off = np.zeros(n + 1, np.int64)
    seq_off[1:] = np.cumsum(seq_cnt)
    # seq ranges of the partials in need order, compacted
    sr_off = np.zeros(T, np.int64)
    sr_off[1:] = np.cumsum(sr_n)[:-1]
    src = np.repeat(np.where(part, first, 0), sr_n) + (np.arange(int(sr_n.sum())) - np.repeat(sr_off, sr_n))
    full_sr = np.zeros(T, np.int64)  # a Full need's sr_off: the seq ranges emitted before it
    full_sr[:] = sr_off
    return {"need_off": need_off, "seq_off": seq_off, "kind": kind,
            "start": rng[:, 0].astype(np.int64),
            "end": np.where(part, rng[:, 0], rng[:, 1]).astype(np.int64),
            "sr_off": full_sr, "sr_n": sr_n,
            "s_start": g["s_start"][src].astype(np.int64), "s_end": g["s_end"][src].astype(np.int64)}


def decode(res, index, npairs):
    out = [dict() for _ in range(npairs)]
    for e, (p, actor) in enumerate(index):
        lst = []
        for k in range(int(res["need_off"][e]), int(res["need_off"][e + 1])):
            if int(res["kind"][k]) == 0:
                lst.append(Full(int(res["start"][k]), int(res["end"][k])))
            else:
                o, m = int(res["sr_off"][k]), int(res["sr_n"][k])
                lst.append(Partial(int(res["start"][k]),
                                   tuple((int(res["s_start"][j]), int(res["s_end"][j])) for j in range(o, o + m))))
        if lst:
            out[p][actor] = lst
    return out


_REQ_IN = ("site", "need_off", "kind", "start", "end", "sr_off", "sr_n", "s_start", "s_end", "grp_ent_off",
           "grp_session")
_REQ_OUT = (("buf", np.uint8, "nbytes"), ("frame_off", np.int64, "nframes", 1, 1), ("frame_entry", np.int64, "nframes"),
            ("frame_round", np.int32, "nframes"), ("frame_needs", np.int32, "nframes"))


def requests_csr(sessions, site_of):
    """Flatten sessions (each a list, in server order, of {actor: [Full | Partial, ...]}) into the
    host arrays of corro_request_in. Servers with an empty map are skipped (peer/mod.rs:1135-1138).
    Returns (arrays, groups) with groups[g] = (session number, server number)."""
    A = {k: [] for k in ("site", "kind", "start", "end", "sr_off", "sr_n", "s_start", "s_end", "grp_session")}
    need_off, grp_ent_off, groups = [0], [0], []
    for sn, servers in enumerate(sessions):
        for sv, needs in enumerate(servers):
            if not needs:
                continue
            groups.append((sn, sv))
            A["grp_session"].append(sn)
            for actor, lst in needs.items():
                A["site"].append(site_of(actor))
                for nd in lst:
                    part = isinstance(nd, Partial)
                    A["kind"].append(1 if part else 0)
                    A["start"].append(nd.version if part else nd.start)
                    A["end"].append(nd.version if part else nd.end)
                    A["sr_off"].append(len(A["s_start"]))
                    A["sr_n"].append(len(nd.seqs) if part else 0)
                    for s, e in (nd.seqs if part else ()):
                        A["s_start"].append(s)
                        A["s_end"].append(e)
                need_off.append(len(A["kind"]))
            grp_ent_off.append(len(A["site"]))
    out = {k: np.array(v, dtype=np.uint32 if k == "site" else np.uint8 if k == "kind" else np.uint64) for k, v in A.items()}
    out["need_off"] = np.array(need_off, np.uint64)
    out["grp_ent_off"] = np.array(grp_ent_off, np.uint64)
    return out, groups


def _plan_requests(engine, arr, chunk, drain, device):
    """corro_plan_requests, both passes, on host numpy arrays or (device=True) CUDA tensors keyed like
    corro_request_in. Returns nframes, nbytes, grp_frame_off, buf, frame_off, frame_entry, frame_round,
    frame_needs in the same kind of memory; with device arrays only the two totals reach the host."""
    mem = Mem(arr["need_off"].device) if device else Mem()
    if not device:
        want = {"site": np.uint32, "kind": np.uint8}
        arr = {k: np.ascontiguousarray(arr[k], dtype=want.get(k, np.uint64)) for k in _REQ_IN}
    r = L.RequestIn()
    r.n = mem.count(arr["site"])
    r.nneeds, r.nseqs, r.ngroups = mem.count(arr["kind"]), mem.count(arr["s_start"]), mem.count(arr["grp_session"])
    r.chunk_size, r.drain = chunk, drain
    for k in _REQ_IN:
        setattr(r, k, mem.ptr(arr[k]))
    return two_pass(L.lib().corro_plan_requests, (engine._h, C.byref(r), mem.const), mem, L.Requests(),
                    (("grp_frame_off", np.int64, r.ngroups + 1),), ("nframes", "nbytes"), _REQ_OUT)


def plan_requests_device(engine, needs, site, grp_ent_off, grp_session, chunk=10, drain=10):
    """Request planning on device-resident needs: `needs` is the CSR dict of _needs_device_1pass (or
    _needs_device), `site` the int32 site ordinal per entry, grp_ent_off / grp_session int64 group
    arrays, all CUDA tensors. Returns CUDA tensors (see _plan_requests); no payload touches the host."""
    arr = {k: needs[k] for k in ("need_off", "kind", "start", "end", "sr_off", "sr_n", "s_start", "s_end")}
    arr.update(site=site, grp_ent_off=grp_ent_off, grp_session=grp_session)
    return _plan_requests(engine, arr, chunk, drain, True)


def split_requests(res, groups, nsessions, nservers):
    """Host result of _plan_requests -> per session, per server, the list of (round, frame bytes)."""
    out = [[[] for _ in range(k)] for k in nservers]
    assert len(out) == nsessions
    buf = res["buf"].tobytes()
    fo, gfo, rnd = res["frame_off"], res["grp_frame_off"], res["frame_round"]
    for g, (sn, sv) in enumerate(groups):
        out[sn][sv] = [(int(rnd[f]), buf[int(fo[f]):int(fo[f + 1])]) for f in range(int(gfo[g]), int(gfo[g + 1]))]
    return out


def plan_sync_requests(engine, sessions, chunk=10, drain=10):
    """parallel_sync's request loop (peer/mod.rs:1131-1318) for many sessions in one call of
    corro_plan_requests. `sessions` is a list of sessions, each a list in server order of
    {actor: [Full | Partial, ...]} (compute_available_needs results; actors are 16-byte ids, registered
    as sites here). Returns, per session and per server, the list of (round, frame bytes) in sending
    order; a server's frames of one round go out in one write. A server with an empty map gets []."""
    actors = sorted({a for servers in sessions for needs in servers for a in needs})
    ords = engine.register_sites(np.frombuffer(b"".join(actors), np.uint8)) if actors else []
    site = {a: int(o) for a, o in zip(actors, ords)}
    arr, groups = requests_csr(sessions, site.__getitem__)
    res = _plan_requests(engine, arr, chunk, drain, False)
    return split_requests(res, groups, len(sessions), [len(s) for s in sessions])


_ENT_KEYS = tuple(k for k, _ in L.SyncEntries._fields_[1:])
# corro_statedec_out's arrays as output tables (see _twopass): pass 0's, then pass 1's over the totals
_STATE_HEAD_OUT = (("frame_status", np.int32, "nframes"), ("frame_actor", np.uint8, "nframes", 16, 0),
                   ("frame_has_ts", np.uint8, "nframes"), ("frame_ts", np.int64, "nframes"),
                   ("pair_status", np.uint8, "npairs"), ("pair_ent_off", np.int64, "npairs", 1, 1))
_STATE_ENT = {"their_head": ("n", 0), "our_head": ("n", 0), "tn_off": ("n", 1), "tn_start": ("ntn", 0), "tn_end": ("ntn", 0),
              "tp_off": ("n", 1), "tp_ver": ("ntp", 0), "tps_off": ("ntp", 1), "tps_start": ("ntps", 0),
              "tps_end": ("ntps", 0), "on_off": ("n", 1), "on_start": ("non", 0), "on_end": ("non", 0),
              "op_off": ("n", 1), "op_ver": ("nop", 0), "ops_off": ("nop", 1), "ops_start": ("nops", 0),
              "ops_end": ("nops", 0)}
_STATE_ENT_OUT = tuple((k, np.int64, tot, 1, extra) for k, (tot, extra) in _STATE_ENT.items()) + (
    ("entry_pair", np.int32, "n"), ("entry_site", np.int32, "n"), ("entry_actor", np.uint8, "n", 16, 0))
_STATE_TOTALS = ("n", "ntn", "ntp", "ntps", "non", "nop", "nops", "nunregistered")


class _StateFrames:
    """corro_decode_states over one set of frames and pairs: pass 0 once, pass 1 as often as asked."""

    def __init__(self, engine, buf, frame_off, pairs, device):
        if device:
            import torch
            mem = Mem(buf.device)
            npdt = {torch.uint8: np.uint8, torch.int32: np.int32, torch.int64: np.int64}
            as_t = lambda a, dt: a.to(device=mem.dev, dtype=dt).contiguous() if hasattr(a, "to") else torch.from_numpy(
                np.asarray(a).astype(npdt[dt])).to(mem.dev)
            buf, frame_off = as_t(buf, torch.uint8), as_t(frame_off, torch.int64)
            pr = as_t(pairs, torch.int32).reshape(-1, 2)
            ours, theirs = pr[:, 0].contiguous(), pr[:, 1].contiguous()
        else:
            mem = Mem()
            buf = np.frombuffer(bytes(buf), np.uint8) if isinstance(buf, (bytes, bytearray)) else np.ascontiguousarray(
                buf, np.uint8)
            frame_off = np.ascontiguousarray(frame_off, np.uint64)
            pr = np.asarray(pairs, np.int64).reshape(-1, 2)
            ours, theirs = np.ascontiguousarray(pr[:, 0], np.uint32), np.ascontiguousarray(pr[:, 1], np.uint32)
        self.keep = (buf, frame_off, ours, theirs)
        r = L.StateDecIn()
        r.buf, r.len = mem.ptr(buf), mem.count(buf)
        r.nframes, r.frame_off = mem.count(frame_off) - 1, mem.ptr(frame_off)
        r.npairs, r.pair_ours, r.pair_theirs = mem.count(ours), mem.ptr(ours), mem.ptr(theirs)
        F, P = r.nframes, r.npairs
        self.tp = TwoPass(L.lib().corro_decode_states, (engine._h, C.byref(r), mem.const), mem, L.StateDecOut())
        self.o = self.tp.o
        self.tp.run(0, _STATE_HEAD_OUT, {"nframes": F, "npairs": P})
        self.totals = {k: getattr(self.o, k) for k in _STATE_TOTALS}
        self.head = self.tp.result()
        self.head["frame_actor"] = self.head["frame_actor"].reshape(F, 16)

    def fill(self):
        """Pass 1: the entry arrays (sites as the engine knows them now)."""
        t = self.totals
        self.tp.run(1, _STATE_ENT_OUT, t)
        res = {**self.head, **self.tp.result()}
        res["entry_actor"] = res["entry_actor"].reshape(t["n"], 16)
        if not self.tp.mem.on_dev:
            res["entry_site"] = res["entry_site"].view(np.uint32)
            for k in _STATE_ENT:
                if k != "our_head":
                    res[k] = res[k].view(np.uint64)
        res["nunregistered"] = t["nunregistered"] = self.o.nunregistered   # (as the site table stands now)
        return res


def entries_from_state_frames(engine, buf, frame_off, pairs, device=False):
    """corro_decode_states, both passes: SyncMessageV1::State frames -> the need diff's entries. `buf` holds
    the frames back to back, frame f = buf[frame_off[f]:frame_off[f + 1]] with its length prefix; `pairs` is
    a list (or n x 2 array) of (ours, theirs) frame indices. Host numpy arrays, or with device=True CUDA
    tensors (buf a CUDA uint8 tensor): then only totals reach the host. Returns the dict of
    entries_from_states' keys (uint64 arrays, our_head int64; int64 CUDA tensors) plus entry_pair,
    entry_actor (n x 16), entry_site (0xFFFFFFFF: not registered; -1 in the int32 tensor), pair_status,
    pair_ent_off, frame_status, frame_actor (nframes x 16), frame_has_ts, frame_ts and nunregistered."""
    return _StateFrames(engine, buf, frame_off, pairs, device).fill()


def requests_from_state_frames(engine, buf, frame_off, sessions, chunk=10, drain=10):
    """Peer state bytes in, request bytes out, on the device: sessions = [(ours_frame, [theirs_frame, ...]),
    ...] over the State frames of the CUDA uint8 tensor `buf`. Decodes every (ours, theirs) pair
    (corro_decode_states), diffs them (corro_compute_needs) and plans the requests (corro_plan_requests)
    with one group per pair in session order. Actors the engine has not seen are registered: only their
    distinct ids are read back, and the entries are filled again. Returns plan_requests_device's result
    plus `groups`, groups[g] = (session number, server number), and `pair_status`."""
    import torch
    groups = [(sn, sv) for sn, (_o, servers) in enumerate(sessions) for sv in range(len(servers))]
    pairs = np.array([(o, t) for o, servers in sessions for t in servers], np.int64).reshape(-1, 2)
    dec = _StateFrames(engine, buf, frame_off, pairs, True)
    ent = dec.fill()
    if ent["nunregistered"]:
        ids = torch.unique(ent["entry_actor"][ent["entry_site"] == -1], dim=0)
        engine.register_sites(ids.cpu().numpy().reshape(-1))
        ent = dec.fill()
    needs = _needs_device(engine, {k: ent[k] for k in _ENT_KEYS})
    dev = ent["their_head"].device
    res = plan_requests_device(engine, needs, ent["entry_site"], ent["pair_ent_off"],
                               torch.tensor([g[0] for g in groups], dtype=torch.int64, device=dev), chunk, drain)
    res["groups"], res["pair_status"] = groups, ent["pair_status"]
    return res


_BOOK_DT = {"actor": np.uint8, "max": np.int64}
_STATEENC_OUT = (("state_status", np.int32, 0), ("frame_off", np.uint64, 1), ("n_heads", np.uint32, 0),
                 ("n_need", np.uint32, 0), ("n_partial", np.uint32, 0))


def concat_books(books):
    """Sync books (Agent.sync_book() dicts) -> one book of shared row arrays plus "state_row_off"
    (len(books) + 1): state b's rows are [state_row_off[b], state_row_off[b + 1])."""
    out = {k: [] for k in L._BOOK_ROWS}
    row_off, ng, npt, ns = [0], 0, 0, 0
    for bk in books:
        a = {k: np.ascontiguousarray(bk[k], _BOOK_DT.get(k, np.uint64)) for k in L._BOOK_ROWS}
        out["actor"].append(a["actor"].reshape(-1))
        out["max"].append(a["max"])
        out["gap_off"].append(a["gap_off"][:-1] + np.uint64(ng))
        out["part_off"].append(a["part_off"][:-1] + np.uint64(npt))
        out["psr_off"].append(a["psr_off"][:-1] + np.uint64(ns))
        for k in ("gap_start", "gap_end", "part_version", "part_last_seq", "psr_start", "psr_end"):
            out[k].append(a[k])
        row_off.append(row_off[-1] + int(a["max"].size))
        ng, npt, ns = ng + int(a["gap_off"][-1]), npt + int(a["part_off"][-1]), ns + int(a["psr_off"][-1])
    for k, end in (("gap_off", ng), ("part_off", npt), ("psr_off", ns)):
        out[k].append(np.array([end], np.uint64))
    res = {k: np.concatenate(v).astype(_BOOK_DT.get(k, np.uint64)) for k, v in out.items()}
    res["state_row_off"] = np.array(row_off, np.uint64)
    return res


class _StateEnc:
    """corro_encode_states over one set of books: pass 0 on construction, pass 1 by write()."""

    def __init__(self, engine, books, self_actors, ts, max_payload, device):
        book = books if isinstance(books, dict) else concat_books(books)
        F = int(book["state_row_off"].shape[0]) - 1
        if isinstance(self_actors, (list, tuple)):
            self_actors = np.frombuffer(b"".join(bytes(a) for a in self_actors), np.uint8)
        if ts is None:
            ts = [None] * F
        has_ts = np.array([t is not None for t in ts], np.uint8)
        tsv = np.array([(t or 0) for t in ts], np.uint64)
        fields = dict(book, self_actor=self_actors, has_ts=has_ts, ts=tsv)
        dts = dict(_BOOK_DT, self_actor=np.uint8, has_ts=np.uint8)
        if device:
            import torch
            for k, a in fields.items():
                if not hasattr(a, "is_cuda"):
                    a = np.array(a, dts.get(k, np.uint64)).reshape(-1)     # (a copy: from_numpy wants it writable)
                    fields[k] = torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()
                else:
                    fields[k] = a.reshape(-1)
        else:
            fields = {k: np.ascontiguousarray(a, dts.get(k, np.uint64)).reshape(-1) for k, a in fields.items()}
        r = L.StateEncIn()
        for k, a in fields.items():
            fields[k], p = engine._in_field(a, dts.get(k, np.uint64), device, k)
            setattr(r, k, p)
        count = (lambda a: int(a.numel())) if device else (lambda a: int(a.size))
        r.nstates, r.nrows = F, count(fields["max"])
        r.ngaps, r.nparts, r.npsr = count(fields["gap_start"]), count(fields["part_version"]), count(fields["psr_start"])
        if count(fields["self_actor"]) != 16 * F or count(fields["has_ts"]) != F:
            raise ValueError("one 16-byte self actor and one ts per state")
        r.max_payload = max_payload
        self.engine, self.fields, self.r, self.F = engine, fields, r, F
        self.alloc, self.ptr, self.sync = engine._two_pass_io(device, fields["max"].device if device else None)
        self.mem = L.CORRO_MEM_DEVICE if device else L.CORRO_MEM_HOST
        self.o = L.StateEncOut()
        res = {k: self.alloc(F + extra, dt) for k, dt, extra in _STATEENC_OUT}
        for k, a in res.items():
            setattr(self.o, k, self.ptr(a))
        self._call(0)
        self.head = {k: res[k][:F + extra] for k, _dt, extra in _STATEENC_OUT}
        self.total_bytes = int(self.o.total_bytes)

    def _call(self, which):
        self.sync()
        L.check(L.lib().corro_encode_states(self.engine._h, C.byref(self.r), self.mem, C.byref(self.o), which))

    def write(self, buf=None):
        """Pass 1 into `buf` (allocated here when None): the frames, total_bytes of them."""
        if buf is None:
            buf = self.alloc(self.total_bytes, np.uint8)
        self.o.buf = self.ptr(buf)
        self._call(1)
        return buf[:self.total_bytes]


def state_frames_from_books(engine, books, self_actors, ts=None, max_payload=0, device=False):
    """corro_encode_states, both passes: sync books -> SyncMessageV1::State frames, one per state, back to
    back. `books`: a list of Agent.sync_book() dicts, or one dict that already holds the shared row arrays
    and "state_row_off" (concat_books; with device=True its arrays may be CUDA tensors, which are used
    where they lie). self_actors: one 16-byte id per state; ts: None, or per state an int or None
    (last_cleared_ts); max_payload: the codec's max_frame_length (0: 2^32 - 1). Host numpy arrays, or with
    device=True CUDA tensors: then only the totals reach the host. Returns "buf" (uint8), "frame_off"
    (nstates + 1), "state_status" (0, CORRO_E_INVALID for a book that is not canonical, CORRO_E_RANGE for a
    payload above max_payload: such a state's frame is empty), "n_heads", "n_need", "n_partial" and
    "total_bytes"."""
    enc = _StateEnc(engine, books, self_actors, ts, max_payload, device)
    res = dict(enc.head)
    res["buf"], res["total_bytes"] = enc.write(), enc.total_bytes
    return res


def requests_from_books(engine, books, self_actors, sessions, ts=None, max_payload=0, chunk=10, drain=10):
    """Sync books in, request bytes out, on the device: state_frames_from_books(device=True), then
    requests_from_state_frames over its frames where they lie (sessions name states by index). Nothing is
    read back in between but the totals."""
    fr = state_frames_from_books(engine, books, self_actors, ts=ts, max_payload=max_payload, device=True)
    res = requests_from_state_frames(engine, fr["buf"], fr["frame_off"], sessions, chunk, drain)
    res["state_status"] = fr["state_status"]
    return res


def batch_compute_available_needs(engine, pairs):
    """compute_available_needs for many (ours, theirs) pairs in one kernel launch pair."""
    ent, index = entries_from_states(pairs)
    res = _needs_host(engine, ent)
    return decode(res, index, len(pairs))
