"""match_changes for subscriptions and update handles over the device engine.

Mirrors corro-types/src/updates.rs: `match_changes` (:420-481) with the two `filter_matchable_change`
(a subscription's, pubsub.rs:294-332, and an update handle's, updates.rs:92-121), `handle_candidates`
(:270-305) and `match_changes_from_db_version` (:483-536). The filter, the first-occurrence dedup and
the compaction run in libcorro_hip.so (csrc/match.hip, corro_match_changes) over the arrays a
process_multiple_changes call left on the device; this module resolves names into the bit matrix the
kernel reads and turns the candidate columns back into per-handle maps.
"""
import ctypes as C

import numpy as np

from . import _lib as L
from ._twopass import Mem, TwoPass, _is_torch

SENTINEL = "-1"
UPDATE, DELETE = "Update", "Delete"
_CS_WORDS = C.sizeof(L.Changeset) // 8
_CS_OFF, _CS_COUNT = L.Changeset.change_off.offset // 8, L.Changeset.change_count.offset // 8


class MatchFilters:
    """The live handles as filter classes. engine: a MergeEngine, or its schema {table: [columns]} in table
    order. subs: one {table: [columns]} per subscription (its query's table_columns); updates: one table
    name per update handle. Handles are numbered subs first, then updates. A filter is a set of column
    slots -- slot(t, cid) = base[t] + cid, cid 0 the row sentinel -- and handles with equal sets share one
    class: `handle_class[h]`, `nclasses`, and `bits`, the nslots x ceil(nclasses / 32) uint32 matrix of
    corro_match_in.col_class_bits. An unknown table or column is a ValueError."""

    def __init__(self, engine, subs=(), updates=()):
        schema = engine.schema if hasattr(engine, "schema") else list(dict(engine).items())
        self.tables = [name for name, _cols in schema]
        cols = {name: list(c) for name, c in schema}
        self.base = {}
        at = 0
        for name in self.tables:
            self.base[name] = at
            at += len(cols[name]) + 1
        self.nslots = at
        self.handles = [("sub", {t: list(c) for t, c in s.items()}) for s in subs] + [("update", t) for t in updates]
        classes = {}
        self.handle_class = []
        for kind, what in self.handles:
            slots = set()
            for table, names in (what.items() if kind == "sub" else [(what, None)]):
                if table not in cols:
                    raise ValueError(f"no such table: {table}")
                if names is None:                       # an update handle takes every change of its table
                    slots.update(range(self.base[table], self.base[table] + len(cols[table]) + 1))
                    continue
                slots.add(self.base[table])             # the sentinel passes any subscription naming the table
                for c in names:
                    if c == SENTINEL:
                        continue
                    if c not in cols[table]:
                        raise ValueError(f"no such column: {table}.{c}")
                    slots.add(self.base[table] + 1 + cols[table].index(c))
            self.handle_class.append(classes.setdefault(frozenset(slots), len(classes)))
        self.nclasses = len(classes)
        if self.nclasses >= 1 << 16:
            raise L.CorroError(-6, "at most 2^16 - 1 filter classes")
        self.words = (self.nclasses + 31) // 32
        self.bits = np.zeros((self.nslots, self.words), np.uint32)
        for slots, c in classes.items():
            for s in slots:
                self.bits[s, c // 32] |= np.uint32(1 << (c % 32))
        self._dev = {}

    def device_bits(self, device):
        """The matrix as a CUDA tensor, uploaded once per device."""
        import torch
        key = str(device)
        if key not in self._dev:
            self._dev[key] = torch.from_numpy(self.bits.view(np.int32).reshape(-1).copy()).to(device)
        return self._dev[key]


def _cs_records(cs, ncs, on_dev, dev):
    """cs as corro_changeset records: a ctypes Changeset array / uint8 record buffer is used as it is;
    an (ncs, 2) array of (change_off, change_count) becomes records that hold nothing else."""
    if isinstance(cs, C.Array):
        if on_dev:
            raise ValueError("device matching takes its changeset headers as a CUDA tensor")
        return cs, (len(cs) if ncs is None else ncs), C.addressof(cs)
    if on_dev:
        import torch
        if not _is_torch(cs) or not cs.is_cuda:
            raise ValueError("device matching takes its changeset headers as a CUDA tensor")
        if cs.dtype == torch.uint8:
            have = int(cs.numel()) // C.sizeof(L.Changeset)
            ncs = have if ncs is None else ncs
            if ncs > have or not cs.is_contiguous():
                raise ValueError("cs holds fewer corro_changeset records than ncs")
            return cs, ncs, cs.data_ptr()
        pairs = cs.reshape(-1, 2).to(torch.int64)
        rec = torch.zeros((max(1, pairs.shape[0]), _CS_WORDS), dtype=torch.int64, device=dev)
        rec[:pairs.shape[0], _CS_OFF] = pairs[:, 0]
        rec[:pairs.shape[0], _CS_COUNT] = pairs[:, 1]
        return rec, int(pairs.shape[0]) if ncs is None else ncs, rec.data_ptr()
    a = np.asarray(cs)
    if a.dtype == np.uint8 and a.ndim == 1:
        a = np.ascontiguousarray(a)
        have = a.size // C.sizeof(L.Changeset)
        return a, (have if ncs is None else ncs), a.ctypes.data
    pairs = a.reshape(-1, 2).astype(np.uint64)
    rec = np.zeros((max(1, pairs.shape[0]), _CS_WORDS), np.uint64)
    rec[:pairs.shape[0], _CS_OFF] = pairs[:, 0]
    rec[:pairs.shape[0], _CS_COUNT] = pairs[:, 1]
    return rec, (int(pairs.shape[0]) if ncs is None else ncs), rec.ctypes.data


_OUT = (("cand_change", np.uint32, "ncand"), ("cand_cs", np.uint32, "ncand"), ("cand_table", np.uint32, "ncand"),
        ("cand_pk", np.uint64, "ncand"), ("cand_cl", np.uint32, "ncand"))


def match_changes(engine, changes, impactful, cs, filters, device=None, ncs=None, timings=None):
    """corro_match_changes, both passes. changes: the batch columns "pk", "table_cid", "cl" (others are
    ignored); impactful: one uint8 flag per change (Processed.impact); cs: the changeset headers -- a
    buffer of corro_changeset records (decode_frames' "cs_dev", a ctypes array on the host) or an
    (ncs, 2) array of (change_off, change_count) -- of which the first `ncs` count. CUDA tensors
    (device=True; nothing but totals reaches the host) or numpy arrays (device=False); None decides by
    the type of changes["pk"]. Returns "ncand", "class_off" (nclasses + 1) and the candidate columns
    "cand_change", "cand_cs", "cand_table", "cand_pk", "cand_cl" in the same memory: class c's candidates
    are [class_off[c], class_off[c + 1]) in ascending change index. timings: a dict that receives
    "pass0_ms" / "pass1_ms", the wall time of each call (a call returns with its stream idle)."""
    import time
    on_dev = _is_torch(changes["pk"]) if device is None else bool(device)
    mem = Mem(changes["pk"].device if on_dev else None)
    n = int(changes["pk"].shape[0])
    s = L.MatchIn()
    s.n = n
    keep = mem.fill(s, changes, (("pk", np.uint64, n), ("table_cid", np.uint32, n), ("cl", np.uint32, n)))
    keep += mem.fill(s, {"impactful": impactful}, (("impactful", np.uint8, n),))
    rec, ncs, p = _cs_records(cs, ncs, on_dev, mem.dev)
    s.ncs, s.cs = ncs, (p if ncs else None)
    s.nclasses, s.nslots = filters.nclasses, filters.nslots
    bits = filters.device_bits(mem.dev) if on_dev else filters.bits
    s.col_class_bits = mem.ptr(bits)
    tp = TwoPass(L.lib().corro_match_changes, (engine._h, C.byref(s), mem.const), mem, L.MatchOut())
    tp.bind((("class_off", np.uint64, filters.nclasses + 1),))
    mem.sync()
    t0 = time.perf_counter()
    tp.call(0)
    t1 = time.perf_counter()
    tot = tp.totals(("ncand",))
    tp.bind(_OUT, tot)
    mem.sync()
    t2 = time.perf_counter()
    tp.call(1)
    if timings is not None:
        timings["pass0_ms"], timings["pass1_ms"] = (t1 - t0) * 1e3, (time.perf_counter() - t2) * 1e3
    return {**tp.result(), **tot}


def read_candidates(engine, result, values=True):
    """The current rows of a match_changes result's candidates (MergeEngine.read_rows of its "cand_table" /
    "cand_pk"), what handle_candidates (updates.rs:270-305) and the subscription matcher read next: key j
    is candidate j, so "status", "key_cl" and "row_off" line up with the candidate columns. The rows stay on the
    device when the result is there."""
    return engine.read_rows(result["cand_table"], result["cand_pk"], values=values)


def query_candidates(engine, result, table, where=(), columns=(), values=True):
    """Does a changed row still satisfy a subscription's WHERE: the keyed form of MergeEngine.query_rows over
    the candidates of one table in a match_changes result, the step that follows read_candidates for a
    subscription with a predicate. Returns query_rows' result (on the device when the match result is
    there) and "cand_index": the candidate each key stands for, so key_status[j] (1 selected, 3 live but
    rejected, 2 deleted, 0 absent) is the answer for candidate cand_index[j] and the selected rows carry
    the projected columns."""
    t = engine.table_index(table)
    ct, pk = result["cand_table"], result["cand_pk"]
    if _is_torch(pk):
        idx = (ct == t).nonzero().reshape(-1)
        keys = pk[idx].contiguous()
    else:
        idx = np.nonzero(np.asarray(ct) == t)[0]
        keys = np.ascontiguousarray(np.asarray(pk)[idx])
    res = engine.query_rows(t, where, columns, keys=keys, values=values)
    res["cand_index"] = idx
    return res


def _host(a, dt):
    if _is_torch(a):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a).view(dt)


def candidates_by_class(result, filters):
    """Per class the list of (changeset index, {table name: {pk key: cl}}) for the changesets with at
    least one candidate, in order; the dicts are insertion-ordered like the reference's IndexMaps."""
    off = _host(result["class_off"], np.uint64).tolist()
    cs = _host(result["cand_cs"], np.uint32).tolist()
    table = _host(result["cand_table"], np.uint32).tolist()
    pk = _host(result["cand_pk"], np.uint64).tolist()
    cl = _host(result["cand_cl"], np.uint32).tolist()
    out = []
    for c in range(filters.nclasses):
        per = []
        for j in range(off[c], off[c + 1]):
            if not per or per[-1][0] != cs[j]:
                per.append((cs[j], {}))
            per[-1][1].setdefault(filters.tables[table[j]], {})[pk[j]] = cl[j]
        out.append(per)
    return out


def candidates_by_handle(result, filters):
    """Per handle (subs first, then updates) what match_changes sends it: a list of (changeset index,
    MatchCandidates) over the changesets that gave it a candidate. Handles of one class share their list."""
    per_class = candidates_by_class(result, filters)
    return [per_class[c] for c in filters.handle_class]


def notify_events(result, filters):
    """handle_candidates over candidates_by_handle: per handle a list of (changeset index, [(Update |
    Delete, pk key)]), an even cl a Delete and any other an Update, tables then pks in map order."""
    return [[(s, [(DELETE if cl % 2 == 0 else UPDATE, pk) for pks in cands.values() for pk, cl in pks.items()])
             for s, cands in per] for per in candidates_by_handle(result, filters)]


def match_extracted(engine, rows, filters):
    """match_changes_from_db_version (updates.rs:483-536), the form process_fully_buffered_changes calls
    (util.rs:668-684): `rows` are the crsql_changes rows of one extract_changes group in seq order ("pk",
    "table_cid", "cl"; CUDA tensors, or numpy arrays that are uploaded). They run as one changeset with
    every flag 1; cl (int64 in extracted rows) is cast to u32 on the device. Returns match_changes' result
    on the device."""
    import torch
    cols = {}
    for k in ("pk", "table_cid", "cl"):
        a = rows[k]
        if not _is_torch(a):
            a = np.ascontiguousarray(a)
            a = torch.from_numpy(a.view({8: np.int64, 4: np.int32}[a.dtype.itemsize])).to(f"cuda:{engine.device}")
        cols[k] = a.contiguous()
    cols["cl"] = cols["cl"].to(torch.int32)
    n = int(cols["pk"].shape[0])
    dev = cols["pk"].device
    imp = torch.ones(n, dtype=torch.uint8, device=dev)
    cs = torch.tensor([[0, n]], dtype=torch.int64, device=dev)
    return match_changes(engine, cols, imp, cs, filters, device=True)


_SUB_TOTALS = ("nevents", "ninsert", "nupdate", "ndelete", "val_data_len")
_SUB_EVENTS = (("type", np.uint8, "nevents"), ("rowid", np.uint64, "nevents"), ("change_id", np.uint64, "nevents"),
               ("pk", np.uint64, "nevents"))
_SUB_ROWS = (("rowid", np.uint64, "nrows"), ("pk", np.uint64, "nrows"))
_SUB_CELLS = (("val_type", np.uint8, "ncells"), ("val_len", np.uint8, "ncells"), ("val0", np.uint64, "ncells"),
              ("val1", np.uint64, "ncells"), ("val_off", np.uint64, "ncells"), ("val_size", np.uint32, "ncells"))
_SUB_DATA = (("val_data", np.uint8, "val_data_len"),)
INSERT = "Insert"
EVENT_TYPES = (INSERT, UPDATE, DELETE)                 # by corro_sub_events.type


class Subscription:
    """One subscription's materialised result set on the device (corro_sub_create): SELECT columns FROM table
    WHERE where, with MergeEngine.query_rows' spelling of where and columns (at least one column). The set is
    filled from the table as it is now -- rowids 1..n in ascending row key, no events -- and advanced by
    update / handle_candidates. row_cap (rows) and val_cap (bytes of long values) are starting sizes, 0 a
    default; the store grows on its own. Close it before its engine."""

    def __init__(self, engine, table, where=(), columns=(), row_cap=0, val_cap=0):
        self.engine, self.table = engine, engine.table_index(table)
        s, keep, mem, _nkeys, self.nproj = engine.query_prepare(table, where, columns, values=False)
        h = C.c_void_p()
        L.check(L.lib().corro_sub_create(engine._h, C.byref(s), mem.const, int(row_cap), int(val_cap), C.byref(h)))
        del keep
        self._h = h

    def close(self):
        if self._h:
            L.lib().corro_sub_destroy(self._h)
            self._h = None

    def _shaped(self, res, rows, mem):
        for k, _dt, _size in _SUB_CELLS:
            res[k] = res[k].reshape(rows, self.nproj)
        if not mem.on_dev:
            raw, off, size = res["val_data"].tobytes(), res["val_off"].reshape(-1), res["val_size"].reshape(-1)
            res["long_values"] = {int(i): raw[int(off[i]):int(off[i]) + int(size[i])] for i in np.nonzero(size)[0]}
        return res

    def two_pass(self, keys):
        """The TwoPass of corro_sub_update over `keys`, for a caller that runs the passes itself (tests,
        bench_sub.py), and the key array to keep alive."""
        if not _is_torch(keys):
            keys = np.ascontiguousarray(keys, np.uint64)
        mem = Mem.of(keys)
        a, p = mem.field(keys, np.uint64, "keys")
        return TwoPass(L.lib().corro_sub_update, (self._h, p, mem.count(a), mem.const), mem, L.SubEvents()), a

    def update(self, keys):
        """Advance the set by the candidate row keys (corro_sub_update, both passes): a numpy array for host
        results, a CUDA tensor for device results (only the totals reach the host). A key listed twice counts
        once. Returns the events, first the Inserts and Updates in ascending row key, then the Deletes in
        ascending rowid: "type" (0 Insert, 1 Update, 2 Delete), "rowid", "change_id" and "pk" per event, the
        cells "val_type", "val_len", "val0", "val1", "val_off", "val_size" shaped (nevents, nproj), "val_data",
        and the totals "nevents", "ninsert", "nupdate", "ndelete", "val_data_len". Host results also carry
        "long_values": {flat cell index: bytes}."""
        tp, keep = self.two_pass(keys)
        tp.run(0)
        tot = tp.totals(_SUB_TOTALS)
        tot["ncells"] = tot["nevents"] * self.nproj
        tp.run(1, _SUB_EVENTS + _SUB_CELLS + _SUB_DATA, tot)
        del keep
        return self._shaped({**tp.result(), **tot}, tot["nevents"], tp.mem)

    def handle_candidates(self, result, cls):
        """update over class `cls`'s candidates of this subscription's table in a match_changes result. On the
        device the candidate columns stay there; the host reads the class's two offsets and, through the
        table filter's nonzero(), the number of keys it keeps (one more synchronisation)."""
        off = result["class_off"][cls:cls + 2]
        a, b = (int(x) for x in (off.cpu().tolist() if _is_torch(off) else np.asarray(off).tolist()))
        ct, pk = result["cand_table"][a:b], result["cand_pk"][a:b]
        if _is_torch(pk):
            keys = pk[(ct == self.table).nonzero().reshape(-1)].contiguous()
        else:
            keys = np.ascontiguousarray(np.asarray(pk)[np.asarray(ct) == self.table])
        return self.update(keys)

    STAGES = ("dedup", "query", "classify", "order_sizes", "fill_gather", "commit")

    def last_timings(self):
        """ms per stage of the last update, per pass ({0: {...}, 1: {...}}), taken while the engine's
        set_profiling is on (corro_sub_last_timings): device events at the stage boundaries, the waits and
        the host's reads of the totals between the kernels included. Pass 0 ends after "order_sizes"."""
        out = {}
        for which in (0, 1):
            arr, n = (C.c_float * L.CORRO_SUB_STAGES)(), C.c_uint32()
            L.check(L.lib().corro_sub_last_timings(self._h, which, arr, L.CORRO_SUB_STAGES, C.byref(n)))
            out[which] = {self.STAGES[k]: float(arr[k]) for k in range(n.value)}
        return out

    def rows(self, device=False):
        """The set in ascending rowid (corro_sub_rows): "nrows", "rowid" and "pk" per row, the cells shaped
        (nrows, nproj) and the long values as in update; CUDA tensors with device=True."""
        mem = Mem(f"cuda:{self.engine.device}") if device else Mem()
        tp = TwoPass(L.lib().corro_sub_rows, (self._h, mem.const), mem, L.SubRowsOut())
        tp.run(0)
        tot = tp.totals(("nrows", "val_data_len"))
        tot["ncells"] = tot["nrows"] * self.nproj
        tp.run(1, _SUB_ROWS + _SUB_CELLS + _SUB_DATA, tot)
        return self._shaped({**tp.result(), **tot}, tot["nrows"], mem)
