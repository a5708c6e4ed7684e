"""MergeEngine: the device-resident replacement of cr-sqlite's `crsql_changes` merge.

One MergeEngine corresponds to one corrosion writer connection with the CRR schema applied
(corro-types/src/agent.rs:480-482 single writer; schema.rs:362-363 crsql_as_crr). `apply` is the
batched form of the per-change loop in process_complete_version
(/root/reference/crates/corro-agent/src/agent/util.rs:1222-1262): changes are applied in index
order, exactly as consecutive `INSERT INTO crsql_changes` statements would be.
"""
import ctypes as C

import numpy as np

from . import _lib as L
from ._twopass import Mem, TwoPass, _int_dtype_ok, _is_torch, two_pass

BATCH_FIELDS = {"pk": np.uint64, "table_cid": np.uint32, "col_version": np.int64,
                "db_version": np.int64, "cl": np.uint32, "seq": np.uint32, "site": np.uint32,
                "val0": np.uint64, "val1": np.uint64, "val_type": np.uint8, "val_len": np.uint8,
                "ts": np.uint64, "val_off": np.uint64, "val_size": np.uint32}
VAL_LONG = L.CORRO_VAL_LONG  # val_len of a TEXT/BLOB value longer than 16 bytes (bytes in "val_data")
LONG_FIELDS = ("val_off", "val_size")
FIXED_FIELDS = {k: v for k, v in BATCH_FIELDS.items() if k not in LONG_FIELDS}
REQUIRED = ("pk", "table_cid", "col_version", "db_version", "cl", "seq", "site", "val0")
ROW_FIELDS = {"pk": np.uint64, "table_cid": np.uint32, "col_version": np.int64,
              "db_version": np.int64, "cl": np.int64, "seq": np.uint32, "site": np.uint32,
              "ts": np.uint64, "val0": np.uint64, "val1": np.uint64, "val_type": np.uint8,
              "val_len": np.uint8}


# corro_encode_in's span arrays: what need_spans and buffered_spans return and encode_changesets takes
SPAN_FIELDS = (("site", np.uint32), ("version", np.int64), ("last_seq", np.uint64), ("ts", np.uint64),
               ("seq_start", np.uint64), ("seq_end", np.uint64), ("row_off", np.uint64), ("row_count", np.uint64))
SPAN_KEYS = tuple(k for k, _dt in SPAN_FIELDS)
# pass-1 output tables (see _twopass): name, dtype, the total that sizes it, and where needed mul, extra
_SPANS_OUT = tuple((k, dt, "nspans") for k, dt in SPAN_FIELDS)
_ENC_OUT = (("buf", np.uint8, "nbytes"), ("frame_off", np.uint64, "nframes", 1, 1),
            ("frame_seq_start", np.uint64, "nframes"), ("frame_seq_end", np.uint64, "nframes"),
            ("frame_row_off", np.uint64, "nframes"), ("frame_rows", np.uint32, "nframes"))
_REQDEC_OUT = (("pair_actor", np.uint8, "npairs", 16, 0), ("pair_site", np.uint32, "npairs"),
               ("pair_need_off", np.uint64, "npairs", 1, 1), ("kind", np.uint8, "nneeds"),
               ("start", np.uint64, "nneeds"), ("end", np.uint64, "nneeds"), ("sr_off", np.uint64, "nneeds"),
               ("sr_n", np.uint64, "nneeds"), ("s_start", np.uint64, "nseqs"), ("s_end", np.uint64, "nseqs"),
               ("need_site", np.uint32, "nneeds"), ("need_keep", np.uint8, "nneeds"),
               ("need_ent_off", np.uint64, "nneeds", 1, 1), ("ent_site", np.uint32, "nents"),
               ("ent_start", np.uint64, "nents"), ("ent_end", np.uint64, "nents"),
               ("ent_seq_start", np.uint32, "nents"), ("ent_seq_end", np.uint32, "nents"),
               ("ent_need", np.uint64, "nents"))


# corro_read_out: the per-key arrays of pass 0, the per-row arrays of pass 1
_READ_PRE = (("status", np.uint8, "n"), ("cl", np.int64, "n"), ("row_off", np.uint64, "n", 1, 1))
_READ_ROWS = tuple(("rows." + k, dt, "nrows") for k, dt in ROW_FIELDS.items())
_READ_LONG = (("val_off", np.uint64, "nrows"), ("val_size", np.uint32, "nrows"), ("val_data", np.uint8, "val_data_len"))


# corro_query_out: the per-row and per-cell arrays of pass 1
_QUERY_ROWS = (("pk", np.uint64, "nrows"), ("cl", np.int64, "nrows"))
_QUERY_CELLS = (("val_type", np.uint8, "ncells"), ("val_len", np.uint8, "ncells"), ("val0", np.uint64, "ncells"),
                ("val1", np.uint64, "ncells"))
_QUERY_LONG = (("val_off", np.uint64, "ncells"), ("val_size", np.uint32, "ncells"), ("val_data", np.uint8, "val_data_len"))
_QUERY_TERMS = (("term_col", np.uint32), ("term_op", np.uint8), ("val_type", np.uint8), ("val_len", np.uint8),
                ("val0", np.uint64), ("val1", np.uint64), ("const_off", np.uint64), ("const_size", np.uint32))


def value_cell(v):
    """A Python value (None, int, float, str, bytes) as the cell the engine stores: (val_type, val_len, val0,
    val1, the bytes of a long value or None). TEXT / BLOB up to 16 bytes lie big-endian in val0 / val1; a
    longer one has val_len VAL_LONG, its first 8 bytes in val0 and its bytes apart."""
    if v is None:
        return (5, 0, 0, 0, None)
    if isinstance(v, (bool, int, np.integer)):
        return (1, 0, int(v) & 0xFFFFFFFFFFFFFFFF, 0, None)
    if isinstance(v, (float, np.floating)):
        return (2, 0, int.from_bytes(np.float64(v).tobytes(), "little"), 0, None)
    ty = 3 if isinstance(v, str) else 4
    b = v.encode() if isinstance(v, str) else bytes(v)
    if len(b) > 16:
        return (ty, VAL_LONG, int.from_bytes(b[:8], "big"), 0, b)
    p = b + b"\0" * (16 - len(b))
    return (ty, len(b), int.from_bytes(p[:8], "big"), int.from_bytes(p[8:], "big"), None)


def cell_value(ty, ln, v0, v1, raw=None):
    """value_cell's inverse: the Python value of a stored cell (raw: a long value's bytes)."""
    ty, ln, v0, v1 = int(ty), int(ln), int(v0) & 0xFFFFFFFFFFFFFFFF, int(v1) & 0xFFFFFFFFFFFFFFFF
    if ty == 5:
        return None
    if ty == 1:
        return v0 - (1 << 64) if v0 >> 63 else v0
    if ty == 2:
        return float(np.frombuffer(v0.to_bytes(8, "little"), np.float64)[0])
    b = raw if ln == VAL_LONG else (v0.to_bytes(8, "big") + v1.to_bytes(8, "big"))[:ln]
    return b.decode() if ty == 3 else bytes(b)


def query_values(res):
    """The cells of a host query_rows(values=True) result as Python values: one list per selected row."""
    n, m = res["val_type"].shape
    lv = res["long_values"]
    return [[cell_value(res["val_type"][r, j], res["val_len"][r, j], res["val0"][r, j], res["val1"][r, j], lv.get(r * m + j))
             for j in range(m)] for r in range(n)]


def rows_as_batch(rows):
    """The rows of a read_rows(values=True) result as a batch apply() takes, in the same memory. Every
    array is passed as it is but cl: corro_rows carries it as int64, corro_changes as uint32."""
    cl = rows["cl"]
    if _is_torch(cl):
        import torch
        cl = cl.to(torch.int32)
    else:
        cl = np.asarray(cl).astype(np.uint32)
    batch = {k: rows[k] for k in FIXED_FIELDS if k != "cl"}
    batch["cl"] = cl
    if "val_data" in rows and Mem.of(rows["val_data"]).count(rows["val_data"]):
        batch.update({k: rows[k] for k in LONG_FIELDS + ("val_data",)})
    return batch


class MergeEngine:
    def __init__(self, schema, capacity_hint=1 << 20, device=0, interned=()):
        """schema: {table_name: [column names]} in table order (cid k = column k-1, cid 0 = '-1').
        interned: tables whose primary key is not one INTEGER column (BLOB / TEXT / composite pks):
        their rows are keyed by corro_pk_keys' interned ids of the packed pk bytes."""
        lib = L.lib()
        self.schema = list(schema.items())
        descs = (L.TableDesc * max(1, len(self.schema)))()
        self._keep = []
        for i, (name, cols) in enumerate(self.schema):
            arr = (C.c_char_p * max(1, len(cols)))(*[c.encode() for c in cols])
            self._keep.append(arr)
            descs[i].name = name.encode()
            descs[i].ncols = len(cols)
            descs[i].col_names = C.cast(arr, C.POINTER(C.c_char_p))
        h = C.c_void_p()
        L.check(lib.corro_ctx_create(descs, len(self.schema), capacity_hint, device, C.byref(h)))
        self._h = h
        self.device = device
        self.interned = set()
        for name in interned:
            self.set_pk_interned(name)

    def close(self):
        if getattr(self, "_h", None):
            L.lib().corro_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    # ---- schema / sites -------------------------------------------------------------------
    def lookup(self, table, cid):
        out = C.c_uint32()
        L.check(L.lib().corro_lookup_cid(self._h, table.encode(), cid.encode(), C.byref(out)))
        return out.value

    def register_sites(self, site_ids):
        ids = np.ascontiguousarray(site_ids, dtype=np.uint8).reshape(-1, 16)
        ords = np.zeros(max(1, ids.shape[0]), np.uint32)
        L.check(L.lib().corro_site_register(self._h, ids.ctypes.data, ids.shape[0], ords.ctypes.data))
        return ords[: ids.shape[0]]

    def site_ids(self):
        """Registered 16-byte site ids by ordinal (crsql_site_id)."""
        c = C.c_uint32()
        L.check(L.lib().corro_site_ids(self._h, None, 0, C.byref(c)))
        buf = np.zeros(max(1, 16 * c.value), np.uint8)
        L.check(L.lib().corro_site_ids(self._h, buf.ctypes.data, c.value, C.byref(c)))
        return [bytes(buf[16 * i:16 * i + 16]) for i in range(c.value)]

    def site_count(self):
        c = C.c_uint32()
        L.check(L.lib().corro_site_count(self._h, C.byref(c)))
        return c.value

    # ---- primary keys ---------------------------------------------------------------------
    def table_index(self, table):
        if isinstance(table, int):
            return table
        for i, (name, _cols) in enumerate(self.schema):
            if name == table:
                return i
        raise L.CorroError(-4, f"no such table: {table}")

    def set_pk_interned(self, table, on=True):
        t = self.table_index(table)
        L.check(L.lib().corro_table_set_pk_interned(self._h, t, 1 if on else 0))
        name = self.schema[t][0]
        (self.interned.add if on else self.interned.discard)(name)

    # ---- metrics -----------------------------------------------------------------------------
    def metrics(self):
        """Cumulative counters (corro_ctx_metrics) as a dict."""
        m = L.Metrics()
        L.check(L.lib().corro_ctx_metrics(self._h, C.byref(m)))
        return {k: getattr(m, k) for k, _ in L.Metrics._fields_}

    def committed(self, table):
        """corro.changes.committed for one table (corro_table_committed)."""
        c = C.c_uint64()
        L.check(L.lib().corro_table_committed(self._h, self.table_index(table), C.byref(c)))
        return c.value

    # ---- column affinity -------------------------------------------------------------------
    def set_column_types(self, table, decl_types):
        """Register the table's declared column types (one per non-pk column, in cid order): their
        SQLite affinities (corro_affinity_of_type) make the engine store each winning value as the
        affinity converts it, as SQLite's base table does (corro_table_set_affinity)."""
        t = self.table_index(table)
        aff = np.array([L.lib().corro_affinity_of_type(str(d).encode()) for d in decl_types], np.uint8)
        L.check(L.lib().corro_table_set_affinity(self._h, t, aff.ctypes.data if len(aff) else None, len(aff)))

    AFFINITY_POLICIES = {"portable": 0, "sqlite-3.37.2": 1}

    def set_affinity_policy(self, policy):
        """"sqlite-3.37.2" (default): convert every value exactly as SQLite 3.37.2 does, never refusing a
        change (as SQLite does), and count the conversions whose stored form may differ in another SQLite
        version (metrics()["aff_sensitive"]). "portable" (strict, opt-in): convert only values whose
        stored form is the same in every SQLite version with correctly rounded conversions, refuse a
        batch holding any other (CorroError, CORRO_E_RANGE, before any write)
        (corro_set_affinity_policy)."""
        L.check(L.lib().corro_set_affinity_policy(self._h, self.AFFINITY_POLICIES[policy]))

    def pk_keys(self, table, packed):
        """Row keys of packed pks (a list of bytes, pack_columns encoding) of one table."""
        t = self.table_index(table)
        lens = np.array([len(b) for b in packed], np.uint64)
        off = np.zeros(len(packed) + 1, np.uint64)
        off[1:] = np.cumsum(lens)
        buf = np.frombuffer(b"".join(bytes(b) for b in packed) or b"\0", np.uint8)
        keys = np.zeros(max(1, len(packed)), np.uint64)
        L.check(L.lib().corro_pk_keys(self._h, t, buf.ctypes.data, off.ctypes.data, len(packed), keys.ctypes.data))
        return keys[:len(packed)]

    def pk_keys_device(self, table, data, off):
        """Row keys of n packed pks held in device memory: `data` a uint8 CUDA tensor of the packed
        bytes, `off` an int64 CUDA tensor of n + 1 offsets into it (corro_pk_keys_device: interned in
        the HBM intern table, nothing crosses PCIe). Returns an int64 CUDA tensor of n keys (uint64
        bits)."""
        import torch
        t = self.table_index(table)
        n = int(off.numel()) - 1
        keys = torch.empty(max(n, 1), dtype=torch.int64, device=off.device)
        torch.cuda.current_stream().synchronize()
        L.check(L.lib().corro_pk_keys_device(self._h, t, data.data_ptr(), off.data_ptr(), n, keys.data_ptr()))
        return keys[:n]

    def pk_find(self, table, packed):
        """pk_keys that only looks (corro_pk_find): the row keys of packed pks, L.CORRO_PK_ABSENT for a
        key an interned table does not hold; the intern table is left as it was. packed: a list of bytes
        (a numpy array of keys comes back), or (data, off) CUDA tensors as pk_keys_device takes them
        (corro_pk_find_device; an int64 CUDA tensor comes back, CORRO_PK_ABSENT reading -1)."""
        t = self.table_index(table)
        if isinstance(packed, tuple):
            import torch
            data, off = packed
            n = int(off.numel()) - 1
            keys = torch.empty(max(n, 1), dtype=torch.int64, device=off.device)
            torch.cuda.current_stream().synchronize()
            L.check(L.lib().corro_pk_find_device(self._h, t, data.data_ptr(), off.data_ptr(), n, keys.data_ptr()))
            return keys[:n]
        lens = np.array([len(b) for b in packed], np.uint64)
        off = np.zeros(len(packed) + 1, np.uint64)
        off[1:] = np.cumsum(lens)
        buf = np.frombuffer(b"".join(bytes(b) for b in packed) or b"\0", np.uint8)
        keys = np.zeros(max(1, len(packed)), np.uint64)
        L.check(L.lib().corro_pk_find(self._h, t, buf.ctypes.data, off.ctypes.data, len(packed), keys.ctypes.data))
        return keys[:len(packed)]

    def pk_count(self, table):
        """Keys the table's intern table holds (corro_pk_count); 0 for a table keyed by its INTEGER pk."""
        c = C.c_uint64()
        L.check(L.lib().corro_pk_count(self._h, self.table_index(table), C.byref(c)))
        return c.value

    def pk_bytes(self, table, keys):
        """Canonical packed pk bytes of row keys of one table."""
        t = self.table_index(table)
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        n = len(keys)
        off = np.zeros(n + 1, np.uint64)
        cap = 64 * n + 64
        while True:
            buf = np.zeros(cap, np.uint8)
            rc = L.lib().corro_pk_bytes(self._h, t, keys.ctypes.data, n, buf.ctypes.data, cap, off.ctypes.data)
            if rc == 0:
                break
            if rc != -6 or int(off[n]) <= cap:
                L.check(rc)
            cap = int(off[n])
        raw = buf.tobytes()
        return [raw[int(off[i]):int(off[i + 1])] for i in range(n)]

    # ---- merge ------------------------------------------------------------------------------
    def apply(self, batch, impact=False):
        """Merge a batch (dict of numpy arrays on the host, or of torch tensors on the GPU).

        Returns the per-change crsql_rows_impacted() growth when impact=True (a numpy array for a
        host batch, a CUDA uint8 tensor for a device batch), else None."""
        return self.apply_prepared(self.prepare(batch, impact))

    def prepare(self, batch, impact=False):
        """Validate a batch and build its C-ABI descriptor (pointers and sizes only) once, so that
        a caller applying the same resident buffers repeatedly (bench.py) pays no per-call
        marshalling; the arrays must stay alive and unchanged in shape while the result is used."""
        for k in REQUIRED:
            if k not in batch or batch[k] is None:
                raise ValueError(f"batch lacks required field {k!r}")
        s = L.Changes()
        keep = []
        on_dev = _is_torch(batch["pk"])
        n = int(batch["pk"].shape[0])
        s.n = n
        for k, dt in BATCH_FIELDS.items():
            a = batch.get(k)
            if a is None:
                setattr(s, k, None)
                continue
            if on_dev:
                if not a.is_cuda or not a.is_contiguous() or not _int_dtype_ok(a, dt):
                    raise ValueError(f"device field {k} must be a contiguous CUDA integer tensor of {np.dtype(dt)} width "
                                     f"(got {a.dtype})")
                if int(a.shape[0]) != n:
                    raise ValueError(f"field {k} has {a.shape[0]} elements, expected {n}")
                setattr(s, k, a.data_ptr() if n else None)
            else:
                a = np.ascontiguousarray(a, dtype=dt)
                if a.shape[0] != n:
                    raise ValueError(f"field {k} has {a.shape[0]} elements, expected {n}")
                keep.append(a)
                setattr(s, k, a.ctypes.data if n else None)
        data = batch.get("val_data")  # long values' bytes (val_off / val_size index them)
        if data is not None:
            if on_dev:
                if not data.is_cuda or not data.is_contiguous() or data.dtype != __import__("torch").uint8:
                    raise ValueError("device val_data must be a contiguous CUDA uint8 tensor")
                s.val_data, s.val_data_len = (data.data_ptr() if data.numel() else None), int(data.numel())
            else:
                data = np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else \
                    np.ascontiguousarray(data, dtype=np.uint8)
                keep.append(data)
                s.val_data, s.val_data_len = (data.ctypes.data if data.size else None), int(data.size)
        out = L.ApplyOut()
        imp = None
        if impact:
            if on_dev:  # device batch -> device impact flags (written in place, no copy)
                import torch
                imp = torch.zeros(max(n, 1), dtype=torch.uint8, device=batch["pk"].device)
                out.impact = imp.data_ptr()
            else:
                imp = np.zeros(max(n, 1), np.uint8)
                out.impact = imp.ctypes.data
        return (s, out, keep, imp, n, on_dev, impact)

    def apply_prepared(self, prep):
        """corro_apply_batch on a descriptor from prepare() (a fresh impact buffer is not made:
        the prepared one is overwritten)."""
        s, out, _keep, imp, n, on_dev, impact = prep
        if on_dev:
            import torch
            torch.cuda.current_stream().synchronize()  # the producer's work on torch's stream
        L.check(L.lib().corro_apply_batch(self._h, C.byref(s), L.CORRO_MEM_DEVICE if on_dev else L.CORRO_MEM_HOST,
                                          C.byref(out)))
        return imp[:n] if impact else None

    def count(self):
        c = C.c_uint64()
        L.check(L.lib().corro_state_count(self._h, C.byref(c)))
        return c.value

    def reset(self):
        L.check(L.lib().corro_state_reset(self._h))

    def export(self):
        """crsql_changes rows (unspecified order) as a dict of numpy arrays."""
        m = self.count()
        out = {k: np.zeros(max(m, 1), dt) for k, dt in ROW_FIELDS.items()}
        r = L.Rows()
        for k, a in out.items():
            setattr(r, k, a.ctypes.data)
        w = C.c_uint64()
        L.check(L.lib().corro_state_export(self._h, C.byref(r), max(m, 1), C.byref(w)))
        rows = {k: a[: w.value] for k, a in out.items()}
        rows["long_values"] = self.long_values(rows)
        return rows

    def read_rows(self, tables, pks, values=True, flags=None):
        """The current rows of the keys (tables[i], pks[i]) in request order (corro_read_rows): table
        indices and row keys as numpy arrays (host results) or CUDA tensors (device results; only totals
        reach the host) -- a match_changes result's "cand_table" / "cand_pk" as they are. Returns "status"
        (0 absent, 1 live, 2 deleted), "key_cl" (corro_read_out.cl) and "row_off" (n + 1) per key, the
        crsql_changes columns of export() per row -- key i owns rows [row_off[i], row_off[i + 1]), sentinel first, then by cid --
        "nrows", and with values the long values' "val_off" / "val_size" / "val_data" and "val_data_len"
        (rows_as_batch turns such a result into a batch for another engine). Host results also carry
        "long_values" like export(). flags overrides the flag word (tests)."""
        mem = Mem.of(pks)
        s = L.ReadIn()
        n = mem.count(pks)
        s.n = n
        s.flags = (L.CORRO_READ_VALUES if values else 0) if flags is None else flags
        keep = mem.fill(s, {"table": tables, "pk": pks}, (("table", np.uint32, n), ("pk", np.uint64, n)))
        post = _READ_ROWS + (_READ_LONG if s.flags & L.CORRO_READ_VALUES else ())
        res = two_pass(L.lib().corro_read_rows, (self._h, C.byref(s), mem.const), mem, L.ReadOut(),
                       tuple((k, dt, n, *me) for k, dt, _n, *me in _READ_PRE), ("nrows", "val_data_len"), post)
        del keep
        res["key_cl"] = res.pop("cl")      # (the rows' own "cl" column keeps the name, as in export())
        res = {(k[5:] if k.startswith("rows.") else k): a for k, a in res.items()}
        if not mem.on_dev:
            if "val_data" in res:
                raw, off, size = res["val_data"].tobytes(), res["val_off"], res["val_size"]
                res["long_values"] = {int(i): raw[int(off[i]):int(off[i]) + int(size[i])] for i in np.nonzero(size)[0]}
            else:
                res["long_values"] = self.long_values(res)
        return res

    def query_prepare(self, table, where=(), columns=(), keys=None, values=True, device=False):
        """corro_query_in for query_rows' arguments: (struct, arrays to keep alive, Mem, nkeys, nproj). The
        arrays live where the keys do (numpy: host; CUDA tensors: device), or for the table form on the
        host unless device is set. For a caller that runs the passes itself (bench_query.py)."""
        t = self.table_index(table)
        if not 0 <= t < len(self.schema):
            raise L.CorroError(-4, f"no such table: {table}")
        cols = self.schema[t][1]

        def cid(c):
            return 0 if c == "pk" else cols.index(c) + 1

        q = {k: [] for k, _dt in _QUERY_TERMS}
        group_off, data = [0], b""
        for g in where:
            for col, op, *v in g:
                ty, ln, w0, w1, b = value_cell(v[0] if v else None)
                q["term_col"].append(cid(col))
                q["term_op"].append(L.QUERY_OPS[" ".join(op.lower().split())])
                q["val_type"].append(ty), q["val_len"].append(ln), q["val0"].append(w0), q["val1"].append(w1)
                q["const_off"].append(len(data)), q["const_size"].append(len(b) if b else 0)
                data += b or b""
            group_off.append(len(q["term_col"]))
        q = {k: np.array(q[k], dt) for k, dt in _QUERY_TERMS}
        q["group_off"] = np.array(group_off if where else [], np.uint32)
        q["proj"] = np.array([cid(c) for c in columns], np.uint32)
        q["const_data"] = np.frombuffer(data, np.uint8)
        flags = (L.CORRO_QUERY_KEYED if keys is not None else 0) | (L.CORRO_QUERY_VALUES if values else 0)
        dts = dict(_QUERY_TERMS + (("group_off", np.uint32), ("proj", np.uint32), ("const_data", np.uint8)))
        q = {k: np.ascontiguousarray(a, dts[k]) for k, a in q.items()}
        on_dev = _is_torch(keys) if keys is not None else bool(device)
        mem = Mem((keys.device if keys is not None else f"cuda:{self.device}")) if on_dev else Mem()
        if on_dev:
            import torch
            signed = {1: np.uint8, 4: np.int32, 8: np.int64}
            q = {k: torch.from_numpy(a.view(signed[a.dtype.itemsize]).copy()).to(mem.dev) for k, a in q.items()}
        s = L.QueryIn()
        s.table, s.flags = t, flags
        s.nterms, s.nproj = mem.count(q["term_col"]), mem.count(q["proj"])
        s.ngroups = max(mem.count(q["group_off"]) - 1, 0)
        s.const_data_len = mem.count(q["const_data"])
        keep = mem.fill(s, q, [(k, dt, None) for k, dt in dts.items()])
        nkeys = 0
        if keys is not None:
            nkeys = mem.count(keys)
            keep += mem.fill(s, {"keys": keys}, (("keys", np.uint64, nkeys),))
            s.nkeys = nkeys
        return s, keep, mem, nkeys, int(s.nproj)

    def query_rows(self, table, where=(), columns=(), keys=None, values=True, device=False):
        """SELECT columns FROM table WHERE where over the live rows of the merged state (corro_query_rows).
        where: a list of groups, each a list of (column name or "pk", op, Python value) -- ops = != <> < <=
        > >= and (without a value) "is null" / "is not null"; a row is selected when every term of some
        group holds, and an empty where selects every live row. columns: the projected names, "pk" for the
        row key. The comparison is SQLite's, the constants converted by the columns' registered affinities
        (set_column_types). keys=None: the whole table in ascending row key (numpy results; CUDA tensors
        with device=True). keys: the keyed form over these row keys in request order -- a numpy array for
        host results, a CUDA tensor for device results (only the totals reach the host).
        Returns "nrows", "pk" and "cl" per selected row, the cells "val_type", "val_len", "val0", "val1"
        shaped (nrows, nproj), for the keyed form "key_status" per key (0 absent, 1 selected, 2 deleted,
        3 live but rejected) and "key_index" per row, and with values the long values' "val_off" /
        "val_size" (per cell) / "val_data" and "val_data_len". Host results with values also carry
        "long_values": {flat cell index: bytes} (query_values turns the cells into Python values)."""
        s, keep, mem, nkeys, nproj = self.query_prepare(table, where, columns, keys, values, device)
        keyed = bool(s.flags & L.CORRO_QUERY_KEYED)
        tp = TwoPass(L.lib().corro_query_rows, (self._h, C.byref(s), mem.const), mem, L.QueryOut())
        tp.run(0, (("key_status", np.uint8, nkeys),) if keyed else ())
        tot = tp.totals(("nrows", "val_data_len"))
        tot["ncells"] = tot["nrows"] * nproj
        post = _QUERY_ROWS + _QUERY_CELLS + ((("key_index", np.uint32, "nrows"),) if keyed else ())
        tp.run(1, post + (_QUERY_LONG if s.flags & L.CORRO_QUERY_VALUES else ()), tot)
        del keep
        res = {**tp.result(), **tot}
        for k, _dt, size in _QUERY_CELLS + _QUERY_LONG[:2]:
            if k in res:
                res[k] = res[k].reshape(tot["nrows"], nproj)
        if not mem.on_dev and "val_data" in res:
            raw_bytes, off, size = res["val_data"].tobytes(), res["val_off"].reshape(-1), res["val_size"].reshape(-1)
            res["long_values"] = {int(i): raw_bytes[int(off[i]):int(off[i]) + int(size[i])] for i in np.nonzero(size)[0]}
        return res

    def local_bound(self, kind, table, cell_off):
        """An upper bound of the rows one local_write of these ops returns (corro_local_bound; host arrays)."""
        kind = np.ascontiguousarray(kind, np.uint8)
        table = np.ascontiguousarray(table, np.uint32)
        cell_off = np.ascontiguousarray(cell_off, np.uint64)
        b = C.c_uint64()
        L.check(L.lib().corro_local_bound(self._h, kind.ctypes.data, table.ctypes.data, cell_off.ctypes.data, len(kind),
                                          C.byref(b)))
        return b.value

    def local_write(self, ops, ts, site, bookie=None, actor_id=None, cap=None, val_data_cap=None):
        """One local transaction (corro_local_write): ops = {"kind" u8, "table" u32, "pk" u64, "cell_off" u64
        (nops + 1), "cid" u32, "val0", "val1" u64, "val_type", "val_len" u8 per cell, and for long values
        "val_off", "val_size", "val_data"} as numpy arrays (host) or CUDA tensors (device: only the totals
        reach the host). cap: the capacity of the returned rows (None: ncols + 1 per op over the widest
        table, plus the cells, which bounds any transaction). Returns "version" (the db_version; 0: nothing written),
        "last_seq", "nrows", the crsql_changes columns of the version's surviving changes in ascending seq
        (what encode_changesets takes), "val_off" / "val_size" / "val_data" / "val_data_len" and
        "op_result" per op. bookie / actor_id: the Bookie that books the version."""
        mem = Mem.of(ops["pk"])
        nops, ncells = mem.count(ops["pk"]), mem.count(ops["cid"])
        s = L.LocalIn()
        s.nops, s.ncells, s.ts, s.site = nops, ncells, int(ts), int(site)
        fields = [("kind", np.uint8, nops), ("table", np.uint32, nops), ("pk", np.uint64, nops),
                  ("cell_off", np.uint64, nops + 1), ("cid", np.uint32, ncells), ("val0", np.uint64, ncells)]
        fields += [(k, dt, ncells) for k, dt in (("val1", np.uint64), ("val_type", np.uint8), ("val_len", np.uint8)) if k in ops]
        dlen = mem.count(ops["val_data"]) if "val_data" in ops else 0
        if dlen:
            fields += [("val_off", np.uint64, ncells), ("val_size", np.uint32, ncells), ("val_data", np.uint8, None)]
            s.val_data_len = dlen
        keep = mem.fill(s, ops, fields)
        if cap is None:
            cap = nops * (max([len(c) for _n, c in self.schema] + [0]) + 1) + ncells
        if val_data_cap is None:
            val_data_cap = dlen + 24 * ncells
        o = L.LocalOut()
        o.cap, o.val_data_cap = cap, val_data_cap
        tp = TwoPass(None, (), mem, o)
        tp.bind(tuple(("rows." + k, dt, cap) for k, dt in ROW_FIELDS.items()) +
                (("val_off", np.uint64, cap), ("val_size", np.uint32, cap), ("val_data", np.uint8, val_data_cap),
                 ("op_result", np.uint8, nops)))
        mem.sync()
        L.check(L.lib().corro_local_write(self._h, bookie._h if bookie is not None else None, actor_id, C.byref(s),
                                          mem.const, C.byref(o)))
        del keep
        n, vb = int(o.nrows), int(o.val_data_len)
        res = {}
        for k, a in tp.result().items():
            k = k[5:] if k.startswith("rows.") else k
            res[k] = a if k == "op_result" else a[:vb] if k == "val_data" else a[:n]
        res.update(version=int(o.db_version), last_seq=int(o.last_seq), nrows=n, val_data_len=vb)
        return res

    def track_touched(self, on=True):
        """List the rows every apply addresses, for export_touched (corro_ctx_track_touched)."""
        L.check(L.lib().corro_ctx_track_touched(self._h, 1 if on else 0))

    def export_touched(self):
        """The complete current clock rows of every row addressed since the previous call
        (corro_state_export_touched): a dict of numpy arrays like export(), rows of one (table, pk)
        contiguous. A host persisting the state replaces each exported row's clock rows with these."""
        lib = L.lib()
        w = C.c_uint64()
        empty = L.Rows()
        rc = lib.corro_state_export_touched(self._h, C.byref(empty), 0, C.byref(w))
        if rc not in (0, -6):
            L.check(rc)
        m = int(w.value)
        out = {k: np.zeros(max(m, 1), dt) for k, dt in ROW_FIELDS.items()}
        if m:
            r = L.Rows()
            for k, a in out.items():
                setattr(r, k, a.ctypes.data)
            L.check(lib.corro_state_export_touched(self._h, C.byref(r), m, C.byref(w)))
        rows = {k: a[: w.value] for k, a in out.items()}
        rows["long_values"] = self.long_values(rows)
        return rows

    def set_store_limit(self, max_heap_records):
        L.check(L.lib().corro_ctx_set_store_limit(self._h, int(max_heap_records)))

    def compact_values(self, dry_run=False):
        """Compact the long-value arena on the device (corro_values_compact): the bytes no present clock
        row names are dropped and every handle is rewritten, so handles taken before the call are
        invalid after it. dry_run only measures. Returns {"live_bytes", "arena_before", "arena_after"}."""
        live, before, after = C.c_uint64(), C.c_uint64(), C.c_uint64()
        L.check(L.lib().corro_values_compact(self._h, 1 if dry_run else 0, C.byref(live), C.byref(before),
                                             C.byref(after)))
        return {"live_bytes": live.value, "arena_before": before.value, "arena_after": after.value}

    def set_values_autocompact(self, min_bytes):
        """Compact the arena at an apply's entry once it holds min_bytes and twice what the previous
        compaction left (corro_ctx_set_values_autocompact; 0 = off). Handles then die at the next apply."""
        L.check(L.lib().corro_ctx_set_values_autocompact(self._h, int(min_bytes)))

    def value_bytes(self, handles):
        """Bytes of long values by their handles (the val1 of rows with val_len == VAL_LONG)."""
        h = np.ascontiguousarray(handles, dtype=np.uint64)
        n = len(h)
        off = np.zeros(n + 1, np.uint64)
        total = int((h & np.uint64(0xFFFFFF)).sum()) if n else 0
        buf = np.zeros(max(total, 1), np.uint8)
        L.check(L.lib().corro_value_bytes(self._h, h.ctypes.data if n else None, n, buf.ctypes.data, total,
                                          off.ctypes.data))
        raw = buf.tobytes()
        return [raw[int(off[i]):int(off[i + 1])] for i in range(n)]

    def long_values(self, rows):
        """{row index: bytes} for the rows (host arrays) that hold a long value."""
        vl = np.asarray(rows["val_len"])
        idx = np.nonzero(vl == VAL_LONG)[0]
        if len(idx) == 0:
            return {}
        vals = self.value_bytes(np.asarray(rows["val1"])[idx])
        return {int(i): v for i, v in zip(idx, vals)}

    def db_versions(self):
        n = self.site_count()
        out = np.zeros(max(n, 1), np.int64)
        L.check(L.lib().corro_db_versions(self._h, out.ctypes.data, n))
        return out[:n]

    # ---- timing (HIP events on the engine stream) ---------------------------------------
    def set_profiling(self, on=True):
        L.check(L.lib().corro_ctx_set_profiling(self._h, 1 if on else 0))

    def last_timings(self, apply_only=True):
        """ms per stage of the last apply: hist, colscan, plan, scatter, merge (fast + general
        kernels), overflow; with apply_only=False also the last sync-need / extraction count and fill
        kernels and the last extraction index build."""
        arr = (C.c_float * 9)()
        n = C.c_uint32()
        L.check(L.lib().corro_last_timings(self._h, arr, 9, C.byref(n)))
        names = ["k_hist", "k_colscan", "k_plan", "k_scatter", "k_merge", "k_merge_ovf"]
        if not apply_only:
            names += ["k_needs_count", "k_needs_fill", "extract_index"]
        return {names[i]: arr[i] for i in range(min(n.value, len(names)))}

    # ---- multi-GPU ingest -----------------------------------------------------------------
    def partition(self, batch, nranks):
        """Stable pk-hash partition of a device batch by owner rank (corro_partition_ranks).
        Returns (partitioned dict of device tensors, per-rank counts list)."""
        import torch
        n = int(batch["pk"].shape[0])
        s, o = L.Changes(), L.Changes()
        s.n = o.n = n
        out = {}
        for k in BATCH_FIELDS:
            a = batch.get(k)
            if a is None:
                setattr(s, k, None)
                setattr(o, k, None)
                continue
            if not a.is_cuda or not a.is_contiguous():
                raise ValueError(f"field {k} must be a contiguous CUDA tensor")
            out[k] = torch.empty_like(a)
            setattr(s, k, a.data_ptr() if n else None)
            setattr(o, k, out[k].data_ptr() if n else None)
        counts = np.zeros(max(1, nranks), np.uint64)
        torch.cuda.current_stream().synchronize()
        L.check(L.lib().corro_partition_ranks(self._h, C.byref(s), nranks, C.byref(o), counts.ctypes.data))
        return out, [int(c) for c in counts[:nranks]]

    def _device_changes(self, batch):
        n = int(batch["pk"].shape[0])
        s = L.Changes()
        s.n = n
        for k, dt in BATCH_FIELDS.items():
            a = batch.get(k)
            if a is None:
                setattr(s, k, None)
                continue
            if not a.is_cuda or not a.is_contiguous() or not _int_dtype_ok(a, dt) or int(a.shape[0]) != n:
                raise ValueError(f"field {k} must be a contiguous CUDA integer tensor of {n} x {np.dtype(dt)} width")
            setattr(s, k, a.data_ptr() if n else None)
        return s

    def partition_packed(self, batch, nranks, with_perm=False):
        """Stable pk-hash partition of a device batch into whole packed records grouped by owner
        rank (corro_partition_packed): returns (uint8 CUDA tensor of n * rec_bytes, rec_bytes,
        per-rank counts, perm or None) -- one tensor, so one all-to-all moves every field."""
        import torch
        s = self._device_changes(batch)
        n = int(s.n)
        rb = C.c_uint32()
        L.check(L.lib().corro_packed_record_bytes(C.byref(s), C.byref(rb)))
        recs = torch.empty(max(n, 1) * rb.value, dtype=torch.uint8, device=batch["pk"].device)
        perm = torch.empty(max(n, 1), dtype=torch.int32, device=batch["pk"].device) if with_perm else None
        counts = np.zeros(max(1, nranks), np.uint64)
        torch.cuda.current_stream().synchronize()
        L.check(L.lib().corro_partition_packed(self._h, C.byref(s), nranks, recs.data_ptr(),
                                               perm.data_ptr() if perm is not None else None, counts.ctypes.data))
        return recs[:n * rb.value], rb.value, [int(c) for c in counts[:nranks]], (perm[:n] if perm is not None else None)

    def partition_var(self, batch, nranks, with_perm=False):
        """The exchange for every table (corro_partition_var): 80-B records grouped by owner rank plus
        the variable-length bytes they ship (canonical pks of interned tables, long values), routed
        by canonical pk bytes for interned tables. Returns (records uint8 tensor, var uint8 tensor,
        per-rank record counts, per-rank byte counts, perm or None)."""
        import torch
        s = self._device_changes(batch)
        data = batch.get("val_data")
        if data is not None:
            s.val_data, s.val_data_len = (data.data_ptr() if data.numel() else None), int(data.numel())
        n = int(s.n)
        dev = batch["pk"].device
        recs = torch.empty(max(n, 1) * 80, dtype=torch.uint8, device=dev)
        perm = torch.empty(max(n, 1), dtype=torch.int32, device=dev) if with_perm else None
        counts = np.zeros(max(1, nranks), np.uint64)
        vcounts = np.zeros(max(1, nranks), np.uint64)
        torch.cuda.current_stream().synchronize()
        lib = L.lib()
        pp = perm.data_ptr() if perm is not None else None
        rc = lib.corro_partition_var(self._h, C.byref(s), nranks, recs.data_ptr(), pp, counts.ctypes.data, None, 0,
                                     vcounts.ctypes.data)
        total = int(vcounts[:nranks].sum())
        var = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
        if rc == -6 and total:
            rc = lib.corro_partition_var(self._h, C.byref(s), nranks, recs.data_ptr(), pp, counts.ctypes.data,
                                         var.data_ptr(), total, vcounts.ctypes.data)
        L.check(rc)
        return (recs[:n * 80], var[:total], [int(c) for c in counts[:nranks]], [int(c) for c in vcounts[:nranks]],
                perm[:n] if perm is not None else None)

    def unpack_var(self, recs, var, src_counts, src_var):
        """Received records + var bytes (concatenated by source rank) -> a device batch with every
        field, val_data = var (corro_unpack_var; interned pks re-keyed on this engine)."""
        import torch
        n = int(recs.numel()) // 80
        dev = recs.device
        tdt = {np.uint64: torch.int64, np.int64: torch.int64, np.uint32: torch.int32, np.uint8: torch.uint8}
        out = {k: torch.empty(max(n, 1), dtype=tdt[dt], device=dev)[:n] for k, dt in BATCH_FIELDS.items()}
        s = L.Changes()
        s.n = n
        for k in BATCH_FIELDS:
            setattr(s, k, out[k].data_ptr() if n else None)
        sc = np.ascontiguousarray(src_counts, np.uint64)
        sv = np.ascontiguousarray(src_var, np.uint64)
        torch.cuda.current_stream().synchronize()
        L.check(L.lib().corro_unpack_var(self._h, recs.data_ptr() if n else None, n,
                                         var.data_ptr() if var.numel() else None, int(var.numel()),
                                         sc.ctypes.data, sv.ctypes.data, len(sc), C.byref(s)))
        out["val_data"] = var
        return out

    # ---- stream-ordered slot exchange (corro_partition_slots / corro_unpack_slots) ------------
    def stream(self):
        """The engine's HIP stream as a torch stream: collectives issued under
        `torch.cuda.stream(engine.stream())` are ordered with the engine's kernels without a host wait."""
        import torch
        if getattr(self, "_tstream", None) is None:
            self._tstream = torch.cuda.ExternalStream(L.lib().corro_ctx_stream(self._h), device=self.device)
        return self._tstream

    def partition_slots(self, batch, nranks, cap, out=None, counts=None, perm=None):
        """Stable pk-hash partition of an INTEGER device batch into fixed slots of `cap` 48-B records
        per destination (corro_partition_slots): returns (uint8 tensor of nranks * cap * 48, int64
        tensor of the true per-destination counts) -- both written on the engine's stream, nothing
        read back (a count past cap means that slot lost records: corro_unpack_slots reports it)."""
        import torch
        s = self._device_changes(batch)
        dev = batch["pk"].device
        if out is None:
            out = torch.empty(nranks * cap * 48, dtype=torch.uint8, device=dev)
        if counts is None:
            counts = torch.empty(nranks, dtype=torch.int64, device=dev)
        L.check(L.lib().corro_partition_slots(self._h, C.byref(s), nranks, cap, out.data_ptr(), counts.data_ptr(),
                                              perm.data_ptr() if perm is not None else None))
        return out, counts

    def apply_slots(self, recs, nsrc, cap, src_counts, impact=False, overflow=None):
        """corro_apply_slots: merge received slots (nsrc * cap 48-B records, a uint8 CUDA tensor) where
        they lie -- no unpack pass. Returns (impact flags by slot position, a uint8 CUDA tensor of
        nsrc * cap, or None; overflow int32 CUDA tensor [1]: 1 when a source overflowed its slot and
        nothing was applied)."""
        import torch
        n = nsrc * cap
        dev = recs.device
        if overflow is None:
            overflow = torch.zeros(1, dtype=torch.int32, device=dev)
        o = L.ApplyOut()
        imp = None
        if impact:
            imp = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
            o.impact = imp.data_ptr()
        L.check(L.lib().corro_apply_slots(self._h, recs.data_ptr(), nsrc, cap, src_counts.data_ptr(), C.byref(o),
                                          overflow.data_ptr()))
        return (imp[:n] if impact else None), overflow

    def slots_flags_back(self, back, nranks, cap, counts, perm, n):
        """corro_slots_flags_back: the all-to-all of the receivers' slot-position flags -> this sender's
        per-input-change flags (uint8 CUDA tensor of n), queued on the engine's stream."""
        import torch
        flags = torch.zeros(max(n, 1), dtype=torch.uint8, device=back.device)
        L.check(L.lib().corro_slots_flags_back(self._h, back.data_ptr(), nranks, cap, counts.data_ptr(), perm.data_ptr(),
                                               flags.data_ptr(), n))
        return flags[:n]

    def unpack_slots(self, recs, nsrc, cap, src_counts, out=None):
        """Received slots -> (SoA device batch of nsrc * cap changes at the same indices, ap int32
        tensor: i for a received change, -1 for padding, overflow int32 tensor [1]) on the engine's
        stream (corro_unpack_slots); merge with apply_mapped."""
        import torch
        n = nsrc * cap
        dev = recs.device
        if out is None:
            tdt = {np.uint64: torch.int64, np.int64: torch.int64, np.uint32: torch.int32, np.uint8: torch.uint8}
            out = {k: torch.empty(max(n, 1), dtype=tdt[BATCH_FIELDS[k]], device=dev)[:n] for k in REQUIRED}
            out["ap"] = torch.empty(max(n, 1), dtype=torch.int32, device=dev)[:n]
            out["overflow"] = torch.zeros(1, dtype=torch.int32, device=dev)
        s = L.Changes()
        s.n = n
        for k in BATCH_FIELDS:
            a = out.get(k) if k in REQUIRED else None
            setattr(s, k, a.data_ptr() if (a is not None and n) else None)
        L.check(L.lib().corro_unpack_slots(self._h, recs.data_ptr(), nsrc, cap, src_counts.data_ptr(), C.byref(s),
                                           out["ap"].data_ptr(), out["overflow"].data_ptr()))
        return out

    def apply_mapped(self, batch, impact=False):
        """corro_apply_mapped: merge a device batch whose changes with ap == -1 (batch["ap"]) are
        skipped, the rest in index order (the slot layout of unpack_slots)."""
        fields = {k: v for k, v in batch.items() if k in BATCH_FIELDS}
        s, o, _keep, imp, n, _on_dev, impact = self.prepare(fields, impact)
        L.check(L.lib().corro_apply_mapped(self._h, C.byref(s), batch["ap"].data_ptr(), C.byref(o)))
        return imp[:n] if impact else None

    def unpack_records(self, recs, rec_bytes, out=None):
        """Packed records (a uint8 CUDA tensor) -> SoA device batch (corro_unpack_records)."""
        import torch
        n = int(recs.numel()) // rec_bytes
        dev = recs.device
        if out is None:
            tdt = {np.uint64: torch.int64, np.int64: torch.int64, np.uint32: torch.int32, np.uint8: torch.uint8}
            keys = [k for k in FIXED_FIELDS if k in REQUIRED or rec_bytes == 80]
            out = {k: torch.empty(max(n, 1), dtype=tdt[BATCH_FIELDS[k]], device=dev)[:n] for k in keys}
        s = L.Changes()
        s.n = n
        for k in BATCH_FIELDS:
            a = out.get(k)
            setattr(s, k, a.data_ptr() if (a is not None and n) else None)
        torch.cuda.current_stream().synchronize()
        L.check(L.lib().corro_unpack_records(self._h, recs.data_ptr() if n else None, n, rec_bytes, C.byref(s)))
        return out

    # ---- wire decode ------------------------------------------------------------------------
    def decode_frames(self, buf, payload=0, device=False, device_headers=False):
        """Decode length-delimited speedy frames (corro_decode_frames; payload 0 = SyncMessage,
        1 = UniPayload) on the GPU. Returns {"cs": ctypes array of corro_changeset (one per
        frame), "status": int32[], "changes": SoA dict, "set_start"/"set_end"}: host numpy arrays,
        or with device=True CUDA tensors that stay on the GPU (the batch
        corro_process_multiple_changes / corro_apply_batch take with CORRO_MEM_DEVICE). With
        device_headers=True (and device=True) also "cs_dev": the status-0 frames' headers as a CUDA
        uint8 tensor of corro_changeset records built on the device, and "n_dev" of them (for
        CORRO_MEM_DEVICE_HEADERS)."""
        lib = L.lib()
        buf = bytes(buf)
        d = L.Decoded()
        mem = L.CORRO_MEM_DEVICE if device else L.CORRO_MEM_HOST
        L.check(lib.corro_decode_frames(self._h, buf, len(buf), payload, mem, C.byref(d), 0))
        F, NC, NS = d.nframes, d.nchanges, d.nsets
        cs = (L.Changeset * max(F, 1))()
        actors = (C.c_uint8 * max(16 * F, 16))()
        status = np.zeros(max(F, 1), np.int32)
        if device:
            import torch
            tdt = {np.uint64: torch.int64, np.int64: torch.int64, np.uint32: torch.int32, np.uint8: torch.uint8}
            ch = {k: torch.zeros(max(NC, 1), dtype=tdt[dt], device="cuda") for k, dt in BATCH_FIELDS.items()}
            ss = torch.zeros(max(NS, 1), dtype=torch.int64, device="cuda")
            se = torch.zeros(max(NS, 1), dtype=torch.int64, device="cuda")
            vdata = torch.zeros(max(len(buf), 1), dtype=torch.uint8, device="cuda")
            ptr = lambda a: a.data_ptr()  # noqa: E731
            torch.cuda.current_stream().synchronize()
        else:
            ch = {k: np.zeros(max(NC, 1), dt) for k, dt in BATCH_FIELDS.items()}
            ss, se = np.zeros(max(NS, 1), np.uint64), np.zeros(max(NS, 1), np.uint64)
            vdata = None
            ptr = lambda a: a.ctypes.data  # noqa: E731
        d.cs, d.actor_ids, d.status = C.addressof(cs), C.addressof(actors), status.ctypes.data
        d.changes.n = NC
        for k, a in ch.items():
            setattr(d.changes, k, ptr(a))
        if device:
            d.changes.val_data, d.changes.val_data_len = vdata.data_ptr(), len(buf)
        d.set_start, d.set_end = ptr(ss), ptr(se)
        cs_dev = None
        if device and device_headers:
            import torch
            cs_dev = torch.zeros(max(F, 1) * C.sizeof(L.Changeset), dtype=torch.uint8, device="cuda")
            d.cs_dev = cs_dev.data_ptr()
            torch.cuda.current_stream().synchronize()
        if F:
            L.check(lib.corro_decode_frames(self._h, buf, len(buf), payload, mem, C.byref(d), 1))
        changes = {k: a[:NC] for k, a in ch.items()}
        if d.changes.val_data:  # long values: offsets into the frame bytes
            changes["val_data"] = vdata[:len(buf)] if device else np.frombuffer(buf, np.uint8)
        else:
            for k in LONG_FIELDS:
                changes.pop(k)
        out = {"cs": cs, "nframes": F, "actors": actors, "status": status[:F],
               "changes": changes, "set_start": ss[:NS], "set_end": se[:NS]}
        if cs_dev is not None:
            out["cs_dev"], out["n_dev"] = cs_dev, int(d.n_dev) if F else 0
        return out

    # ---- changeset extraction (server side of a sync need) ---------------------------------
    def extract_changes(self, needs):
        """crsql_changes rows per need (corro_extract_changes): needs = {"site": u32[], "start":
        u64[], "end": u64[], optional "seq_start"/"seq_end": u32[]} as numpy arrays (host) or CUDA
        tensors (device). Returns grp_off/row_off (n+1), per group version/last_seq/ts/grp_row_off/
        grp_rows, and "rows" (crsql_changes fields), groups of a need in DESCENDING version order."""
        lib = L.lib()
        on_dev = _is_torch(needs["site"])
        n = int(needs["site"].shape[0])
        s = L.ExtractIn()
        s.n = n
        keep = []
        for k, dt in (("site", np.uint32), ("start", np.uint64), ("end", np.uint64), ("seq_start", np.uint32),
                      ("seq_end", np.uint32)):
            a = needs.get(k)
            if a is None:
                setattr(s, k, None)
                continue
            if on_dev:
                if not a.is_cuda or not a.is_contiguous() or not _int_dtype_ok(a, dt):
                    raise ValueError(f"device need field {k} must be a contiguous CUDA integer tensor of "
                                     f"{np.dtype(dt)} width (got {a.dtype})")
                setattr(s, k, a.data_ptr() if n else None)
            else:
                a = np.ascontiguousarray(a, dtype=dt)
                keep.append(a)
                setattr(s, k, a.ctypes.data if n else None)
        mem = L.CORRO_MEM_DEVICE if on_dev else L.CORRO_MEM_HOST
        if on_dev:
            import torch
            dev = needs["site"].device

            def alloc(cnt, dt):
                tdt = {np.uint64: torch.int64, np.int64: torch.int64, np.uint32: torch.int32,
                       np.uint8: torch.uint8}[dt]
                return torch.empty(max(cnt, 1), dtype=tdt, device=dev)

            def ptr(a):
                return a.data_ptr()
            torch.cuda.current_stream().synchronize()
        else:
            def alloc(cnt, dt):
                return np.zeros(max(cnt, 1), dt)

            def ptr(a):
                return a.ctypes.data
        o = L.ExtractOut()
        gc, rc = alloc(n, np.uint64), alloc(n, np.uint64)
        o.grp_count, o.row_count = ptr(gc), ptr(rc)
        if n:
            L.check(lib.corro_extract_changes(self._h, C.byref(s), mem, C.byref(o), 0))
        if on_dev:
            import torch
            go = torch.zeros(n + 1, dtype=torch.int64, device=dev)
            ro = torch.zeros(n + 1, dtype=torch.int64, device=dev)
            go[1:] = torch.cumsum(gc[:n], 0)
            ro[1:] = torch.cumsum(rc[:n], 0)
            G, R = int(go[-1].item()), int(ro[-1].item())
        else:
            go = np.zeros(n + 1, np.uint64)
            ro = np.zeros(n + 1, np.uint64)
            go[1:] = np.cumsum(gc[:n])
            ro[1:] = np.cumsum(rc[:n])
            G, R = int(go[-1]), int(ro[-1])
        res = {"grp_off": go, "row_off": ro, "version": alloc(G, np.int64), "last_seq": alloc(G, np.uint64),
               "ts": alloc(G, np.uint64), "grp_row_off": alloc(G, np.uint64), "grp_rows": alloc(G, np.uint64)}
        rows = {k: alloc(R, dt) for k, dt in ROW_FIELDS.items()}
        o.grp_off, o.row_off = ptr(go), ptr(ro)
        for k in ("version", "last_seq", "ts", "grp_row_off", "grp_rows"):
            setattr(o, k, ptr(res[k]))
        for k, a in rows.items():
            setattr(o.rows, k, ptr(a))
        if n:
            if on_dev:
                torch.cuda.current_stream().synchronize()
            L.check(lib.corro_extract_changes(self._h, C.byref(s), mem, C.byref(o), 1))
        for k in ("version", "last_seq", "ts", "grp_row_off", "grp_rows"):
            res[k] = res[k][:G]
        res["rows"] = {k: a[:R] for k, a in rows.items()}
        return res

    # ---- wire encode (the send half of a sync need) ------------------------------------------
    def encode_changesets(self, spans, rows, max_buf_size=8192, payload=0, cluster_id=0):
        """Rows -> chunked Changeset::Full messages -> length-delimited frames on the GPU
        (corro_encode_changesets). spans = {"site": u32[], "version": i64[], "last_seq", "ts",
        "seq_start", "seq_end", "row_off", "row_count": u64[]}, one entry per ChunkedChanges the
        reference would build; rows = the crsql_changes fields (extract_changes' "rows"). numpy arrays
        (host) or CUDA tensors (device: nothing but the two totals leaves the GPU). Returns "buf"
        (uint8, the frames in span order then chunk order), "frame_off" (nframes + 1),
        "span_frame_off" (n + 1) and per frame "frame_seq_start", "frame_seq_end", "frame_row_off",
        "frame_rows", in the same memory, plus "nframes" / "nbytes"."""
        row_fields = [(k, dt) for k, dt in ROW_FIELDS.items() if k != "ts"]
        on_dev = _is_torch(spans["site"])
        n, R = int(spans["site"].shape[0]), int(rows["pk"].shape[0])
        s = L.EncodeIn()
        s.n, s.nrows = n, R
        s.max_buf_size, s.payload, s.cluster_id = int(max_buf_size), int(payload), int(cluster_id)
        keep = []
        for src, dst, fields, cnt in ((spans, s, SPAN_FIELDS, n), (rows, s.rows, row_fields, R)):
            for k, dt in fields:
                a = src[k]
                if on_dev:
                    if not a.is_cuda or not a.is_contiguous() or not _int_dtype_ok(a, dt) or int(a.shape[0]) != cnt:
                        raise ValueError(f"device field {k} must be a contiguous CUDA integer tensor of "
                                         f"{cnt} x {np.dtype(dt)} width")
                    setattr(dst, k, a.data_ptr() if cnt else None)
                else:
                    a = np.ascontiguousarray(a, dtype=dt)
                    if a.shape[0] != cnt:
                        raise ValueError(f"field {k} must hold {cnt} entries")
                    keep.append(a)
                    setattr(dst, k, a.ctypes.data if cnt else None)
        mem = Mem.of(spans["site"])
        res = two_pass(L.lib().corro_encode_changesets, (self._h, C.byref(s), mem.const), mem, L.Encoded(),
                       (("span_frame_off", np.uint64, n + 1),), ("nframes", "nbytes"), _ENC_OUT)
        if n == 0:
            res["span_frame_off"][:1] = 0
        return res

    # ---- sync request decode (the server's half of plan_requests) ---------------------------
    def _two_pass_io(self, on_dev, dev):
        """alloc / ptr / sync for a two-pass call's arrays: numpy (host) or CUDA tensors on dev."""
        if on_dev:
            import torch
            tdt = {np.uint64: torch.int64, np.int64: torch.int64, np.uint32: torch.int32, np.int32: torch.int32,
                   np.uint8: torch.uint8}

            def alloc(cnt, dt):
                return torch.empty(max(cnt, 1), dtype=tdt[dt], device=dev)

            def ptr(a):
                return a.data_ptr()
            return alloc, ptr, torch.cuda.current_stream().synchronize

        def alloc(cnt, dt):
            return np.zeros(max(cnt, 1), dt)

        def ptr(a):
            return a.ctypes.data
        return alloc, ptr, lambda: None

    @staticmethod
    def _in_field(a, dt, on_dev, name, cnt=None):
        """One input array as (kept object, pointer or None): a contiguous CUDA integer tensor of dt's
        width, or a numpy array converted to dt."""
        if on_dev:
            if not _is_torch(a) or not a.is_cuda or not a.is_contiguous() or not _int_dtype_ok(a, dt):
                raise ValueError(f"device field {name} must be a contiguous CUDA integer tensor of {np.dtype(dt)} width")
            n = int(a.numel())
        else:
            a = np.ascontiguousarray(a, dtype=dt)
            n = int(a.size)
        if cnt is not None and n != cnt:
            raise ValueError(f"field {name} must hold {cnt} entries (got {n})")
        if n == 0:
            return a, None
        return a, (a.data_ptr() if on_dev else a.ctypes.data)

    def decode_requests(self, buf, frame_off, book=None):
        """SyncMessageV1::Request frames -> decoded, screened needs and their extraction entries on the
        GPU (corro_decode_requests). buf: the frames back to back (bytes / numpy uint8, or a CUDA uint8
        tensor); frame_off: nframes + 1 byte offsets of the length prefixes, in the same memory -- the
        "buf" / "frame_off" a peer's plan_requests_device returns. book (optional, same memory):
        {"known": u8[], "max": i64[] (-1 = None), "gap_off": u64[nsites + 1], "gap_start", "gap_end":
        u64[]} over site ordinals; None = no screen. Returns "frame_status" (int32), "frame_pair_off",
        per pair "pair_actor" (16 bytes each), "pair_site", "pair_need_off", per need "kind", "start",
        "end", "sr_off", "sr_n", "need_site", "need_keep", "need_ent_off", "s_start" / "s_end", the
        entries "ent_site", "ent_start", "ent_end", "ent_seq_start", "ent_seq_end", "ent_need", and
        the totals "nframes", "npairs", "nneeds", "nseqs", "nents". With device input only the totals
        reach the host."""
        mem = Mem.of(buf)
        if not mem.on_dev and not isinstance(buf, np.ndarray):
            buf = np.frombuffer(bytes(buf), np.uint8)
        r = L.ReqDecIn()
        b, r.buf = mem.field(buf, np.uint8, "buf")
        fo, r.frame_off = mem.field(frame_off, np.uint64, "frame_off")
        keep = [b, fo]
        r.len = mem.count(b)
        if mem.count(fo) < 1:
            raise ValueError("frame_off holds nframes + 1 offsets")
        F = mem.count(fo) - 1
        r.nframes = F
        if book is not None:
            S = mem.count(book["known"]) if mem.on_dev else np.asarray(book["known"]).size
            r.book_nsites = S
            for k, dst, dt, cnt in (("known", "book_known", np.uint8, S), ("max", "book_max", np.int64, S),
                                    ("gap_off", "gap_off", np.uint64, S + 1), ("gap_start", "gap_start", np.uint64, None),
                                    ("gap_end", "gap_end", np.uint64, None)):
                a, p = mem.field(book[k], dt, "book." + k, cnt)
                keep.append(a)
                setattr(r, dst, p)
            r.book_ngaps = mem.count(keep[-1])
        res = two_pass(L.lib().corro_decode_requests, (self._h, C.byref(r), mem.const), mem, L.ReqDecOut(),
                       (("frame_status", np.int32, F), ("frame_pair_off", np.uint64, F + 1)),
                       ("npairs", "nneeds", "nseqs", "nents"), _REQDEC_OUT)
        res["nframes"] = F
        return res

    def need_spans(self, dec, ext):
        """Decoded needs + the extraction of their entries -> corro_encode_in's span arrays on the GPU
        (corro_need_spans). dec: decode_requests' result; ext: extract_changes' result for dec's ent_*
        arrays (same memory). Returns the spans dict encode_changesets takes ("site", "version",
        "last_seq", "ts", "seq_start", "seq_end", "row_off", "row_count") plus "need_span_off"
        (nneeds + 1), "in_state" (per need: a kept Partial's version is in the state) and "nspans"."""
        mem = Mem.of(dec["kind"])
        T, Q, E = int(dec["nneeds"]), int(dec["nseqs"]), int(dec["nents"])
        G = int(ext["version"].shape[0])
        s = L.SpansIn()
        s.nneeds, s.nseqs, s.nents, s.ngroups = T, Q, E, G
        keep = mem.fill(s, dec, (("kind", np.uint8, T), ("sr_off", np.uint64, T), ("sr_n", np.uint64, T),
                                 ("s_start", np.uint64, Q), ("s_end", np.uint64, Q), ("need_keep", np.uint8, T),
                                 ("need_ent_off", np.uint64, T + 1), ("need_site", np.uint32, T)))
        keep += mem.fill(s, ext, (("grp_off", np.uint64, E + 1), ("version", np.int64, G), ("last_seq", np.uint64, G),
                                  ("ts", np.uint64, G), ("grp_row_off", np.uint64, G), ("grp_rows", np.uint64, G)))
        return two_pass(L.lib().corro_need_spans, (self._h, C.byref(s), mem.const), mem, L.SpansOut(),
                        (("need_span_off", np.uint64, T + 1), ("in_state", np.uint8, T)), ("nspans",), _SPANS_OUT)

    def need_tails(self, dec, ext, sp, bufbook, payload=0, cluster_id=0):
        """The Changeset::Empty frames that end the answers to the decoded needs, on the GPU
        (corro_need_tails). dec: decode_requests' result; ext: extract_changes' result for dec's ent_*
        arrays; sp: need_spans' result (its "in_state"); bufbook: {"gap_off", "gap_start", "gap_end"
        (the needed() gaps, as decode_requests' book has them), "buf_off": u64[nsites + 1], "buf_version":
        u64[] (the buffered versions per site ordinal, ascending)}, all in the same memory. Returns
        "nranges", "need_tail_off" (nneeds + 1), "need_host" (per need: 1 = it touches a buffered version
        and the host answers its tail), "range_start", "range_end", "buf" (one frame per range: 49 bytes
        for payload 0, 55 for the uni payload 1) and "frame_off"."""
        mem = Mem.of(dec["kind"])
        T, E = int(dec["nneeds"]), int(dec["nents"])
        G = int(ext["version"].shape[0])
        S = len(bufbook["gap_off"]) - 1
        if S < 0:
            raise ValueError("gap_off holds nsites + 1 offsets")
        r = L.TailsIn()
        r.nneeds, r.nents, r.ngroups, r.book_nsites = T, E, G, S
        r.payload, r.cluster_id = payload, cluster_id
        keep = mem.fill(r, dec, (("kind", np.uint8, T), ("start", np.uint64, T), ("end", np.uint64, T),
                                 ("need_keep", np.uint8, T), ("need_site", np.uint32, T),
                                 ("need_ent_off", np.uint64, T + 1)))
        keep += mem.fill(r, sp, (("in_state", np.uint8, T),))
        keep += mem.fill(r, ext, (("grp_off", np.uint64, E + 1), ("version", np.int64, G)))
        keep += mem.fill(r, bufbook, (("gap_off", np.uint64, S + 1), ("gap_start", np.uint64, None),
                                      ("gap_end", np.uint64, None), ("buf_off", np.uint64, S + 1),
                                      ("buf_version", np.uint64, None)))
        r.book_ngaps, r.book_nbuf = int(keep[-3].shape[0]), int(keep[-1].shape[0])
        if int(keep[-4].shape[0]) != r.book_ngaps:
            raise ValueError("gap_start and gap_end must hold the same number of gaps")
        res = two_pass(L.lib().corro_need_tails, (self._h, C.byref(r), mem.const), mem, L.TailsOut(),
                       (("need_tail_off", np.uint64, T + 1), ("need_host", np.uint8, T)), ("nranges", "nbytes"),
                       (("range_start", np.uint64, "nranges"), ("range_end", np.uint64, "nranges"),
                        ("buf", np.uint8, "nbytes"), ("frame_off", np.uint64, "nranges", 1, 1)))
        del res["nbytes"]
        return res

    def _assemble(self, dec, sp, enc, tl, payload, bsp=None, benc=None):
        """assemble_answers, or with bsp assemble_answers_buffered: the same base input and output."""
        mem = Mem.of(dec["frame_pair_off"])
        F, NP, T = int(dec["nframes"]), int(dec["npairs"]), int(dec["nneeds"])
        NS, NR = int(sp["nspans"]), int(tl["nranges"])
        rb = L.AssembleIn() if bsp is None else L.AssembleBufferedIn()
        r = rb if bsp is None else rb.base
        r.nframes, r.npairs, r.nneeds, r.nspans, r.nranges, r.payload = F, NP, T, NS, NR, int(payload)
        r.enc_nframes, r.enc_nbytes = (int(enc["nframes"]), int(enc["nbytes"])) if NS else (0, 0)
        r.tail_nbytes = int(tl["buf"].shape[0])
        keep = mem.fill(r, dec, (("frame_pair_off", np.uint64, F + 1), ("pair_need_off", np.uint64, NP + 1),
                                 ("need_keep", np.uint8, T)))
        keep += mem.fill(r, sp, (("need_span_off", np.uint64, T + 1),))
        keep += mem.fill(r, tl, (("need_tail_off", np.uint64, T + 1), ("need_host", np.uint8, T),
                                 ("buf", np.uint8, None, "tail_buf")))
        if NS:
            keep += mem.fill(r, enc, (("span_frame_off", np.uint64, NS + 1),
                                      ("frame_off", np.uint64, r.enc_nframes + 1, "enc_frame_off"),
                                      ("buf", np.uint8, r.enc_nbytes, "enc_buf")))
        fn = L.lib().corro_assemble_answers
        if bsp is not None:
            fn = L.lib().corro_assemble_answers_buffered
            BS = rb.nbspans = int(bsp["nspans"])
            rb.benc_nframes, rb.benc_nbytes = (int(benc["nframes"]), int(benc["nbytes"])) if BS else (0, 0)
            keep += mem.fill(rb, bsp, (("need_bspan_off", np.uint64, T + 1),))
            if BS:
                keep += mem.fill(rb, benc, (("span_frame_off", np.uint64, BS + 1, "bspan_frame_off"),
                                            ("frame_off", np.uint64, rb.benc_nframes + 1, "benc_frame_off"),
                                            ("buf", np.uint8, rb.benc_nbytes, "benc_buf")))
        return two_pass(fn, (self._h, C.byref(rb), mem.const), mem, L.Assembled(),
                        (("need_ans_off", np.uint64, T + 1), ("frame_ans_off", np.uint64, F + 1),
                         ("frame_host", np.uint8, F)), ("nbytes",), (("buf", np.uint8, "nbytes"),))

    def assemble_answers(self, dec, sp, enc, tl, payload=0):
        """The per-frame answers to the decoded request frames in one buffer, on the GPU
        (corro_assemble_answers): per need, in frame order then wire order, its encoded frames and then
        its Empty tail frames. dec: decode_requests' result; sp: need_spans' result (its
        "need_span_off"); enc: encode_changesets' result for sp's spans; tl: need_tails' result, all in
        the same memory (CUDA tensors on one device, or numpy); payload as given to the encoder and to
        need_tails. Returns, in that memory, "buf" (uint8), "need_ans_off" (nneeds + 1), "frame_ans_off" (nframes + 1: the answer of frame f
        is buf[off[f]:off[f + 1]]) and "frame_host" (per frame: 1 = a kept need of it has need_host,
        and the host splices that need's bookie messages in at need_ans_off[t + 1]), plus "nbytes"."""
        return self._assemble(dec, sp, enc, tl, payload)

    _BUFIDX_IN = (("ver_off", "ver_off", np.uint64), ("version", "idx_version", np.uint64),
                  ("last_seq", "idx_last_seq", np.int64), ("ts", "idx_ts", np.uint64), ("on_device", "on_device", np.uint8),
                  ("sr_off", "vsr_off", np.uint64), ("sr_start", "vsr_start", np.uint64), ("sr_end", "vsr_end", np.uint64),
                  ("seg_off", "seg_off", np.uint64), ("seg_pool_off", "seg_pool_off", np.uint64),
                  ("seg_seq0", "seg_seq0", np.uint32), ("seg_n", "seg_n", np.uint32))

    def buffered_spans(self, bookie, dec, ext, sp, tl, idx):
        """The buffered (partial) versions' chunks of the decoded needs as spans and rows, gathered from
        the bookie's device row pool (corro_buffered_spans). bookie: the agent's Bookie; dec / ext / sp:
        as for need_tails; tl: need_tails' result for the books of serve.device_buffered_index (its
        "need_host"); idx: that index's "dev" arrays. CUDA tensors only: the pool rows stay on the
        device. Returns the spans dict encode_changesets takes, "need_bspan_off" (nneeds + 1),
        "nspans", "rows" (the crsql_changes fields, "ts" included) and "nrows"."""
        if not _is_torch(dec["kind"]):
            raise ValueError("buffered_spans takes CUDA tensors: the pool rows are on the device")
        mem = Mem(dec["kind"].device)
        T, Q, E = int(dec["nneeds"]), int(dec["nseqs"]), int(dec["nents"])
        G = int(ext["version"].shape[0])
        S = int(idx["ver_off"].shape[0]) - 1
        NV = int(idx["version"].shape[0])
        if S < 0 or int(idx["sr_off"].shape[0]) != NV + 1 or int(idx["seg_off"].shape[0]) != NV + 1:
            raise ValueError("ver_off holds nsites + 1 offsets, sr_off and seg_off one per version + 1")
        r = L.BufSpansIn()
        r.nneeds, r.nseqs, r.nents, r.ngroups, r.idx_nsites, r.idx_nver = T, Q, E, G, S, NV
        r.idx_nsr, r.idx_nseg = int(idx["sr_start"].shape[0]), int(idx["seg_pool_off"].shape[0])
        keep = mem.fill(r, dec, (("kind", np.uint8, T), ("start", np.uint64, T), ("end", np.uint64, T),
                                 ("sr_off", np.uint64, T), ("sr_n", np.uint64, T), ("s_start", np.uint64, Q),
                                 ("s_end", np.uint64, Q), ("need_keep", np.uint8, T), ("need_site", np.uint32, T),
                                 ("need_ent_off", np.uint64, T + 1)))
        keep += mem.fill(r, sp, (("in_state", np.uint8, T),))
        keep += mem.fill(r, tl, (("need_host", np.uint8, T),))
        keep += mem.fill(r, ext, (("grp_off", np.uint64, E + 1), ("version", np.int64, G)))
        keep += mem.fill(r, idx, [(k, dt, None, dst) for k, dst, dt in self._BUFIDX_IN])
        for k, n in (("last_seq", NV), ("ts", NV), ("on_device", NV), ("sr_end", r.idx_nsr), ("seg_seq0", r.idx_nseg),
                     ("seg_n", r.idx_nseg)):
            if int(idx[k].shape[0]) != n:
                raise ValueError(f"index field {k} must hold {n} entries")
        res = two_pass(L.lib().corro_buffered_spans, (self._h, bookie._h, C.byref(r), mem.const), mem, L.BufSpansOut(),
                       (("need_bspan_off", np.uint64, T + 1),), ("nspans", "nrows"),
                       _SPANS_OUT + tuple(("rows." + k, dt, "nrows") for k, dt in ROW_FIELDS.items()))
        res["rows"] = {k: res.pop("rows." + k) for k in ROW_FIELDS}
        return res

    def assemble_answers_buffered(self, dec, sp, enc, bsp, benc, tl, payload=0):
        """assemble_answers with the buffered frames as a third piece between a need's encoded frames
        and its Empty tail frames (corro_assemble_answers_buffered). bsp: buffered_spans' result (its
        "need_bspan_off"); benc: encode_changesets' result for bsp's spans and rows (None when bsp
        holds no span). The other arguments and the result are assemble_answers'."""
        return self._assemble(dec, sp, enc, tl, payload, bsp, benc)

    # ---- sync need diff -------------------------------------------------------------------
    def compute_needs(self, entries):
        """Batched compute_available_needs over CSR entries (see corrosion_amd.sync)."""
        from .sync import _needs_host
        return _needs_host(self, entries)
