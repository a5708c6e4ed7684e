"""The two-pass calls of the C ABI, marshalled once.

A two-pass entry point is called with pass 0 to size its result (it fills the arrays that are sized by the
input and writes totals into the output struct) and with pass 1 to fill the arrays sized by those totals.
Mem says where the arrays live; TwoPass / two_pass allocate them, point the output struct at them,
synchronise, call, check and trim.

An output table holds (name, dtype, size) or (name, dtype, size, mul, extra): the array `name` of the output
struct (a dotted name reaches into a nested struct) has size * mul + extra elements, where size is an int
or the name of a total."""
import ctypes as C

import numpy as np

from . import _lib as L


def _is_torch(x):
    return type(x).__module__.startswith("torch")


def _int_dtype_ok(t, dt):
    """A device field's tensor must be an integer type of the field's width (signed or unsigned: the
    C ABI reads the bits); a float, bool or wider/narrower tensor is rejected, not reinterpreted."""
    import torch
    ok = {8: (torch.int64, getattr(torch, "uint64", None)), 4: (torch.int32, getattr(torch, "uint32", None)),
          2: (torch.int16, getattr(torch, "uint16", None)), 1: (torch.uint8, torch.int8)}
    return t.dtype in ok.get(np.dtype(dt).itemsize, ())


class Mem:
    """Where a call's arrays live: host numpy (Mem()) or CUDA tensors on `dev` (Mem(dev))."""

    def __init__(self, dev=None):
        self.dev, self.on_dev = dev, dev is not None
        self.const = L.CORRO_MEM_DEVICE if self.on_dev else L.CORRO_MEM_HOST
        if self.on_dev:
            import torch
            self._torch = torch
            self._tdt = {np.uint64: torch.int64, np.int64: torch.int64, np.uint32: torch.int32, np.int32: torch.int32,
                         np.uint8: torch.uint8}

    @classmethod
    def of(cls, a):
        """The memory kind of the array a."""
        return cls(a.device) if _is_torch(a) else cls()

    def alloc(self, count, dt):
        """An output array of at least one element (so that it always has an address)."""
        if self.on_dev:
            return self._torch.empty(max(count, 1), dtype=self._tdt[dt], device=self.dev)
        return np.zeros(max(count, 1), dt)

    def count(self, a):
        return int(a.numel() if self.on_dev else a.size)

    def ptr(self, a):
        if self.on_dev:
            return a.data_ptr() if a.numel() else None
        return a.ctypes.data if a.size else None

    def sync(self):
        if self.on_dev:
            self._torch.cuda.current_stream().synchronize()

    @staticmethod
    def trim(a, n):
        """a at its exact length n: alloc gave it max(n, 1) elements, so only an empty result is cut."""
        return a if n else a[:0]

    def field(self, a, dt, name, cnt=None):
        """One input array as (kept object, pointer or None): a contiguous CUDA integer tensor of dt's
        width, or a numpy array converted to dt."""
        if self.on_dev:
            if not _is_torch(a) or not a.is_cuda or not a.is_contiguous() or not _int_dtype_ok(a, dt):
                raise ValueError(f"device field {name} must be a contiguous CUDA integer tensor of {np.dtype(dt)} width")
        else:
            a = np.ascontiguousarray(a, dtype=dt)
        n = self.count(a)
        if cnt is not None and n != cnt:
            raise ValueError(f"field {name} must hold {cnt} entries (got {n})")
        return a, self.ptr(a)

    def fill(self, s, src, fields):
        """Point the input struct s at src's arrays: fields holds (key, dtype, count or None) or, where
        the struct's member has another name, (key, dtype, count, member). Returns the arrays to keep
        alive until the call is over."""
        keep = []
        for k, dt, cnt, *dst in fields:
            a, p = self.field(src[k], dt, k, cnt)
            keep.append(a)
            setattr(s, dst[0] if dst else k, p)
        return keep


class TwoPass:
    """One two-pass call: fn(*lead, &o, which), with o's arrays in mem. lead holds every argument in
    front of the output struct (handles, the input struct by reference, mem.const). For a caller that
    runs pass 1 more than once, or times the bare call; the others use two_pass."""

    def __init__(self, fn, lead, mem, o):
        self.fn, self.lead, self.mem, self.o = fn, lead, mem, o
        self.out = {}                                          # name -> (array, exact length)

    def bind(self, table, sizes=None):
        """Allocate the table's arrays and point o at them."""
        alloc, ptr, o, out = self.mem.alloc, self.mem.ptr, self.o, self.out
        for name, dt, size, *me in table:
            n = sizes[size] if isinstance(size, str) else size
            if me:
                n = n * me[0] + me[1]
            a = alloc(n, dt)
            if "." in name:                                    # a member of a nested struct
                *path, leaf = name.split(".")
                st = o
                for p in path:
                    st = getattr(st, p)
                setattr(st, leaf, ptr(a))
            else:
                setattr(o, name, ptr(a))
            out[name] = (a, n)

    def call(self, which):
        """The bare call (the caller has synchronised)."""
        L.check(self.fn(*self.lead, C.byref(self.o), which))

    def run(self, which, table=(), sizes=None):
        self.bind(table, sizes)
        self.mem.sync()
        self.call(which)

    def totals(self, names):
        return {k: int(getattr(self.o, k)) for k in names}

    def result(self):
        """The arrays bound since the last result(), trimmed to their exact lengths."""
        trim, out = self.mem.trim, self.out
        self.out = {}
        return {k: trim(a, n) for k, (a, n) in out.items()}


def two_pass(fn, lead, mem, o, pre, totals, post):
    """Both passes: the arrays of `pre` before pass 0, the `totals` read after it, the arrays of `post`
    (sized over those totals) before pass 1. Returns every array, trimmed, and the totals, by name."""
    tp = TwoPass(fn, lead, mem, o)
    tp.run(0, pre)
    tot = tp.totals(totals)
    tp.run(1, post, tot)
    return {**tp.result(), **tot}


# corro_bookie_image: the books (host arrays whatever `mem` is) and the rows (in `mem`)
IMAGE_BOOKS = (("actor_ids", np.uint8, "nactors", 16, 0), ("max", np.int64, "nactors"), ("gap_off", np.uint64, "nactors", 1, 1),
               ("gap_start", np.uint64, "ngaps"), ("gap_end", np.uint64, "ngaps"), ("seq_off", np.uint64, "nactors", 1, 1),
               ("seq_version", np.uint64, "nseqrows"), ("seq_start", np.uint64, "nseqrows"), ("seq_end", np.uint64, "nseqrows"),
               ("seq_last", np.uint64, "nseqrows"), ("seq_ts", np.uint64, "nseqrows"), ("site_ids", np.uint8, "nsites", 16, 0))
IMAGE_ROWS = (("pk", np.uint64), ("table_cid", np.uint32), ("col_version", np.int64), ("db_version", np.int64),
              ("cl", np.uint32), ("seq", np.uint32), ("site", np.uint32), ("val0", np.uint64), ("val1", np.uint64),
              ("val_type", np.uint8), ("val_len", np.uint8), ("ts", np.uint64))
IMAGE_LONG = (("val_off", np.uint64, "nrows"), ("val_size", np.uint32, "nrows"), ("val_data", np.uint8, "val_data_len"))


def save_image(fn, ctx, bk, mem):
    """corro_bookie_save's two passes: the image's books as host arrays and its rows in `mem`, by name
    ("rows" holds the row arrays), with the counts. fn(ctx, bk, &image, mem, pass)."""
    o = L.BookieImage()
    books = TwoPass(lambda c, b, op, which: fn(c, b, op, mem.const, which), (ctx, bk), Mem(), o)
    books.run(0)
    tot = books.totals(("nactors", "ngaps", "nseqrows", "nsites", "stamp"))
    tot["nrows"], tot["val_data_len"] = int(o.rows.n), int(o.rows.val_data_len)
    rows = TwoPass(None, (), mem, o)
    rows.bind(tuple(("rows." + k, dt, "nrows") for k, dt in IMAGE_ROWS), tot)
    if tot["val_data_len"]:
        rows.bind(tuple(("rows." + k, dt, size) for k, dt, size in IMAGE_LONG), tot)
    mem.sync()
    books.run(1, IMAGE_BOOKS, tot)
    res = {**books.result(), **tot}
    res["actor_ids"] = res["actor_ids"].reshape(-1, 16)
    res["site_ids"] = res["site_ids"].reshape(-1, 16)
    res["rows"] = {k[5:]: a for k, a in rows.result().items()}
    return res


def load_image(fn, ctx, bk, image):
    """corro_bookie_load of an image as save_image gives it (or one built by hand): the books are numpy
    arrays, the rows numpy arrays or CUDA tensors. fn(ctx, bk, &image, mem)."""
    o = L.BookieImage()
    host = Mem()
    na, ng, ns = len(image["max"]), len(image["gap_start"]), len(image["seq_version"])
    nsites = int(np.asarray(image["site_ids"]).size // 16)
    o.nactors, o.ngaps, o.nseqrows, o.nsites = na, ng, ns, nsites
    counts = {"actor_ids": 16 * na, "max": na, "gap_off": na + 1, "gap_start": ng, "gap_end": ng, "seq_off": na + 1,
              "seq_version": ns, "seq_start": ns, "seq_end": ns, "seq_last": ns, "seq_ts": ns, "site_ids": 16 * nsites}
    keep = host.fill(o, {k: np.asarray(image[k]).reshape(-1) for k in counts},
                     [(k, dt, counts[k]) for k, dt, *_ in IMAGE_BOOKS])
    rows = image.get("rows") or {}
    n = Mem.of(rows["pk"]).count(rows["pk"]) if "pk" in rows else 0
    mem = Mem.of(rows["pk"]) if n else host
    o.rows.n = n
    if n:
        keep += mem.fill(o.rows, rows, [(k, dt, n) for k, dt in IMAGE_ROWS])
        if "val_data" in rows and mem.count(rows["val_data"]):
            keep += mem.fill(o.rows, rows, [("val_off", np.uint64, n), ("val_size", np.uint32, n), ("val_data", np.uint8, None)])
            o.rows.val_data_len = mem.count(rows["val_data"])
    mem.sync()
    L.check(fn(ctx, bk, C.byref(o), mem.const))
    del keep
