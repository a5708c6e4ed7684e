"""CPU check of the two-pass call helper (corrosion_amd/_twopass.py) in host mode: a Python callable stands
in for the C function. On pass 0 it writes through the pass-0 pointer and sets the totals; on pass 1 it
writes through the pointers it was given. Sizes are the smallest that can go wrong: totals 0, 1 and 2."""
import ctypes as C

import numpy as np
import pytest

from corrosion_amd import _lib as L
from corrosion_amd._twopass import Mem, TwoPass, two_pass


class In(C.Structure):
    _fields_ = [("n", C.c_uint64), ("a", C.c_void_p), ("b", C.c_void_p)]


class Inner(C.Structure):
    _fields_ = [("x", C.c_void_p)]


class Out(C.Structure):
    _fields_ = [("head", C.c_void_p), ("nvals", C.c_uint64), ("nbytes", C.c_uint64), ("vals", C.c_void_p),
                ("off", C.c_void_p), ("wide", C.c_void_p), ("buf", C.c_void_p), ("inner", Inner)]


POST = (("vals", np.uint32, "nvals"), ("off", np.uint64, "nvals", 1, 1), ("wide", np.uint8, "nvals", 16, 0),
        ("buf", np.uint8, "nbytes"), ("inner.x", np.int64, "nvals"))


class RecMem(Mem):
    """Host memory that notes the size of every array it allocates."""

    def __init__(self):
        super().__init__()
        self.sizes = []

    def alloc(self, count, dt):
        a = super().alloc(count, dt)
        self.sizes.append(int(a.size))
        return a


def view(ptr, ctype, n):
    assert ptr, "an output pointer is NULL"
    return (ctype * n).from_address(ptr)


class StandIn:
    """fn(handle, &in, mem, &out, pass): `total` values and 3 * total bytes; fail[pass] is its status."""

    def __init__(self, total, fail=(0, 0)):
        self.total, self.fail, self.calls = total, fail, []

    def __call__(self, handle, s_ref, mem, o_ref, which):
        s, o = s_ref._obj, o_ref._obj
        self.calls.append((handle, mem, which, s.a, s.b))
        if self.fail[which]:
            return self.fail[which]
        T = self.total
        if which == 0:
            view(o.head, C.c_int32, 2)[:] = [7, 8]
            o.nvals, o.nbytes = T, 3 * T
            return 0
        view(o.off, C.c_uint64, T + 1)[:] = range(T + 1)        # written even at T == 0: the arrays have an address
        for ptr, ct, n, base in ((o.vals, C.c_uint32, T, 100), (o.wide, C.c_uint8, 16 * T, 1),
                                 (o.buf, C.c_uint8, 3 * T, 50), (o.inner.x, C.c_int64, T, -5)):
            view(ptr, ct, max(n, 1))[:n] = range(base, base + n)
        return 0


def run(fn, a=(1, 2, 3)):
    mem, s = RecMem(), In()
    keep = mem.fill(s, {"a": a, "b": []}, (("a", np.uint64, len(a)), ("b", np.uint32, None)))
    s.n = len(a)
    res = two_pass(fn, (1234, C.byref(s), mem.const), mem, Out(), (("head", np.int32, 2),), ("nvals", "nbytes"), POST)
    return res, mem, keep


@pytest.mark.parametrize("total", [0, 1, 2])
def test_two_pass_sizes_dtypes_and_values(total):
    fn = StandIn(total)
    res, mem, keep = run(fn)
    T = total
    want = {"head": (np.int32, 2), "vals": (np.uint32, T), "off": (np.uint64, T + 1), "wide": (np.uint8, 16 * T),
            "buf": (np.uint8, 3 * T), "inner.x": (np.int64, T)}
    assert set(res) == set(want) | {"nvals", "nbytes"}
    assert (res["nvals"], res["nbytes"]) == (T, 3 * T)
    for k, (dt, n) in want.items():
        assert isinstance(res[k], np.ndarray) and res[k].dtype == dt and res[k].shape == (n,), k
    assert res["head"].tolist() == [7, 8]
    assert res["vals"].tolist() == list(range(100, 100 + T))
    assert res["off"].tolist() == list(range(T + 1))
    assert res["wide"].tolist() == list(range(1, 1 + 16 * T))
    assert res["buf"].tolist() == list(range(50, 50 + 3 * T))
    assert res["inner.x"].tolist() == list(range(-5, -5 + T))
    # one allocation per table entry, in table order: never empty, and exactly total * mul + extra above that
    assert mem.sizes == [2] + [max(n, 1) for n in (T, T + 1, 16 * T, 3 * T, T)]
    # pass 0 then pass 1, the leading arguments handed through; the empty input arrives as NULL
    assert [(c[0], c[1], c[2]) for c in fn.calls] == [(1234, L.CORRO_MEM_HOST, 0), (1234, L.CORRO_MEM_HOST, 1)]
    assert all(c[3] == keep[0].ctypes.data and c[4] is None for c in fn.calls)
    assert keep[0].dtype == np.uint64 and keep[0].tolist() == [1, 2, 3]


def test_failing_pass_raises_and_stops():
    fn = StandIn(2, fail=(-1, 0))
    with pytest.raises(L.CorroError) as e:
        run(fn)
    assert e.value.code == -1 and [c[2] for c in fn.calls] == [0]       # pass 1 is not called
    fn = StandIn(2, fail=(0, -6))
    with pytest.raises(L.CorroError) as e:
        run(fn)
    assert e.value.code == -6 and [c[2] for c in fn.calls] == [0, 1]


def test_input_field_errors():
    mem, s = Mem(), In()
    with pytest.raises(ValueError) as e:
        mem.fill(s, {"a": [1, 2, 3]}, (("a", np.uint64, 2),))
    assert str(e.value) == "field a must hold 2 entries (got 3)"
    with pytest.raises(ValueError) as e:
        mem.field(np.zeros(0, np.uint8), np.uint8, "book.known", 1)
    assert str(e.value) == "field book.known must hold 1 entries (got 0)"
    a, p = mem.field([5], np.uint32, "site", 1)
    assert a.dtype == np.uint32 and p == a.ctypes.data
    assert mem.field([], np.uint32, "site")[1] is None


def test_pass_one_again_and_a_callers_buffer():
    """TwoPass for the callers that run pass 1 more than once, or into a buffer of their own: the caller
    sets the pointer and runs the pass with an empty table."""
    fn, mem, s, o = StandIn(2), RecMem(), In(), Out()
    tp = TwoPass(fn, (0, C.byref(s), mem.const), mem, o)
    tp.run(0, (("head", np.int32, 2),))
    tot = tp.totals(("nvals", "nbytes"))
    table = tuple(e for e in POST if e[0] != "buf")
    mine = np.full(9, 255, np.uint8)
    o.buf = mem.ptr(mine)
    tp.run(1, table, tot)
    first = tp.result()
    assert mine.tolist() == [50, 51, 52, 53, 54, 55, 255, 255, 255] and "buf" not in first
    tp.run(1, table, tot)
    again = tp.result()
    assert again["vals"].tolist() == first["vals"].tolist() == [100, 101]
    assert again["vals"].ctypes.data != first["vals"].ctypes.data         # a fresh set of arrays per run
    assert "head" in first and "head" not in again                       # result() hands an array over once
    assert [c[2] for c in fn.calls] == [0, 1, 1]
