"""CPU checks of corro_bookie_sync_book and corro_encode_states: the ctypes mirrors of their three structs
against the header as gcc lays it out, the exported symbols, and the refusals that come before any device
work."""
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import corrosion_amd as ca
from corrosion_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = {"SyncBook": "corro_sync_book", "StateEncIn": "corro_stateenc_in", "StateEncOut": "corro_stateenc_out"}


def _c_layout():
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        pytest.skip("no C compiler")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "corro_hip.h"', "int main(void) {"]
    for py, c in PAIRS.items():
        lines.append(f'  printf("{py} size %zu\\n", sizeof({c}));')
        for name, _t in getattr(L, py)._fields_:
            lines.append(f'  printf("{py} {name} %zu\\n", offsetof({c}, {name}));')
    lines += ["  return 0;", "}"]
    d = tempfile.mkdtemp(prefix="corro_abi_stateenc_")
    try:
        src, exe = os.path.join(d, "layout.c"), os.path.join(d, "layout")
        with open(src, "w") as f:
            f.write("\n".join(lines) + "\n")
        subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        out = subprocess.check_output([exe]).decode()
    finally:
        shutil.rmtree(d, ignore_errors=True)
    return {(py, name): int(v) for py, name, v in (ln.split() for ln in out.splitlines())}


def test_structs_match_header_layout():
    got = _c_layout()
    for py in PAIRS:
        st = getattr(L, py)
        assert C.sizeof(st) == got[(py, "size")], py
        for name, _t in st._fields_:
            assert getattr(st, name).offset == got[(py, name)], f"{py}.{name}"
    # the encoder's row arrays are the sync book's, every one of them, in its order
    book = [n for n, _ in L.SyncBook._fields_]
    enc = [n for n, _ in L.StateEncIn._fields_]
    assert enc[enc.index("nrows"):enc.index("nrows") + len(book)] == book


def test_symbols_are_exported_and_listed():
    for sym in ("corro_bookie_sync_book", "corro_encode_states"):
        assert sym in L.EXPORTS
        assert hasattr(L.lib(), sym)
    assert L.lib().corro_abi_version() == 3


class _Call:
    """Two states over three rows (one gap, one partial with one present range), every output array present
    and holding sentinels."""

    def __init__(self):
        u64 = lambda *v: np.array(v, np.uint64)
        self.arr = {"self_actor": np.zeros(32, np.uint8), "has_ts": np.zeros(2, np.uint8), "ts": u64(0, 0),
                    "state_row_off": u64(0, 2, 3), "actor": np.zeros(48, np.uint8), "max": np.array([5, -1, 7], np.int64),
                    "gap_off": u64(0, 1, 1, 1), "gap_start": u64(2), "gap_end": u64(3),
                    "part_off": u64(0, 0, 0, 1), "part_version": u64(7), "part_last_seq": u64(9),
                    "psr_off": u64(0, 1), "psr_start": u64(0), "psr_end": u64(4)}
        r = L.StateEncIn()
        r.nstates, r.nrows, r.ngaps, r.nparts, r.npsr = 2, 3, 1, 1, 1
        for k, a in self.arr.items():
            setattr(r, k, a.ctypes.data)
        self.r = r
        o = L.StateEncOut()
        self.out = {}
        for name, t in L.StateEncOut._fields_:
            if t is C.c_void_p:
                self.out[name] = np.full(64, 7, np.uint8)
                setattr(o, name, self.out[name].ctypes.data)
        self.o = o
        self.fake = C.create_string_buffer(8)      # a context handle that must not be dereferenced

    def __call__(self, which=0, mem=L.CORRO_MEM_HOST):
        before = self.o.total_bytes
        rc = L.lib().corro_encode_states(C.addressof(self.fake), C.byref(self.r), mem, C.byref(self.o), which)
        assert all((a == 7).all() for a in self.out.values())       # a refused call writes nothing
        assert self.o.total_bytes == before
        return rc


def test_arguments_are_screened_before_any_device_call():
    fn = L.lib().corro_encode_states
    c = _Call()
    assert fn(None, C.byref(c.r), L.CORRO_MEM_HOST, C.byref(c.o), 0) == -1
    assert fn(C.addressof(c.fake), None, L.CORRO_MEM_HOST, C.byref(c.o), 0) == -1
    assert fn(C.addressof(c.fake), C.byref(c.r), L.CORRO_MEM_HOST, None, 0) == -1
    assert b"NULL" in L.lib().corro_last_error()
    assert c(mem=7) == -1 and b"mem" in L.lib().corro_last_error()
    assert c(which=2) == -1 and b"pass" in L.lib().corro_last_error()
    for field in c.arr:
        c = _Call()
        setattr(c.r, field, None)
        assert c() == -1, field
    for field in ("state_status", "frame_off", "n_heads", "n_need", "n_partial"):
        c = _Call()
        setattr(c.o, field, None)
        assert c() == -1, field
    c = _Call()
    c.o.total_bytes = 41
    c.o.buf = None
    assert c(which=1) == -1 and b"buf" in L.lib().corro_last_error()
    for field in ("nstates", "nrows", "ngaps", "nparts", "npsr"):
        c = _Call()
        setattr(c.r, field, 1 << 31)
        assert c() == -6, field


@pytest.mark.parametrize("field,values", [("state_row_off", [0, 3, 2]), ("state_row_off", [0, 2, 4]),
                                          ("gap_off", [0, 1, 1, 2]), ("gap_off", [0, 0, 0, 0]),
                                          ("part_off", [0, 0, 0, 2]), ("psr_off", [0, 0])], ids=str)
def test_offsets_that_disagree_with_the_counts_are_refused(field, values):
    """state_row_off that decreases or passes nrows, global offset arrays whose ends are not their counts."""
    c = _Call()
    c.arr[field][:] = values
    assert c() == -1 and b"state_row_off" in L.lib().corro_last_error()
    assert c(which=1) == -1


def test_refuses_without_a_device():
    if ca.device_count() > 0:
        pytest.skip("a GPU is visible")
    c = _Call()
    assert c() == -7                                                 # CORRO_E_NO_DEVICE
    assert c(which=1) == -7


def test_sync_book_of_an_empty_bookie_and_its_refusals():
    """The host half needs no device: an empty bookie gives a book of no rows and closed offset arrays, and
    pass 1 with counts that are not the bookie's writes nothing."""
    bk = ca.agent.Bookie()
    book = bk.sync_book()
    assert book["actor"].shape == (0, 16) and book["max"].size == 0
    assert [list(book[k]) for k in ("gap_off", "part_off", "psr_off")] == [[0], [0], [0]]
    fn = L.lib().corro_bookie_sync_book
    o = L.SyncBook()
    assert fn(None, C.byref(o), 0) == -1 and fn(bk._h, None, 0) == -1
    assert fn(bk._h, C.byref(o), 2) == -1 and b"pass" in L.lib().corro_last_error()
    arrays = {}
    for name, t in L.SyncBook._fields_:
        if t is C.c_void_p:
            arrays[name] = np.full(32, 7, np.uint8)
            setattr(o, name, arrays[name].ctypes.data)
    for field in ("nrows", "ngaps", "nparts", "npsr"):
        assert fn(bk._h, C.byref(o), 0) == 0 and getattr(o, field) == 0
        setattr(o, field, 1)
        assert fn(bk._h, C.byref(o), 1) == -1 and b"counts differ" in L.lib().corro_last_error()
        assert all((a == 7).all() for a in arrays.values())
    assert fn(bk._h, C.byref(o), 0) == 0
    o.gap_off = None
    assert fn(bk._h, C.byref(o), 1) == -1 and b"NULL" in L.lib().corro_last_error()
