"""CPU checks of corro_need_tails: the ctypes mirrors of its two structs against the header as gcc lays
it out, the exported symbol, and the refusals that come before any device work."""
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import pytest

import corrosion_amd as ca
from corrosion_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = {"TailsIn": "corro_tails_in", "TailsOut": "corro_tails_out"}


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
    d = tempfile.mkdtemp(prefix="corro_abi_tails_")
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
    # the arrays shared with the neighbours keep their names
    names = lambda st: {n for n, _ in st._fields_}
    assert {"kind", "start", "end", "need_keep", "need_site", "need_ent_off"} <= names(L.TailsIn) & names(L.ReqDecOut)
    assert {"grp_off", "version"} <= names(L.TailsIn) & names(L.SpansIn)
    assert "in_state" in names(L.TailsIn) & names(L.SpansOut)
    assert {"gap_off", "gap_start", "gap_end", "book_nsites", "book_ngaps"} <= names(L.TailsIn) & names(L.ReqDecIn)
    assert [n for n, _ in L.TailsOut._fields_][:2] == ["nranges", "nbytes"]


def test_symbol_is_exported_and_listed():
    assert "corro_need_tails" in L.EXPORTS
    assert hasattr(L.lib(), "corro_need_tails")
    assert L.lib().corro_abi_version() == 3


def test_every_declared_symbol_is_still_listed():
    from tests import test_abi
    test_abi.test_library_exports_every_declared_symbol()
    test_abi.test_abi_version()


def _minimal():
    """No need, no entry, no group, no book: the smallest call that reaches the device check."""
    keep = [(C.c_uint64 * 1)(0), (C.c_uint64 * 1)(0), (C.c_uint64 * 1)(7)]
    r = L.TailsIn()
    r.need_ent_off = C.addressof(keep[0])
    r.grp_off = C.addressof(keep[1])
    o = L.TailsOut()
    o.nranges, o.nbytes = 9, 9 * 49
    o.need_tail_off = C.addressof(keep[2])
    return r, o, keep


def _call(r, o, mem=L.CORRO_MEM_HOST, pas=0):
    fake = C.create_string_buffer(8)   # a context handle that must not be dereferenced
    return L.lib().corro_need_tails(C.addressof(fake), C.byref(r), mem, C.byref(o), pas)


def test_arguments_are_screened_before_any_device_call():
    fn = L.lib().corro_need_tails
    r, o, _keep = _minimal()
    fake = C.create_string_buffer(8)
    assert fn(None, C.byref(r), L.CORRO_MEM_HOST, C.byref(o), 0) == -1
    assert fn(C.addressof(fake), None, L.CORRO_MEM_HOST, C.byref(o), 0) == -1
    assert fn(C.addressof(fake), C.byref(r), L.CORRO_MEM_HOST, None, 0) == -1
    assert b"NULL" in L.lib().corro_last_error()
    assert _call(r, o, mem=7) == -1
    assert b"mem" in L.lib().corro_last_error()
    assert _call(r, o, pas=2) == -1
    assert b"pass" in L.lib().corro_last_error()
    r.payload = 2
    assert _call(r, o) == -1
    assert b"payload" in L.lib().corro_last_error()


NEED_ARRAYS = ("kind", "start", "end", "need_keep", "need_site", "in_state")


def test_refuses_missing_arrays_and_a_partial_book():
    for field in ("need_ent_off", "grp_off"):
        r, o, _keep = _minimal()
        setattr(r, field, None)
        assert _call(r, o) == -1, field
    some = (C.c_uint64 * 4)()
    for missing in NEED_ARRAYS:                             # one need, one of its arrays missing
        r, o, _keep = _minimal()
        r.nneeds = 1
        for field in NEED_ARRAYS:
            setattr(r, field, None if field == missing else C.addressof(some))
        o.need_host = C.addressof(some)
        assert _call(r, o) == -1, missing
        assert b"NULL" in L.lib().corro_last_error()
    r, o, _keep = _minimal()
    r.ngroups = 1                                           # groups without their versions
    assert _call(r, o) == -1
    r, o, _keep = _minimal()
    o.need_tail_off = None
    assert _call(r, o) == -1
    r, o, _keep = _minimal()
    r.nneeds = 1
    for field in NEED_ARRAYS:
        setattr(r, field, C.addressof(some))
    assert _call(r, o) == -1                                # a need and no need_host
    # a book given in part
    for fields in (("gap_off",), ("buf_off",), ("gap_off", "buf_off", "book_ngaps"), ("gap_off", "buf_off", "book_nbuf"),
                   ("book_nsites",), ("gap_off", "buf_off", "gap_start", "book_ngaps")):
        r, o, _keep = _minimal()
        for field in fields:
            setattr(r, field, 1 if field.startswith("book_") else C.addressof(some))
        assert _call(r, o) == -1, fields
        assert b"book" in L.lib().corro_last_error()
    # pass 1: ranges and no range arrays; totals that cannot be pass 0's
    r, o, keep = _minimal()
    assert _call(r, o, pas=1) == -1
    assert b"NULL" in L.lib().corro_last_error()
    o.nbytes = 9 * 49 + 1
    assert _call(r, o, pas=1) == -1
    assert b"pass 0" in L.lib().corro_last_error()
    r, o, keep = _minimal()
    o.nranges, o.nbytes = 1 << 32, (1 << 32) * 49
    assert _call(r, o, pas=1) == -6
    r, o, keep = _minimal()
    r.nneeds = 1 << 40
    for field in NEED_ARRAYS:
        setattr(r, field, C.addressof(some))
    o.need_host = C.addressof(some)
    assert _call(r, o) == -6
    assert keep[2][0] == 7


def test_refuses_without_a_device():
    if ca.device_count() > 0:
        pytest.skip("a GPU is visible")
    r, o, keep = _minimal()
    assert _call(r, o) == -7                                # CORRO_E_NO_DEVICE
    assert keep[2][0] == 7 and (o.nranges, o.nbytes) == (9, 9 * 49)   # nothing was written: the sentinels stand
    some = (C.c_uint64 * 4)(7, 7, 7, 7)
    o.range_start = o.range_end = o.buf = o.frame_off = C.addressof(some)
    assert _call(r, o, pas=1) == -7
    assert list(some) == [7, 7, 7, 7]
