"""CPU checks of the request planning entry point (corro_plan_requests): the ctypes mirrors of its two
structs against the header as gcc lays it out, the exported symbol, and the refusals that come before
any device work."""
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import pytest

import corrosion_amd as ca
from corrosion_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = {"RequestIn": "corro_request_in", "Requests": "corro_requests"}


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
    d = tempfile.mkdtemp(prefix="corro_abi_req_")
    try:
        src, exe = os.path.join(d, "layout.c"), os.path.join(d, "layout")
        with open(src, "w") as f:
            f.write("\n".join(lines) + "\n")
        subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        out = subprocess.check_output([exe]).decode()
    finally:
        shutil.rmtree(d, ignore_errors=True)
    return {(py, name): int(v) for py, name, v in (ln.split() for ln in out.splitlines())}


def test_request_structs_match_header_layout():
    got = _c_layout()
    for py in PAIRS:
        st = getattr(L, py)
        assert C.sizeof(st) == got[(py, "size")], py
        for name, _t in st._fields_:
            assert getattr(st, name).offset == got[(py, name)], f"{py}.{name}"
    assert [n for n, _ in L.Requests._fields_] == ["nframes", "nbytes", "grp_frame_off", "buf", "frame_off",
                                                   "frame_entry", "frame_round", "frame_needs"]
    # the need CSR is corro_needs_out's, under the same names
    assert {"need_off", "kind", "start", "end", "sr_off", "sr_n", "s_start", "s_end"} <= (
        {n for n, _ in L.RequestIn._fields_} & {n for n, _ in L.NeedsOut._fields_})
    assert {"n", "site", "nneeds", "nseqs", "ngroups", "grp_ent_off", "grp_session", "chunk_size", "drain"} <= {
        n for n, _ in L.RequestIn._fields_}


def test_symbol_is_exported_and_listed():
    assert "corro_plan_requests" in L.EXPORTS
    assert hasattr(L.lib(), "corro_plan_requests")
    assert L.lib().corro_abi_version() == 3


def _minimal():
    keep = [(C.c_uint64 * 2)(0, 0), (C.c_uint64 * 1)(0)]
    r = L.RequestIn()
    r.need_off = C.addressof(keep[0])
    r.grp_ent_off = C.addressof(keep[1])
    r.chunk_size, r.drain = 10, 10
    o = L.Requests()
    gfo = (C.c_uint64 * 1)(7)
    o.grp_frame_off = C.addressof(gfo)
    return r, o, keep + [gfo]


def test_arguments_are_screened_before_any_device_call():
    lib = L.lib()
    r, o, _keep = _minimal()
    fake = C.create_string_buffer(8)   # a context handle that must not be dereferenced
    assert lib.corro_plan_requests(None, C.byref(r), L.CORRO_MEM_HOST, C.byref(o), 0) == -1
    assert lib.corro_plan_requests(C.addressof(fake), None, L.CORRO_MEM_HOST, C.byref(o), 0) == -1
    assert b"NULL" in lib.corro_last_error()
    assert lib.corro_plan_requests(C.addressof(fake), C.byref(r), 7, C.byref(o), 0) == -1
    assert lib.corro_plan_requests(C.addressof(fake), C.byref(r), L.CORRO_MEM_HOST, C.byref(o), 2) == -1
    for field in ("chunk_size", "drain"):
        r, o, _keep = _minimal()
        setattr(r, field, 0)
        assert lib.corro_plan_requests(C.addressof(fake), C.byref(r), L.CORRO_MEM_HOST, C.byref(o), 0) == -1
        assert b"chunk_size and drain" in lib.corro_last_error()


def test_refuses_without_a_device():
    if ca.device_count() > 0:
        pytest.skip("a GPU is visible")
    lib = L.lib()
    r, o, keep = _minimal()
    fake = C.create_string_buffer(8)
    assert lib.corro_plan_requests(C.addressof(fake), C.byref(r), L.CORRO_MEM_HOST, C.byref(o), 0) == -7  # CORRO_E_NO_DEVICE
    assert keep[-1][0] == 7   # nothing was written
