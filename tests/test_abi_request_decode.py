"""CPU checks of the request decode entry points (corro_decode_requests, corro_need_spans): the ctypes
mirrors of their four structs against the header as gcc lays it out, the exported symbols, and the
refusals that come before any device work."""
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import pytest

import corrosion_amd as ca
from corrosion_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = {"ReqDecIn": "corro_reqdec_in", "ReqDecOut": "corro_reqdec_out", "SpansIn": "corro_spans_in",
         "SpansOut": "corro_spans_out"}


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
    d = tempfile.mkdtemp(prefix="corro_abi_reqdec_")
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
    # the decoded needs carry corro_needs_out's names, and the spans corro_encode_in's
    names = lambda st: {n for n, _ in st._fields_}
    assert {"kind", "start", "end", "sr_off", "sr_n", "s_start", "s_end"} <= names(L.ReqDecOut) & names(L.NeedsOut)
    assert {"site", "version", "last_seq", "ts", "seq_start", "seq_end", "row_off", "row_count"} <= (
        names(L.SpansOut) & names(L.EncodeIn))
    assert {"grp_off", "version", "last_seq", "ts", "grp_row_off", "grp_rows"} <= names(L.SpansIn) & names(L.ExtractOut)
    assert [n for n, _ in L.ReqDecOut._fields_][:4] == ["npairs", "nneeds", "nseqs", "nents"]


def test_symbols_are_exported_and_listed():
    for name in ("corro_decode_requests", "corro_need_spans"):
        assert name in L.EXPORTS
        assert hasattr(L.lib(), name)
    assert L.lib().corro_abi_version() == 3


def _minimal_decode():
    keep = [(C.c_uint64 * 1)(0), (C.c_uint64 * 1)(7), (C.c_int32 * 1)(7)]
    r = L.ReqDecIn()
    r.frame_off = C.addressof(keep[0])
    o = L.ReqDecOut()
    o.npairs = o.nneeds = o.nseqs = o.nents = 9
    o.frame_pair_off = C.addressof(keep[1])
    o.frame_status = C.addressof(keep[2])
    return r, o, keep


def _minimal_spans():
    keep = [(C.c_uint64 * 1)(0), (C.c_uint64 * 1)(0), (C.c_uint64 * 1)(7)]
    r = L.SpansIn()
    r.need_ent_off = C.addressof(keep[0])
    r.grp_off = C.addressof(keep[1])
    o = L.SpansOut()
    o.nspans = 9
    o.need_span_off = C.addressof(keep[2])
    return r, o, keep


CALLS = [("corro_decode_requests", _minimal_decode), ("corro_need_spans", _minimal_spans)]


@pytest.mark.parametrize("name,minimal", CALLS, ids=[c[0] for c in CALLS])
def test_arguments_are_screened_before_any_device_call(name, minimal):
    fn = getattr(L.lib(), name)
    r, o, _keep = minimal()
    fake = C.create_string_buffer(8)   # a context handle that must not be dereferenced
    assert fn(None, C.byref(r), L.CORRO_MEM_HOST, C.byref(o), 0) == -1
    assert fn(C.addressof(fake), None, L.CORRO_MEM_HOST, C.byref(o), 0) == -1
    assert fn(C.addressof(fake), C.byref(r), L.CORRO_MEM_HOST, None, 0) == -1
    assert b"NULL" in L.lib().corro_last_error()
    assert fn(C.addressof(fake), C.byref(r), 7, C.byref(o), 0) == -1
    assert b"mem" in L.lib().corro_last_error()
    assert fn(C.addressof(fake), C.byref(r), L.CORRO_MEM_HOST, C.byref(o), 2) == -1
    assert b"pass" in L.lib().corro_last_error()


def test_decode_refuses_missing_arrays_and_a_partial_book():
    fn = L.lib().corro_decode_requests
    fake = C.create_string_buffer(8)
    r, o, _keep = _minimal_decode()
    r.frame_off = None
    assert fn(C.addressof(fake), C.byref(r), L.CORRO_MEM_HOST, C.byref(o), 0) == -1
    r, o, _keep = _minimal_decode()
    r.len = 4                                               # bytes without a buffer
    assert fn(C.addressof(fake), C.byref(r), L.CORRO_MEM_HOST, C.byref(o), 0) == -1
    r, o, _keep = _minimal_decode()
    o.frame_pair_off = None
    assert fn(C.addressof(fake), C.byref(r), L.CORRO_MEM_HOST, C.byref(o), 0) == -1
    r, o, keep = _minimal_decode()
    known = (C.c_uint8 * 1)(1)
    r.book_nsites, r.book_known = 1, C.addressof(known)     # known without max / gap_off
    assert fn(C.addressof(fake), C.byref(r), L.CORRO_MEM_HOST, C.byref(o), 0) == -1
    assert b"book" in L.lib().corro_last_error()
    r, o, _keep = _minimal_decode()
    r.nframes = 1 << 31
    assert fn(C.addressof(fake), C.byref(r), L.CORRO_MEM_HOST, C.byref(o), 0) == -6
    r, o, keep = _minimal_decode()
    o.npairs = o.nneeds = o.nseqs = o.nents = 0             # pass 1 always writes the closing offsets
    assert fn(C.addressof(fake), C.byref(r), L.CORRO_MEM_HOST, C.byref(o), 1) == -1
    assert keep[1][0] == 7 and keep[2][0] == 7


def test_spans_refuse_missing_arrays():
    fn = L.lib().corro_need_spans
    fake = C.create_string_buffer(8)
    for field in ("need_ent_off", "grp_off"):
        r, o, _keep = _minimal_spans()
        setattr(r, field, None)
        assert fn(C.addressof(fake), C.byref(r), L.CORRO_MEM_HOST, C.byref(o), 0) == -1
    r, o, _keep = _minimal_spans()
    r.nneeds = 1                                            # needs without their arrays
    assert fn(C.addressof(fake), C.byref(r), L.CORRO_MEM_HOST, C.byref(o), 0) == -1
    r, o, _keep = _minimal_spans()
    o.need_span_off = None
    assert fn(C.addressof(fake), C.byref(r), L.CORRO_MEM_HOST, C.byref(o), 0) == -1
    r, o, _keep = _minimal_spans()
    o.nspans = 3                                            # pass 1 with spans and no span arrays
    assert fn(C.addressof(fake), C.byref(r), L.CORRO_MEM_HOST, C.byref(o), 1) == -1


@pytest.mark.parametrize("name,minimal", CALLS, ids=[c[0] for c in CALLS])
def test_refuses_without_a_device(name, minimal):
    if ca.device_count() > 0:
        pytest.skip("a GPU is visible")
    r, o, keep = minimal()
    fake = C.create_string_buffer(8)
    before = [k[0] for k in keep]
    assert 7 in before
    assert getattr(L.lib(), name)(C.addressof(fake), C.byref(r), L.CORRO_MEM_HOST, C.byref(o), 0) == -7  # CORRO_E_NO_DEVICE
    assert [k[0] for k in keep] == before                   # nothing was written: the sentinels stand
    assert (getattr(o, "npairs", 9), getattr(o, "nspans", 9)) == (9, 9)
