"""CPU checks of corro_assemble_answers: the ctypes mirrors of its two structs against the header as gcc
lays it out, the exported symbol, and the refusals that come before any device work."""
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import pytest

import corrosion_amd as ca
from corrosion_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = {"AssembleIn": "corro_assemble_in", "Assembled": "corro_assembled"}


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
    d = tempfile.mkdtemp(prefix="corro_abi_assemble_")
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
    assert {"frame_pair_off", "pair_need_off", "need_keep"} <= names(L.AssembleIn) & names(L.ReqDecOut)
    assert "need_span_off" in names(L.AssembleIn) & names(L.SpansOut)
    assert "span_frame_off" in names(L.AssembleIn) & names(L.Encoded)
    assert {"need_tail_off", "need_host"} <= names(L.AssembleIn) & names(L.TailsOut)
    assert [n for n, _ in L.Assembled._fields_] == ["nbytes", "need_ans_off", "frame_ans_off", "frame_host", "buf"]


def test_symbol_is_exported_and_listed():
    assert "corro_assemble_answers" in L.EXPORTS
    assert hasattr(L.lib(), "corro_assemble_answers")
    assert L.lib().corro_abi_version() == 3


def test_every_declared_symbol_is_still_listed():
    from tests import test_abi
    test_abi.test_library_exports_every_declared_symbol()
    test_abi.test_abi_version()


def _minimal():
    """No frame, no pair, no need, no span, no range: the smallest call that reaches the device check."""
    keep = [(C.c_uint64 * 1)(0) for _ in range(4)] + [(C.c_uint64 * 1)(7), (C.c_uint64 * 1)(7)]
    r = L.AssembleIn()
    r.frame_pair_off, r.pair_need_off = C.addressof(keep[0]), C.addressof(keep[1])
    r.need_span_off, r.need_tail_off = C.addressof(keep[2]), C.addressof(keep[3])
    o = L.Assembled()
    o.nbytes = 9
    o.need_ans_off, o.frame_ans_off = C.addressof(keep[4]), C.addressof(keep[5])
    return r, o, keep


def _call(r, o, mem=L.CORRO_MEM_HOST, pas=0):
    fake = C.create_string_buffer(8)   # a context handle that must not be dereferenced
    return L.lib().corro_assemble_answers(C.addressof(fake), C.byref(r), mem, C.byref(o), pas)


def test_arguments_are_screened_before_any_device_call():
    fn = L.lib().corro_assemble_answers
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


def test_refuses_missing_arrays_and_sizes_that_cannot_be():
    some = (C.c_uint64 * 4)()
    for field in ("frame_pair_off", "pair_need_off", "need_span_off", "need_tail_off"):
        r, o, _keep = _minimal()
        setattr(r, field, None)
        assert _call(r, o) == -1, field
        assert b"NULL" in L.lib().corro_last_error()
    for missing in ("need_keep", "need_host"):                 # one need, one of its arrays missing
        r, o, _keep = _minimal()
        r.nneeds = 1
        r.need_keep = r.need_host = C.addressof(some)
        setattr(r, missing, None)
        assert _call(r, o) == -1, missing
    for missing in ("span_frame_off", "enc_frame_off", "enc_buf"):     # spans without the encoder's arrays
        r, o, _keep = _minimal()
        r.nspans, r.enc_nbytes = 1, 8
        r.span_frame_off = r.enc_frame_off = r.enc_buf = C.addressof(some)
        setattr(r, missing, None)
        assert _call(r, o) == -1, missing
        assert b"NULL" in L.lib().corro_last_error()
    r, o, _keep = _minimal()
    r.nranges, r.tail_nbytes = 1, 49                           # a range and no tail buffer
    assert _call(r, o) == -1
    for payload, nbytes in ((0, 55), (1, 49), (0, 48), (0, 0)):        # tail_nbytes is not nranges frames
        r, o, _keep = _minimal()
        r.nranges, r.tail_nbytes, r.payload, r.tail_buf = 1, nbytes, payload, C.addressof(some)
        assert _call(r, o) == -1, (payload, nbytes)
        assert b"tail_nbytes" in L.lib().corro_last_error()
    for field in ("need_ans_off", "frame_ans_off"):
        r, o, _keep = _minimal()
        setattr(o, field, None)
        assert _call(r, o) == -1, field
    r, o, _keep = _minimal()
    r.nframes = 1                                               # a frame and no frame_host
    assert _call(r, o) == -1
    r, o, _keep = _minimal()
    assert _call(r, o, pas=1) == -1                             # bytes and no buffer
    assert b"buf" in L.lib().corro_last_error()
    for field in ("nframes", "npairs", "nneeds", "nspans", "enc_nframes", "enc_nbytes"):
        r, o, keep = _minimal()
        r.need_keep = r.need_host = r.span_frame_off = r.enc_frame_off = r.enc_buf = o.frame_host = C.addressof(some)
        setattr(r, field, 1 << 40)
        assert _call(r, o) == -6, field
    r, o, keep = _minimal()
    r.nranges, r.tail_nbytes, r.tail_buf = 1 << 32, (1 << 32) * 49, C.addressof(some)
    assert _call(r, o) == -6
    assert keep[4][0] == 7 and keep[5][0] == 7 and o.nbytes == 9


def test_refuses_without_a_device():
    if ca.device_count() > 0:
        pytest.skip("a GPU is visible")
    r, o, keep = _minimal()
    assert _call(r, o) == -7                                   # CORRO_E_NO_DEVICE
    assert keep[4][0] == 7 and keep[5][0] == 7 and o.nbytes == 9       # nothing was written: the sentinels stand
    some = (C.c_uint64 * 4)(7, 7, 7, 7)
    o.buf = C.addressof(some)
    assert _call(r, o, pas=1) == -7
    assert list(some) == [7, 7, 7, 7]
