"""CPU checks of the wire-encode entry point (corro_encode_changesets): the ctypes mirrors of its two
structs against the header as gcc lays it out, the exported symbol, and the argument screen that
runs before any device call."""
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import pytest

from corrosion_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = {"EncodeIn": "corro_encode_in", "Encoded": "corro_encoded"}


def _flat(st, prefix=""):
    """(dotted field name, offset) of a ctypes struct, nested structs included."""
    for name, t in st._fields_:
        yield prefix + name, getattr(st, name).offset
        if issubclass(t, C.Structure):
            for sub, off in _flat(t, prefix + name + "."):
                yield sub, getattr(st, name).offset + off


def _c_layout():
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        pytest.skip("no C compiler")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "corro_hip.h"', "int main(void) {"]
    for py, c in PAIRS.items():
        lines.append(f'  printf("{py} size %zu\\n", sizeof({c}));')
        for name, _off in _flat(getattr(L, py)):
            lines.append(f'  printf("{py} {name} %zu\\n", offsetof({c}, {name}));')
    lines += ["  return 0;", "}"]
    d = tempfile.mkdtemp(prefix="corro_abi_enc_")
    try:
        src, exe = os.path.join(d, "layout.c"), os.path.join(d, "layout")
        with open(src, "w") as f:
            f.write("\n".join(lines) + "\n")
        subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        out = subprocess.check_output([exe]).decode()
    finally:
        shutil.rmtree(d, ignore_errors=True)
    return {(py, name): int(v) for py, name, v in (ln.split() for ln in out.splitlines())}


def test_encode_structs_match_header_layout():
    got = _c_layout()
    for py in PAIRS:
        st = getattr(L, py)
        assert C.sizeof(st) == got[(py, "size")], py
        names = [n for n, _ in _flat(st)]
        assert len(names) == len(set(names))
        for name, off in _flat(st):
            assert off == got[(py, name)], f"{py}.{name}"
    # the fields the issue's contract names
    assert [n for n, _ in L.Encoded._fields_][:2] == ["nframes", "nbytes"]
    assert {"site", "version", "last_seq", "ts", "seq_start", "seq_end", "row_off", "row_count", "rows", "nrows",
            "max_buf_size", "payload", "cluster_id"} <= {n for n, _ in L.EncodeIn._fields_}


def test_symbol_is_exported_and_listed():
    assert "corro_encode_changesets" in L.EXPORTS
    assert hasattr(L.lib(), "corro_encode_changesets")
    assert L.lib().corro_abi_version() == 3


def test_null_arguments_are_refused_before_any_device_call():
    lib = L.lib()
    out = L.Encoded()
    assert lib.corro_encode_changesets(None, None, L.CORRO_MEM_HOST, C.byref(out), 0) == -1   # CORRO_E_INVALID
    # a non-NULL context handle is not dereferenced before `in` is checked
    fake = C.create_string_buffer(8)
    assert lib.corro_encode_changesets(C.addressof(fake), None, L.CORRO_MEM_HOST, C.byref(out), 0) == -1
    assert b"NULL" in lib.corro_last_error()
