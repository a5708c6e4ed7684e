"""The C boundary of the row read (corro_read_rows, corro_pk_find, corro_pk_find_device), CPU only: the
ctypes mirrors of corro_read_in / corro_read_out against the layout gcc gives include/corro_hip.h, the
exported symbols, and the argument screen that runs before any device is touched."""
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import pytest

from corrosion_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = {"ReadIn": "corro_read_in", "ReadOut": "corro_read_out"}
E_INVALID = -1


def _c_layout():
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        pytest.skip("no C compiler")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "corro_hip.h"', "int main(void) {"]
    for py, c in PAIRS.items():
        lines.append(f'  printf("{py} size %zu\\n", sizeof({c}));')
        for name, _t in getattr(L, py)._fields_:
            lines.append(f'  printf("{py} {name} %zu\\n", offsetof({c}, {name}));')
    lines += ['  printf("flag values %u\\n", (unsigned)CORRO_READ_VALUES);',
              '  printf("absent is_max %d\\n", CORRO_PK_ABSENT == 0xFFFFFFFFFFFFFFFFull);', "  return 0;", "}"]
    d = tempfile.mkdtemp(prefix="corro_read_abi_")
    try:
        src, exe = os.path.join(d, "layout.c"), os.path.join(d, "layout")
        with open(src, "w") as f:
            f.write("\n".join(lines) + "\n")
        subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        out = subprocess.check_output([exe]).decode()
    finally:
        shutil.rmtree(d, ignore_errors=True)
    got = {}
    for ln in out.splitlines():
        py, name, v = ln.split()
        got[(py, name)] = int(v)
    return got


def test_read_structs_match_the_header_layout():
    got = _c_layout()
    for py in PAIRS:
        st = getattr(L, py)
        assert C.sizeof(st) == got[(py, "size")], py
        for name, _t in st._fields_:
            assert getattr(st, name).offset == got[(py, name)], f"{py}.{name}"
    assert got[("flag", "values")] == L.CORRO_READ_VALUES
    assert got[("absent", "is_max")] == 1 and L.CORRO_PK_ABSENT == 2**64 - 1


def test_read_symbols_are_exported():
    lib = L.lib()
    for name in ("corro_read_rows", "corro_pk_find", "corro_pk_find_device"):
        assert name in L.EXPORTS
        assert hasattr(lib, name)


def test_null_arguments_are_invalid_before_any_device_call():
    lib = L.lib()
    i, o = L.ReadIn(), L.ReadOut()
    for mem in (L.CORRO_MEM_HOST, L.CORRO_MEM_DEVICE):
        for which in (0, 1):
            assert lib.corro_read_rows(None, C.byref(i), mem, C.byref(o), which) == E_INVALID
    keys = (C.c_uint64 * 1)()
    off = (C.c_uint64 * 2)(0, 2)
    assert lib.corro_pk_find(None, 0, b"\x01\x01", off, 1, keys) == E_INVALID
    assert lib.corro_pk_find_device(None, 0, b"\x01\x01", off, 1, keys) == E_INVALID
