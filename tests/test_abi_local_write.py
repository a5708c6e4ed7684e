"""The C boundary of the local write (corro_local_write, corro_local_bound), CPU only: the ctypes mirrors of
corro_local_in / corro_local_out against the layout gcc gives include/corro_hip.h, the op kinds and the new
error code, the exported symbols, and the argument screen that runs before any device is touched. (The bound
helper reads the schema of a context, which only a device gives: its value is checked in the GPU suite and
against tests/local_write_model.bound.)"""
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import pytest

import local_write_model as M
from corrosion_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = {"LocalIn": "corro_local_in", "LocalOut": "corro_local_out"}
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
    lines += ['  printf("op kinds %d\\n", CORRO_OP_INSERT + 10 * CORRO_OP_UPDATE + 100 * CORRO_OP_UPSERT + 1000 * CORRO_OP_DELETE);',
              '  printf("e constraint %d\\n", (int)CORRO_E_CONSTRAINT);', "  return 0;", "}"]
    d = tempfile.mkdtemp(prefix="corro_local_abi_")
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


def test_local_structs_match_the_header_layout():
    got = _c_layout()
    for py in PAIRS:
        st = getattr(L, py)
        assert C.sizeof(st) == got[(py, "size")], py
        for name, _t in st._fields_:
            assert getattr(st, name).offset == got[(py, name)], f"{py}.{name}"
    assert got[("op", "kinds")] == L.CORRO_OP_INSERT + 10 * L.CORRO_OP_UPDATE + 100 * L.CORRO_OP_UPSERT + 1000 * L.CORRO_OP_DELETE
    assert (L.CORRO_OP_INSERT, L.CORRO_OP_UPDATE, L.CORRO_OP_UPSERT, L.CORRO_OP_DELETE) == (M.INSERT, M.UPDATE, M.UPSERT, M.DELETE)
    assert got[("e", "constraint")] == L.CORRO_E_CONSTRAINT == -8 and L.ERRORS[-8] == "CORRO_E_CONSTRAINT"


def test_local_symbols_are_exported():
    lib = L.lib()
    for name in ("corro_local_write", "corro_local_bound"):
        assert name in L.EXPORTS
        assert hasattr(lib, name)


def test_null_arguments_are_invalid_before_any_device_call():
    lib = L.lib()
    i, o = L.LocalIn(), L.LocalOut()
    for mem in (L.CORRO_MEM_HOST, L.CORRO_MEM_DEVICE):
        assert lib.corro_local_write(None, None, None, C.byref(i), mem, C.byref(o)) == E_INVALID
    b = C.c_uint64()
    assert lib.corro_local_bound(None, None, None, None, 0, C.byref(b)) == E_INVALID


def test_model_bound_counts_as_the_header_states():
    tables = [{"name": "t", "pk": "integer", "cols": [["a", ""], ["b", ""], ["c", ""]]}, {"name": "p", "pk": "integer", "cols": []}]
    stmts = [(M.INSERT, 0, 1, [(1, 1)]), (M.UPSERT, 0, 1, []), (M.UPDATE, 0, 1, [(1, 1), (2, 2)]), (M.DELETE, 0, 1, []),
             (M.UPSERT, 1, 1, []), (M.UPDATE, 1, 1, [])]
    assert M.bound(tables, stmts) == 4 + 4 + 2 + 1 + 1 + 0
