"""The C boundary of the row query (corro_query_rows), CPU only: the ctypes mirrors of corro_query_in /
corro_query_out against the layout gcc gives include/corro_hip.h, the flag, op and limit constants, the
exported symbol, and the argument screen that runs before any device is touched."""
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import pytest

from corrosion_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = {"QueryIn": "corro_query_in", "QueryOut": "corro_query_out"}
CONSTS = ("CORRO_QUERY_KEYED", "CORRO_QUERY_VALUES", "CORRO_QUERY_MAX_TERMS", "CORRO_QUERY_MAX_GROUPS",
          "CORRO_QUERY_MAX_PROJ", "CORRO_QOP_EQ", "CORRO_QOP_NE", "CORRO_QOP_LT", "CORRO_QOP_LE", "CORRO_QOP_GT",
          "CORRO_QOP_GE", "CORRO_QOP_IS_NULL", "CORRO_QOP_IS_NOT_NULL")
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
    lines += [f'  printf("const {name} %u\\n", (unsigned){name});' for name in CONSTS]
    lines += ["  return 0;", "}"]
    d = tempfile.mkdtemp(prefix="corro_query_abi_")
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


def test_query_structs_match_the_header_layout():
    got = _c_layout()
    for py in PAIRS:
        st = getattr(L, py)
        assert C.sizeof(st) == got[(py, "size")], py
        for name, _t in st._fields_:
            assert getattr(st, name).offset == got[(py, name)], f"{py}.{name}"


def test_query_constants_match_the_header():
    got = _c_layout()
    assert got[("const", "CORRO_QUERY_KEYED")] == L.CORRO_QUERY_KEYED == 1
    assert got[("const", "CORRO_QUERY_VALUES")] == L.CORRO_QUERY_VALUES == 2
    assert got[("const", "CORRO_QUERY_MAX_TERMS")] == L.CORRO_QUERY_MAX_TERMS >= 64
    assert got[("const", "CORRO_QUERY_MAX_GROUPS")] == L.CORRO_QUERY_MAX_GROUPS >= 64
    assert got[("const", "CORRO_QUERY_MAX_PROJ")] == L.CORRO_QUERY_MAX_PROJ >= 256
    ops = {"CORRO_QOP_EQ": "=", "CORRO_QOP_NE": "!=", "CORRO_QOP_LT": "<", "CORRO_QOP_LE": "<=", "CORRO_QOP_GT": ">",
           "CORRO_QOP_GE": ">=", "CORRO_QOP_IS_NULL": "is null", "CORRO_QOP_IS_NOT_NULL": "is not null"}
    for n, (name, sql) in enumerate(ops.items()):
        assert got[("const", name)] == L.QUERY_OPS[sql] == n
    assert L.QUERY_OPS["=="] == L.QUERY_OPS["="] and L.QUERY_OPS["<>"] == L.QUERY_OPS["!="]


def test_query_symbol_is_exported():
    assert "corro_query_rows" in L.EXPORTS
    assert hasattr(L.lib(), "corro_query_rows")


def test_null_arguments_are_invalid_before_any_device_call():
    lib = L.lib()
    i, o = L.QueryIn(), L.QueryOut()
    for mem in (L.CORRO_MEM_HOST, L.CORRO_MEM_DEVICE):
        for which in (0, 1):
            assert lib.corro_query_rows(None, C.byref(i), mem, C.byref(o), which) == E_INVALID
