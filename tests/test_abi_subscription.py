"""The C boundary of the subscription store (corro_sub_create / _destroy / _update / _rows), CPU only: the
ctypes mirrors of corro_sub_events / corro_sub_rows_out against the layout gcc gives include/corro_hip.h, the
event type constants, the exported symbols, and the argument screen that runs before any device is touched."""
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import pytest

from corrosion_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = {"SubEvents": "corro_sub_events", "SubRowsOut": "corro_sub_rows_out"}
CONSTS = ("CORRO_SUB_INSERT", "CORRO_SUB_UPDATE", "CORRO_SUB_DELETE", "CORRO_SUB_STAGES")
SYMBOLS = ("corro_sub_create", "corro_sub_destroy", "corro_sub_update", "corro_sub_rows", "corro_sub_last_timings")
E_INVALID = -1


@pytest.fixture(scope="module")
def layout():
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
    d = tempfile.mkdtemp(prefix="corro_sub_abi_")
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


def test_subscription_structs_match_the_header_layout(layout):
    for py in PAIRS:
        st = getattr(L, py)
        assert C.sizeof(st) == layout[(py, "size")], py
        for name, _t in st._fields_:
            assert getattr(st, name).offset == layout[(py, name)], f"{py}.{name}"
    assert [n for n, _t in L.SubEvents._fields_[:5]] == ["nevents", "ninsert", "nupdate", "ndelete", "val_data_len"]


def test_event_type_constants_match_the_header(layout):
    assert layout[("const", "CORRO_SUB_INSERT")] == L.CORRO_SUB_INSERT == 0
    assert layout[("const", "CORRO_SUB_UPDATE")] == L.CORRO_SUB_UPDATE == 1
    assert layout[("const", "CORRO_SUB_DELETE")] == L.CORRO_SUB_DELETE == 2
    assert layout[("const", "CORRO_SUB_STAGES")] == L.CORRO_SUB_STAGES == 6


def test_subscription_symbols_are_exported():
    for name in SYMBOLS:
        assert name in L.EXPORTS
        assert hasattr(L.lib(), name)


def test_null_arguments_are_invalid_before_any_device_call():
    lib = L.lib()
    q, ev, rows, h = L.QueryIn(), L.SubEvents(), L.SubRowsOut(), C.c_void_p()
    q.nproj = 1
    for mem in (L.CORRO_MEM_HOST, L.CORRO_MEM_DEVICE):
        assert lib.corro_sub_create(None, C.byref(q), mem, 0, 0, C.byref(h)) == E_INVALID
        assert h.value is None
        for which in (0, 1):
            assert lib.corro_sub_update(None, None, 0, mem, C.byref(ev), which) == E_INVALID
            assert lib.corro_sub_rows(None, mem, C.byref(rows), which) == E_INVALID
            ms, n = (C.c_float * 6)(), C.c_uint32()
            assert lib.corro_sub_last_timings(None, which, ms, 6, C.byref(n)) == E_INVALID
    lib.corro_sub_destroy(None)                         # (a NULL handle is ignored)
