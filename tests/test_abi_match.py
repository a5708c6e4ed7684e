"""CPU checks of corro_match_changes: the ctypes mirrors of its two structs against the header as gcc lays
it out, the exported symbol, the refusals that come before any device work, and MatchFilters' classes and
bit matrix (no device call)."""
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import corrosion_amd as ca
from corrosion_amd import _lib as L
from corrosion_amd.updates import MatchFilters

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = {"MatchIn": "corro_match_in", "MatchOut": "corro_match_out", "Changeset": "corro_changeset"}


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
    d = tempfile.mkdtemp(prefix="corro_abi_match_")
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
    # updates.py writes (change_off, change_count) pairs into records of u64 words
    assert C.sizeof(L.Changeset) % 8 == 0 and L.Changeset.change_off.offset % 8 == 0


def test_symbol_is_exported_and_listed():
    assert "corro_match_changes" in L.EXPORTS
    assert hasattr(L.lib(), "corro_match_changes")
    assert L.lib().corro_abi_version() == 3


class _Call:
    """Four changes in two changesets (one empty header between them), two classes over three column slots;
    every output array present and holding sentinels."""

    def __init__(self, ranges=((0, 3), (0, 0), (3, 1))):
        self.arr = {"pk": np.array([1, 1, 2, 1], np.uint64), "table_cid": np.array([0, 1, 2, 0], np.uint32),
                    "cl": np.array([1, 1, 1, 2], np.uint32), "impactful": np.ones(4, np.uint8),
                    "col_class_bits": np.array([3, 1, 2], np.uint32)}
        self.cs = (L.Changeset * len(ranges))()
        for h, (off, cnt) in zip(self.cs, ranges):
            h.change_off, h.change_count = off, cnt
        r = L.MatchIn()
        r.n, r.ncs, r.nclasses, r.nslots = 4, len(ranges), 2, 3
        for k, a in self.arr.items():
            setattr(r, k, a.ctypes.data)
        r.cs = C.addressof(self.cs)
        self.r = r
        o = L.MatchOut()
        self.out = {}
        for name, t in L.MatchOut._fields_:
            if t is C.c_void_p:
                self.out[name] = np.full(64, 7, np.uint8)
                setattr(o, name, self.out[name].ctypes.data)
        self.o = o
        self.fake = C.create_string_buffer(8)      # a context handle that must not be dereferenced

    def __call__(self, which=0, mem=L.CORRO_MEM_HOST):
        before = self.o.ncand
        rc = L.lib().corro_match_changes(C.addressof(self.fake), C.byref(self.r), mem, C.byref(self.o), which)
        assert all((a == 7).all() for a in self.out.values())       # a refused call writes nothing
        assert self.o.ncand == before
        return rc


def test_arguments_are_screened_before_any_device_call():
    fn = L.lib().corro_match_changes
    c = _Call()
    assert fn(None, C.byref(c.r), L.CORRO_MEM_HOST, C.byref(c.o), 0) == -1
    assert fn(C.addressof(c.fake), None, L.CORRO_MEM_HOST, C.byref(c.o), 0) == -1
    assert fn(C.addressof(c.fake), C.byref(c.r), L.CORRO_MEM_HOST, None, 0) == -1
    assert b"NULL" in L.lib().corro_last_error()
    assert c(mem=7) == -1 and b"mem" in L.lib().corro_last_error()
    assert c(mem=L.CORRO_MEM_DEVICE_HEADERS) == -1
    assert c(which=2) == -1 and b"pass" in L.lib().corro_last_error()
    for which in (0, 1):
        for field in list(c.arr) + ["cs"]:
            c = _Call()
            setattr(c.r, field, None)
            assert c(which=which) == -1, field
    c = _Call()
    c.o.class_off = None
    assert c() == -1 and b"class_off" in L.lib().corro_last_error()
    for field in ("cand_change", "cand_cs", "cand_table", "cand_pk", "cand_cl"):
        c = _Call()
        c.o.ncand = 2
        setattr(c.o, field, None)
        assert c(which=1) == -1, field
    for field in ("n", "ncs"):
        c = _Call()
        setattr(c.r, field, 1 << 31)
        assert c() == -6, field
    c = _Call()
    c.r.nclasses = 1 << 16
    assert c() == -6 and b"classes" in L.lib().corro_last_error()


def test_arrays_of_a_zero_count_may_be_null():
    """NULL is refused only while the array's count is not 0: with no change, no changeset and no class the
    call passes the argument screen (and here, without a device, ends at the device check)."""
    if ca.device_count() > 0:
        pytest.skip("a GPU is visible")             # (the call would go on to read the fake context)
    c = _Call()
    c.r.n = c.r.ncs = c.r.nclasses = 0
    for field in list(c.arr) + ["cs"]:
        setattr(c.r, field, None)
    assert c() == -7


@pytest.mark.parametrize("ranges", [((2, 2), (0, 2)), ((0, 3), (2, 2)), ((0, 3), (0, 0), (2, 1)), ((0, 5),),
                                    ((5, 1),), ((0, 2), (3, (1 << 64) - 2))], ids=str)
def test_host_ranges_that_descend_overlap_or_leave_the_batch_are_refused(ranges):
    c = _Call(ranges)
    assert c() == -1 and b"ranges" in L.lib().corro_last_error()
    assert c(which=1) == -1


def test_refuses_without_a_device():
    if ca.device_count() > 0:
        pytest.skip("a GPU is visible")
    c = _Call()
    assert c() == -7                                                 # CORRO_E_NO_DEVICE
    assert c(which=1) == -7
    assert c(mem=L.CORRO_MEM_DEVICE) == -7                           # device arrays are screened on the device


# ---- MatchFilters --------------------------------------------------------------------------------------

SCHEMA = {"t": ["a", "b"], "u": ["x", "y", "z"]}       # slots: t -1 a b = 0 1 2, u -1 x y z = 3 4 5 6


def test_duplicate_handles_fold_into_one_class():
    f = MatchFilters(SCHEMA, subs=[{"t": ["a"]}, {"t": ["a"]}, {"t": ["b"]}, {"t": ["a", "-1"]}],
                     updates=["u", "t", "u"])
    assert f.handle_class == [0, 0, 1, 0, 2, 3, 2] and f.nclasses == 4
    assert f.nslots == 7 and f.words == 1 and f.tables == ["t", "u"]
    # a subscription that lists every column of a table is the update handle's filter on it
    g = MatchFilters(SCHEMA, subs=[{"t": ["b", "a"]}], updates=["t"])
    assert g.handle_class == [0, 0] and g.nclasses == 1


def test_bit_matrix_word_by_word():
    f = MatchFilters(SCHEMA, subs=[{"t": ["b"]}, {"u": ["x"], "t": []}], updates=["u"])
    assert f.bits.dtype == np.uint32 and f.bits.shape == (7, 1)
    #            class 0: t.-1 t.b     class 1: t.-1 u.-1 u.x     class 2: all of u
    assert f.bits[:, 0].tolist() == [0b011, 0, 0b001, 0b110, 0b110, 0b100, 0b100]


def test_bit_matrix_second_word():
    """34 distinct classes: class 32 and 33 land in bits 0 and 1 of the second word."""
    cols = [f"c{k}" for k in range(40)]
    subs = [{"w": [cols[k]]} for k in range(32)] + [{"w": [cols[5], cols[6]]}, {"w": [cols[39]]}]
    f = MatchFilters({"w": cols}, subs=subs)
    assert f.nclasses == 34 and f.words == 2 and f.bits.shape == (41, 2)
    assert f.bits[0].tolist() == [0xFFFFFFFF, 0b11]                  # the sentinel: every class
    assert f.bits[1 + 5].tolist() == [1 << 5, 0b01]
    assert f.bits[1 + 6].tolist() == [1 << 6, 0b01]
    assert f.bits[1 + 39].tolist() == [0, 0b10]
    assert f.bits[1 + 31].tolist() == [1 << 31, 0]
    assert f.bits[1 + 33].tolist() == [0, 0]


def test_unknown_names_are_value_errors():
    with pytest.raises(ValueError, match="table"):
        MatchFilters(SCHEMA, subs=[{"nope": []}])
    with pytest.raises(ValueError, match="table"):
        MatchFilters(SCHEMA, updates=["nope"])
    with pytest.raises(ValueError, match="column"):
        MatchFilters(SCHEMA, subs=[{"t": ["x"]}])
    f = MatchFilters(SCHEMA)
    assert f.nclasses == 0 and f.bits.shape == (7, 0)
