"""CPU checks of corro_decode_states: the ctypes mirrors of its two structs against the header as gcc lays
it out, the exported symbol, and the refusals that come before any device work."""
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import corrosion_amd as ca
from corrosion_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = {"StateDecIn": "corro_statedec_in", "StateDecOut": "corro_statedec_out"}


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
    d = tempfile.mkdtemp(prefix="corro_abi_statedec_")
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
    names = [n for n, _ in L.StateDecOut._fields_]
    assert names[:8] == ["n", "ntn", "ntp", "ntps", "non", "nop", "nops", "nunregistered"]
    # the entries are corro_sync_entries' arrays, every one of them, in its order
    ent = [n for n, _ in L.SyncEntries._fields_[1:]]
    assert names[names.index("their_head"):names.index("their_head") + len(ent)] == ent


def test_symbol_is_exported_and_listed():
    assert "corro_decode_states" in L.EXPORTS
    assert hasattr(L.lib(), "corro_decode_states")
    assert L.lib().corro_abi_version() == 3


class _Call:
    """One frame of 8 bytes, one pair, every output array present and holding sentinels."""

    def __init__(self):
        self.buf = np.zeros(8, np.uint8)
        self.frame_off = np.array([0, 8], np.uint64)
        self.ours, self.theirs = np.zeros(1, np.uint32), np.zeros(1, np.uint32)
        r = L.StateDecIn()
        r.buf, r.len, r.nframes, r.frame_off = self.buf.ctypes.data, 8, 1, self.frame_off.ctypes.data
        r.npairs, r.pair_ours, r.pair_theirs = 1, self.ours.ctypes.data, self.theirs.ctypes.data
        self.r = r
        o = L.StateDecOut()
        self.out = {}
        for name, t in L.StateDecOut._fields_:
            if t is C.c_void_p:
                self.out[name] = np.full(32, 7, np.uint8)
                setattr(o, name, self.out[name].ctypes.data)
        self.o = o
        self.fake = C.create_string_buffer(8)      # a context handle that must not be dereferenced

    def __call__(self, which=0, mem=L.CORRO_MEM_HOST):
        rc = L.lib().corro_decode_states(C.addressof(self.fake), C.byref(self.r), mem, C.byref(self.o), which)
        assert all((a == 7).all() for a in self.out.values())       # a refused call writes nothing
        return rc


def test_arguments_are_screened_before_any_device_call():
    fn = L.lib().corro_decode_states
    c = _Call()
    assert fn(None, C.byref(c.r), L.CORRO_MEM_HOST, C.byref(c.o), 0) == -1
    assert fn(C.addressof(c.fake), None, L.CORRO_MEM_HOST, C.byref(c.o), 0) == -1
    assert fn(C.addressof(c.fake), C.byref(c.r), L.CORRO_MEM_HOST, None, 0) == -1
    assert b"NULL" in L.lib().corro_last_error()
    assert c(mem=7) == -1 and b"mem" in L.lib().corro_last_error()
    assert c(which=2) == -1 and b"pass" in L.lib().corro_last_error()
    for field in ("frame_off", "buf", "pair_ours", "pair_theirs"):
        c = _Call()
        setattr(c.r, field, None)
        assert c() == -1, field
    for field in ("frame_status", "frame_actor", "frame_has_ts", "frame_ts", "pair_status", "pair_ent_off"):
        c = _Call()
        setattr(c.o, field, None)
        assert c() == -1, field
    for field in ("tn_off", "tps_off", "ops_off"):                   # pass 1 always writes the closing offsets
        c = _Call()
        setattr(c.o, field, None)
        assert c(which=1) == -1, field
    c = _Call()
    c.o.n = 2
    c.o.their_head = None
    assert c(which=1) == -1
    for field in ("nframes", "npairs"):
        c = _Call()
        setattr(c.r, field, 1 << 31)
        assert c() == -6, field


def test_bad_frame_off_is_refused():
    c = _Call()
    c.frame_off[:] = [8, 0]                                          # decreases
    assert c() == -1 and b"frame_off" in L.lib().corro_last_error()
    c = _Call()
    c.frame_off[:] = [0, 9]                                          # passes len
    assert c() == -1 and b"frame_off" in L.lib().corro_last_error()
    assert c(which=1) == -1


@pytest.mark.parametrize("side", ["ours", "theirs"])
def test_a_pair_index_out_of_range_is_refused(side):
    c = _Call()
    getattr(c, side)[0] = 1                                          # nframes is 1
    assert c() == -1 and b"pair" in L.lib().corro_last_error()
    assert c(which=1) == -1


@pytest.mark.parametrize("totals", [{"ntn": 1}, {"ntp": 2}, {"non": 1}, {"nop": 1}, {"n": 1, "ntps": 1}, {"n": 1, "nops": 3}],
                         ids=str)
def test_pass_1_totals_no_pass_0_returns_are_refused(totals):
    """Sizes that differ from pass 0's are found on the device (tests/test_gpu_state_decode.py); the ones
    no pass 0 can return are refused here, before any device work."""
    c = _Call()
    for k, v in totals.items():
        setattr(c.o, k, v)
    assert c(which=1) == -1
    assert b"sizes differ from pass 0" in L.lib().corro_last_error()


def test_refuses_without_a_device():
    if ca.device_count() > 0:
        pytest.skip("a GPU is visible")
    c = _Call()
    assert c() == -7                                                 # CORRO_E_NO_DEVICE
    assert c.o.n == 0
