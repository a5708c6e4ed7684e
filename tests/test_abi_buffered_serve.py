"""CPU checks of the buffered serve path: the ctypes mirrors of its structs against the header as gcc
lays it out, the three exported symbols, the refusals of the two device entry points that come before
any device work, corro_bookie_buffered_index on a bookie that holds nothing, and the derived books as a
model: needed() united with the pool versions, fed to the need-tails model, gives start ..= end minus
the found, the gaps and every buffered version."""
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import corrosion_amd as ca
from corrosion_amd import _lib as L
from tests import buffered_util as B
from tests import need_tails_util as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = {"BufferedIndex": "corro_buffered_index", "BufSpansIn": "corro_bufspans_in", "BufSpansOut": "corro_bufspans_out",
         "AssembleBufferedIn": "corro_assemble_buffered_in"}
NAMES = ("corro_bookie_buffered_index", "corro_buffered_spans", "corro_assemble_answers_buffered")


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
    d = tempfile.mkdtemp(prefix="corro_abi_buffered_")
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
    names = lambda st: {n for n, _ in st._fields_}
    # the span arrays are the encoder's, the need arrays the decoder's, and the assembly takes the old input whole
    assert {"site", "version", "last_seq", "ts", "seq_start", "seq_end", "row_off", "row_count"} <= \
        names(L.BufSpansOut) & names(L.EncodeIn)
    assert {"kind", "start", "end", "sr_off", "sr_n", "s_start", "s_end", "need_keep", "need_site", "need_ent_off"} <= \
        names(L.BufSpansIn) & names(L.ReqDecOut)
    assert {"seg_off", "seg_pool_off", "seg_seq0", "seg_n", "ver_off", "on_device"} <= names(L.BufSpansIn) & names(L.BufferedIndex)
    assert L.AssembleBufferedIn._fields_[0] == ("base", L.AssembleIn)


def test_symbols_are_exported_and_listed():
    for name in NAMES:
        assert name in L.EXPORTS
        assert hasattr(L.lib(), name)
    assert L.lib().corro_abi_version() == 3


def test_every_declared_symbol_is_still_listed():
    from tests import test_abi
    test_abi.test_library_exports_every_declared_symbol()


def _spans_minimal():
    keep = [(C.c_uint64 * 1)(0) for _ in range(5)] + [(C.c_uint64 * 1)(7)]
    r = L.BufSpansIn()
    r.need_ent_off, r.grp_off, r.ver_off, r.vsr_off, r.seg_off = (C.addressof(k) for k in keep[:5])
    o = L.BufSpansOut()
    o.nspans = 9
    o.need_bspan_off = C.addressof(keep[5])
    return r, o, keep


def _spans_call(r, o, mem=L.CORRO_MEM_DEVICE, pas=0):
    fake, bk = C.create_string_buffer(8), ca.agent.Bookie()    # a context handle that must not be dereferenced
    return L.lib().corro_buffered_spans(C.addressof(fake), bk._h, C.byref(r), mem, C.byref(o), pas)


def test_buffered_spans_screens_its_arguments_before_any_device_call():
    fn = L.lib().corro_buffered_spans
    r, o, keep = _spans_minimal()
    fake, bk = C.create_string_buffer(8), ca.agent.Bookie()
    dev = L.CORRO_MEM_DEVICE
    assert fn(None, bk._h, C.byref(r), dev, C.byref(o), 0) == -1
    assert fn(C.addressof(fake), None, C.byref(r), dev, C.byref(o), 0) == -1
    assert fn(C.addressof(fake), bk._h, None, dev, C.byref(o), 0) == -1
    assert fn(C.addressof(fake), bk._h, C.byref(r), dev, None, 0) == -1
    assert b"NULL" in L.lib().corro_last_error()
    for mem in (L.CORRO_MEM_HOST, 7):                           # the pool rows stay on the device
        assert _spans_call(r, o, mem=mem) == -1
        assert b"mem" in L.lib().corro_last_error()
    assert _spans_call(r, o, pas=2) == -1
    assert b"pass" in L.lib().corro_last_error()
    some = (C.c_uint64 * 4)()
    for field in ("need_ent_off", "grp_off", "ver_off", "vsr_off", "seg_off"):
        r, o, keep = _spans_minimal()
        setattr(r, field, None)
        assert _spans_call(r, o) == -1, field
        assert b"NULL" in L.lib().corro_last_error()
    need_arrays = ("kind", "start", "end", "sr_off", "sr_n", "need_keep", "need_site", "in_state", "need_host")
    for missing in need_arrays:                                 # one need, one of its arrays missing
        r, o, keep = _spans_minimal()
        r.nneeds = 1
        for k in need_arrays:
            setattr(r, k, C.addressof(some))
        setattr(r, missing, None)
        assert _spans_call(r, o) == -1, missing
    for count, arrays in (("idx_nver", ("idx_version", "idx_last_seq", "idx_ts", "on_device")),
                          ("idx_nsr", ("vsr_start", "vsr_end")), ("idx_nseg", ("seg_pool_off", "seg_seq0", "seg_n")),
                          ("nseqs", ("s_start", "s_end")), ("ngroups", ("version",))):
        for missing in arrays:
            r, o, keep = _spans_minimal()
            setattr(r, count, 1)
            for k in arrays:
                setattr(r, k, C.addressof(some))
            setattr(r, missing, None)
            assert _spans_call(r, o) == -1, missing
    r, o, keep = _spans_minimal()
    o.need_bspan_off = None
    assert _spans_call(r, o) == -1
    r, o, keep = _spans_minimal()
    o.nspans = 1                                                # a span and no span array
    assert _spans_call(r, o, pas=1) == -1
    for field in ("nneeds", "nseqs", "nents", "ngroups", "idx_nver", "idx_nsr", "idx_nseg"):
        r, o, keep = _spans_minimal()
        for k, _t in L.BufSpansIn._fields_:
            if getattr(r, k) is None:
                setattr(r, k, C.addressof(some))
        setattr(r, field, 1 << 40)
        assert _spans_call(r, o) == -6, field
    assert keep[5][0] == 7 and o.nspans == 9                    # nothing was written


def _asm_minimal():
    keep = [(C.c_uint64 * 1)(0) for _ in range(5)] + [(C.c_uint64 * 1)(7), (C.c_uint64 * 1)(7)]
    rb = L.AssembleBufferedIn()
    r = rb.base
    r.frame_pair_off, r.pair_need_off = C.addressof(keep[0]), C.addressof(keep[1])
    r.need_span_off, r.need_tail_off = C.addressof(keep[2]), C.addressof(keep[3])
    rb.need_bspan_off = C.addressof(keep[4])
    o = L.Assembled()
    o.nbytes = 9
    o.need_ans_off, o.frame_ans_off = C.addressof(keep[5]), C.addressof(keep[6])
    return rb, o, keep


def _asm_call(rb, o, mem=L.CORRO_MEM_HOST, pas=0):
    fake = C.create_string_buffer(8)
    return L.lib().corro_assemble_answers_buffered(C.addressof(fake), C.byref(rb), mem, C.byref(o), pas)


def test_assemble_buffered_screens_its_arguments_before_any_device_call():
    fn = L.lib().corro_assemble_answers_buffered
    rb, o, keep = _asm_minimal()
    fake = C.create_string_buffer(8)
    assert fn(None, C.byref(rb), L.CORRO_MEM_HOST, C.byref(o), 0) == -1
    assert fn(C.addressof(fake), None, L.CORRO_MEM_HOST, C.byref(o), 0) == -1
    assert fn(C.addressof(fake), C.byref(rb), L.CORRO_MEM_HOST, None, 0) == -1
    assert b"NULL" in L.lib().corro_last_error()
    assert _asm_call(rb, o, mem=7) == -1
    assert b"mem" in L.lib().corro_last_error()
    assert _asm_call(rb, o, pas=2) == -1
    assert b"pass" in L.lib().corro_last_error()
    rb.base.payload = 2
    assert _asm_call(rb, o) == -1
    assert b"payload" in L.lib().corro_last_error()
    some = (C.c_uint64 * 4)()
    for field in ("frame_pair_off", "pair_need_off", "need_span_off", "need_tail_off"):     # the base's screen holds
        rb, o, keep = _asm_minimal()
        setattr(rb.base, field, None)
        assert _asm_call(rb, o) == -1, field
    rb, o, keep = _asm_minimal()
    rb.need_bspan_off = None
    assert _asm_call(rb, o) == -1
    assert b"buffered" in L.lib().corro_last_error()
    for missing in ("bspan_frame_off", "benc_frame_off", "benc_buf"):   # buffered spans without the second encoder's arrays
        rb, o, keep = _asm_minimal()
        rb.nbspans, rb.benc_nbytes = 1, 8
        rb.bspan_frame_off = rb.benc_frame_off = rb.benc_buf = C.addressof(some)
        setattr(rb, missing, None)
        assert _asm_call(rb, o) == -1, missing
    for field in ("nbspans", "benc_nframes", "benc_nbytes"):
        rb, o, keep = _asm_minimal()
        rb.bspan_frame_off = rb.benc_frame_off = rb.benc_buf = C.addressof(some)
        setattr(rb, field, 1 << 40)
        assert _asm_call(rb, o) == -6, field
    assert keep[5][0] == 7 and keep[6][0] == 7 and o.nbytes == 9


def test_refuse_without_a_device():
    if ca.device_count() > 0:
        pytest.skip("a GPU is visible")
    r, o, keep = _spans_minimal()
    assert _spans_call(r, o) == -7                              # CORRO_E_NO_DEVICE
    assert keep[5][0] == 7 and o.nspans == 9
    rb, o, keep = _asm_minimal()
    assert _asm_call(rb, o) == -7
    assert keep[5][0] == 7 and keep[6][0] == 7 and o.nbytes == 9


def test_index_of_a_bookie_that_holds_nothing():
    """Two sites the bookie never saw: every CSR is empty; a second pass with other counts is refused."""
    bk = ca.agent.Bookie()
    ids = np.frombuffer(bytes([1]) * 16 + bytes([2]) * 16, np.uint8).copy()
    o = L.BufferedIndex()
    o.nver = 5
    fn = L.lib().corro_bookie_buffered_index
    assert fn(bk._h, ids.ctypes.data, 2, C.byref(o), 0) == 0
    assert [getattr(o, k) for k in ("nver", "nsr", "nseg", "ntail_gap", "nhost_buf")] == [0] * 5
    offs = {k: np.full(3, 9, np.uint64) for k in ("ver_off", "tail_gap_off", "host_buf_off")}
    offs.update({k: np.full(1, 9, np.uint64) for k in ("sr_off", "seg_off")})
    for k, a in offs.items():
        setattr(o, k, a.ctypes.data)
    assert fn(bk._h, ids.ctypes.data, 2, C.byref(o), 1) == 0
    assert all(not a.any() for a in offs.values())
    o.nver = 1
    assert fn(bk._h, ids.ctypes.data, 2, C.byref(o), 1) == -1
    assert b"pass 0" in L.lib().corro_last_error()
    assert fn(None, ids.ctypes.data, 2, C.byref(o), 0) == -1
    assert fn(bk._h, None, 2, C.byref(o), 0) == -1
    assert fn(bk._h, ids.ctypes.data, 2, None, 0) == -1
    assert fn(bk._h, ids.ctypes.data, 2, C.byref(o), 2) == -1


def test_derived_books_give_the_wanted_tails_model():
    """Seeded random books: with G' = needed() + the pool versions and P' = the host-row versions, the
    need-tails model gives need_host exactly for a need that touches an unfound host-row version, and
    otherwise start ..= end minus the found versions, the real gaps and every buffered version."""
    from corrosion_amd.serve import _subtract
    rng = np.random.default_rng(20260)
    seen_dev = seen_host = 0
    for trial in range(400):
        a = N.random_case(rng)
        S = len(a["gap_off"]) - 1
        books, gap_off, gs, ge, buf_off, bv = {}, [0], [], [], [0], []
        for site in range(S):
            gaps = [(int(a["gap_start"][g]), int(a["gap_end"][g])) for g in range(int(a["gap_off"][site]), int(a["gap_off"][site + 1]))]
            buffered = [int(v) for v in a["buf_version"][int(a["buf_off"][site]):int(a["buf_off"][site + 1])]]
            dev = [v for v in buffered if rng.random() < 0.6]
            hostb = [v for v in buffered if v not in dev]
            derived = B.derive_tail_gaps(gaps, dev)
            assert B.is_canonical(derived), (trial, site)
            assert {v for s, e in derived for v in range(s, e + 1)} == {v for s, e in gaps for v in range(s, e + 1)} | set(dev)
            books[site] = (gaps, buffered, dev, hostb)
            gs += [s for s, _ in derived]
            ge += [e for _, e in derived]
            gap_off.append(len(gs))
            bv += hostb
            buf_off.append(len(bv))
        b = dict(a)
        b.update(gap_off=np.asarray(gap_off, np.uint64), gap_start=np.asarray(gs, np.uint64), gap_end=np.asarray(ge, np.uint64),
                 buf_off=np.asarray(buf_off, np.uint64), buf_version=np.asarray(bv, np.uint64))
        off, host, ranges = N.model(b, 4)
        for t in range(len(a["kind"])):
            site, s, e = int(a["need_site"][t]), int(a["start"][t]), int(a["end"][t])
            got = [(x, y) for _site, x, y in ranges[off[t]:off[t + 1]]]
            if not a["need_keep"][t] or site >= S:
                assert got == [] and host[t] == 0
                continue
            gaps, buffered, dev, hostb = books[site]
            if a["kind"][t] == 0:
                k = int(a["need_ent_off"][t])
                F = [int(v) for v in a["version"][int(a["grp_off"][k]):int(a["grp_off"][k + 1])]]
                touched = [v for v in hostb if s <= v <= e and v not in F]
                seen_dev += any(s <= v <= e and v not in F for v in dev) and not touched
                want = [] if touched or s > e else _subtract([(s, e)], [(v, v) for v in F] + gaps + [(v, v) for v in buffered])
            elif a["in_state"][t]:
                touched, want = [], []
            else:
                touched = [s] if s in hostb else []
                want = [] if touched or s in dev or any(x <= s <= y for x, y in gaps) else [(s, s)]
            seen_host += bool(touched)
            assert host[t] == (1 if touched else 0), (trial, t)
            assert got == want, (trial, t)
    assert seen_dev > 20 and seen_host > 20                     # both kinds of buffered version were met
