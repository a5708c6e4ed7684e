"""CPU checks of corro_bookie_save / corro_bookie_load: the exports and the ctypes mirror of
corro_bookie_image against the header as gcc lays it out, and the books' half of the load -- from_conn
(agent.rs:1282-1351) and the startup loop's ready listing (run_root.rs:139-201) -- against the host model
(tests/restore_model.py) with ctx = NULL: the reload round-trip at the end of test_booked_insert_db
(agent.rs:1860-1865) for every step of the gaps KATs, the from_conn quirks, the refusals, and a save /
load / save round trip of a bookie without rows. No device is touched."""
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import corrosion_amd as ca
from corrosion_amd import _lib as L
from tests import restore_model as M
from tests._util import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = [bytes([k + 1]) * 16 for k in range(6)]


def _c_layout():
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        pytest.skip("no C compiler")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "corro_hip.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(corro_bookie_image));']
    for name, _t in L.BookieImage._fields_:
        lines.append(f'  printf("{name} %zu\\n", offsetof(corro_bookie_image, {name}));')
    lines += ["  return 0;", "}"]
    d = tempfile.mkdtemp(prefix="corro_abi_image_")
    try:
        src, exe = os.path.join(d, "layout.c"), os.path.join(d, "layout")
        with open(src, "w") as f:
            f.write("\n".join(lines) + "\n")
        subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        out = subprocess.check_output([exe]).decode()
    finally:
        shutil.rmtree(d, ignore_errors=True)
    return {name: int(v) for name, v in (ln.split() for ln in out.splitlines())}


def test_struct_matches_header_layout():
    got = _c_layout()
    assert C.sizeof(L.BookieImage) == got["size"]
    for name, _t in L.BookieImage._fields_:
        assert getattr(L.BookieImage, name).offset == got[name], name
    assert dict(L.BookieImage._fields_)["rows"] is L.Changes


def test_symbols_are_exported_and_listed():
    for name in ("corro_bookie_save", "corro_bookie_load"):
        assert name in L.EXPORTS
        assert hasattr(L.lib(), name)
    assert L.lib().corro_abi_version() == 3
    from tests import test_abi
    test_abi.test_library_exports_every_declared_symbol()


def _load(actors, site_ids=()):
    bk = ca.agent.Bookie()
    bk.load(M.make_image(actors, site_ids))
    return bk


def test_reload_round_trip_of_every_gaps_kat_step():
    """agent.rs:1860-1865: after every insert_db step, a bookie loaded from (max, gaps so far) reads back
    like the one that lived through the inserts."""
    steps = load_golden("gaps_kats.json")["steps"]
    allv, n = [], 0
    for st in steps:
        if st.get("reset"):
            allv = []
            continue
        allv += st["insert"]
        if st["gaps"] is None:
            continue
        mx = max(e for _, e in allv)
        gaps = [tuple(g) for g in st["gaps"]]
        books, ready = M.startup([(A[0], mx, [], gaps)])
        bk = _load([(A[0], mx, [], gaps)])
        M.check_bookie(bk, books)
        assert bk.needed(A[0]) == gaps and bk.last(A[0]) == mx
        assert bk.take_ready() == ready == []
        n += 1
    assert n >= 5


QUIRKS = {
    "partial above max raises it": [(A[0], 3, [(9, 0, 2, 5, 11)], [])],
    "partial with max None": [(A[0], None, [(4, 1, 2, 5, 11)], [])],
    "gap above max stays and does not raise it": [(A[0], 5, [], [(8, 12)])],
    "first seq row wins last_seq and ts": [(A[0], 7, [(7, 0, 1, 9, 100), (7, 5, 6, 3, 200)], [])],
    "touching and overlapping seq rows coalesce": [(A[0], 2, [(2, 0, 3, 20, 1), (2, 4, 6, 20, 1), (2, 5, 9, 20, 1), (2, 15, 16, 20, 1)], [])],
    "gaps unsorted and touching coalesce": [(A[0], 40, [], [(20, 25), (3, 4), (5, 9), (26, 26), (30, 31)])],
    "ready: 0..=last_seq complete": [(A[0], 6, [(6, 0, 4, 9, 1), (6, 5, 9, 9, 1)], [])],
    "not ready: only seq 0 missing (is_complete would pass)": [(A[0], 6, [(6, 1, 9, 9, 1)], [])],
    "last_seq 0": [(A[0], 1, [(1, 0, 0, 0, 1)], [])],
    "several actors, any order": [(A[3], 2, [(3, 0, 0, 1, 5)], [(1, 1)]), (A[1], None, [], []), (A[2], 9, [(4, 0, 1, 1, 5), (2, 1, 1, 1, 5)], [(5, 6)])],
}


@pytest.mark.parametrize("name", sorted(QUIRKS))
def test_from_conn_quirks(name):
    actors = QUIRKS[name]
    books, ready = M.startup(actors)
    bk = _load(actors, site_ids=A)
    M.check_bookie(bk, books)
    assert bk.take_ready() == ready
    assert bk.take_ready() == []
    img = bk.save()
    # the seq books keep the rows given, a version's last_seq and ts from its first row
    for k, actor in enumerate(img["actor_ids"]):
        bv = books[bytes(actor)]
        lo, hi = int(img["seq_off"][k]), int(img["seq_off"][k + 1])
        for j in range(lo, hi):
            p = bv.partials[int(img["seq_version"][j])]
            assert (int(img["seq_last"][j]), int(img["seq_ts"][j])) == (p.last_seq, p.ts)


def test_quirk_expectations_are_what_they_claim():
    """The model itself, on the cases whose names promise an outcome."""
    b, r = M.startup(QUIRKS["partial above max raises it"])
    assert b[A[0]].max == 9 and r == []
    b, r = M.startup(QUIRKS["gap above max stays and does not raise it"])
    assert b[A[0]].max == 5 and b[A[0]].needed == [(8, 12)]
    b, r = M.startup(QUIRKS["first seq row wins last_seq and ts"])
    assert (b[A[0]].partials[7].last_seq, b[A[0]].partials[7].ts) == (9, 100)
    b, r = M.startup(QUIRKS["touching and overlapping seq rows coalesce"])
    assert b[A[0]].partials[2].seqs == [(0, 9), (15, 16)]
    b, r = M.startup(QUIRKS["gaps unsorted and touching coalesce"])
    assert b[A[0]].needed == [(3, 9), (20, 26), (30, 31)]
    assert M.startup(QUIRKS["ready: 0..=last_seq complete"])[1] == [(A[0], 6)]
    assert M.startup(QUIRKS["not ready: only seq 0 missing (is_complete would pass)"])[1] == []
    assert M.startup(QUIRKS["last_seq 0"])[1] == [(A[0], 1)]


def _empty(bk):
    return bk.sync_book()["actor"].shape[0] == 0 and bk.take_ready() == []


def test_repeated_actor_is_refused_and_leaves_the_bookie_empty():
    bk = ca.agent.Bookie()
    with pytest.raises(ca.CorroError) as e:
        bk.load(M.make_image([(A[0], 3, [(5, 0, 1, 4, 1)], [(1, 2)]), (A[1], 4, [], []), (A[0], 9, [], [])], site_ids=A))
    assert e.value.code == -1 and "repeated" in str(e.value)
    assert _empty(bk) and bk.last(A[0]) is None and bk.partial(A[0], 5) is None
    bk.load(M.make_image([(A[0], 3, [], [])]))                 # still loadable
    assert bk.last(A[0]) == 3


def test_load_into_a_used_bookie_is_refused():
    bk = _load([(A[0], 3, [], [])])
    with pytest.raises(ca.CorroError) as e:
        bk.load(M.make_image([(A[1], 4, [], [])]))
    assert e.value.code == -1 and "empty bookie" in str(e.value)
    assert bk.last(A[0]) == 3 and bk.last(A[1]) is None


def test_malformed_images_are_refused():
    for actors, sites, word in (([(A[0], 3, [(5, 0, 1, 4, 1)], [])], (), "site_ids"),      # seq rows, no ordinal
                                ([(A[0], 3, [(5, 2, 1, 4, 1)], [])], A, "start_seq"),
                                ([(A[0], 3, [], [(4, 2)])], A, "gap")):
        bk = ca.agent.Bookie()
        with pytest.raises(ca.CorroError) as e:
            bk.load(M.make_image(actors, sites))
        assert e.value.code == -1 and word in str(e.value)
        assert _empty(bk)
    img = M.make_image([(A[0], 3, [], [(1, 2)])])
    img["gap_off"] = np.array([0, 5], np.uint64)               # past ngaps
    bk = ca.agent.Bookie()
    with pytest.raises(ca.CorroError):
        bk.load(img)
    assert _empty(bk)
    img = M.make_image([(A[0], 3, [], [])], A, rows=M.make_rows([(0, 1, 0)]))   # rows without a context
    with pytest.raises(ca.CorroError) as e:
        ca.agent.Bookie().load(img)
    assert e.value.code == -1 and "context" in str(e.value)


def test_save_load_save_of_a_rows_free_bookie():
    actors = [(A[4], 12, [(12, 0, 3, 9, 77), (12, 6, 9, 9, 77), (10, 2, 2, 5, 70)], [(2, 3), (7, 9)]),
              (A[1], None, [], []), (A[2], 30, [], [(1, 29)]), (A[0], 5, [(5, 0, 1, 1, 3)], [])]
    bk = _load(actors, site_ids=A)
    first = bk.save()
    assert first["nrows"] == 0 and first["rows"]["pk"].shape == (0,)
    assert [bytes(a) for a in first["actor_ids"]] == sorted(a for a, *_ in actors)    # ActorId byte order
    assert list(first["max"]) == [5, -1, 30, 12]
    bk2 = ca.agent.Bookie()
    bk2.load(first)
    second = bk2.save()
    assert M.image_equal(first, second)
    assert sorted(bk.take_ready()) == sorted(bk2.take_ready()) == [(A[0], 5)]
    for a, *_ in actors:
        assert bk.last(a) == bk2.last(a) and bk.needed(a) == bk2.needed(a)


def test_save_refuses_a_bookie_that_changed_between_the_passes():
    bk = _load([(A[0], 5, [], [(2, 3)])])
    img = L.BookieImage()
    fn = L.lib().corro_bookie_save
    assert fn(None, bk._h, C.byref(img), L.CORRO_MEM_HOST, 0) == 0
    assert (img.nactors, img.ngaps, img.nseqrows, img.rows.n) == (1, 1, 0, 0)
    bufs = {k: np.full(64, 0xAB, np.uint8) for k in L._IMAGE_BOOKS}
    for k, a in bufs.items():
        setattr(img, k, a.ctypes.data)
    img.stamp ^= 1                                              # same counts, another bookie
    assert fn(None, bk._h, C.byref(img), L.CORRO_MEM_HOST, 1) == -1
    assert b"changed" in L.lib().corro_last_error()
    assert all((a == 0xAB).all() for a in bufs.values())        # nothing written
    img.stamp ^= 1
    assert fn(None, bk._h, C.byref(img), L.CORRO_MEM_HOST, 1) == 0
    assert bytes(bufs["actor_ids"][:16]) == A[0]
    assert fn(None, bk._h, C.byref(img), L.CORRO_MEM_HOST, 2) == -1
    assert fn(None, bk._h, C.byref(img), 7, 0) == -1
    assert fn(None, None, C.byref(img), L.CORRO_MEM_HOST, 0) == -1
