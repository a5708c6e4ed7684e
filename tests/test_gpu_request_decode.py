"""GPU request decode (corro_decode_requests, csrc/req_decode.hip) against the host codec
(wire.decode_sync_request) and the looping restatement of process_sync's screen
(tests/req_decode_util.py), from host and from device memory. Every array is compared exactly."""
import ctypes as C
import struct

import numpy as np
import pytest

from corrosion_amd import _lib as L
from corrosion_amd import sync as S
from tests import req_decode_util as U

pytestmark = pytest.mark.gpu
ACT = [bytes([i + 1]) * 16 for i in range(6)]
SITE_OF = {a: i for i, a in enumerate(ACT)}
STRANGER = b"\xEE" * 16
_ENGINE = []


def engine():
    if not _ENGINE:
        import corrosion_amd as ca
        e = ca.MergeEngine({"t": ["a"]}, capacity_hint=1024)
        assert list(e.register_sites(np.frombuffer(b"".join(ACT), np.uint8))) == list(range(6))
        _ENGINE.append(e)
    return _ENGINE[0]


def to_dev(a):
    import torch
    view = {8: np.int64, 4: np.int32, 1: np.uint8}[a.dtype.itemsize]
    return torch.from_numpy(np.ascontiguousarray(a).view(view).copy()).cuda()


def host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def same(got, exp, what=""):
    for k in ("nframes", "npairs", "nneeds", "nseqs", "nents"):
        assert got[k] == exp[k], (what, k, got[k], exp[k])
    for k, dt in U.FIELDS.items():
        g = host(got[k]).view(dt) if host(got[k]).dtype.itemsize == np.dtype(dt).itemsize else host(got[k])
        assert g.shape == exp[k].shape and (g == exp[k]).all(), (what, k, g.tolist()[:40], exp[k].tolist()[:40])


def decode(frames, books, mem):
    buf, off = U.cat(frames)
    book = None if books is None else U.book_arrays(books, len(ACT))
    if mem == "device":
        book = None if book is None else {k: to_dev(v) for k, v in book.items()}
        res = engine().decode_requests(to_dev(buf), to_dev(off), book)
        assert res["kind"].is_cuda and res["ent_site"].is_cuda
        return res
    return engine().decode_requests(buf, off, book)


def check(cases, books=None, what=""):
    """cases: [(frame bytes, expected status)], decoded from host and from device memory."""
    exp = U.expected(cases, SITE_OF, books)
    for mem in ("host", "device"):
        same(decode([f for f, _ in cases], books, mem), exp, f"{what} {mem}")
    return exp


MIXED = [(ACT[0], [S.Full(1, 10), S.Partial(4, ()), S.Partial(9, ((0, 1), (3, 3), (7, 20)))]),
         (ACT[3], [S.Partial(2, ((5, 6),)), S.Full(3, 3)])]
BOOKS = {0: ([(4, 5)], 12), 3: ([], 2), 4: ([(1, 1)], None)}


def test_basic_shapes():
    check([], what="no frames")
    check([(U.request_frame([(ACT[1], [S.Full(1, 1)])]), 0)], what="one Full")
    exp = check([(U.request_frame(MIXED), 0)], what="two pairs")
    assert exp["npairs"] == 2 and exp["nseqs"] == 4 and exp["nents"] == 1 + 1 + 4 + 2 + 1
    exp = check([(U.request_frame(MIXED), 0)], BOOKS, "two pairs, screened")
    assert exp["need_keep"].tolist() == [1, 0, 1, 1, 0]
    # one frame more than the kernel's 256-lane workgroup: the last lane sits alone in its workgroup
    many = [(U.request_frame([(ACT[i % 6], [S.Full(i, i + i % 3), S.Partial(i, ((0, i),))][:1 + i % 2])]), 0)
            for i in range(257)]
    exp = check(many, BOOKS, "257 frames")
    assert exp["nframes"] == 257 and 0 < exp["need_keep"].sum() < exp["nneeds"]
    check([(U.request_frame([]), 0), (U.request_frame([(ACT[2], [])]), 0)], what="no pairs, no needs")


def test_round_trip_of_the_planner_output():
    """corro_plan_requests' device output of a two-server session, fed to the decoder where it lies."""
    sessions = [[{ACT[0]: [S.Full(1, 35), S.Partial(40, ((0, 3), (9, 9)))], ACT[1]: [S.Full(5, 7)]},
                 {ACT[0]: [S.Full(20, 50), S.Partial(40, ((2, 5),))], ACT[2]: [S.Partial(3, ((1, 1),))]}]]
    arr, _groups = S.requests_csr(sessions, SITE_OF.__getitem__)
    plan = S._plan_requests(engine(), {k: to_dev(v) for k, v in arr.items()}, 10, 10, True)
    assert plan["nframes"] >= 8
    buf, fo = host(plan["buf"]).tobytes(), host(plan["frame_off"])
    frames = [buf[int(fo[f]):int(fo[f + 1])] for f in range(plan["nframes"])]
    exp = U.expected([(f, 0) for f in frames], SITE_OF)
    got = engine().decode_requests(plan["buf"], plan["frame_off"])
    same(got, exp, "planner output")
    assert exp["npairs"] == plan["nframes"] and (exp["need_keep"] == 1).all()
    # per frame, the needs the planner reports: frame_needs of them, for the entry's actor
    site = arr["site"][host(plan["frame_entry"])]
    assert (host(got["pair_site"]).view(np.uint32) == site).all()
    assert (np.diff(host(got["pair_need_off"]).astype(np.int64)) == host(plan["frame_needs"])).all()


def _malformed():
    good = U.request_frame([(ACT[0], [S.Full(1, 3)])])
    two = U.request_payload([(ACT[1], [S.Full(2, 9), S.Partial(5, ((0, 7),))])])
    f = lambda payload: struct.pack(">I", len(payload)) + payload
    head = struct.pack("<III", 0, 4, 1) + ACT[1]
    big = 0xFFFFFFFF
    cases = [(f"prefix {k}", f(two[:k]), U.E_INVALID) for k in range(len(two))]
    cases += [
        ("no length prefix", b"\0\0", U.E_INVALID),
        ("trailing byte", f(two + b"\0"), U.E_INVALID),
        ("length prefix + 1", struct.pack(">I", len(two) + 1) + two, U.E_INVALID),
        ("length prefix - 1", struct.pack(">I", len(two) - 1) + two, U.E_INVALID),
        ("npairs 2^32 - 1", f(struct.pack("<III", 0, 4, big) + two[12:]), U.E_INVALID),
        ("nneeds 2^32 - 1", f(head + struct.pack("<I", big) + two[32:]), U.E_INVALID),
        ("nseqs 2^32 - 1", f(head + struct.pack("<I", 1) + struct.pack("<IQI", 1, 5, big) + struct.pack("<QQ", 0, 7)),
         U.E_INVALID),
        ("need tag 2", f(head + struct.pack("<I", 2) + U.need_bytes(S.Full(1, 2)) + struct.pack("<IB", 2, 0)), 2),
        ("need tag 2 first", f(head + struct.pack("<I", 1) + struct.pack("<IBQ", 2, 1, 99)), 2),
        ("need tag 3", f(head + struct.pack("<I", 1) + struct.pack("<IQQ", 3, 1, 2)), U.E_INVALID),
        ("message tag 1", f(struct.pack("<II", 0, 1) + two[8:]), 1),
        ("message tag 0", f(struct.pack("<II", 0, 0)), 1),
        ("message tag 5", f(struct.pack("<II", 0, 5) + two[8:]), U.E_INVALID),
        ("message version 1", f(struct.pack("<II", 1, 4) + two[8:]), U.E_INVALID),
        ("Full end 2^63", f(U.request_payload([(ACT[1], [S.Full(1, 1 << 63)])])), U.E_RANGE),
        ("Full start 2^63", f(U.request_payload([(ACT[1], [S.Full(1 << 63, 2)])])), U.E_RANGE),
        ("Partial version 2^63", f(U.request_payload([(ACT[1], [S.Full(1, 2), S.Partial(1 << 63, ())])])), U.E_RANGE),
        ("version 2^63 - 1", f(U.request_payload([(ACT[1], [S.Full(1, (1 << 63) - 1)])])), 0),
        ("seq 2^32", f(U.request_payload([(ACT[1], [S.Partial(5, ((1 << 32, (1 << 32) + 5), (7, 1 << 40)))])])), 0),
    ]
    return good, cases


def test_malformed_frames_between_good_frames():
    """Every malformed frame sits between two good frames, which must decode as if it were not there."""
    good, bad = _malformed()
    assert len(bad) >= 100
    cases = [(good, 0)]
    for _name, fb, st in bad:
        cases += [(fb, st), (good, 0)]
    exp = check(cases, what="malformed")
    alone = U.expected([(good, 0)], SITE_OF)
    kept = [i for i, (_f, st) in enumerate(cases) if st == 0]
    assert exp["nneeds"] == len(kept) >= len(bad) + 3        # one need per good frame, the seq-2^32 frame included
    assert exp["ent_seq_start"].max() == 0xFFFFFFFF          # ... and its seq bounds were clamped
    assert exp["s_end"].max() == 1 << 40                     # while the need keeps them as sent
    # each case alone between its two neighbours, with its name in the failure message
    for name, fb, st in bad[::7] + bad[-20:]:
        e3 = check([(good, 0), (fb, st), (good, 0)], BOOKS, name)
        assert e3["frame_status"].tolist() == [0, st, 0]
        last = int(e3["frame_pair_off"][2])
        assert e3["start"][int(e3["pair_need_off"][last])] == alone["start"][0]


def _raw_call(frame_off, length, nframes):
    """Pass 0 through ctypes on host arrays, every output preset to 77."""
    buf = np.zeros(max(1, length), np.uint8)
    st = np.full(nframes + 1, 77, np.int32)
    fpo = np.full(nframes + 2, 77, np.uint64)
    r, o = L.ReqDecIn(), L.ReqDecOut()
    r.buf, r.len, r.nframes, r.frame_off = buf.ctypes.data, length, nframes, frame_off.ctypes.data
    o.npairs = o.nneeds = o.nseqs = o.nents = 77
    o.frame_status, o.frame_pair_off = st.ctypes.data, fpo.ctypes.data
    rc = L.lib().corro_decode_requests(engine()._h, C.byref(r), L.CORRO_MEM_HOST, C.byref(o), 0)
    untouched = (st == 77).all() and (fpo == 77).all() and (o.npairs, o.nneeds, o.nseqs, o.nents) == (77,) * 4
    return rc, untouched


def test_bad_frame_off_fails_the_call_and_writes_nothing():
    good = U.request_frame([(ACT[0], [S.Full(1, 3)])])
    n = len(good)
    assert _raw_call(np.array([0, 2 * n, n, 3 * n], np.uint64), 3 * n, 3) == (-1, True)      # not monotone
    assert b"frame_off" in L.lib().corro_last_error()
    assert _raw_call(np.array([0, n, 2 * n, 3 * n + 1], np.uint64), 3 * n, 3) == (-1, True)  # leaves len
    assert _raw_call(np.array([0, n, 1 << 62, 3 * n], np.uint64), 3 * n, 3) == (-1, True)
    rc, untouched = _raw_call(np.array([0, n, 2 * n, 3 * n], np.uint64), 3 * n, 3)           # (zero bytes: 3 bad frames)
    assert rc == 0 and not untouched
    # through the wrapper, from device memory, and a book that is not canonical
    import corrosion_amd as ca
    buf, off = U.cat([good, good])
    off[1] = off[2] + 1
    with pytest.raises(ca.CorroError) as e:
        engine().decode_requests(to_dev(buf), to_dev(off))
    assert e.value.code == -1
    buf, off = U.cat([good, good])
    for gaps in ([(5, 6), (7, 9)], [(5, 9), (2, 3)], [(6, 5)]):                                # touching, unsorted, empty
        with pytest.raises(ca.CorroError) as e:
            engine().decode_requests(buf, off, U.book_arrays({0: (gaps, 20)}, len(ACT)))
        assert e.value.code == -1
    check([(good, 0), (good, 0)], {0: ([(5, 6), (8, 9)], 20), 1: ([(1, 9)], 20)}, "canonical book")


def test_unknown_actor_is_not_registered():
    eng = engine()
    before = eng.site_count()
    cases = [(U.request_frame([(STRANGER, [S.Full(1, 5), S.Partial(2, ((0, 1),))]), (ACT[2], [S.Full(1, 5)])]), 0)]
    for books in (None, {2: ([], 9)}):
        exp = check(cases, books, "stranger")
        assert exp["pair_site"].tolist() == [U.NONE, 2] and exp["need_keep"].tolist() == [0, 0, 1]
        assert exp["nents"] == 1
    assert eng.site_count() == before == len(ACT)


def test_random_screen_against_the_looping_model():
    rng = np.random.default_rng(U.SCREEN_SEED)
    kept = total = 0
    for trial in range(200):
        books, frames = U.random_screen_trial(rng, ACT)
        cases = [(f, 0) for f in frames]
        exp = check(cases, books, f"trial {trial}")
        kept += int(exp["need_keep"].sum())
        total += exp["nneeds"]
        if trial % 20 == 0:                                  # with no book everything is kept
            e0 = check(cases, None, f"trial {trial}, no book")
            assert (e0["need_keep"] == 1).all()
    assert 0.1 < kept / total < 0.9, (kept, total)


def test_entries_are_the_ones_handle_needs_frames_builds():
    """need_ent_off / ent_* against the loop of serve.handle_needs_frames, restated over the kept needs."""
    cases = [(U.request_frame(MIXED), 0), (U.request_frame([(ACT[4], [S.Partial(3, ((2, 1 << 33),)), S.Full(1, 1)])]), 0)]
    exp = check(cases, BOOKS, "entries")
    ent = []
    for fb, _st in cases:
        from corrosion_amd import wire as W
        for actor, needs in W.decode_sync_request(fb[4:]):
            site = SITE_OF[actor]
            for nd in needs:
                if not U.keeps(BOOKS.get(site), nd):
                    continue
                if isinstance(nd, S.Full):
                    ent.append((site, nd.start, nd.end, 0, 0xFFFFFFFF))
                else:
                    for s, e in [(0, 0xFFFFFFFF)] + [tuple(r) for r in nd.seqs]:
                        ent.append((site, nd.version, nd.version, max(0, min(s, 0xFFFFFFFF)), max(0, min(e, 0xFFFFFFFF))))
    got = list(zip(*(exp[k].tolist() for k in ("ent_site", "ent_start", "ent_end", "ent_seq_start", "ent_seq_end"))))
    assert got == ent and len(ent) >= 6
    assert np.diff(exp["need_ent_off"].astype(np.int64)).tolist() == [1, 0, 4, 2, 0, 2, 0]
