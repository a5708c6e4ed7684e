"""GPU need tails (corro_need_tails, csrc/need_tails.hip): the Changeset::Empty frames that end the
answers to a sync request, computed on the device. Expected values come from the loop over the
versions of tests/need_tails_util.py (pinned by tests/test_need_tails_model.py), from wire.frames, and
from the unchanged host path serve.handle_needs_frames -- never from the code under test. Bar: exact."""
import ctypes as C

import numpy as np
import pytest

from corrosion_amd import _lib as L
from corrosion_amd import sync as S
from tests import need_tails_util as U

pytestmark = pytest.mark.gpu
ACT = [bytes([0x31 + i]) * 16 for i in range(4)]
NONE = 0xFFFFFFFF
_ENGINE = []


def engine():
    if not _ENGINE:
        import corrosion_amd as ca
        e = ca.MergeEngine({"t": ["a"]}, capacity_hint=1024)
        assert list(e.register_sites(np.frombuffer(b"".join(ACT), np.uint8))) == list(range(4))
        _ENGINE.append(e)
    return _ENGINE[0]


def to_dev(a):
    import torch
    view = {8: np.int64, 4: np.int32, 1: np.uint8}[a.dtype.itemsize]
    return torch.from_numpy(np.ascontiguousarray(a).view(view).copy()).cuda()


def host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def call(a, mem="host", payload=0, cluster_id=0):
    put = to_dev if mem == "device" else (lambda x: x)
    dec = {k: put(a[k]) for k in U.DEC_KEYS}
    dec.update(nneeds=len(a["kind"]), nents=len(a["grp_off"]) - 1)
    ext = {"grp_off": put(a["grp_off"]), "version": put(a["version"])}
    got = engine().need_tails(dec, ext, {"in_state": put(a["in_state"])}, {k: put(a[k]) for k in U.BOOK_KEYS},
                              payload, cluster_id)
    assert mem == "host" or got["buf"].is_cuda
    return got


def check(a, what, mems=("host", "device"), payloads=(0, 1)):
    off, need_host, ranges = U.model(a, len(ACT))
    for mem in mems:
        for payload in payloads:
            got = call(a, mem, payload, 513 * payload)
            w = (what, mem, payload)
            assert got["nranges"] == len(ranges), w
            assert host(got["need_tail_off"]).astype(np.int64).tolist() == off, w
            assert host(got["need_host"]).tolist() == need_host, w
            assert host(got["range_start"]).astype(np.int64).tolist() == [s for _, s, _ in ranges], w
            assert host(got["range_end"]).astype(np.int64).tolist() == [e for _, _, e in ranges], w
            assert host(got["buf"]).tobytes() == U.frames(ranges, ACT, payload, 513 * payload), w
            fs = U.FRAME[payload]
            assert host(got["frame_off"]).astype(np.int64).tolist() == [fs * i for i in range(len(ranges) + 1)], w
    return off, need_host, ranges


def synthetic():
    """site 0: the gap 10..12 and the buffered version 30; site 1: nothing; site 2: 70 gaps; site 4 is in
    the book and not in the site table."""
    book = {0: ([(10, 12)], [30]), 1: ([], []), 2: ([(3 * k, 3 * k) for k in range(1, 71)], []), 4: ([], [])}
    c = U.Case(book, 5)
    c.full(0, 1, 9, [2, 3, 4, 6, 7, 8])                    # cleared at each end and in the middle
    c.full(0, 1, 9, [1, 2, 5, 6, 7, 8, 9])                 # two adjacent cleared versions: one range
    c.full(0, 8, 16, [8, 14, 15, 16])                      # cleared next to a found version and next to the gap
    c.full(1, 5, 9, [5, 6, 7, 8, 9])                       # wholly found
    c.full(1, 5, 30, [5, 6, 7, 8, 9])                      # reaches above the last found version
    c.full(1, 7, 7)                                        # start == end, cleared
    c.full(1, 7, 7, [7])                                   # start == end, found
    c.full(1, 1, 50, [4], keep=0)                          # dropped by the screen
    c.full(NONE, 1, 50, keep=0)                            # an actor that is not registered
    c.full(9, 1, 3)                                        # kept, past the book
    c.full(4, 1, 3)                                        # kept, in the book, past the site table
    c.full(1, 40, 41)
    c.partial(1, 9, in_state=1, nseq=2)                    # in the state
    c.partial(0, 11)                                       # in the gap
    c.partial(0, 20, nseq=0)                               # cleared
    c.partial(0, 30, nseq=3)                               # buffered: the host's
    c.partial(0, 30, keep=0)
    c.full(0, 25, 35, [26])                                # the buffered version inside: the host's
    c.full(0, 31, 35)                                      # ... just below the need
    c.full(0, 25, 29, [27])                                # ... just above it
    c.full(0, 28, 32, [30])                                # ... inside and found: not the host's
    c.full(2, 1, 220, [3 * k + 1 for k in range(1, 71)])   # more than 64 found versions and more than 64 gaps
    c.full(2, 3, 3)                                        # wholly in a gap
    return c


def test_entry_point_alone_on_synthetic_arrays():
    a = synthetic().arrays()
    off, need_host, ranges = check(a, "synthetic")
    per = [[(s, e) for _, s, e in ranges[off[t]:off[t + 1]]] for t in range(len(need_host))]
    assert per[:7] == [[(1, 1), (5, 5), (9, 9)], [(3, 4)], [(9, 9), (13, 13)], [], [(10, 30)], [(7, 7)], []]
    assert per[7:12] == [[], [], [], [], [(40, 41)]]
    assert per[12:17] == [[], [], [(20, 20)], [], []] and need_host[12:17] == [0, 0, 0, 1, 0]
    assert per[17:21] == [[], [(31, 35)], [(25, 26), (28, 29)], [(28, 29), (31, 32)]] and need_host[17:21] == [1, 0, 0, 0]
    assert per[21] == [(1, 2)] + [(3 * k + 2, 3 * k + 2) for k in range(1, 70)] + [(212, 220)] and per[22] == []
    assert sum(need_host) == 2
    # no need at all, and a book with no site
    check(U.Case({}, 0).arrays(), "empty")
    check(U.Case({}, 0).full(0, 1, 3).arrays(), "no book")


def test_six_hundred_needs_cross_workgroups():
    c = U.Case({0: ([(1000, 1001)], [7]), 1: ([], [])}, 2)
    for i in range(600):
        if i % 7 == 3:
            c.partial(i % 2, i + 1, in_state=i % 3 == 0)
        else:
            c.full(i % 2, i + 1, i + 3 + i % 5, [i + 2] if i % 3 else [], keep=0 if i % 11 == 5 else 1)
    off, need_host, ranges = check(c.arrays(), "600 needs")
    assert len(ranges) > 600 and 0 < sum(need_host) < 20


def test_seeded_random_books():
    kept = flagged = emitting = 0
    for seed in range(1000, 1200):
        a = U.random_case(np.random.default_rng(seed))
        assert len(a["kind"]) <= 40 and int(a["end"].max()) < 200
        off, need_host, _ = check(a, f"seed {seed}", mems=("device" if seed % 2 else "host",))
        kept += int(a["need_keep"].sum())
        flagged += sum(need_host)
        emitting += sum(1 for t in range(len(need_host)) if off[t + 1] > off[t])
    # by the model alone: most kept needs are served on the device, and many of them emit a range
    assert flagged * 2 < kept and emitting * 4 >= kept, (kept, flagged, emitting)


# ---- validation ---------------------------------------------------------------------------------

def raw(a, pas, outs, nranges=0, payload=0):
    """One call on host arrays with the caller's output arrays; returns (rc, TailsOut)."""
    r = L.TailsIn()
    r.nneeds, r.nents, r.ngroups = len(a["kind"]), len(a["grp_off"]) - 1, len(a["version"])
    r.book_nsites, r.book_ngaps, r.book_nbuf = len(a["gap_off"]) - 1, len(a["gap_start"]), len(a["buf_version"])
    r.payload = payload
    keep = {k: np.ascontiguousarray(v, U.DTYPES[k]) for k, v in a.items()}
    for k, v in keep.items():
        setattr(r, k, v.ctypes.data if v.size else None)
    o = L.TailsOut()
    o.nranges, o.nbytes = nranges, nranges * U.FRAME[payload]
    for k, v in outs.items():
        setattr(o, k, v.ctypes.data)
    rc = L.lib().corro_need_tails(engine()._h, C.byref(r), L.CORRO_MEM_HOST, C.byref(o), pas)
    return rc, o


def sentinels(n):
    return {"need_tail_off": np.full(n + 1, 7, np.uint64), "need_host": np.full(n + 1, 7, np.uint8),
            "range_start": np.full(64, 7, np.uint64), "range_end": np.full(64, 7, np.uint64),
            "buf": np.full(64 * 55, 7, np.uint8), "frame_off": np.full(65, 7, np.uint64)}


def base_case():
    c = U.Case({0: ([(10, 12), (20, 21)], [30, 31]), 1: ([(5, 5)], [8])}, 2)
    c.full(0, 1, 9, [2, 3, 4]).partial(1, 3, nseq=1).full(1, 1, 4, [1]).full(0, 40, 44, [44, 42])
    return c.arrays()


def mutate(field, idx, val):
    def f(a):
        a[field] = a[field].copy()
        a[field][idx] = val
    return f


def _two_entries(a):                                        # a kept Full need that owns two entries
    a["need_ent_off"] = np.array([0, 2, 3, 4, 5], np.uint64)


def _no_entry(a):                                           # a kept Partial need that owns none
    a["need_ent_off"] = np.array([0, 1, 1, 2, 3], np.uint64)
    a["grp_off"] = a["grp_off"][[0, 1, 4, 5]]


BAD = {
    "kind above 1": mutate("kind", 1, 2),
    "need_ent_off decreases": mutate("need_ent_off", 1, 9),
    "need_ent_off leaves nents": mutate("need_ent_off", 4, 6),
    "grp_off decreases": mutate("grp_off", 1, 1 << 40),
    "grp_off leaves ngroups": mutate("grp_off", 5, 7),
    "gap_off decreases": mutate("gap_off", 1, 4),
    "gap_off leaves the gaps": mutate("gap_off", 2, 4),
    "buf_off decreases": mutate("buf_off", 1, 1 << 50),
    "buf_off leaves the versions": mutate("buf_off", 2, 4),
    "a Full need with two entries": _two_entries,
    "a Partial need with no entry": _no_entry,
    "gaps not sorted": mutate("gap_start", 1, 3),
    "gaps touch": mutate("gap_start", 1, 13),
    "a gap that ends before it starts": mutate("gap_end", 2, 4),
    "buffered versions repeat": mutate("buf_version", 1, 30),
    "buffered versions descend": mutate("buf_version", 0, 32),
    "group versions ascend": mutate("version", 4, 41),
    "group versions repeat": mutate("version", 1, 4),
    "a group version outside the need": mutate("version", 0, 10),
    "a negative group version": mutate("version", 3, -1),
}


@pytest.mark.parametrize("name", list(BAD))
def test_validation_refuses_and_writes_nothing(name):
    good = base_case()
    outs = sentinels(len(good["kind"]))
    rc, o = raw(good, 0, outs)
    assert rc == 0 and o.nranges == len(U.model(good, 4)[2]) == 6       # the base case itself is served
    n = int(o.nranges)
    bad = dict(good)
    BAD[name](bad)
    for pas in (0, 1):
        outs = sentinels(len(good["kind"]))
        rc, o = raw(bad, pas, outs, nranges=n if pas else 0)
        assert rc == -1, (name, pas)
        assert all((v == 7).all() for v in outs.values()), (name, pas)


def test_pass_one_totals_must_be_pass_zero_s():
    good = base_case()
    for n in (5, 7):
        outs = sentinels(len(good["kind"]))
        rc, _ = raw(good, 1, outs, nranges=n)
        assert rc == -1 and b"pass 0" in L.lib().corro_last_error()
        assert all((v == 7).all() for v in outs.values())
    outs = sentinels(len(good["kind"]))
    assert raw(good, 1, outs, nranges=6)[0] == 0
    assert outs["range_start"][:6].tolist() == [1, 5, 3, 2, 40, 43] and (outs["range_start"][6:] == 7).all()
    assert outs["range_end"][:7].tolist() == [1, 9, 3, 4, 41, 43, 7]
    assert (outs["buf"][6 * 49:] == 7).all() and outs["frame_off"][:8].tolist() == [0, 49, 98, 147, 196, 245, 294, 7]


# ---- through an agent ---------------------------------------------------------------------------

class State:
    pass


@pytest.fixture(scope="module")
def st():
    """A: actor A0 versions 1..6 and 8..14 (7 is a gap) and seqs 0..1 of version 15 buffered; actor A1
    versions 1..12, then 13 and 14 rewriting every cell of its versions 2 and 3 (known, with no row
    left: two adjacent cleared versions)."""
    from corrosion_amd.agent import ChangeV1, Full
    from tests import req_decode_util as R
    from tests.test_gpu_serve_requests import A0, A1, _agent, _changes, _msg
    s = State()
    s.a = _agent(bytes([0xA0]) * 16)
    msgs = [_msg(A0, 0, v) for v in list(range(1, 7)) + list(range(8, 15))] + [_msg(A0, 0, 15, (0, 1))]
    msgs += [_msg(A1, 1, v) for v in range(1, 13)]
    msgs.append(ChangeV1(A1, Full(13, _changes(A1, 1, 2, dbv=13, cv=2), (0, 2), 2, ts=2013)))
    msgs.append(ChangeV1(A1, Full(14, _changes(A1, 1, 3, dbv=14, cv=2), (0, 2), 2, ts=2014)))
    res = s.a.process_multiple_changes(msgs)
    assert res.known.count("current") == len(msgs) - 1 and res.known.count("partial") == 1, res.known
    assert s.a.bookie.needed(A0) == [(7, 7)] and s.a.bookie.last(A0) == 15 and s.a.bookie.needed(A1) == []
    s.msgs = msgs
    s.buffered = [(A0, S.Full(14, 16)), (A0, S.Partial(15, ((0, 1),))), (A0, S.Full(15, 15))]
    s.frames = [
        (R.request_frame([(A1, [S.Full(1, 4), S.Full(1, 20), S.Partial(2, ((0, 2),)), S.Partial(5, ((1, 1),)),
                                S.Full(3, 3), S.Full(14, 30)])]), 0),
        (R.request_frame([(A0, [S.Full(1, 5), S.Full(5, 9), s.buffered[0][1], S.Full(7, 7), S.Full(10, 14)]),
                          (A1, [S.Partial(3, ((0, 0), (2, 2)))]),
                          (A0, [s.buffered[1][1], S.Partial(16, ((0, 0),)), S.Partial(10, ((0, 2),)), s.buffered[2][1]])]), 0),
    ]
    return s


def test_answers_equal_the_host_path_and_the_host_walk_is_left_to_the_buffered(st, monkeypatch):
    from corrosion_amd import serve, wire
    from tests import req_decode_util as R
    from tests.test_gpu_serve_requests import A1, expected_answers
    buf, off = R.cat([f for f, _ in st.frames])
    kws = ({}, dict(max_buf_size=150, payload=1, cluster_id=77))
    exps = [expected_answers(st.a, st.frames, **kw) for kw in kws]
    assert exps[0][1] == [[1, 1, 1, 1, 1, 1], [1, 1, 1, 0, 1, 1, 1, 0, 1, 1]]
    # the host path's answer to A1's Full(1, 4) ends with the one Empty of the two cleared versions
    empty23 = U.frames([(0, 2, 3)], [A1])
    assert serve.handle_needs_frames(st.a, [(A1, S.Full(1, 4))])[0].endswith(empty23)
    assert exps[0][0][0].count(empty23) == 2
    calls = []
    real = serve._bookie_messages

    def counted(agent, actor, need, *a, **kw):
        calls.append((actor, need))
        return real(agent, actor, need, *a, **kw)
    monkeypatch.setattr(serve, "_bookie_messages", counted)
    for kw, (exp, _keeps) in zip(kws, exps):
        del calls[:]
        timings = {}
        status, got = serve.handle_request_frames(st.a, buf, off, timings=timings, **kw)
        assert status.tolist() == [0, 0]
        assert got == exp
        assert calls == st.buffered                       # only the needs that touch the buffered version
        assert "tails" in timings and "bookie" in timings
    assert wire.PAYLOAD_UNI == 1


def test_whole_loop_with_cleared_versions(st):
    """B is behind A, which holds two cleared versions of A1: after one round of requests and answers B's
    rows equal A's and B's bookie has no gap left where the cleared versions are."""
    from tests import req_decode_util as R
    from tests.test_gpu_serve_requests import A0, A1, _agent, _canon
    b = _agent(bytes([0xB0]) * 16)
    b.process_multiple_changes([m for m in st.msgs if m.actor_id == A0 and m.changeset.version <= 3])
    assert _canon(b) != _canon(st.a)
    needs = b.generate_sync().compute_available_needs(st.a.generate_sync(), b.engine)
    assert set(needs) == {A0, A1}
    planned = S.plan_sync_requests(b.engine, [[needs]])
    frames = [f for _round, f in planned[0][0]]
    buf, off = R.cat(frames)
    status, answers = st.a.handle_request_frames(buf, off)
    assert (status == 0).all() and sum(map(len, answers)) > 0
    assert U.frames([(0, 2, 3)], [A1]) in b"".join(answers)
    res, dstatus = b.process_frames(b"".join(answers))
    assert (host(dstatus) == 0).all() and "current" in res.known
    for actor, version in res.ready:
        b.process_fully_buffered_changes(actor, version)
    assert _canon(b) == _canon(st.a)
    assert b.bookie.last(A1) == 14 and b.bookie.needed(A1) == []
    assert b.bookie.contains_all(A1, (2, 3))
