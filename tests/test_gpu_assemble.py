"""GPU answer assembly (corro_assemble_answers, csrc/answer_assemble.hip): the per-frame answers to a
buffer of sync requests in one device buffer. Expected values come from the numpy model of
tests/assemble_util.py (pinned by tests/test_assemble_model.py) and, end to end, from the unchanged
serve.handle_request_frames -- never from the code under test. Bar: exact."""
import ctypes as C

import numpy as np
import pytest

from corrosion_amd import _lib as L
from corrosion_amd import sync as S
from tests import assemble_util as U

pytestmark = pytest.mark.gpu
_ENGINE = []
GUARD = 32                                                     # canary bytes on each side of the output buffer


def engine():
    if not _ENGINE:
        import corrosion_amd as ca
        _ENGINE.append(ca.MergeEngine({"t": ["a"]}, capacity_hint=1024))
    return _ENGINE[0]


def to_dev(a, shift=0):
    """A copy of `a` on the device; uint8 data may start `shift` bytes past a 16-byte aligned address."""
    import torch
    if a.dtype.itemsize == 1:
        big = torch.zeros(len(a) + shift + 16, dtype=torch.uint8, device="cuda")
        assert big.data_ptr() % 16 == 0
        big[shift:shift + len(a)] = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()
        return big[shift:shift + len(a)]
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy()).cuda()


def host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def raw(a, pas, mem="device", nbytes=0, enc_shift=0, tail_shift=0, out_shift=0, room=None, null=(), payload=None):
    """One pass through the C ABI on canary-filled outputs. Returns (rc, nbytes, outs): outs as host
    arrays, "buf" with GUARD canary bytes before and after `room` bytes."""
    import torch
    c = U.counts(a)
    r = L.AssembleIn()
    for k, v in c.items():
        setattr(r, k, v)
    if payload is not None:                                    # (the arrays are still the case's own)
        r.payload = payload
    keep = []
    for k, dt in U.DTYPES.items():
        v = np.ascontiguousarray(a[k], dt)
        if mem == "device":
            v = to_dev(v, {"enc_buf": enc_shift, "tail_buf": tail_shift}.get(k, 0))
            p = v.data_ptr() if v.numel() else None
        else:
            p = v.ctypes.data if v.size else None
        if k in null or (c["nspans"] == 0 and k in ("span_frame_off", "enc_frame_off", "enc_buf")):
            p = None
        keep.append(v)
        setattr(r, k, p)
    room = nbytes if room is None else room
    sizes = {"need_ans_off": (c["nneeds"] + 2, np.uint64), "frame_ans_off": (c["nframes"] + 2, np.uint64),
             "frame_host": (c["nframes"] + 1, np.uint8), "buf": (GUARD + out_shift + room + GUARD + 16, np.uint8)}
    outs = {}
    o = L.Assembled()
    o.nbytes = nbytes
    for k, (n, dt) in sizes.items():
        if mem == "device":
            outs[k] = torch.full((n,), 7, dtype=torch.int64 if dt == np.uint64 else torch.uint8, device="cuda")
            p = outs[k].data_ptr()
            assert p % 16 == 0
        else:
            outs[k] = np.full(n, 7, dt)
            p = outs[k].ctypes.data
        setattr(o, k, None if k in null else p + (GUARD + out_shift if k == "buf" else 0))
    if mem == "device":
        torch.cuda.synchronize()
    rc = L.lib().corro_assemble_answers(engine()._h, C.byref(r), L.CORRO_MEM_DEVICE if mem == "device" else L.CORRO_MEM_HOST,
                                        C.byref(o), pas)
    outs = {k: host(v).view(sizes[k][1]) for k, v in outs.items()}
    assert (outs["buf"][:out_shift] == 7).all()
    outs["buf"] = outs["buf"][out_shift:]
    return rc, int(o.nbytes), outs


def untouched(outs):
    return all((v == 7).all() for v in outs.values())


def check(a, what, mem="device", **kw):
    """Both passes against the model; nothing is written outside the arrays' extents."""
    buf, nao, fao, fh = U.model(a)
    T, F = len(nao) - 1, len(fh)
    rc, n, o0 = raw(a, 0, mem, **kw)
    assert rc == 0, (what, L.lib().corro_last_error())
    assert n == len(buf), what
    assert o0["need_ans_off"][:T + 1].tolist() == nao and o0["need_ans_off"][T + 1] == 7, what
    assert o0["frame_ans_off"][:F + 1].tolist() == fao and o0["frame_ans_off"][F + 1] == 7, what
    assert o0["frame_host"][:F].tolist() == fh and o0["frame_host"][F] == 7, what
    assert (o0["buf"] == 7).all(), what
    rc, n1, o1 = raw(a, 1, mem, nbytes=n, **kw)
    assert rc == 0 and n1 == n, (what, L.lib().corro_last_error())
    got = o1["buf"][GUARD:GUARD + n].tobytes()
    if got != buf:
        bad = next(i for i in range(n) if got[i] != buf[i])
        raise AssertionError(f"{what}: byte {bad} of {n} differs")
    assert (o1["buf"][:GUARD] == 7).all() and (o1["buf"][GUARD + n:] == 7).all(), what
    assert all((o1[k] == 7).all() for k in ("need_ans_off", "frame_ans_off", "frame_host")), what    # pass 0's arrays
    return buf, nao, fao, fh


def kept(*pieces):
    return [(nb, nt, 1, 0) for nb, nt in pieces]


# ---- directed shapes ------------------------------------------------------------------------------

@pytest.mark.parametrize("payload", (0, 1))
def test_piece_boundaries_on_every_residue(payload):
    """Encoded pieces of 0..48, 49, 55, 64 and 65 bytes, tails of 0..2 frames between them, behind a
    first piece of 0..15 bytes: piece boundaries fall on every residue mod 16, from both sides."""
    rng = np.random.default_rng(10 + payload)
    lengths = list(range(49)) + [49, 55, 64, 65]
    seen = set()
    for first in range(16):
        order = lengths if first % 2 == 0 else lengths[::-1]
        a = U.build(kept((first, 0), *[(n, (n + first) % 3) for n in order]), rng, payload, junk=first % 3)
        _, nao, _, _ = check(a, f"first {first}", out_shift=first if first % 4 == 1 else 0)
        seen |= {x % 16 for x in nao}
    assert seen == set(range(16))


@pytest.mark.parametrize("payload", (0, 1))
def test_blocks_that_span_three_or_more_pieces(payload):
    rng = np.random.default_rng(20 + payload)
    one = [(1, 0)]
    needs = kept(*(one * 40)) + [(0, 0, 0, 0)] * 3 + kept(*(one * 5), (30, 1), *(one * 20), (2, 0), (0, 1), *(one * 33), (3, 0))
    for out_shift in (0, 7):
        check(U.build(needs, rng, payload, pairs=[50, len(needs) - 50]), "one-byte pieces", out_shift=out_shift)
    check(U.build(kept(*(one * 300)), rng, payload, split=False), "300 one-byte pieces")


def _empties(k, where):
    """Needs that give a run of exactly k empty pieces between a tail that holds bytes and an encoded
    piece that holds bytes (where = "start" / "middle"), or after the last bytes (where = "end")."""
    if where == "end":
        return ([(7, 0, 1, 0)] if k % 2 else []) + [(0, 0, 0, 0)] * (k // 2)
    return [(0, 0, 0, 0)] * (k // 2) + ([(0, 1, 1, 0)] if k % 2 else [])


@pytest.mark.parametrize("payload", (0, 1))
def test_runs_of_empty_pieces(payload):
    """1, 2 and 1000 empty pieces in a row at the start, in the middle and at the end. 1000 of them are
    longer than the window of offsets the copy kernel keeps in LDS."""
    assert 1000 > U.WINDOW
    rng = np.random.default_rng(30 + payload)
    for ks, km, ke in ((1, 1, 1), (2, 2, 2), (1000, 1000, 1000), (1000, 1, 2), (2, 1000, 1), (1, 2, 1000)):
        needs = _empties(ks, "start") + kept((20, 1)) + _empties(km, "middle") + kept((33, 2)) + _empties(ke, "end")
        a = U.build(needs, rng, payload)
        buf, _, _, _ = check(a, f"runs {ks} {km} {ke}")
        assert len(buf) == 20 + 33 + 3 * U.FRAME[payload] + (7 if ke % 2 else 0) + (ks % 2 + km % 2) * U.FRAME[payload]


@pytest.mark.parametrize("payload", (0, 1))
def test_one_piece_or_none_and_the_smallest_outputs(payload):
    rng = np.random.default_rng(40 + payload)
    check(U.build(kept((5, 0), (0, 2), (0, 0), (5, 1)), rng, payload), "encoded only, tail only, neither, both")
    for what, needs in (("encoded only", kept((9, 0))), ("tail only", kept((0, 1))), ("neither", kept((0, 0))),
                        ("unkept", [(0, 0, 0, 0)]), ("no need", [])):
        for mem in ("device", "host"):
            check(U.build(needs, rng, payload), what, mem)
    for total in (0, 1, 15, 16, 17):                           # as one piece and as two
        for out_shift in (0, 1, 15):
            check(U.build(kept((total, 0)), rng, payload, split=False), f"{total} bytes", out_shift=out_shift)
            check(U.build(kept((total // 2, 0), (total - total // 2, 0)), rng, payload), f"{total} bytes in two",
                  out_shift=out_shift)


@pytest.mark.parametrize("payload", (0, 1))
def test_just_over_two_tiles(payload):
    """A tile boundary inside a piece and one exactly on a piece boundary, with the buffer at the start of
    an aligned block and 3 bytes into one (the tiles are cut in the buffer's address range)."""
    rng = np.random.default_rng(50 + payload)
    a = U.build(kept((5000, 0), (7000, 0), (4384, 0), (5, 0)), rng, payload, split=False)
    _, nao, _, _ = check(a, "tiles, aligned")
    assert nao[1] < U.TILE < nao[2] and nao[3] == 2 * U.TILE and nao[-1] == 2 * U.TILE + 5
    fs = U.FRAME[payload]
    a = U.build(kept((U.TILE - 3, 0), (3000, 1), (2 * U.TILE - (U.TILE - 3) - 3000 - fs + 40, 0)), rng, payload)
    _, nao, _, _ = check(a, "tiles, 3 bytes in", out_shift=3)
    assert nao[1] + 3 == U.TILE and nao[2] + 3 < 2 * U.TILE < nao[3] + 3
    for mem in ("device", "host"):                             # a host-memory call stages the same bytes
        check(U.build(kept((U.TILE, 2), (0, 0), (U.TILE + 1, 0)), rng, payload), "tiles, " + mem, mem)


def test_source_buffers_at_every_misalignment():
    rng = np.random.default_rng(60)
    for s in range(1, 16):
        needs = kept((200 + s, 1), (3, 0), (0, 2), (100, 0), (17, 3), (64, 0), (1, 1), (300, 0))
        a = U.build(needs, rng, s % 2, junk=s % 3)
        check(a, f"enc + {s}", enc_shift=s)
        check(a, f"tail + {s}", tail_shift=s)
        check(a, f"all three + {s}", enc_shift=s, tail_shift=(7 * s) % 16, out_shift=(5 * s) % 16)
        check(a, f"same misalignment {s}", enc_shift=s, tail_shift=s, out_shift=s)


@pytest.mark.parametrize("payload", (0, 1))
def test_frames_pairs_and_frame_host(payload):
    rng = np.random.default_rng(70 + payload)
    #        bytes tails keep host
    needs = [(5, 0, 1, 1), (6, 1, 1, 0), (7, 1, 1, 0),         # frame 1: the first need is the host's
             (8, 1, 1, 0), (0, 0, 0, 1), (9, 2, 1, 0),         # frame 3: an unkept need with the flag
             (4, 1, 1, 0), (3, 0, 1, 1),                       # frame 4, two pairs: the last need is the host's
             (2, 1, 1, 0)]                                     # frame 6
    a = U.build(needs, rng, payload, pairs=[0, 3, 0, 3, 0, 1, 1, 1, 0], frames=[1, 1, 0, 2, 3, 0, 1, 1, 0])
    _, _, fao, fh = check(a, "frames")
    assert fh == [0, 1, 0, 0, 1, 0, 0, 0, 0]
    assert [fao[f + 1] - fao[f] > 0 for f in range(9)] == [False, True, False, True, True, False, True, False, False]
    check(a, "frames, host memory", "host")


@pytest.mark.parametrize("payload", (0, 1))
def test_no_spans_and_no_ranges(payload):
    rng = np.random.default_rng(80 + payload)
    a = U.build(kept((0, 1), (0, 0), (0, 3)), rng, payload, split=False, pairs=[1, 2])
    a["span_frame_off"], a["need_span_off"] = np.zeros(1, np.uint64), np.zeros(4, np.uint64)
    assert U.counts(a)["nspans"] == 0
    for mem in ("device", "host"):
        buf, _, _, _ = check(a, "no spans", mem)              # raw() passes NULL for the encoder's three arrays
        assert len(buf) == 4 * U.FRAME[payload]
    b = U.build(kept((10, 0), (0, 0), (31, 0)), rng, payload)
    assert U.counts(b)["nranges"] == 0 and len(b["tail_buf"]) == 0
    for mem in ("device", "host"):
        check(b, "no ranges", mem)                             # ... and NULL for the tail buffer
    c = dict(a, need_tail_off=np.zeros(4, np.uint64), tail_buf=np.zeros(0, np.uint8))
    check(c, "neither")


def test_seeded_random_cases():
    total = hosted = 0
    for seed in range(2000, 2200):
        rng = np.random.default_rng(seed)
        a = U.random_case(rng)
        assert len(a["frame_pair_off"]) - 1 <= 64 and len(a["need_keep"]) <= 300
        dev = seed % 4 != 0
        s = rng.integers(0, 16, 3) if dev and seed % 3 else (0, 0, 0)
        buf, _, _, fh = check(a, f"seed {seed}", "device" if dev else "host", enc_shift=int(s[0]), tail_shift=int(s[1]),
                              out_shift=int(s[2]))
        total += len(buf)
        hosted += sum(fh)
    assert total > 1_000_000 and hosted > 100, (total, hosted)


def test_through_the_engine():
    rng = np.random.default_rng(90)
    a = U.random_case(rng)
    while len(a["need_keep"]) < 50:
        a = U.random_case(rng)
    buf, nao, fao, fh = U.model(a)
    c = U.counts(a)
    for put in (to_dev, lambda x: x):
        dec = {"nframes": c["nframes"], "npairs": c["npairs"], "nneeds": c["nneeds"],
               **{k: put(a[k]) for k in ("frame_pair_off", "pair_need_off", "need_keep")}}
        sp = {"nspans": c["nspans"], "need_span_off": put(a["need_span_off"])}
        enc = {"nframes": c["enc_nframes"], "nbytes": c["enc_nbytes"], "span_frame_off": put(a["span_frame_off"]),
               "frame_off": put(a["enc_frame_off"]), "buf": put(a["enc_buf"])}
        tl = {"nranges": c["nranges"], "need_tail_off": put(a["need_tail_off"]), "need_host": put(a["need_host"]),
              "buf": put(a["tail_buf"])}
        got = engine().assemble_answers(dec, sp, enc, tl, a["payload"])
        assert got["nbytes"] == len(buf) and host(got["buf"]).tobytes() == buf
        assert host(got["need_ans_off"]).astype(np.int64).tolist() == nao
        assert host(got["frame_ans_off"]).astype(np.int64).tolist() == fao
        assert host(got["frame_host"]).tolist() == fh
        assert hasattr(got["buf"], "is_cuda") == (put is to_dev)


# ---- validation -----------------------------------------------------------------------------------

def base_case():
    rng = np.random.default_rng(100)
    needs = [(40, 1, 1, 0), (0, 0, 0, 0), (25, 0, 1, 1), (0, 2, 1, 0), (60, 1, 1, 0), (9, 0, 1, 0)]
    return U.build(needs, rng, 0, pairs=[2, 1, 3], frames=[1, 2], junk=2)


def mutate(field, idx, val):
    def f(a):
        a[field] = a[field].copy()
        a[field][idx] = val
    return f


def _tail_bytes(a):
    a["tail_buf"] = a["tail_buf"][:-1]


BAD = {f"{k} decreases": mutate(k, 1, 1 << 40) for k in U.OFFSETS}
BAD.update({f"{k} ends past its bound": mutate(k, -1, 1 << 20) for k in U.OFFSETS})
BAD.update({
    "frame_pair_off ends one past npairs": mutate("frame_pair_off", -1, 4),
    "pair_need_off ends one past nneeds": mutate("pair_need_off", -1, 7),
    "need_tail_off ends one past nranges": mutate("need_tail_off", -1, 9),
    "need_span_off starts above its next": mutate("need_span_off", 0, 1 << 50),
    "tail_nbytes is not nranges frames": _tail_bytes,
})


@pytest.mark.parametrize("name", list(BAD))
def test_validation_refuses_and_writes_nothing(name):
    good = base_case()
    n = len(U.model(good)[0])
    for mem in ("device", "host"):
        check(good, "base case", mem)                          # the base case itself is served
        bad = dict(good)
        BAD[name](bad)
        for pas in (0, 1):
            rc, nb, outs = raw(bad, pas, mem, nbytes=n if pas else 0)
            assert rc == -1, (name, mem, pas)
            assert untouched(outs) and nb == (n if pas else 0), (name, mem, pas)


def test_missing_arrays_and_bad_arguments_on_the_device():
    good = base_case()
    n = len(U.model(good)[0])
    for field in list(U.DTYPES) + ["need_ans_off", "frame_ans_off", "frame_host"]:
        rc, _, outs = raw(good, 0, null=(field,))
        assert rc == -1 and untouched(outs), field
    rc, _, outs = raw(good, 1, nbytes=n, null=("buf",))
    assert rc == -1 and untouched(outs)
    for payload in (2, 255):
        rc, _, outs = raw(good, 0, payload=payload)
        assert rc == -1 and untouched(outs) and b"payload" in L.lib().corro_last_error()
    rc, _, outs = raw(good, 2)
    assert rc == -1 and untouched(outs) and b"pass" in L.lib().corro_last_error()
    # the other payload's frame size: the same tail buffer is not a whole number of 55-byte frames
    rc, _, outs = raw(good, 0, payload=1)
    assert rc == -1 and untouched(outs) and b"tail_nbytes" in L.lib().corro_last_error()


def test_pass_one_nbytes_must_be_pass_zero_s():
    good = base_case()
    n = len(U.model(good)[0])
    for mem in ("device", "host"):
        for wrong in (n - 1, n + 1, 0):
            rc, nb, outs = raw(good, 1, mem, nbytes=wrong, room=n + 1)
            assert rc == -1 and b"pass 0" in L.lib().corro_last_error(), (mem, wrong)
            assert untouched(outs) and nb == wrong


# ---- through an agent -----------------------------------------------------------------------------

class State:
    pass


@pytest.fixture(scope="module")
def st():
    """A: actor A0 versions 1..6 and 8..14 (7 is a gap) and seqs 0..1 of version 15 buffered; actor A1
    versions 1..12, then 13 and 14 rewriting every cell of its versions 2 and 3 (cleared versions)."""
    from corrosion_amd.agent import ChangeV1, Full
    from tests import req_decode_util as R
    from tests.test_gpu_serve_requests import A0, A1, STRANGER, _agent, _changes, _msg
    s = State()
    s.a = _agent(bytes([0xA0]) * 16)
    msgs = [_msg(A0, 0, v) for v in list(range(1, 7)) + list(range(8, 15))] + [_msg(A0, 0, 15, (0, 1))]
    msgs += [_msg(A1, 1, v) for v in range(1, 13)]
    msgs.append(ChangeV1(A1, Full(13, _changes(A1, 1, 2, dbv=13, cv=2), (0, 2), 2, ts=2013)))
    msgs.append(ChangeV1(A1, Full(14, _changes(A1, 1, 3, dbv=14, cv=2), (0, 2), 2, ts=2014)))
    res = s.a.process_multiple_changes(msgs)
    assert res.known.count("current") == len(msgs) - 1 and res.known.count("partial") == 1, res.known
    s.buffered = [(A0, S.Full(14, 16)), (A0, S.Partial(15, ((0, 1),))), (A0, S.Full(15, 15))]
    s.frames = [
        R.request_frame([(A1, [S.Full(1, 4), S.Full(1, 20), S.Partial(2, ((0, 2),)), S.Partial(5, ((1, 1),)),
                               S.Full(3, 3), S.Full(14, 30)])]),
        R.request_frame([(STRANGER, [S.Full(1, 9)])]),
        # device-served needs before and after each host need of the frame, and a screened one between
        R.request_frame([(A0, [S.Full(1, 5), S.Full(5, 9), s.buffered[0][1], S.Full(7, 7), S.Full(10, 14)]),
                         (A1, [S.Partial(3, ((0, 0), (2, 2)))]),
                         (A0, [s.buffered[1][1], S.Partial(16, ((0, 0),)), S.Partial(10, ((0, 2),)), s.buffered[2][1]])]),
        R.request_frame([(A0, [S.Full(1, 2)])])[:-1],          # malformed
        R.request_frame([(A0, [S.Full(7, 7), S.Full(20, 25)])]),               # every need screened out
        R.request_frame([(A0, [s.buffered[2][1]]), (A1, [S.Full(12, 12)])]),   # the host need comes first
        R.request_frame([(A1, [S.Full(2, 3)])]),               # tail frames alone
    ]
    # a peer that holds nothing asks for everything
    b = _agent(bytes([0xB0]) * 16)
    needs = b.generate_sync().compute_available_needs(s.a.generate_sync(), b.engine)
    assert set(needs) == {A0, A1}
    s.frames += [f for _round, f in S.plan_sync_requests(b.engine, [[needs]])[0][0]]
    return s


KWS = ({}, dict(payload=1, cluster_id=77), dict(max_buf_size=150), dict(max_buf_size=150, payload=1, cluster_id=513))


@pytest.mark.parametrize("kw", KWS, ids=("sync", "uni", "sync-150", "uni-150"))
def test_answers_equal_handle_request_frames(st, kw, monkeypatch):
    from corrosion_amd import serve
    from tests import req_decode_util as R
    buf, off = R.cat(st.frames)
    calls = []
    real = serve._bookie_messages

    def counted(agent, actor, need, *a, **k):
        calls.append((actor, need))
        return real(agent, actor, need, *a, **k)
    monkeypatch.setattr(serve, "_bookie_messages", counted)
    status, want = serve.handle_request_frames(st.a, buf, off, **kw)
    assert status.tolist()[:7] == [0, 0, 0, R.E_INVALID, 0, 0, 0] and (status[7:] == 0).all()
    assert [bool(w) for w in want[:7]] == [True, False, True, False, False, True, True] and sum(map(len, want[7:])) > 0
    want_calls = list(calls)
    del calls[:]
    timings = {}
    got_status, got = serve.handle_request_frames_assembled(st.a, buf, off, timings=timings, **kw)
    assert got_status.tolist() == status.tolist()
    assert [len(g) for g in got] == [len(w) for w in want]
    assert got == want
    assert all(type(g) is bytes for g in got)
    # the host walk is left to the needs that touch the buffered version, in frames 2 and 5 and wherever
    # the peer that holds nothing asks for A0's versions 14..16
    assert calls == want_calls and calls[:4] == st.buffered + [st.buffered[2]]
    assert set(timings) == {"book", "decode", "extract", "spans", "encode", "tails", "assemble", "readback", "bookie"}
    # the same from a peer's device output
    import torch
    dbuf = torch.from_numpy(np.frombuffer(buf.tobytes(), np.uint8).copy()).cuda()
    doff = torch.from_numpy(np.ascontiguousarray(off, np.uint64).view(np.int64)).cuda()
    assert serve.handle_request_frames_assembled(st.a, dbuf, doff, **kw)[1] == want


def test_answers_without_a_host_need_and_with_nothing_to_answer(st):
    from corrosion_amd import serve
    from tests import req_decode_util as R
    for pick in ([0, 1, 6], [4], [1, 3], [4, 1, 4]):           # the last three: every need screened out or none
        buf, off = R.cat([st.frames[i] for i in pick])
        for kw in KWS[:2]:
            status, want = serve.handle_request_frames(st.a, buf, off, **kw)
            got_status, got = serve.handle_request_frames_assembled(st.a, buf, off, **kw)
            assert got_status.tolist() == status.tolist() and got == want, pick
            assert any(want) == (pick == [0, 1, 6])
    assert serve.handle_request_frames_assembled(st.a, b"", np.zeros(1, np.uint64))[1] == []
