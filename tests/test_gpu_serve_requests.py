"""serve.handle_request_frames: request bytes -> response bytes on the device (corro_decode_requests,
corro_extract_changes, corro_need_spans, corro_encode_changesets). The expected bytes come from the
path that was there before it -- wire.decode_sync_request, the looping screen of
tests/req_decode_util.py and serve.handle_needs_frames one need at a time -- never from the code under
test. Bar: byte-exact."""
import numpy as np
import pytest

from corrosion_amd import sync as S
from tests import req_decode_util as U

pytestmark = pytest.mark.gpu

A0, A1 = bytes([0x11]) * 16, bytes([0x22]) * 16
STRANGER = bytes([0xEE]) * 16
SCHEMA = {"tests": ["text", "num"], "testsblob": ["text", "blob"]}
SPAN_FIELDS = ("site", "version", "last_seq", "ts", "seq_start", "seq_end", "row_off", "row_count")


def _changes(actor, a, v, dbv=None, cv=1):
    """Version v of actor number a: three changes (seq 0..2) to rows of their own; every fifth version
    carries a long TEXT, every fourth a long BLOB under an interned (BLOB) pk."""
    from corrosion_amd.agent import Change
    from tests.test_gpu_pk import _pack
    # (pks of 1010 .. 2161: two packed bytes with the top bit clear, so they read back as themselves;
    # unpack_columns sign-extends, wire.unpack_int_pk states the quirk)
    base, d = 1000 + (a * 100 + v) * 10, dbv or v
    return [Change("tests", base, "text", "z" * 300 if v % 5 == 0 else f"t{v}", cv, d, 0, actor, 1),
            Change("tests", base + 1, "num", v * 7 - 3, cv, d, 1, actor, 1),
            Change("testsblob", _pack([bytes([a, v]) * 3]), "blob", bytes(range(20)) if v % 4 == 0 else b"b", cv, d, 2, actor, 1)]


def _msg(actor, a, v, seqs=(0, 2)):
    from corrosion_amd.agent import ChangeV1, Full
    ch = [c for c in _changes(actor, a, v) if seqs[0] <= c.seq <= seqs[1]]
    return ChangeV1(actor, Full(v, ch, seqs, 2, ts=1000 + v))


def _agent(actor_id):
    import corrosion_amd as ca
    ag = ca.agent.Agent(SCHEMA, capacity_hint=1 << 12, actor_id=actor_id, interned=("testsblob",))
    ag.site(A0)
    ag.site(A1)
    return ag


class State:
    pass


@pytest.fixture(scope="module")
def st():
    """A: actor A0 versions 1..6 and 8..14 (7 is a gap) and seqs 0..1 of version 15 buffered; actor A1
    versions 1..12, then 13 rewriting every cell of its version 2 (known, with no row left)."""
    from corrosion_amd.agent import ChangeV1, Full
    s = State()
    s.a = _agent(bytes([0xA0]) * 16)
    msgs = [_msg(A0, 0, v) for v in list(range(1, 7)) + list(range(8, 15))] + [_msg(A0, 0, 15, (0, 1))]
    msgs += [_msg(A1, 1, v) for v in range(1, 13)]
    msgs.append(ChangeV1(A1, Full(13, _changes(A1, 1, 2, dbv=13, cv=2), (0, 2), 2, ts=2013)))
    res = s.a.process_multiple_changes(msgs)
    assert res.known.count("current") == len(msgs) - 1 and res.known.count("partial") == 1, res.known
    assert s.a.bookie.needed(A0) == [(7, 7)] and s.a.bookie.last(A0) == 15 and s.a.bookie.needed(A1) == []
    s.msgs = msgs
    s.frames = [
        (U.request_frame([(A0, [S.Full(1, 5), S.Full(5, 9), S.Full(7, 7), S.Full(20, 25), S.Full(14, 16)])]), 0),
        (U.request_frame([(A1, [S.Full(1, 4), S.Partial(3, ((0, 0), (2, 2))), S.Partial(2, ((0, 2),)),
                                S.Partial(5, ((1, 1), (7, 9)))]),
                          (A0, [S.Partial(15, ((0, 1),)), S.Partial(7, ((0, 1),)), S.Partial(16, ((0, 0),)),
                                S.Partial(15, ((1, 2),)), S.Partial(10, ((0, 2),))])]), 0),
        (U.request_frame([(STRANGER, [S.Full(1, 9)])]), 0),
        (U.request_frame([(A0, [S.Full(1, 2)])])[:-1], U.E_INVALID),
        (U.request_frame([(A1, [S.Full(1, 2)])])[:-20] + b"\x02\0\0\0" + b"\0" * 16, 2),
        (U.request_frame([(A1, [S.Full(12, 12)])]), 0),
    ]
    s.keep = [[1, 1, 0, 0, 1], [1, 1, 1, 1, 1, 0, 0, 1, 1], [0], [], [], [1]]
    return s


def books_of(agent):
    """The bookie as the screen's model takes it, for the registered sites that have a version."""
    out = {}
    for site, actor in enumerate(agent.engine.site_ids()):
        last, needed = agent.bookie.last(actor), agent.bookie.needed(actor)
        if last is not None or needed:
            out[site] = (needed, last)
    return out


def expected_answers(agent, frames, **kw):
    """Per frame, the bytes of the host path: decode, screen, handle_needs_frames per kept need."""
    from corrosion_amd import serve, wire
    sites = {a: i for i, a in enumerate(agent.engine.site_ids())}
    books = books_of(agent)
    out, keeps = [], []
    for fb, status in frames:
        parts, kp = [], []
        if status == 0:
            for actor, needs in wire.decode_sync_request(fb[4:]):
                for nd in needs:
                    k = actor in sites and U.keeps(books.get(sites[actor]), nd)
                    kp.append(1 if k else 0)
                    if k:
                        parts.append(serve.handle_needs_frames(agent, [(actor, nd)], **kw)[0])
                        assert parts[-1], (actor, nd)          # every kept need here has an answer
        out.append(b"".join(parts))
        keeps.append(kp)
    return out, keeps


def to_dev(a):
    import torch
    view = {8: np.int64, 4: np.int32, 1: np.uint8}[a.dtype.itemsize]
    return torch.from_numpy(np.ascontiguousarray(a).view(view).copy()).cuda()


def host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def test_answers_equal_the_host_path_need_by_need(st):
    from corrosion_amd import serve
    nsites = st.a.engine.site_count()
    exp, keeps = expected_answers(st.a, st.frames)
    assert keeps == st.keep
    buf, off = U.cat([f for f, _ in st.frames])
    status, got = serve.handle_request_frames(st.a, buf.tobytes(), off)
    assert status.tolist() == [s for _, s in st.frames]
    assert got == exp
    assert got[2] == got[3] == got[4] == b"" and all(got[i] for i in (0, 1, 5))
    status, got = st.a.handle_request_frames(to_dev(buf), to_dev(off))      # a peer's device output
    assert status.tolist() == [s for _, s in st.frames] and got == exp
    assert st.a.engine.site_count() == nsites                                # the stranger was not registered
    # small chunks and the uni payload: the device path cuts and tags the frames as the host path does
    kw = dict(max_buf_size=150, payload=1, cluster_id=77)
    exp, _ = expected_answers(st.a, st.frames, **kw)
    assert serve.handle_request_frames(st.a, buf, off, **kw)[1] == exp
    assert serve.handle_request_frames(st.a, b"", np.zeros(1, np.uint64))[1] == []


def _decode_extract(st):
    import torch
    from corrosion_amd import serve
    eng = st.a.engine
    buf, off = U.cat([f for f, _ in st.frames])
    dec = eng.decode_requests(to_dev(buf), to_dev(off), serve.device_book(st.a, torch.device("cuda", eng.device)))
    ext = eng.extract_changes({"site": dec["ent_site"], "start": dec["ent_start"], "end": dec["ent_end"],
                               "seq_start": dec["ent_seq_start"], "seq_end": dec["ent_seq_end"]})
    return dec, ext


def test_need_spans_alone(st):
    """The span arrays against the rules of serve.handle_needs_frames, computed here from the decode and
    the extraction brought to the host; from device and from host memory."""
    eng = st.a.engine
    dec, ext = _decode_extract(st)
    d = {k: host(v) for k, v in dec.items() if hasattr(v, "cpu")}
    x = {k: host(v) for k, v in ext.items() if k != "rows"}
    assert d["need_keep"].tolist() == sum(st.keep, [])
    go = x["grp_off"].astype(np.int64)
    spans, off, ins = [], [0], []
    for t in range(dec["nneeds"]):
        k, state = int(d["need_ent_off"][t]), 0
        if d["need_keep"][t] and d["kind"][t] == 0:
            for g in range(go[k], go[k + 1]):                                  # db_version DESC
                spans.append((d["need_site"][t], x["version"][g], x["last_seq"][g], x["ts"][g], 0, x["last_seq"][g],
                              x["grp_row_off"][g], x["grp_rows"][g]))
        elif d["need_keep"][t] and go[k + 1] > go[k]:
            state, m = 1, go[k]
            for j in range(int(d["sr_n"][t])):
                g0, g1 = go[k + 1 + j], go[k + 2 + j]
                q = int(d["sr_off"][t]) + j
                spans.append((d["need_site"][t], x["version"][m], x["last_seq"][m], x["ts"][m], d["s_start"][q],
                              d["s_end"][q], x["grp_row_off"][g0 if g1 > g0 else 0], x["grp_rows"][g0] if g1 > g0 else 0))
        off.append(len(spans))
        ins.append(state)
    # in the state: A1's Partial 3 and 5, A0's Partial 10; not: A1's cleared 2, A0's buffered 15
    assert ins == [0] * 5 + [0, 1, 0, 1] + [0, 0, 0, 0, 1] + [0] + [0]
    assert any(s[7] == 0 for s in spans)                                       # the seq range 7..9 found no row
    want = {k: [int(s[i]) for s in spans] for i, k in enumerate(SPAN_FIELDS)}
    dh = {k: v for k, v in d.items()}
    dh.update(nneeds=dec["nneeds"], nseqs=dec["nseqs"], nents=dec["nents"])
    for got in (eng.need_spans(dec, ext), eng.need_spans(dh, x)):
        assert got["nspans"] == len(spans) >= 15
        assert host(got["need_span_off"]).astype(np.int64).tolist() == off
        assert host(got["in_state"]).tolist() == ins
        for k in SPAN_FIELDS:
            assert host(got[k]).astype(np.int64).tolist() == want[k], k
    # offsets are validated before anything is read through them
    import corrosion_amd as ca
    for field, idx, val in (("need_ent_off", 1, 1 << 40), ("need_ent_off", 3, 0), ("sr_n", 6, 1 << 50), ("kind", 0, 2)):
        bad = dict(dh)
        bad[field] = dh[field].copy()
        bad[field][idx] = val
        with pytest.raises(ca.CorroError) as e:
            eng.need_spans(bad, x)
        assert e.value.code == -1, field
    badx = dict(x)
    badx["grp_off"] = x["grp_off"].copy()
    badx["grp_off"][-1] = len(x["version"]) + 1
    with pytest.raises(ca.CorroError):
        eng.need_spans(dh, badx)


def _canon(agent):
    from corrosion_amd import serve
    eng = agent.engine
    rows = eng.export()
    ch = serve.rows_to_changes(eng, dict(enumerate(eng.site_ids())), rows, 0, len(rows["pk"]))
    return sorted((c.table, c.pk, c.cid, repr(c.val), c.col_version, c.db_version, c.seq, c.site_id, c.cl) for c in ch)


def test_whole_loop_between_two_agents(st):
    """B is behind A: B's sync state and the need diff give needs, the planner request bytes, A's
    handle_request_frames the answer, B's process_frames applies it: B's rows equal A's."""
    b = _agent(bytes([0xB0]) * 16)
    b.process_multiple_changes([m for m in st.msgs if m.actor_id == A0 and m.changeset.version <= 3])
    assert _canon(b) != _canon(st.a)
    needs = b.generate_sync().compute_available_needs(st.a.generate_sync(), b.engine)
    assert set(needs) == {A0, A1}
    planned = S.plan_sync_requests(b.engine, [[needs]])
    frames = [f for _round, f in planned[0][0]]
    assert len(frames) >= 3
    buf, off = U.cat(frames)
    status, answers = st.a.handle_request_frames(buf, off)
    assert (status == 0).all() and sum(map(len, answers)) > 0
    res, dstatus = b.process_frames(b"".join(answers))
    assert (host(dstatus) == 0).all() and "current" in res.known
    for actor, version in res.ready:
        b.process_fully_buffered_changes(actor, version)
    assert _canon(b) == _canon(st.a)
    assert b.bookie.last(A1) == 13 and b.bookie.needed(A1) == []
