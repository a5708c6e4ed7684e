"""serve.handle_request_frames_buffered: a sync need's buffered (partial) versions answered from the
device row pool (corro_bookie_buffered_index, corro_buffered_spans, a second corro_encode_changesets,
corro_assemble_answers_buffered). The state is built with Agent.process_frames, so the partial rows land
in the pool. The expected bytes are wire.frames(serve.handle_needs(...)) on a second, identically fed
agent -- the host walk materialises a version, so it never runs on the agent under test before the
device path. Bar: byte-exact, both payloads."""
import ctypes as C

import numpy as np
import pytest

from corrosion_amd import _lib as L
from corrosion_amd import sync as S
from corrosion_amd.engine import ROW_FIELDS
from tests import buffered_util as B
from tests import req_decode_util as U

pytestmark = pytest.mark.gpu

A0, A1 = bytes([0x11]) * 16, bytes([0x22]) * 16
SCHEMA = {"tests": ["text", "num"], "testsblob": ["text", "blob"]}
KW = (dict(), dict(max_buf_size=150, payload=1, cluster_id=77))   # 150: a span of 2+ rows makes several frames


def _changes(actor, a, v, long_at=None):
    """Version v of actor number a: six changes (seq 0..5) to rows of their own, short values (pool rows
    hold no long value) unless long_at names a seq; seqs 2 and 5 go to an interned (BLOB) pk."""
    from corrosion_amd.agent import Change
    from tests.test_gpu_pk import _pack
    base = 1000 + (a * 100 + v) * 10
    ch = [Change("tests", base, "text", f"t{v}", 1, v, 0, actor, 1),
          Change("tests", base + 1, "num", v * 7 - 3, 1, v, 1, actor, 1),
          Change("testsblob", _pack([bytes([a, v]) * 3]), "blob", b"b" * (v % 7), 1, v, 2, actor, 1),
          Change("tests", base + 2, "text", None, 1, v, 3, actor, 1),
          Change("tests", base + 3, "num", 2.5 * v, 1, v, 4, actor, 1),
          Change("testsblob", _pack([bytes([a, v, 9]) * 2]), "text", "x" * 16, 1, v, 5, actor, 1)]
    if long_at is not None:
        ch[long_at].val = "z" * 300
    return ch


def _msg(actor, a, v, seqs=(0, 5), long_at=None):
    from corrosion_amd.agent import ChangeV1, Full
    ch = [c for c in _changes(actor, a, v, long_at) if seqs[0] <= c.seq <= seqs[1]]
    return ChangeV1(actor, Full(v, ch, seqs, 5, ts=1000 + v))


def feed():
    """Actor A0: versions 1..3 and 6 whole, 4 and 7 never seen (gaps), 5 in two non-adjacent halves
    (0..1 and 4..5: two bookkeeping ranges, two segments), 8 as seqs 0..2, 9 as two adjacent pieces
    (0..1, 2..3: one bookkeeping range over two segments), 12 whole and then 11 as seqs 3..5, 10 as seqs
    0..1 with a long value (host rows). Actor A1: versions 1..2 whole, 3 as seqs 2..3. One call per
    list, in this order."""
    return [[_msg(A0, 0, v) for v in (1, 2, 3)] + [_msg(A0, 0, 5, (0, 1)), _msg(A0, 0, 6)],
            [_msg(A0, 0, 5, (4, 5)), _msg(A0, 0, 8, (0, 2)), _msg(A0, 0, 9, (0, 1)), _msg(A1, 1, 1), _msg(A1, 1, 2)],
            [_msg(A0, 0, 9, (2, 3)), _msg(A0, 0, 12), _msg(A1, 1, 3, (2, 3))],
            [_msg(A0, 0, 11, (3, 5)), _msg(A0, 0, 10, (0, 1), long_at=1)]]


def build(actor_id=bytes([0xA0]) * 16):
    import corrosion_amd as ca
    from corrosion_amd import wire
    ag = ca.agent.Agent(SCHEMA, capacity_hint=1 << 12, actor_id=actor_id, interned=("testsblob",))
    ag.site(A0)
    ag.site(A1)
    for msgs in feed():
        res, status = ag.process_frames(wire.frames(msgs))
        assert not np.asarray(status).any() and all(isinstance(k, str) for k in res.known), res.known
    return ag


# the frames without a host-row version, and the one with (version 10 holds host rows)
DEVICE_FRAMES = [
    # found 1..3 and 6, gaps 4 and 7, buffered 5 8 9; an unkept need (all of it a gap) between two served ones
    [(A0, [S.Full(1, 9), S.Full(4, 4), S.Full(5, 5), S.Full(7, 8)])],
    # seq ranges inside, across and outside the bookkeeping ranges (0,1) (4,5) of version 5, and inverted ones
    [(A0, [S.Partial(5, ((0, 0), (1, 4), (2, 3), (5, 9), (0, 5), (5, 4), (3, 0))), S.Partial(7, ((0, 1),)),
           S.Partial(8, ((0, 5), (1, 1))), S.Partial(9, ((1, 2), (3, 4))), S.Partial(2, ((0, 1),)), S.Partial(11, ((0, 5),))]),
     (A1, [S.Full(1, 6), S.Partial(3, ((0, 5),)), S.Partial(3, ((0, 1),))])],
    [(A1, [S.Full(3, 3)]), (A0, [S.Full(11, 14)])],
]
HOST_FRAMES = [[(A0, [S.Full(8, 10), S.Full(5, 5), S.Partial(10, ((0, 5),)), S.Full(9, 12)])]]


def books_of(agent):
    out = {}
    for site, actor in enumerate(agent.engine.site_ids()):
        last, needed = agent.bookie.last(actor), agent.bookie.needed(actor)
        if last is not None or needed:
            out[site] = (needed, last)
    return out


def expected_answers(agent, frames, max_buf_size=8192, payload=0, cluster_id=0):
    """Per frame, wire.frames(handle_needs(...)) of its kept needs on `agent` (host walk: it materialises)."""
    from corrosion_amd import serve, wire
    sites = {a: i for i, a in enumerate(agent.engine.site_ids())}
    books = books_of(agent)
    out = []
    for pairs in frames:
        parts = []
        for actor, needs in pairs:
            for nd in needs:
                if actor in sites and U.keeps(books.get(sites[actor]), nd):
                    msgs = serve.handle_needs(agent, [(actor, nd)], max_buf_size)[0]
                    if payload == wire.PAYLOAD_SYNC:
                        parts.append(wire.frames(msgs, wire.PAYLOAD_SYNC))
                    else:
                        parts.append(b"".join(wire.frame(wire.encode_uni_change(cv, cluster_id)) for cv in msgs))
        out.append(b"".join(parts))
    return out


def index_of(agent):
    from corrosion_amd import serve
    h = serve.buffered_index(agent)
    out = {}
    for site in range(len(h["ver_off"]) - 1):
        for i in range(int(h["ver_off"][site]), int(h["ver_off"][site + 1])):
            sr = [(int(h["sr_start"][j]), int(h["sr_end"][j])) for j in range(int(h["sr_off"][i]), int(h["sr_off"][i + 1]))]
            segs = [(int(h["seg_pool_off"][j]), int(h["seg_seq0"][j]), int(h["seg_n"][j]))
                    for j in range(int(h["seg_off"][i]), int(h["seg_off"][i + 1]))]
            out.setdefault(site, {})[int(h["version"][i])] = (int(h["on_device"][i]), int(h["last_seq"][i]), int(h["ts"][i]), sr, segs)
    return out, h


class State:
    pass


@pytest.fixture(scope="module")
def st():
    from corrosion_amd import serve
    s = State()
    s.a, s.twin = build(), build()
    s.idx0, s.h0 = index_of(s.a)
    s.buf, s.off = U.cat([U.request_frame(p) for p in DEVICE_FRAMES])
    s.got, s.timings = [], {}
    for kw in KW:                                              # the device path first: nothing ran on a's bookie yet
        s.got.append(serve.handle_request_frames_buffered(s.a, s.buf.tobytes(), s.off, timings=s.timings, **kw))
    s.idx1, _ = index_of(s.a)
    s.twin_idx0, _ = index_of(s.twin)
    s.twin_got = serve.handle_request_frames_assembled(s.twin, s.buf.tobytes(), s.off)
    s.twin_idx1, _ = index_of(s.twin)
    s.exp = [expected_answers(s.twin, DEVICE_FRAMES, **kw) for kw in KW]
    return s


def test_index_matches_the_per_version_probes(st):
    """corro_bookie_buffered_index against corro_bookie_buffered_versions / _seq_bookkeeping / needed(),
    and its derived books against their restatement; the shapes the other tests lean on are there."""
    from corrosion_amd import serve
    a, h = st.a, st.h0
    for site, actor in enumerate(a.engine.site_ids()):
        versions = serve._buffered_versions(st.twin.bookie, actor, 0, 0xFFFFFFFFFFFFFFFF)
        assert sorted(st.idx0.get(site, {})) == versions
        dev, hostb = [], []
        for v in versions:
            on_dev, last, ts, sr, segs = st.idx0[site][v]
            probe = serve._seq_bookkeeping(st.twin.bookie, actor, v)
            assert sr == [r for r, _l, _t in probe] and all((l, t) == (last, ts) for _r, l, t in probe)
            (dev if on_dev else hostb).append(v)
            assert bool(segs) == bool(on_dev)
            assert all(a0 + n0 <= b0 for (_, a0, n0), (_, b0, _n) in zip(segs, segs[1:]))
        g0, g1 = int(h["tail_gap_off"][site]), int(h["tail_gap_off"][site + 1])
        derived = [(int(h["tail_gap_start"][g]), int(h["tail_gap_end"][g])) for g in range(g0, g1)]
        assert derived == B.derive_tail_gaps(a.bookie.needed(actor), dev) and B.is_canonical(derived)
        assert [int(v) for v in h["host_buf_version"][int(h["host_buf_off"][site]):int(h["host_buf_off"][site + 1])]] == hostb
    i0 = st.idx0[0]
    assert sorted(i0) == [5, 8, 9, 10, 11] and [i0[v][0] for v in sorted(i0)] == [1, 1, 1, 0, 1]
    assert i0[5][3] == [(0, 1), (4, 5)] and [(q, n) for _, q, n in i0[5][4]] == [(0, 2), (4, 2)]
    assert i0[9][3] == [(0, 3)] and [(q, n) for _, q, n in i0[9][4]] == [(0, 2), (2, 2)]
    assert st.idx0[1][3][3] == [(2, 3)] and a.bookie.needed(A0) == [(4, 4), (7, 7)]


@pytest.mark.parametrize("k", range(len(KW)))
def test_answers_equal_the_host_walk_on_the_twin(st, k):
    status, got = st.got[k]
    assert status.tolist() == [0] * len(DEVICE_FRAMES)
    for f, (g, e) in enumerate(zip(got, st.exp[k])):
        assert g == e, (k, f)
    assert all(got)
    if k == 0:
        assert got == st.twin_got[1]                           # and the assembled path (host walk) on the twin
        assert "buffered" in st.timings and {"tails", "assemble", "encode"} <= set(st.timings)


def test_serving_materialises_nothing(st):
    """After the device path the index is what it was: every pool version still on the device, the same
    segments. The same request through handle_request_frames_assembled read them out of the twin's pool."""
    assert st.idx1 == st.idx0 == st.twin_idx0
    served = {(0, 5), (0, 8), (0, 9), (0, 11), (1, 3)}
    assert all(st.idx0[s][v][0] == 1 for s, v in served)
    assert all(st.twin_idx1[s][v][0] == 0 and not st.twin_idx1[s][v][4] for s, v in served)


def _stages(agent, buf, off, payload=0):
    """The device stages of handle_request_frames_buffered up to the tails, as tensors."""
    import torch
    from corrosion_amd import serve
    eng = agent.engine
    dev = torch.device("cuda", eng.device)
    tb = torch.from_numpy(np.frombuffer(bytes(buf), np.uint8).copy()).to(dev)
    to = torch.from_numpy(np.ascontiguousarray(off, np.uint64).view(np.int64)).to(dev)
    dec = eng.decode_requests(tb, to, serve.device_book(agent, dev))
    ext = eng.extract_changes({"site": dec["ent_site"], "start": dec["ent_start"], "end": dec["ent_end"],
                               "seq_start": dec["ent_seq_start"], "seq_end": dec["ent_seq_end"]})
    sp = eng.need_spans(dec, ext)
    idx = serve.device_buffered_index(agent, dev)
    tl = eng.need_tails(dec, ext, sp, idx["book"], payload, 0)
    return dec, ext, sp, idx, tl


def _needs_of(dec, ext, sp, tl):
    h = {k: dec[k].cpu().numpy() for k in ("kind", "start", "end", "sr_off", "sr_n", "s_start", "s_end", "need_keep",
                                           "need_site", "need_ent_off")}
    ins, host = sp["in_state"].cpu().numpy(), tl["need_host"].cpu().numpy()
    go, ver = ext["grp_off"].cpu().numpy(), ext["version"].cpu().numpy()
    out = []
    for t in range(len(h["kind"])):
        seqs = [(int(h["s_start"][q]), int(h["s_end"][q])) for q in range(int(h["sr_off"][t]), int(h["sr_off"][t] + h["sr_n"][t]))] \
            if h["kind"][t] else []
        found = set()
        if h["need_keep"][t] and h["kind"][t] == 0:
            k = int(h["need_ent_off"][t])
            found = {int(v) for v in ver[int(go[k]):int(go[k + 1])]}
        out.append((int(h["kind"][t]), int(h["need_site"][t]), int(h["start"][t]), int(h["end"][t]), seqs,
                    int(h["need_keep"][t]), int(host[t]), int(ins[t]), found))
    return out


ROW_KEYS = ("pk", "table_cid", "col_version", "db_version", "cl", "seq", "site", "ts", "val0", "val1", "val_type", "val_len")


def _pool_rows(agent, idx):
    """Every on_device version's rows by pool offset: the rows from the host probe of a third agent fed
    the same way (the probe materialises, so it runs on neither agent of the fixture), placed by idx's
    segments."""
    from corrosion_amd import serve
    third = build()
    rows = {}
    for site, actor in enumerate(third.engine.site_ids()):
        for v, (on_dev, _l, _t, _sr, segs) in idx.get(site, {}).items():
            if not on_dev:
                continue
            r, m = serve._buffered_rows(third.bookie, actor, v, 0, 0xFFFFFFFF)
            by_seq = {int(r["seq"][k]): {key: int(r[key][k]) for key in ROW_KEYS} for k in range(m)}
            for po, q0, n in segs:
                for q in range(q0, q0 + n):
                    rows[po + (q - q0)] = by_seq[q]
    return rows


def test_buffered_spans_against_the_model_with_seq_holes_and_empty_spans(st):
    """corro_buffered_spans alone, on the real pool with an index edited by hand: version 5's bookkeeping
    made one range 0..5 over its two segments (a seq hole 2..3 inside a bookkeeping range), version 8
    given a second range 4..5 that no segment covers (spans with no row), version 9's first segment
    cut to one row. Spans, offsets and all twelve row columns against the restated rules."""
    import torch
    eng = st.a.engine
    dec, ext, sp, idx, tl = _stages(st.a, st.buf, st.off)
    h = {k: v.copy() for k, v in idx["host"].items()}
    book, _ = index_of(st.a)
    pool = _pool_rows(st.a, book)
    on, last, ts, _sr, segs = book[0][5]
    book[0][5] = (on, last, ts, [(0, 5)], segs)
    on, last, ts, sr, segs = book[0][8]
    book[0][8] = (on, last, ts, sr + [(4, 5)], segs)
    on, last, ts, sr, segs = book[0][9]
    book[0][9] = (on, last, ts, sr, [(segs[0][0], segs[0][1], 1)] + segs[1:])
    # the edited index as arrays, in the index's own order
    arr = {k: [] for k in ("version", "last_seq", "ts", "on_device", "sr_start", "sr_end", "seg_pool_off", "seg_seq0", "seg_n")}
    ver_off, sr_off, seg_off = [0], [0], [0]
    for site in range(len(h["ver_off"]) - 1):
        for v in sorted(book.get(site, {})):
            on, last, ts, sr, segs = book[site][v]
            arr["version"].append(v); arr["last_seq"].append(last); arr["ts"].append(ts); arr["on_device"].append(on)
            arr["sr_start"] += [s for s, _ in sr]; arr["sr_end"] += [e for _, e in sr]
            arr["seg_pool_off"] += [p for p, _, _ in segs]; arr["seg_seq0"] += [q for _, q, _ in segs]
            arr["seg_n"] += [n for _, _, n in segs]
            sr_off.append(len(arr["sr_start"])); seg_off.append(len(arr["seg_pool_off"]))
        ver_off.append(len(arr["version"]))
    arr.update(ver_off=ver_off, sr_off=sr_off, seg_off=seg_off)
    dt = {"last_seq": np.int64, "on_device": np.uint8, "seg_seq0": np.uint32, "seg_n": np.uint32}

    def up(k):
        a = np.asarray(arr[k], dt.get(k, np.uint64))
        return torch.from_numpy(a.view({8: np.int64, 4: np.int32, 1: np.uint8}[a.itemsize]).copy()).cuda()
    didx = {k: up(k) for k in arr}
    got = eng.buffered_spans(st.a.bookie, dec, ext, sp, tl, didx)
    off, spans = B.span_model(_needs_of(dec, ext, sp, tl), book)
    assert got["need_bspan_off"].cpu().numpy().tolist() == off and got["nspans"] == len(spans)
    g = {k: got[k].cpu().numpy() for k in ("site", "version", "last_seq", "ts", "seq_start", "seq_end", "row_off", "row_count")}
    rows = {k: got["rows"][k].cpu().numpy() for k in ROW_KEYS}
    ro = 0
    for i, (site, v, last, ts, s, e, src) in enumerate(spans):
        assert (int(g["site"][i]), int(g["version"][i]), int(g["last_seq"][i]), int(g["ts"][i])) == (site, v, last, ts), i
        assert (int(g["seq_start"][i]), int(g["seq_end"][i])) == (s, e), i
        assert (int(g["row_off"][i]), int(g["row_count"][i])) == (ro, len(src)), i
        for j, p in enumerate(src):
            for key in ROW_KEYS:                               # (the bits: the tensors are signed views)
                mask = (1 << (8 * np.dtype(ROW_FIELDS[key]).itemsize)) - 1
                assert int(rows[key][ro + j]) & mask == pool[p][key] & mask, (i, j, key)
        ro += len(src)
    assert got["nrows"] == ro
    assert any(not src for *_x, src in spans)                  # a span with no row
    assert any(v == 5 and (s, e) == (0, 5) and len(src) == 4 for _s, v, _l, _t, s, e, src in spans)   # the hole


def test_buffered_spans_refuses_a_bad_index_and_writes_nothing(st):
    """A segment past the pool's top, offsets that are not monotone, versions that do not ascend:
    CORRO_E_INVALID, and the outputs keep their sentinels."""
    import torch
    eng = st.a.engine
    dec, ext, sp, idx, tl = _stages(st.a, st.buf, st.off)

    def broken(key, fn):
        d = dict(idx["dev"])
        a = d[key].clone()
        fn(a)
        d[key] = a
        return d
    cases = {"segment past the top": broken("seg_pool_off", lambda a: a.__setitem__(0, 1 << 40)),
             "segment length past the top": broken("seg_n", lambda a: a.__setitem__(1, 0x7FFFFFFF)),
             "ver_off not monotone": broken("ver_off", lambda a: a.__setitem__(1, 99)),
             "seg_off not monotone": broken("seg_off", lambda a: a.__setitem__(1, 50)),
             "sr_off not monotone": broken("sr_off", lambda a: a.__setitem__(2, 0)),
             "versions unsorted": broken("version", lambda a: a.__setitem__(1, int(a[0]))),
             "segments overlap": broken("seg_seq0", lambda a: a.__setitem__(1, 1))}
    for name, d in cases.items():
        with pytest.raises(L.CorroError) as e:
            eng.buffered_spans(st.a.bookie, dec, ext, sp, tl, d)
        assert e.value.code == -1, name
    # the second pass of a good first pass, handed a broken index: nothing is written
    T = int(dec["nneeds"])
    sent = torch.full((T + 1,), 7, dtype=torch.int64, device="cuda")
    r = L.BufSpansIn()
    r.nneeds, r.nseqs, r.nents, r.ngroups = T, int(dec["nseqs"]), int(dec["nents"]), int(ext["version"].shape[0])
    for k in ("kind", "start", "end", "sr_off", "sr_n", "s_start", "s_end", "need_keep", "need_site", "need_ent_off"):
        setattr(r, k, dec[k].data_ptr())
    r.in_state, r.need_host = sp["in_state"].data_ptr(), tl["need_host"].data_ptr()
    r.grp_off, r.version = ext["grp_off"].data_ptr(), ext["version"].data_ptr()
    d = cases["segment past the top"]
    r.idx_nsites, r.idx_nver = int(d["ver_off"].shape[0]) - 1, int(d["version"].shape[0])
    r.idx_nsr, r.idx_nseg = int(d["sr_start"].shape[0]), int(d["seg_pool_off"].shape[0])
    for k, dst, _dt in eng._BUFIDX_IN:
        setattr(r, dst, d[k].data_ptr())
    o = L.BufSpansOut()
    o.need_bspan_off = sent.data_ptr()
    torch.cuda.synchronize()
    assert L.lib().corro_buffered_spans(eng._h, st.a.bookie._h, C.byref(r), L.CORRO_MEM_DEVICE, C.byref(o), 0) == -1
    assert b"pool" in L.lib().corro_last_error()
    assert sent.cpu().tolist() == [7] * (T + 1) and o.nspans == 0


def test_assembly_with_every_buffered_piece_empty_is_the_two_piece_assembly(st):
    """corro_assemble_answers_buffered over the twin's stages, whose index holds no pool version any more
    (the host walk read them out): buffer and offsets are corro_assemble_answers' exactly."""
    eng = st.twin.engine
    dec, ext, sp, idx, tl = _stages(st.twin, st.buf, st.off)
    spans = {k: sp[k] for k in ("site", "version", "last_seq", "ts", "seq_start", "seq_end", "row_off", "row_count")}
    enc = eng.encode_changesets(spans, ext["rows"], 8192, 0, 0)
    bsp = eng.buffered_spans(st.twin.bookie, dec, ext, sp, tl, idx["dev"])
    assert bsp["nspans"] == 0 and bsp["nrows"] == 0 and not bsp["need_bspan_off"].cpu().numpy().any()
    two = eng.assemble_answers(dec, sp, enc, tl, 0)
    three = eng.assemble_answers_buffered(dec, sp, enc, bsp, None, tl, 0)
    assert two["nbytes"] == three["nbytes"] > 0
    for k in ("buf", "need_ans_off", "frame_ans_off", "frame_host"):
        assert np.array_equal(two[k].cpu().numpy(), three[k].cpu().numpy()), k


def test_a_need_that_touches_a_host_row_version_takes_the_splice(st):
    """Version 10 holds host rows (a long value): a need over it and pool versions stays need_host and
    gives the host walk's bytes through the splice; the frame's other needs are served from the pool."""
    from corrosion_amd import serve
    a, twin = build(bytes([0xA1]) * 16), build(bytes([0xA1]) * 16)
    buf, off = U.cat([U.request_frame(p) for p in HOST_FRAMES + DEVICE_FRAMES[:1]])
    dec, ext, sp, idx, tl = _stages(a, buf, off)
    assert tl["need_host"].cpu().numpy().tolist()[:4] == [1, 0, 1, 1]
    got = [serve.handle_request_frames_buffered(a, buf.tobytes(), off, **kw) for kw in KW[:1]]
    exp = expected_answers(twin, HOST_FRAMES + DEVICE_FRAMES[:1])
    assert got[0][1] == exp and all(exp)
    idx1, _ = index_of(a)
    assert idx1[0][5][0] == 1 and idx1[0][9][0] == 0           # 5 only met device needs; the host walk read 9 out


def test_round_trip_and_the_later_halves(st):
    """A serves, B applies the answer: B holds the same partial versions. A then receives what it missed of
    version 5; process_fully_buffered_changes on A gives the state of a twin that was never asked."""
    from corrosion_amd import wire
    import corrosion_amd as ca
    a, twin = build(bytes([0xA2]) * 16), build(bytes([0xA2]) * 16)
    buf, off = U.cat([U.request_frame(p) for p in DEVICE_FRAMES[:1]])
    _status, answers = a.handle_request_frames_buffered(buf.tobytes(), off)
    b = ca.agent.Agent(SCHEMA, capacity_hint=1 << 12, actor_id=bytes([0xB0]) * 16, interned=("testsblob",))
    res, dstatus = b.process_frames(b"".join(answers))
    assert not np.asarray(dstatus).any() and "partial" in res.known and "current" in res.known
    for v in (5, 8, 9):
        assert b.bookie.partial(A0, v) == a.bookie.partial(A0, v)
    assert b.bookie.needed(A0) == [(4, 4), (7, 7)]

    def finish(ag):
        res, _ = ag.process_frames(wire.frames([_msg(A0, 0, 5, (2, 3))]))
        assert res.ready == [(A0, 5)]
        assert ag.process_fully_buffered_changes(A0, 5)
        rows = ag.engine.export()
        order = np.lexsort((rows["seq"], rows["db_version"], rows["site"]))
        return {k: rows[k][order].tolist() for k in ROW_KEYS if k != "ts"}, ag.bookie.needed(A0), ag.bookie.partial(A0, 5)
    assert finish(a) == finish(twin)
