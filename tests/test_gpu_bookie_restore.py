"""corro_bookie_save / corro_bookie_load on the device: a bookie that lived through real traffic
(Agent.process_frames, so its canonical partial rows lie in the device row pool) is saved to the host and
to the device, loaded into fresh agents, and must then read, serve and go on exactly like the original;
hand-built images pin the load kernels at their row-order and segment edges; the rejects leave the bookie
empty and the context usable. The books' half is pinned on the CPU (tests/test_abi_bookie_image.py).

The traffic is fixed, not drawn: the coverage the round trip needs (an on-device multi-segment version, a
host-rows version, a ready version, an actor with gaps) is asserted before the save."""
import numpy as np
import pytest

from corrosion_amd import _lib as L
from corrosion_amd import sync as S
from tests import req_decode_util as U
from tests import restore_model as M

pytestmark = pytest.mark.gpu

SCHEMA = {"tests": ["text", "num"], "other": ["a", "b"]}
ACT = [bytes([0x10 * (k + 1)]) * 16 for k in range(8)]
ACT[2], ACT[5] = ACT[5], ACT[2]                                # ordinal order != ActorId order
K = 8                                                          # changes per version: seqs 0..7
ROW_KEYS = ("pk", "table_cid", "col_version", "db_version", "cl", "seq", "site", "ts", "val0", "val1", "val_type", "val_len")


def _changes(a, v, long_at=None):
    from corrosion_amd.agent import Change
    base = 300 + (a * 10 + v) * 40                              # (pks inside 2^8 .. 2^15)
    ch = []
    for s in range(K):
        if s % 3 == 0:
            ch.append(Change("tests", base + s // 2, "text", f"a{a}v{v}s{s}", 1, v, s, ACT[a], 1))
        elif s % 3 == 1:
            ch.append(Change("tests", base + s // 2, "num", a * 100 + v * 7 + s, 1, v, s, ACT[a], 1))
        else:
            ch.append(Change("other", base + s, "b", 0.5 * s + v, 1, v, s, ACT[a], 1))
    if long_at is not None:
        ch[long_at].val = "long value " * 30
    return ch


def full(a, v, seqs=(0, K - 1), long_at=None):
    from corrosion_amd.agent import ChangeV1, Full
    return ChangeV1(ACT[a], Full(v, [c for c in _changes(a, v, long_at) if seqs[0] <= c.seq <= seqs[1]], seqs, K - 1,
                                 ts=5000 + 10 * a + v))


def empty(a, s, e):
    from corrosion_amd.agent import ChangeV1, Empty
    return ChangeV1(ACT[a], Empty((s, e)))


def traffic():
    """Three calls over eight actors: complete versions and Empty ranges that leave gaps; partial versions
    in one (0/9, 7/5), two (1/2; 5/2 adjacent) and three (1/3) disjoint seq pieces; a partial with a long
    TEXT value (2/1: host rows); a version whose two pieces together are complete but not applied (3/2)."""
    return [
        [full(0, 1), full(0, 2), full(0, 4), full(1, 1), full(1, 2, (0, 1)), full(1, 3, (2, 3)), full(3, 1), full(3, 2, (0, 3)),
         empty(4, 1, 5), full(6, 1), full(5, 2, (0, 1))],
        [empty(0, 6, 7), full(0, 9, (0, 2)), full(1, 2, (4, 5)), full(1, 3, (0, 0)), full(2, 1, (0, 3), long_at=1), full(4, 8),
         full(6, 2), full(6, 3), full(5, 2, (2, 3)), full(7, 5, (3, 7))],
        [full(1, 3, (6, 7)), full(3, 2, (4, 7)), full(6, 3)],
    ]


def follow_up():
    """The missing pieces, and re-sends of pieces and whole versions both sides already hold."""
    return [
        [full(1, 2, (2, 3)), full(1, 2, (0, 1)), full(0, 9, (3, 7)), full(0, 2), full(7, 5, (0, 2)), full(2, 1, (4, 7)),
         full(5, 2, (4, 7)), full(0, 3)],
        [full(1, 3, (1, 1)), full(1, 2, (6, 7)), full(3, 2, (4, 7)), empty(4, 6, 7), full(7, 1)],
    ]


def new_agent(tag=0xA0):
    import corrosion_amd as ca
    ag = ca.agent.Agent(SCHEMA, capacity_hint=1 << 12, actor_id=bytes([tag]) * 16)
    for a in ACT:
        ag.site(a)
    return ag


def feed(ag, calls):
    from corrosion_amd import wire
    out = []
    for msgs in calls:
        res, status = ag.process_frames(wire.frames(msgs))
        assert not np.asarray(status).any()
        out.append((res.known, res.impact.cpu().numpy().tolist(), sorted(res.ready)))
    return out


def index_of(agent, offsets=True):
    from tests.test_gpu_serve_buffered import index_of as raw
    idx, _h = raw(agent)
    if not offsets:
        # without the pool offsets, and with touching segments joined: a bookie that received seqs 0..1 and
        # 2..3 in two calls holds two segments, a loaded one the maximal run 0..3 (the seqs held are the same)
        def runs(segs):
            out = []
            for _p, q, n in segs:
                if out and out[-1][0] + out[-1][1] == q:
                    out[-1] = (out[-1][0], out[-1][1] + n)
                else:
                    out.append((q, n))
            return out
        idx = {s: {v: (on, last, ts, sr, runs(segs)) for v, (on, last, ts, sr, segs) in vs.items()} for s, vs in idx.items()}
    return idx


def sorted_state(ag, ts=True):
    rows = ag.engine.export()
    order = np.lexsort((rows["seq"], rows["db_version"], rows["site"], rows["pk"], rows["table_cid"]))
    out = {k: rows[k][order].tolist() for k in ROW_KEYS if ts or k != "ts"}
    # a long value's val1 is a handle into this context's value arena: compared by the bytes it names
    out["val1"] = [rows["long_values"].get(int(i), int(rows["val1"][i])) for i in order]
    return out


def reseed(dst, src):
    """INTEGRATION.md "Startup": the persisted clock rows applied as one batch."""
    rows = src.engine.export()
    if len(rows["pk"]):
        batch = {k: np.ascontiguousarray(rows[k]) for k in ROW_KEYS}
        batch["cl"] = batch["cl"].astype(np.uint32)
        dst.engine.apply(batch)


def buffered_rows(ag):
    """Every buffered version's rows through corro_bookie_buffered (this reads pool keys out to the host)."""
    from corrosion_amd import serve
    out = {}
    for actor in ACT:
        for v in serve._buffered_versions(ag.bookie, actor, 0, 0xFFFFFFFFFFFFFFFF):
            r, m = serve._buffered_rows(ag.bookie, actor, v, 0, 0xFFFFFFFF)
            out[(actor, v)] = ([tuple(int(r[k][j]) for k in ROW_KEYS) for j in range(m)],
                               [serve._buffered_long(ag.bookie, actor, v, r)(j) for j in range(m)],
                               serve._seq_bookkeeping(ag.bookie, actor, v))
    return out


def books(ag):
    return {a: (ag.bookie.last(a), ag.bookie.needed(a), {v: ag.bookie.partial(a, v) for v in range(0, 12)}) for a in ACT}


REQUESTS = [[(ACT[1], [S.Full(1, 4), S.Partial(3, ((0, 7),)), S.Partial(2, ((1, 4), (5, 9)))]), (ACT[5], [S.Full(1, 3)])],
            [(ACT[0], [S.Full(1, 10), S.Partial(9, ((0, 1), (2, 7)))]), (ACT[7], [S.Full(1, 5)]), (ACT[3], [S.Full(2, 2)])],
            [(ACT[2], [S.Full(1, 1)])]]                         # touches the host-rows version


class State:
    pass


@pytest.fixture(scope="module")
def rt():
    s = State()
    s.a = new_agent()
    s.hist = feed(s.a, traffic())
    s.ready_a = sorted(r for _k, _i, rd in s.hist for r in rd)
    s.idx_a = index_of(s.a)
    s.img_host = s.a.save_bookie()
    s.img_dev = s.a.save_bookie(device=True)
    s.idx_a_after = index_of(s.a)
    s.b, s.c = new_agent(0xA0), new_agent(0xA0)
    for ag, img in ((s.b, s.img_dev), (s.c, s.img_host)):
        reseed(ag, s.a)
        ag.load_bookie(img)
    return s


def test_the_traffic_leaves_every_shape_the_round_trip_needs(rt):
    site = {a: k for k, a in enumerate(rt.a.engine.site_ids())}
    i1 = rt.idx_a[site[ACT[1]]]
    assert i1[3][0] == 1 and [(q, n) for _p, q, n in i1[3][4]] == [(0, 1), (2, 2), (6, 2)]      # on-device, three segments
    assert i1[2][0] == 1 and len(i1[2][4]) == 2
    assert rt.idx_a[site[ACT[2]]][1][0] == 0                                                  # host rows (long value)
    assert rt.idx_a[site[ACT[5]]][2][3] == [(0, 3)] and len(rt.idx_a[site[ACT[5]]][2][4]) == 2   # one range, two segments
    assert rt.ready_a == [(ACT[3], 2)]                                                        # complete, not applied
    assert rt.a.bookie.needed(ACT[0]) == [(3, 3), (5, 5), (8, 8)] and rt.a.bookie.needed(ACT[4]) == [(6, 7)]
    assert rt.a.bookie.needed(ACT[7]) == [(1, 4)]
    assert rt.img_host["nrows"] == 3 + 4 + 5 + 4 + 8 + 4 + 5 and rt.img_host["val_data_len"] == 330


def test_host_and_device_images_are_equal_and_save_changes_nothing(rt):
    import torch
    assert all(isinstance(v, torch.Tensor) and v.is_cuda for v in rt.img_dev["rows"].values())
    assert all(isinstance(v, np.ndarray) for v in rt.img_host["rows"].values())
    assert M.image_equal(rt.img_host, rt.img_dev)
    assert rt.idx_a_after == rt.idx_a                           # same keys, same segments, same pool offsets
    r = rt.img_host["rows"]
    key = list(zip(r["site"].tolist(), r["db_version"].tolist(), r["seq"].tolist()))
    assert key == sorted(key) and len(set(key)) == len(key)
    assert [bytes(a) for a in rt.img_host["actor_ids"]] == sorted(ACT)


@pytest.mark.parametrize("which", ["b", "c"])
def test_loaded_bookie_reads_like_the_original(rt, which):
    ag = getattr(rt, which)
    assert books(ag) == books(rt.a)
    sa, sb = rt.a.sync_book(), ag.sync_book()
    assert sorted(sa) == sorted(sb) and all(np.array_equal(sa[k], sb[k]) for k in sa)
    assert ag.generate_sync_frame() == rt.a.generate_sync_frame()
    assert index_of(ag, offsets=False) == index_of(rt.a, offsets=False)
    assert M.image_equal(ag.save_bookie(), rt.img_host)         # and it saves to the same image


def test_loaded_bookie_lists_the_ready_versions(rt):
    assert sorted(rt.b.take_ready()) == sorted(rt.c.take_ready()) == rt.ready_a
    assert rt.b.take_ready() == []


def test_loaded_bookie_serves_and_goes_on_like_the_original(rt):
    """(one test: each step changes the three bookies in the same way)"""
    buf, off = U.cat([U.request_frame(p) for p in REQUESTS])
    ans = [ag.handle_request_frames_buffered(buf.tobytes(), off) for ag in (rt.a, rt.b, rt.c)]
    assert ans[0][0].tolist() == ans[1][0].tolist() == ans[2][0].tolist()
    assert ans[0][1] == ans[1][1] == ans[2][1] and all(ans[0][1])
    rows = [buffered_rows(ag) for ag in (rt.a, rt.b, rt.c)]
    assert rows[0] == rows[1] == rows[2] and len(rows[0]) == 7
    assert any(len(lv) > 16 for _r, longs, _s in rows[0].values() for lv in longs)
    more = [feed(ag, follow_up()) for ag in (rt.a, rt.b, rt.c)]
    assert more[0] == more[1] == more[2]
    ready = sorted(set(rt.ready_a + [r for _k, _i, rd in more[0] for r in rd]))
    assert (ACT[1], 2) in ready and (ACT[2], 1) in ready and (ACT[1], 3) not in ready
    for ag in (rt.a, rt.b, rt.c):
        for actor, v in ready:
            ag.process_fully_buffered_changes(actor, v)
    assert sorted_state(rt.a) == sorted_state(rt.b) == sorted_state(rt.c)
    assert books(rt.a) == books(rt.b) == books(rt.c)
    # and all of it against the CPU restatement replaying the whole history
    from oracle.agent import AgentOracle, Changeset, _batch
    from corrosion_amd.agent import Full, encode_value
    ids = rt.a.engine.site_ids()
    site = {a: k for k, a in enumerate(ids)}
    ref = AgentOracle(np.frombuffer(b"".join(ids), np.uint8).reshape(-1, 16))

    def conv(cv):
        cs = cv.changeset
        if not isinstance(cs, Full):
            return Changeset(cv.actor_id, "empty", versions=tuple(cs.versions))
        rr = []
        for ch in cs.changes:
            t, v0, _v1, _ln = encode_value(ch.val)
            rr.append(dict(pk=ch.pk, table_cid=rt.a.engine.lookup(ch.table, ch.cid), col_version=ch.col_version,
                           db_version=ch.db_version, cl=ch.cl, seq=ch.seq, site=site[ch.site_id], val0=v0, val_type=t))
        return Changeset(cv.actor_id, "full", version=cs.version, seqs=tuple(cs.seqs), last_seq=cs.last_seq, ts=cs.ts, rows=rr)
    known = [ref.process([conv(cv) for cv in call])[0] for call in traffic() + follow_up()]
    assert known == [k for k, _i, _r in rt.hist + more[0]]
    assert sorted(set(ref.ready)) == ready
    for actor, v in ready:                                      # process_fully_buffered_changes
        buf_rows = [r for _q, r in sorted(ref.buffered.pop((actor, v)).items())]
        ref.fold.apply(_batch(buf_rows, [ref.book(actor).partials[v].ts] * len(buf_rows)))
        assert ref.book(actor).gaps.insert_db([(v, v)]) == 0
    canon = lambda rows: sorted(zip(*[np.asarray(rows[k]).tolist() for k in
                                      ("table_cid", "pk", "val_type", "val0", "col_version", "db_version", "site", "cl", "seq")]))
    assert canon(rt.b.engine.export()) == canon(ref.export())
    for a in ACT:
        assert rt.b.bookie.last(a) == ref.last(a) and rt.b.bookie.needed(a) == ref.needed(a)


# ---- hand-built images: row order and segment edges ------------------------------------------------

def _runs(lengths):
    """seqs of runs of the given lengths separated by one-seq holes, and the (seq0, n) segments"""
    seqs, segs, q = [], [], 0
    for n in lengths:
        segs.append((q, n))
        seqs += list(range(q, q + n))
        q += n + 1
    return seqs, segs


def _edge_cases():
    seqs, segs = _runs([1, 63, 64, 65, 255, 256, 257])
    big = 2 ** 63 - 1
    return {
        "wave and workgroup boundaries": ([(0, 5, q) for q in seqs], {(0, 5): segs}),
        "next version continues the seqs": ([(0, 7, q) for q in range(4)] + [(0, 8, q) for q in range(4, 8)],
                                            {(0, 7): [(0, 4)], (0, 8): [(4, 4)]}),
        "next site continues the seqs": ([(0, 7, q) for q in range(4)] + [(1, 7, q) for q in range(4, 8)],
                                         {(0, 7): [(0, 4)], (1, 7): [(4, 4)]}),
        "single row": ([(1, 3, 6)], {(1, 3): [(6, 1)]}),
        "db_version 2^63 - 1": ([(0, big, 0), (0, big, 1), (0, big - 1, 2), (1, big, 3)],
                                {(0, big): [(0, 2)], (0, big - 1): [(2, 1)], (1, big): [(3, 1)]}),
        "seq 2^32 - 1": ([(0, 4, 2 ** 32 - 2), (0, 4, 2 ** 32 - 3), (0, 4, 0), (1, 4, 2 ** 32 - 1), (1, 4, 2 ** 32 - 2), (1, 5, 2 ** 31)],
                         {(0, 4): [(0, 1), (2 ** 32 - 3, 2)], (1, 4): None, (1, 5): [(2 ** 31, 1)]}),   # None: host rows
    }


EDGES = _edge_cases()
ORDERS = ("sorted", "reverse", "shuffle")


def _load_rows(keys, device):
    """A fresh agent with two sites and an image of canonical rows for the keys, rows on the host or the device."""
    import torch
    ag = new_agent()
    rows = M.make_rows(keys)
    if device:
        rows = {k: torch.from_numpy(v.view({8: np.int64, 4: np.int32, 1: np.uint8}[v.itemsize]).copy()).cuda() for k, v in rows.items()}
    versions = sorted({(s, v) for s, v, _q in keys})
    actors = [(ACT[s], None, [(v, min(q for s2, v2, q in keys if (s2, v2) == (s, v)), max(q for s2, v2, q in keys if (s2, v2) == (s, v)),
                               2 ** 32 - 1, 9) for s2, v in versions if s2 == s], []) for s in sorted({s for s, _v in versions})]
    ag.load_bookie(M.make_image(actors, site_ids=ACT, rows=rows))
    return ag


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name", sorted(EDGES))
def test_row_order_and_segment_edges(name, order):
    from corrosion_amd import serve
    keys, want = EDGES[name]
    keys = sorted(keys)
    if order == "reverse":
        keys = keys[::-1]
    elif order == "shuffle":
        keys = [keys[i] for i in np.random.default_rng(11).permutation(len(keys))]
    ag = _load_rows(keys, device=order != "reverse")
    idx = index_of(ag)
    got = {(s, v): ([(q, n) for _p, q, n in segs] if on else None) for s, vs in idx.items() for v, (on, _l, _t, _sr, segs) in vs.items()}
    assert got == want
    offs = sorted((p, n) for vs in idx.values() for _on, _l, _t, _sr, segs in vs.values() for p, _q, n in segs)
    assert all(p0 + n0 == p1 for (p0, n0), (p1, _n) in zip(offs, offs[1:])) and (not offs or offs[0][0] == 0)   # packed, in key order
    exp = M.make_rows(sorted(keys))
    img = ag.save_bookie(device=True)
    for k in exp:                                               # the pool rows, through the device save
        assert np.array_equal(img["rows"][k].cpu().numpy().view(np.uint8), exp[k].view(np.uint8)), k
    for (s, v) in want:                                         # and every version through corro_bookie_buffered
        r, m = serve._buffered_rows(ag.bookie, ACT[s], v, 0, 0xFFFFFFFF)
        sel = [j for j, (s2, v2, _q) in enumerate(sorted(keys)) if (s2, v2) == (s, v)]
        assert m == len(sel)
        for k in ROW_KEYS:
            assert [int(x) for x in r[k][:m]] == [int(exp[k][j]) for j in sel], (s, v, k)


# ---- rejects: the bookie stays empty, the context usable ---------------------------------------------

def _image(keys, site_ids=ACT):
    return M.make_image([(ACT[0], 3, [(4, 0, 1, 5, 9)], [(1, 2)])], site_ids=site_ids, rows=M.make_rows(keys))


def _reject(ag, img, code, word):
    with pytest.raises(L.CorroError) as e:
        ag.load_bookie(img)
    assert e.value.code == code and word in str(e.value), str(e.value)
    assert ag.sync_book()["actor"].shape[0] == 0 and ag.take_ready() == [] and index_of(ag) == {}
    good = [(0, 4, 0), (0, 4, 1), (1, 2, 5)]
    ag.load_bookie(_image(good))                                # a following valid load succeeds
    assert ag.bookie.last(ACT[0]) == 4 and index_of(ag, offsets=False)[0][4][4] == [(0, 2)]
    res, status = ag.process_frames(__import__("corrosion_amd").wire.frames([full(6, 1)]))   # and the context works
    assert res.known == ["current"]


def test_reject_duplicate_key():
    _reject(new_agent(), _image([(0, 4, 0), (1, 2, 5), (0, 4, 1), (1, 2, 5)]), -1, "primary key")


def test_reject_unregistered_site_ordinal():
    import corrosion_amd as ca
    ag = ca.agent.Agent(SCHEMA, capacity_hint=1 << 12)
    ag.site(ACT[0])
    ag.site(ACT[1])
    with pytest.raises(L.CorroError) as e:                      # ordinal 2 is in site_ids but not in the context
        ag.load_bookie(_image([(0, 4, 0), (2, 2, 5)]))
    assert e.value.code == -1 and "not registered" in str(e.value)
    _reject(ag, _image([(0, 4, 0), (9, 2, 5)]), -1, "outside site_ids")


def test_reject_site_ids_mismatch():
    swapped = [ACT[0], ACT[2], ACT[1]] + ACT[3:]
    _reject(new_agent(), _image([(0, 4, 0), (1, 2, 5)], site_ids=swapped), -1, "another id")


def test_reject_injected_pool_reservation_fault(monkeypatch):
    ag = new_agent()
    monkeypatch.setenv("CORRO_FAULT", "bufpool_reserve")
    with pytest.raises(L.CorroError) as e:
        ag.load_bookie(_image([(0, 4, 0), (1, 2, 5)]))
    assert e.value.code == -2 and "bufpool_reserve" in str(e.value)
    monkeypatch.delenv("CORRO_FAULT")
    _reject(ag, _image([(0, 4, 0), (0, 4, 0)]), -1, "primary key")


def test_a_load_without_rows_on_a_gpu_context_skips_the_pool():
    ag = new_agent()
    actors = [(ACT[0], 6, [(6, 0, 3, 3, 1)], [(2, 3)]), (ACT[1], None, [], [])]
    ag.load_bookie(M.make_image(actors, site_ids=ACT))
    books_, ready = M.startup(actors)
    M.check_bookie(ag.bookie, books_)
    assert ag.take_ready() == ready == [(ACT[0], 6)]
    assert index_of(ag) == {}
    img = ag.save_bookie(device=True)
    assert img["nrows"] == 0 and img["rows"]["pk"].numel() == 0
