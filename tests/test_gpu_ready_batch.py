"""corro_process_fully_buffered_batch on the device: a list of ready versions drained as one batch out of
the device row pool (Agent.process_ready) against a twin -- same calls, same site registration -- drained
with corro_process_fully_buffered pair by pair in the same list order. Afterwards the merged state (long
values by their bytes), crsql_db_versions, the committed counts, every actor's Booked versions, the sync
book, the (empty) buffered index and the (empty) ready list are equal, and per pair result == 2 exactly
where the twin reports rows impacted. The traffic is fixed, not drawn; each case asserts the shape it is
there for (pool segments, host-held keys, window sizes) before the drain.

A ready version of one row has two seqs, of which one brought no change: its row arrives as a wire frame
(seqs 0..0, last_seq 1: into the pool), its empty piece (seqs 1..1) through Agent.process_multiple_changes,
since a Full frame on the wire cannot be empty."""
import os

import numpy as np
import pytest

from corrosion_amd import _lib as L

pytestmark = pytest.mark.gpu

SCHEMA = {"tests": ["text", "num"], "other": ["a", "b"]}
ACT = [bytes([0x10 * (k + 1)]) * 16 for k in range(6)]
ACT[1], ACT[4] = ACT[4], ACT[1]                                # ordinal order != ActorId order
ROW_KEYS = ("pk", "table_cid", "col_version", "db_version", "cl", "seq", "site", "ts", "val0", "val1", "val_type", "val_len")
RB_T = 256       # ready_batch.hip: batch rows per workgroup of k_rb_gather
RB_WIN = 257     # ready_batch.hip: pieces its LDS window holds -- RB_T one-row pieces and the one reaching in
VMAX = 130       # snapshot(): partials are read for versions 0 .. VMAX - 1 (the largest version a case creates is 120)


def changes(a, v, k, site=None):
    """version v of actor a: k changes, seq s on its own cell (so every row impacts)"""
    from corrosion_amd.agent import Change
    out = []
    for s in range(k):
        pk = 1000 + (a * 128 + v) * 600 + s // 2
        if s % 2 == 0:
            out.append(Change("tests", pk, "num", a * 1000 + v * 10 + s, 1, v, s, ACT[a] if site is None else site, 1))
        else:
            out.append(Change("other", pk, "b", 0.25 * s + v, 1, v, s, ACT[a] if site is None else site, 1))
    return out


def piece(a, v, k, lo, hi, ch=None, ts=None):
    """seqs lo..hi of the k-change version v of actor a"""
    from corrosion_amd.agent import ChangeV1, Full
    ch = changes(a, v, k) if ch is None else ch
    return ChangeV1(ACT[a], Full(v, ch[lo:hi + 1], (lo, hi), k - 1, ts=7000 + 16 * a + v if ts is None else ts))


def new_agent():
    import corrosion_amd as ca
    ag = ca.agent.Agent(SCHEMA, capacity_hint=1 << 12, actor_id=b"\xA0" * 16)
    for a in ACT:
        ag.site(a)
    return ag


def feed(ag, calls):
    """each call through Agent.process_frames; the ready versions in the order the calls reported them"""
    from corrosion_amd import wire
    ready = []
    for msgs in calls:
        res, status = ag.process_frames(wire.frames(msgs))
        assert not np.asarray(status).any()
        ready += res.ready
    return ready


def index_of(ag):
    from tests.test_gpu_serve_buffered import index_of as raw
    return raw(ag)[0]


def snapshot(ag):
    rows = ag.engine.export()
    order = np.lexsort((rows["seq"], rows["db_version"], rows["site"], rows["pk"], rows["table_cid"]))
    state = {k: rows[k][order].tolist() for k in ROW_KEYS}
    # a long value's val1 is a handle into this context's value arena: compared by the bytes it names
    state["val1"] = [rows["long_values"].get(int(i), int(rows["val1"][i])) for i in order]
    book = ag.sync_book()
    return {"state": state, "db_versions": ag.engine.db_versions().tolist(),
            "committed": {t: ag.engine.committed(t) for t in SCHEMA},
            "books": {a: (ag.bookie.last(a), ag.bookie.needed(a), {v: ag.bookie.partial(a, v) for v in range(0, VMAX)}) for a in ACT},
            "sync_book": {k: np.asarray(book[k]).tolist() for k in sorted(book)}, "index": index_of(ag)}


def drain_both(x, y, pairs):
    """x: the batch; y: the twin, pair by pair. Returns x's results after the comparison."""
    got = x.process_ready(pairs)
    want = [y.process_fully_buffered_changes(a, v) for a, v in pairs]
    assert [(a, v) for a, v, _r in got] == list(pairs)
    assert all(r in (0, 1, 2) for _a, _v, r in got)
    assert [r == 2 for _a, _v, r in got] == want
    sx, sy = snapshot(x), snapshot(y)
    assert sx == sy
    assert sx["index"] == {} and x.take_ready() == [] and y.take_ready() == []
    return [r for _a, _v, r in got]


def one_row(a, v):
    """the two pieces of a one-row version: its row (a wire frame) and its empty second seq (host headers)"""
    from corrosion_amd.agent import ChangeV1, Full
    ts = 7000 + 16 * a + v
    return ChangeV1(ACT[a], Full(v, changes(a, v, 1), (0, 0), 1, ts=ts)), ChangeV1(ACT[a], Full(v, [], (1, 1), 1, ts=ts))


def twins(calls, empties=()):
    """empties: the empty pieces of one-row versions, one process_multiple_changes call behind the frames"""
    x, y = new_agent(), new_agent()
    rx, ry = feed(x, calls), feed(y, calls)
    if empties:
        ex, ey = x.process_multiple_changes(list(empties)), y.process_multiple_changes(list(empties))
        assert ex.known == ey.known == ["partial"] * len(empties)
        rx, ry = rx + ex.ready, ry + ey.ready
    assert rx == ry
    return x, y, rx


def segs_of(ag, a, v):
    site = {s: k for k, s in enumerate(ag.engine.site_ids())}[ACT[a]]
    on_dev, _last, _ts, _sr, segs = index_of(ag)[site][v]
    return on_dev, [(q, n) for _p, q, n in segs]


# ---- segment order ------------------------------------------------------------------------------------

def segment_calls():
    """0/1 received as seqs 2..3 then 0..1 (two calls), 0/2 in three pieces out of order, 2/1 whole in two
    adjacent pieces of one call, 1/1 complete on arrival (state the ready versions then merge over)"""
    return [[piece(0, 1, 4, 2, 3), piece(0, 2, 7, 5, 6), piece(1, 1, 3, 0, 2), piece(2, 1, 6, 0, 2), piece(2, 1, 6, 3, 5)],
            [piece(0, 1, 4, 0, 1), piece(0, 2, 7, 0, 1)],
            [piece(0, 2, 7, 2, 4)]]


def test_segments_are_applied_in_seq_order_whatever_order_they_arrived_in():
    x, y, ready = twins(segment_calls())
    assert ready == [(ACT[2], 1), (ACT[0], 1), (ACT[0], 2)]
    assert segs_of(x, 0, 1) == (1, [(0, 2), (2, 2)])            # pool segments, sorted by seq0: arrival was 2..3, 0..1
    assert segs_of(x, 0, 2) == (1, [(0, 2), (2, 3), (5, 2)])
    assert drain_both(x, y, ready) == [2, 2, 2]
    # and the merged state against the CPU restatement's sequential fold of the same rows in list order
    from oracle.agent import AgentOracle, Changeset, _batch
    from corrosion_amd.agent import encode_value
    ids = x.engine.site_ids()
    site = {a: k for k, a in enumerate(ids)}
    ref = AgentOracle(np.frombuffer(b"".join(ids), np.uint8).reshape(-1, 16))

    def conv(cv):
        cs, rr = cv.changeset, []
        for ch in cs.changes:
            t, v0, _v1, _ln = encode_value(ch.val)
            rr.append(dict(pk=ch.pk, table_cid=x.engine.lookup(ch.table, ch.cid), col_version=ch.col_version,
                           db_version=ch.db_version, cl=ch.cl, seq=ch.seq, site=site[ch.site_id], val0=v0, val_type=t))
        return Changeset(cv.actor_id, "full", version=cs.version, seqs=tuple(cs.seqs), last_seq=cs.last_seq, ts=cs.ts, rows=rr)
    for call in segment_calls():
        ref.process([conv(cv) for cv in call])
    assert sorted(ref.ready) == sorted(ready)
    for actor, v in ready:
        buf_rows = [r for _q, r in sorted(ref.buffered.pop((actor, v)).items())]
        ref.fold.apply(_batch(buf_rows, [ref.book(actor).partials[v].ts] * len(buf_rows)))
        assert ref.book(actor).gaps.insert_db([(v, v)]) == 0
    canon = lambda rows: sorted(zip(*[np.asarray(rows[k]).tolist() for k in      # noqa: E731
                                      ("table_cid", "pk", "val_type", "val0", "col_version", "db_version", "site", "cl", "seq")]))
    assert canon(x.engine.export()) == canon(ref.export())
    for a in ACT:
        assert x.bookie.last(a) == ref.last(a) and x.bookie.needed(a) == ref.needed(a)


def test_maximal_run_segments_of_a_loaded_bookie():
    """the same after save_bookie / load_bookie: the loaded pool holds one maximal run per version, and
    process_ready() without arguments takes the list the load found"""
    from tests.test_gpu_bookie_restore import reseed
    src, y, ready = twins(segment_calls())
    x = new_agent()
    reseed(x, src)
    x.load_bookie(src.save_bookie(device=True))
    assert segs_of(x, 0, 2) == (1, [(0, 7)]) and segs_of(src, 0, 2)[1] == [(0, 2), (2, 3), (5, 2)]
    got = x.process_ready()
    listed = [(a, v) for a, v, _r in got]
    assert sorted(listed) == sorted(ready) and [r for _a, _v, r in got] == [2, 2, 2]
    assert [y.process_fully_buffered_changes(a, v) for a, v in listed] == [True] * 3
    sx, sy = snapshot(x), snapshot(y)
    sx.pop("committed"), sy.pop("committed")                    # (the reseeded context did not count the buffered changes)
    assert sx == sy and sx["index"] == {} and x.take_ready() == []


# ---- workgroup and search-window edges ------------------------------------------------------------------

def two_piece_calls(sizes, cut):
    """version j // 5 + 1 of actor j % 5 with sizes[j] rows, in two pieces cut at cut(j, k), second halves in
    a second call in reverse order; a one-row version as one_row() gives it. Returns (calls, empties)."""
    first, second, empties = [], [], []
    for j, k in enumerate(sizes):
        a, v = j % 5, j // 5 + 1
        if k == 1:
            row, hole = one_row(a, v)
            first.append(row)
            empties.append(hole)
            continue
        c = cut(j, k)
        first.append(piece(a, v, k, 0, c - 1))
        second.append(piece(a, v, k, c, k - 1))
    return [first, second[::-1]], empties


def in_creation_order(ready):
    return sorted(ready, key=lambda p: (p[1], ACT.index(p[0])))


def test_versions_of_1_255_256_257_rows_and_one_row_pieces():
    sizes = [1, 255, 256, 257, 2, 1, 3]
    x, y, ready = twins(*two_piece_calls(sizes, lambda j, k: 1 if k < 10 else k // 3))
    assert len(ready) == len(sizes)
    assert segs_of(x, 0, 1) == (1, [(0, 1)]) and segs_of(x, 0, 2) == (1, [(0, 1)])      # one row, in the pool
    assert segs_of(x, 4, 1) == (1, [(0, 1), (1, 1)]) and segs_of(x, 3, 1) == (1, [(0, 85), (85, 172)])
    pairs = in_creation_order(ready)                            # 1, 255, 256, 257, 2, 1, 3 rows: edges at 1, 256, 512, 769, 771, 772
    assert drain_both(x, y, pairs) == [2] * len(sizes)


def test_300_short_versions_whose_piece_windows_span_workgroups():
    """1 to 5 rows a version in pieces of 1 to 4 rows: ~900 rows, ~540 pieces, every workgroup's window
    begins inside a version; the one-row versions stand between the others in the list"""
    sizes = [1 + (j * 7) % 5 for j in range(300)]
    x, y, ready = twins(*two_piece_calls(sizes, lambda j, k: 1 + j % (k - 1)))
    assert len(ready) == 300 and sizes.count(1) == 60 and sum(sizes) > 3 * RB_T
    assert drain_both(x, y, in_creation_order(ready)) == [2] * 300


def test_one_row_pieces_fill_the_lds_window():
    """600 versions of two one-row pieces: every 256-row workgroup sees 256 pieces start inside its rows and
    one reach in (RB_WIN = 257 entries), the densest window there is -- no list needs more, since the host
    emits no empty piece"""
    n = 600
    assert 2 * n > 4 * RB_T and RB_WIN == RB_T + 1
    first = [piece(j % 5, j // 5 + 1, 2, 1, 1) for j in range(n)]
    second = [piece(j % 5, j // 5 + 1, 2, 0, 0) for j in range(n)]
    x, y, ready = twins([first, second])
    assert len(ready) == n
    assert drain_both(x, y, ready[1:] + ready[:1]) == [2] * n   # (an odd first row: windows start mid-version)


# ---- list order is application order -------------------------------------------------------------------

@pytest.mark.parametrize("lesser_first", [False, True])
def test_list_order_is_application_order(lesser_first):
    """0/1 and 1/1 write one cell with the same col_version, 1/1 the lesser value: listed second it loses
    (result 1), listed first it is merged and then overwritten (result 2). 2/1 and 2/2 write another cell,
    2/2 with the higher col_version, and are listed (v2, v1): v1 loses. Every result as the twin reports."""
    from corrosion_amd.agent import Change

    def cell(a, v, pk, val, cv):                               # (both seqs on the one cell: a version is two seqs at least)
        return [Change("tests", pk, "num", val, cv, v, s, ACT[a], 1) for s in range(2)]
    vs = {(0, 1): cell(0, 1, 77, 50, 1), (1, 1): cell(1, 1, 77, 40, 1), (2, 1): cell(2, 1, 78, 5, 1), (2, 2): cell(2, 2, 78, 6, 2)}
    calls = [[piece(a, v, 2, 0, 0, ch) for (a, v), ch in vs.items()], [piece(a, v, 2, 1, 1, ch) for (a, v), ch in vs.items()]]
    x, y, ready = twins(calls)
    assert sorted(ready) == sorted((ACT[a], v) for a, v in vs)
    ab = [(ACT[1], 1), (ACT[0], 1)] if lesser_first else [(ACT[0], 1), (ACT[1], 1)]
    assert drain_both(x, y, ab + [(ACT[2], 2), (ACT[2], 1)]) == ([2, 2] if lesser_first else [2, 1]) + [2, 1]


# ---- host-held keys next to pool keys ------------------------------------------------------------------

def test_host_held_keys_in_the_same_list_as_pool_keys():
    """3/1 holds a TEXT longer than 16 bytes, 4/1 a change whose site is not the actor's (non-canonical):
    both keys live on the host and enter the batch between pool keys; the long values compare by bytes"""
    long_ch = changes(3, 1, 5)
    long_ch[1].table, long_ch[1].cid, long_ch[1].val = "tests", "text", "a long TEXT value " * 9
    long_ch[3].table, long_ch[3].cid, long_ch[3].val = "tests", "text", "short"
    foreign = changes(4, 1, 4)
    foreign[2].site_id = ACT[5]
    calls = [[piece(0, 1, 6, 0, 2), piece(3, 1, 5, 0, 1, long_ch), piece(4, 1, 4, 2, 3, foreign), piece(1, 1, 4, 0, 1), piece(2, 1, 300, 0, 99)],
             [piece(3, 1, 5, 2, 4, long_ch), piece(0, 1, 6, 3, 5), piece(4, 1, 4, 0, 1, foreign), piece(1, 1, 4, 2, 3), piece(2, 1, 300, 100, 299)]]
    x, y, ready = twins(calls)
    assert len(ready) == 5
    assert segs_of(x, 3, 1)[0] == 0 and segs_of(x, 4, 1)[0] == 0 and segs_of(x, 0, 1)[0] == 1 and segs_of(x, 2, 1)[0] == 1
    pairs = [(ACT[0], 1), (ACT[3], 1), (ACT[2], 1), (ACT[4], 1), (ACT[1], 1)]
    assert drain_both(x, y, pairs) == [2] * 5
    longs = [v for v in snapshot(x)["state"]["val1"] if isinstance(v, (bytes, bytearray))]
    assert longs == [("a long TEXT value " * 9).encode()]


# ---- pairs that are not applicable, mixed in -----------------------------------------------------------

def test_pairs_that_are_not_applicable_get_0_and_keep_their_entries():
    calls = [[piece(0, 1, 4, 0, 1), piece(0, 2, 4, 0, 1), piece(1, 1, 3, 0, 2), piece(2, 1, 4, 2, 3)],
             [piece(0, 1, 4, 2, 3), piece(2, 1, 4, 0, 1)]]
    x, y, ready = twins(calls)
    assert ready == [(ACT[0], 1), (ACT[2], 1)]
    unknown = b"\xEE" * 16
    pairs = [(unknown, 1), (ACT[0], 2), (ACT[0], 1), (ACT[1], 1), (ACT[5], 3), (ACT[0], 1), (ACT[2], 1), (ACT[0], 2)]
    before = snapshot(x)
    got = x.process_ready(pairs)
    assert [r for _a, _v, r in got] == [0, 0, 2, 0, 0, 0, 2, 0]   # unknown actor, seq gap, not partial, unheld actor, listed twice
    want = [y.process_fully_buffered_changes(a, v) for a, v in pairs]
    assert want == [r == 2 for _a, _v, r in got]
    sx, sy = snapshot(x), snapshot(y)
    assert sx == sy
    site0 = {s: k for k, s in enumerate(x.engine.site_ids())}[ACT[0]]
    assert sx["index"] == {site0: {2: before["index"][site0][2]}}   # 0/2 as it was, pool offsets included
    assert sx["books"][ACT[0]][2][2] == before["books"][ACT[0]][2][2] == ([(0, 1)], 3)
    assert x.take_ready() == []


def test_a_version_with_a_complete_seq_book_and_no_row():
    """two empty partial pieces (host headers: the wire form carries no empty Full): the twin decides"""
    from corrosion_amd.agent import ChangeV1, Full
    x, y = new_agent(), new_agent()
    for ag in (x, y):
        r1 = ag.process_multiple_changes([ChangeV1(ACT[0], Full(1, [], (0, 1), 3, ts=5))])
        r2 = ag.process_multiple_changes([ChangeV1(ACT[0], Full(1, [], (2, 3), 3, ts=5))])
        assert feed(ag, [[piece(1, 1, 4, 0, 1)], [piece(1, 1, 4, 2, 3)]]) == [(ACT[1], 1)]
    assert r1.known == ["partial"] and r2.known == ["partial"] and r2.ready == [(ACT[0], 1)]
    assert drain_both(x, y, [(ACT[0], 1), (ACT[1], 1)]) == [1, 2]


# ---- atomicity -------------------------------------------------------------------------------------------

def test_a_failure_before_the_apply_leaves_everything_as_it_was():
    """CORRO_FAULT=ready_gather: a host-side early return after the walk and the gather, before the apply.
    On a loaded bookie, so that the ready list is there to be left alone."""
    from tests.test_gpu_bookie_restore import reseed
    src, y, ready = twins(segment_calls())
    x = new_agent()
    reseed(x, src)
    x.load_bookie(src.save_bookie())
    before = snapshot(x)
    os.environ["CORRO_FAULT"] = "ready_gather"
    try:
        with pytest.raises(L.CorroError) as e:
            x.process_ready(ready)
    finally:
        del os.environ["CORRO_FAULT"]
    assert e.value.code == -3 and "ready_gather" in str(e.value)
    assert snapshot(x) == before
    assert sorted(x.take_ready()) == sorted(ready)              # the ready list was neither read nor drained
    assert [r for _a, _v, r in x.process_ready(ready)] == [2, 2, 2]
    assert [y.process_fully_buffered_changes(a, v) for a, v in ready] == [True] * 3
    sx, sy = snapshot(x), snapshot(y)
    sx.pop("committed"), sy.pop("committed")
    assert sx == sy and sx["index"] == {}


# ---- the chain -------------------------------------------------------------------------------------------

def test_process_frames_then_process_ready_then_match_extracted():
    """a mixed call (complete versions, partial halves) through Agent.process_frames, the ready versions
    through Agent.process_ready, and updates.match_extracted over the versions with result 2: the twin's
    matches. (process_frames hands the ready list to its caller, so process_ready gets it as `pairs`;
    the no-argument form is checked on a loaded bookie above.)"""
    import torch
    from corrosion_amd import updates as U
    calls = [[piece(0, 1, 6, 0, 5), piece(1, 1, 4, 0, 1), piece(2, 1, 5, 3, 4), piece(0, 2, 4, 0, 1), piece(3, 1, 2, 0, 1)],
             [piece(2, 1, 5, 0, 2), piece(0, 2, 4, 2, 3), piece(1, 1, 4, 2, 3), piece(0, 1, 6, 0, 5)]]
    x, y, ready = twins(calls)
    assert len(ready) == 3
    got = x.process_ready(ready)
    want = [y.process_fully_buffered_changes(a, v) for a, v in ready]
    assert [r for _a, _v, r in got] == [2, 2, 2] and want == [True] * 3
    assert x.process_ready() == []
    dev = lambda v, dt: torch.tensor(v, dtype=dt, device="cuda")     # noqa: E731
    def matches(ag):
        filters = U.MatchFilters(ag.engine, subs=[{"tests": ["num"]}, {"other": ["b"]}], updates=["tests", "other"])
        out = []
        for a, v, r in got:
            if r != 2:
                continue
            ext = ag.engine.extract_changes({"site": dev([ag.site(a)], torch.int32), "start": dev([v], torch.int64),
                                             "end": dev([v], torch.int64)})
            res = U.match_extracted(ag.engine, ext["rows"], filters)
            out.append([[(s, [(t, list(pks.items())) for t, pks in cands.items()]) for s, cands in per]
                        for per in U.candidates_by_handle(res, filters)])
        return out
    mx, my = matches(x), matches(y)
    assert mx == my and len(mx) == 3 and all(any(per for per in m) for m in mx)
    assert snapshot(x) == snapshot(y)
