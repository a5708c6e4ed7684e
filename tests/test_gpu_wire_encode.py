"""GPU wire encode (corro_encode_changesets, csrc/wire_encode.hip): rows in HBM -> chunked
Changeset::Full messages -> frames. The expected bytes always come from the host object path --
wire.frames over serve.handle_needs, or over serve.ChunkedChanges / send_change_chunks -- never from
the code under test. Bar: byte-exact."""
import numpy as np
import pytest

from tests._util import load_golden

pytestmark = pytest.mark.gpu

ACT = [bytes([i + 1]) * 16 for i in range(3)]
SCHEMA = {"tests": ["text", "num", "real", "blob"], "testsblob": ["text", "blob"]}
NVER = 14
SPAN_FIELDS = ("site", "version", "last_seq", "ts", "seq_start", "seq_end", "row_off", "row_count")


def _values():
    return [None, 0, -5, 1 << 62, -(1 << 63), 1.5, -2.5e300, "", "a", "x" * 16, "y" * 17, "z" * 300,
            b"", b"\x01", bytes(range(16)), bytes(range(17)), bytes(range(256)) + b"\xfe" * 44]


def _messages():
    """3 actors x 14 versions x 5 changes: every value kind and length class, integer pks 0 / negative /
    1..8 bytes, BLOB and composite pks (interned), the "-1" sentinel."""
    from corrosion_amd.agent import Change, ChangeV1, Full
    from tests.test_gpu_pk import _pack
    vals = _values()
    int_pks = [0, -3, 7, 255, 256, 1 << 20, 1 << 40, (1 << 63) - 1]
    blob_pks = [_pack([b""]), _pack([b"k"]), _pack([bytes(range(40))]), _pack([5, "abc"]), _pack([b"\x00" * 7 + b"\x05", "5"])]
    msgs, n = [], 0
    for a, actor in enumerate(ACT):
        for v in range(1, NVER + 1):
            ch = []
            for k in range(5):
                # every pk is used once, so no change loses its merge
                if n % 2 == 0:
                    t, pk = "tests", (int_pks[n // 2] if n // 2 < len(int_pks) else 1000 + n)
                else:
                    t, pk = "testsblob", (blob_pks[n // 2] if n // 2 < len(blob_pks) else _pack([n.to_bytes(3, "big")]))
                cols = SCHEMA[t]
                if n % 11 == 3:
                    cid, val = "-1", None
                else:
                    cid, val = cols[(n // 2 + a) % len(cols)], vals[n % len(vals)]
                ch.append(Change(t, pk, cid, val, 1, v, k, actor, 1))
                n += 1
            msgs.append(ChangeV1(actor, Full(v, ch, (0, 4), 4, ts=1000 + v)))
    # one long value overwritten by another (a dead span in the arena, for the compaction case)
    first = next(c for m in msgs if m.actor_id == ACT[0] for c in m.changeset.changes
                 if isinstance(c.val, str) and len(c.val) > 16)
    over = Change(first.table, first.pk, first.cid, "w" * 200, 2, NVER + 1, 0, ACT[0], 1)
    msgs.append(ChangeV1(ACT[0], Full(NVER + 1, [over], (0, 0), 0, ts=2000)))
    return msgs


class State:
    pass


@pytest.fixture(scope="module")
def st():
    import corrosion_amd as ca
    from corrosion_amd.agent import Full
    from corrosion_amd.sync import Full as NFull
    s = State()
    s.agent = ca.agent.Agent(SCHEMA, capacity_hint=1 << 12, interned=("testsblob",))
    for a in ACT:
        s.agent.site(a)
    res = s.agent.process_multiple_changes(_messages())
    assert all(k == "current" for k in res.known), res.known
    s.needs = [(ACT[0], 1, NVER + 1), (ACT[1], 1, NVER), (ACT[2], 1, NVER)]
    s.exp = [m for out in s.agent.handle_needs([(a, NFull(lo, hi)) for a, lo, hi in s.needs]) for m in out]
    assert all(isinstance(m.changeset, Full) for m in s.exp)
    return s


def full_spans(agent, needs):
    """Host extraction of Full needs -> (spans, rows) as numpy arrays: one span per version found."""
    nd = {"site": np.array([agent.site(a) for a, _, _ in needs], np.uint32),
          "start": np.array([lo for _, lo, _ in needs], np.uint64), "end": np.array([hi for _, _, hi in needs], np.uint64)}
    res = agent.engine.extract_changes(nd)
    per = np.diff(res["grp_off"].astype(np.int64))
    spans = {"site": np.repeat(nd["site"], per), "version": res["version"], "last_seq": res["last_seq"], "ts": res["ts"],
             "seq_start": np.zeros(len(res["version"]), np.uint64), "seq_end": res["last_seq"].copy(),
             "row_off": res["grp_row_off"], "row_count": res["grp_rows"]}
    return spans, res["rows"]


def to_dev(d):
    import torch
    return {k: torch.from_numpy(np.ascontiguousarray(v).view({8: np.int64, 4: np.int32, 1: np.uint8}[v.dtype.itemsize])).cuda()
            for k, v in d.items()}


def host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def enc_bytes(enc):
    return host(enc["buf"]).tobytes()


def uni_frames(msgs, cluster_id):
    from corrosion_amd import wire
    return b"".join(wire.frame(wire.encode_uni_change(m, cluster_id)) for m in msgs)


# ---- 1. byte-exact, mixed values ----------------------------------------------------------------

def test_state_covers_the_value_and_pk_classes(st):
    ch = [c for m in st.exp for c in m.changeset.changes]
    assert len(ch) >= 200
    assert any(c.cid == "-1" for c in ch) and any(c.val is None for c in ch)
    assert any(isinstance(c.val, int) and c.val < 0 for c in ch) and any(isinstance(c.val, float) for c in ch)
    for typ in (str, bytes):
        assert {0, 1, 16, 17, 300} <= {len(c.val) for c in ch if isinstance(c.val, typ)}
    pks = [c.pk for c in ch if c.table == "tests"]
    assert 0 in pks and any(p >= 1 << 63 for p in pks)          # pk 0 and a negative pk (as its u64 key)
    assert any(isinstance(c.pk, bytes) for c in ch)
    assert len({c.site_id for c in ch}) == 3


@pytest.mark.parametrize("payload,cluster", [(0, 0), (1, 0x1234)])
def test_encode_bytes_equal_the_object_path(st, payload, cluster):
    from corrosion_amd import wire
    eng = st.agent.engine
    spans, rows = full_spans(st.agent, st.needs)
    exp = wire.frames(st.exp, wire.PAYLOAD_SYNC) if payload == 0 else uni_frames(st.exp, cluster)
    dev = eng.encode_changesets(to_dev(spans), to_dev(rows), 8192, payload, cluster)
    assert dev["buf"].is_cuda and dev["frame_off"].is_cuda
    assert dev["nframes"] == len(st.exp) and enc_bytes(dev) == exp
    hst = eng.encode_changesets(spans, rows, 8192, payload, cluster)
    assert enc_bytes(hst) == exp
    for k in ("frame_off", "span_frame_off", "frame_seq_start", "frame_seq_end", "frame_row_off", "frame_rows"):
        assert (host(dev[k]).astype(np.int64) == host(hst[k]).astype(np.int64)).all(), k
    fo = host(hst["frame_off"])
    assert int(fo[0]) == 0 and int(fo[-1]) == len(exp)


# ---- 2. chunker KATs on the device --------------------------------------------------------------

KATS = load_golden("chunker_kats.json")["cases"]


def uniform_span(eng, seqs, start, last, last_seq):
    """One span of INTEGER rows of table 0 with the given seqs: every row has the same estimated size."""
    n = len(seqs)
    rows = {"pk": np.full(n, 7, np.uint64), "table_cid": np.full(n, eng.lookup("tests", "num"), np.uint32),
            "col_version": np.ones(n, np.int64), "db_version": np.ones(n, np.int64), "cl": np.ones(n, np.int64),
            "seq": np.array(seqs, np.uint32), "site": np.zeros(n, np.uint32), "val0": np.arange(n, dtype=np.uint64),
            "val1": np.zeros(n, np.uint64), "val_type": np.ones(n, np.uint8), "val_len": np.zeros(n, np.uint8)}
    spans = {"site": np.zeros(1, np.uint32), "version": np.ones(1, np.int64), "last_seq": np.array([last_seq], np.uint64),
             "ts": np.array([9], np.uint64), "seq_start": np.array([start], np.uint64),
             "seq_end": np.array([last], np.uint64), "row_off": np.zeros(1, np.uint64),
             "row_count": np.array([n], np.uint64)}
    return spans, rows


def frames_of(enc, seqs):
    ro, rn = host(enc["frame_row_off"]), host(enc["frame_rows"])
    s0, s1 = host(enc["frame_seq_start"]), host(enc["frame_seq_end"])
    return [([int(x) for x in seqs[int(ro[f]):int(ro[f]) + int(rn[f])]], int(s0[f]), int(s1[f]))
            for f in range(enc["nframes"])]


@pytest.mark.parametrize("case", KATS, ids=[c["name"] for c in KATS])
def test_chunker_kats_on_the_device(st, case):
    from corrosion_amd import serve
    from corrosion_amd.agent import Change
    eng = st.agent.engine
    size = serve.estimated_byte_size(Change("tests", 7, "num", 1, 1, 1, 0, ACT[0], 1))
    base = serve.estimated_byte_size(Change("", b"", "", None, 0, 0, 0, b"\0" * 16, 0))
    mx = case["max_bytes"] * size // base if "max_bytes" in case else case["max_changes"] * size
    spans, rows = uniform_span(eng, case["input"], case["start"], case["last"], case["last"] + 1)
    enc = eng.encode_changesets(to_dev(spans), to_dev(rows), mx)
    assert frames_of(enc, case["input"]) == [(c[0], c[1], c[2]) for c in case["chunks"]]
    assert [int(x) for x in host(enc["span_frame_off"])] == [0, len(case["chunks"])]


def test_empty_whole_version_chunk_is_dropped(st):
    eng = st.agent.engine
    spans, rows = uniform_span(eng, [], 0, 5, 5)
    enc = eng.encode_changesets(to_dev(spans), to_dev(rows), 100)
    assert enc["nframes"] == 0 and enc["nbytes"] == 0 and [int(x) for x in host(enc["span_frame_off"])] == [0, 0]
    spans, rows = uniform_span(eng, [], 2, 5, 5)
    enc = eng.encode_changesets(to_dev(spans), to_dev(rows), 100)
    assert frames_of(enc, []) == [([], 2, 5)]
    from corrosion_amd import serve, wire
    out = []
    serve.send_change_chunks(out, serve.ChunkedChanges([], 2, 5, 100), ACT[0], 1, 5, 9)
    assert enc_bytes(enc) == wire.frames(out)


# ---- 3. chunk boundaries ------------------------------------------------------------------------

@pytest.fixture(scope="module")
def big():
    import corrosion_amd as ca
    from corrosion_amd.agent import Change, ChangeV1, Full
    s = State()
    s.agent = ca.agent.Agent(SCHEMA, capacity_hint=1 << 12, interned=("testsblob",))
    s.ch = [Change("tests", 1000 + k, "num", k, 1, 1, k, ACT[0], 1) for k in range(300)]
    s.agent.process_multiple_changes([ChangeV1(ACT[0], Full(1, s.ch, (0, 299), 299, ts=5))])
    return s


def _row_size(big):
    from corrosion_amd import serve
    sizes = {serve.estimated_byte_size(c) for c in big.ch}
    assert len(sizes) == 1
    return sizes.pop()


@pytest.mark.parametrize("which", ["default", "one_row_per_frame", "one_huge_frame", "exact_threshold"])
def test_chunk_boundaries(big, which):
    from corrosion_amd import serve, wire
    from corrosion_amd.agent import ChangeV1, Full
    mx = {"default": 8192, "one_row_per_frame": 1, "one_huge_frame": 1 << 30,
          "exact_threshold": 100 * _row_size(big)}[which]
    exp = [ChangeV1(ACT[0], Full(1, c, s, 299, ts=5)) for c, s in serve.ChunkedChanges(big.ch, 0, 299, mx)]
    assert len(exp) == {"default": len(exp), "one_row_per_frame": 300, "one_huge_frame": 1, "exact_threshold": 3}[which]
    if which == "default":
        assert len(exp) > 2
    if which == "one_huge_frame":
        assert len(wire.frames(exp)) > 16384          # larger than the encoder's LDS tile
    spans, rows = full_spans(big.agent, [(ACT[0], 1, 1)])
    enc = big.agent.engine.encode_changesets(to_dev(spans), to_dev(rows), mx)
    assert enc["nframes"] == len(exp)
    assert enc_bytes(enc) == wire.frames(exp)
    assert frames_of(enc, host(rows["seq"])) == [([c.seq for c in m.changeset.changes], *m.changeset.seqs) for m in exp]


# ---- 4. round trip through the decoder -----------------------------------------------------------

def test_round_trip_through_decode_frames(st):
    eng = st.agent.engine
    spans, rows = full_spans(st.agent, st.needs)
    enc = eng.encode_changesets(to_dev(spans), to_dev(rows), 2048)
    dec = eng.decode_frames(enc_bytes(enc), device=True)
    assert dec["nframes"] == enc["nframes"] and (dec["status"] == 0).all()
    ch = {k: host(v) for k, v in dec["changes"].items()}
    ro, rn = host(enc["frame_row_off"]), host(enc["frame_rows"])
    idx = np.concatenate([np.arange(int(ro[f]), int(ro[f]) + int(rn[f])) for f in range(enc["nframes"])])
    assert len(idx) == len(rows["pk"]) == len(ch["pk"])
    for f in range(enc["nframes"]):
        cs = dec["cs"][f]
        assert (cs.change_count, cs.seq_start, cs.seq_end) == (int(rn[f]), int(host(enc["frame_seq_start"])[f]),
                                                               int(host(enc["frame_seq_end"])[f]))
    for k in ("table_cid", "col_version", "db_version", "cl", "seq", "site", "val_type", "val_len", "val0"):
        assert (ch[k].astype(np.int64) == rows[k][idx].astype(np.int64)).all(), k
    # an INTEGER pk comes back as unpack_columns reads its packed bytes (get_int sign-extends them, so
    # 255 packed in one byte reads as -1: wire.unpack_int_pk states the quirk); an interned key as itself
    from corrosion_amd import wire
    want_pk = [int(p) if (int(tc) >> 16) == 1 else wire.unpack_int_pk(wire.pack_int_pk(int(p))) & 0xFFFFFFFFFFFFFFFF
               for p, tc in zip(rows["pk"][idx], rows["table_cid"][idx])]
    assert [int(p) for p in ch["pk"].view(np.uint64)] == want_pk
    assert any(int(p) != w for p, w in zip(rows["pk"][idx], want_pk))     # (the state holds such a pk: 255)
    long = rows["val_len"][idx] == 255
    assert long.sum() >= 8
    assert (ch["val1"].view(np.uint64)[~long] == rows["val1"][idx][~long]).all()
    data = ch["val_data"].tobytes()
    want = eng.value_bytes(rows["val1"][idx][long])
    got = [data[int(o):int(o) + int(n)] for o, n in zip(ch["val_off"][long], ch["val_size"][long])]
    assert got == want


# ---- 5. handle_needs_frames ----------------------------------------------------------------------

def test_handle_needs_frames_full_partial_empty_buffered_and_gap():
    from tests.test_gpu_agent import TA1, Node, agent
    from corrosion_amd import wire
    from corrosion_amd.agent import ChangeV1, Empty, Full
    from corrosion_amd.sync import Full as NFull, Partial as NPartial
    ta1, b = Node(TA1), agent()
    ta1.insert_rows(1, 12)
    b.process_multiple_changes(ta1.get_rows([((1, 5), None), ((6, 6), (0, 1))]))
    b.process_multiple_changes([ChangeV1(TA1, Empty((7, 7)))])
    needs = [(TA1, NFull(1, 8)), (TA1, NPartial(6, ((0, 1),))), (TA1, NPartial(3, ((1, 2),))),
             (TA1, NPartial(9, ((0, 3),)))]
    exp = b.handle_needs(needs)
    kinds = [[type(m.changeset) for m in out] for out in exp]
    assert kinds[0] == [Full] * 6 + [Empty] and kinds[1] == [Full] and kinds[2] == [Full] and kinds[3] == [Empty]
    got = b.handle_needs_frames(needs)
    assert got == [wire.frames(out) for out in exp]
    assert b.handle_needs_frames(needs, payload=1, cluster_id=77) == [uni_frames(out, 77) for out in exp]
    # a gap: 11 applied with 8..10 unseen
    b.process_multiple_changes(ta1.get_rows([((11, 11), None)]))
    needs = [(TA1, NFull(7, 12))]
    exp = b.handle_needs(needs)
    assert [type(m.changeset) for m in exp[0]] == [Full, Empty, Empty]
    assert b.handle_needs_frames(needs) == [wire.frames(exp[0])]
    # small chunks: the device path cuts the versions where the object path does
    exp = b.handle_needs([(TA1, NFull(1, 5))], max_buf_size=150)
    assert len(exp[0]) > 5
    assert b.handle_needs_frames([(TA1, NFull(1, 5))], max_buf_size=150) == [wire.frames(exp[0])]


# ---- 6. refusals ---------------------------------------------------------------------------------

@pytest.mark.parametrize("what,code", [("table", -1), ("cid", -1), ("site", -1), ("span", -1), ("span_site", -1)])
@pytest.mark.parametrize("device", [False, True])
def test_malformed_input_is_refused_and_the_context_stays_usable(st, what, code, device):
    import corrosion_amd as ca
    from corrosion_amd import wire
    eng = st.agent.engine
    spans, rows = full_spans(st.agent, st.needs)
    bad_s, bad_r = {k: v.copy() for k, v in spans.items()}, {k: v.copy() for k, v in rows.items()}
    if what == "table":
        bad_r["table_cid"][17] = np.uint32(len(SCHEMA) << 16)
    elif what == "cid":
        bad_r["table_cid"][17] = np.uint32((bad_r["table_cid"][17] & 0xFFFF0000) | 9)
    elif what == "site":
        bad_r["site"][5] = np.uint32(eng.site_count())
    elif what == "span":
        bad_s["row_count"][-1] = np.uint64(len(rows["pk"]) + 1)
    else:
        bad_s["site"][0] = np.uint32(1000)
    conv = to_dev if device else (lambda d: d)
    with pytest.raises(ca.CorroError) as e:
        eng.encode_changesets(conv(bad_s), conv(bad_r))
    assert e.value.code == code
    good = eng.encode_changesets(conv(spans), conv(rows))
    assert enc_bytes(good) == wire.frames(st.exp)


def test_bad_value_handle_and_interned_key_are_refused(st):
    import corrosion_amd as ca
    eng = st.agent.engine
    spans, rows = full_spans(st.agent, st.needs)
    arena = eng.metrics()["arena_bytes"]
    for field, pick, value in (("val1", rows["val_len"] == 255, np.uint64((arena << 24) | 17)),
                               ("pk", (rows["table_cid"] >> 16) == 1, np.uint64(1 << 40))):
        bad = {k: v.copy() for k, v in rows.items()}
        bad[field][np.nonzero(pick)[0][0]] = value
        with pytest.raises(ca.CorroError) as e:
            eng.encode_changesets(to_dev(spans), to_dev(bad))
        assert e.value.code == -1, field


# ---- 7. after a value-arena compaction -----------------------------------------------------------

def test_same_bytes_after_values_compact(st):
    from corrosion_amd import wire
    eng = st.agent.engine
    spans, rows = full_spans(st.agent, st.needs)
    before = enc_bytes(eng.encode_changesets(to_dev(spans), to_dev(rows)))
    assert before == wire.frames(st.exp)
    r = eng.compact_values()
    assert r["arena_after"] < r["arena_before"]
    spans2, rows2 = full_spans(st.agent, st.needs)
    long = rows["val_len"] == 255
    assert (rows2["val_len"] == rows["val_len"]).all() and (rows2["val1"][long] != rows["val1"][long]).any()
    assert enc_bytes(eng.encode_changesets(to_dev(spans2), to_dev(rows2))) == before
