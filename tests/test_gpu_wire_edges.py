"""corro_decode_frames (csrc/wire.hip) against the plain host decoder tests/wire_model.py at the
decoder's malformed-input, size-switch and host-loop edges. Every test builds its frames on the
host, decodes them in one call (two where host and device mode are compared; one per payload kind
where both kinds are covered, since a call takes one kind) and compares per frame: the status always;
for a status-0 frame every header and change field, long values through val_off / val_size, site
ordinals through register_sites, interned row keys through pk_bytes. A rejected frame's slots are
unspecified and not read. Known-good frames are interleaved everywhere and must decode unchanged."""
import ctypes
import struct

import numpy as np
import pytest

from corrosion_amd import wire
from corrosion_amd.agent import Change, ChangeV1, Empty, EmptySet
from tests import wire_cases as W
from tests import wire_model as M

pytestmark = pytest.mark.gpu

SYNC, UNI = wire.PAYLOAD_SYNC, wire.PAYLOAD_UNI
FIELDS = ("pk", "table_cid", "col_version", "db_version", "cl", "seq", "site", "val0", "val1", "val_type", "val_len",
          "ts")
CS_KIND = {"full": 0, "empty": 1, "empty_set": 2}


def engine():
    import corrosion_amd as ca
    return ca.MergeEngine(W.SCHEMA, capacity_hint=1 << 12, interned=W.INTERNED)


def frame_buffer(payloads):
    offs, pos = [], 0
    for p in payloads:
        offs.append(pos + 4)
        pos += 4 + len(p)
    return b"".join(wire.frame(p) for p in payloads), offs


def host_arrays(dec):
    """the decoded change arrays as numpy arrays of the C ABI's types (device mode: copied back)"""
    from corrosion_amd.engine import BATCH_FIELDS
    out = {}
    for k, a in dec["changes"].items():
        if type(a).__module__.startswith("torch"):
            a = a.cpu().numpy()
        out[k] = a.view(BATCH_FIELDS[k]) if k in BATCH_FIELDS else a
    return out


def check(eng, payloads, kind, good=(), label="", **mode):
    """decode `payloads` in one call and compare every frame with the model; returns (dec, models)"""
    buf, offs = frame_buffer(payloads)
    models = [M.decode(p, kind, W.SCHEMA, W.INTERNED) for p in payloads]
    dec = eng.decode_frames(buf, kind, **mode)
    assert dec["nframes"] == len(payloads)
    want = np.array([m[0] for m in models], np.int32)
    got = np.asarray(dec["status"])
    print(f"{label}: {len(payloads)} frames, model: {int((want == 0).sum())} accepted, {int((want == -1).sum())} "
          f"malformed, {int((want == -6).sum())} out of range, {int((want == 1).sum())} not changesets")
    diff = np.nonzero(want != got)[0]
    assert diff.size == 0, [(int(f), int(want[f]), int(got[f]), len(payloads[f])) for f in diff[:10]]
    assert all(got[g] == 0 for g in good) and len(good) > 0
    ok = [m for m in models if m[0] == 0]
    ids = sorted({m[1]["actor"] for m in ok} | {c["site"] for m in ok for c in m[2]})
    site = dict(zip(ids, eng.register_sites(np.frombuffer(b"".join(ids), np.uint8).reshape(-1, 16)).tolist()))
    arr = host_arrays(dec)
    cols = [arr[k].tolist() for k in FIELDS]
    ss, se = (np.asarray(a.cpu() if mode.get("device") else a).view(np.uint64).tolist()
              for a in (dec["set_start"], dec["set_end"]))
    keyed = {}
    for f, (st, hdr, chs) in enumerate(models):
        if st:
            continue
        cs = dec["cs"][f]
        assert ctypes.string_at(cs.actor_id, 16) == hdr["actor"] and cs.site == site[hdr["actor"]], f
        assert (cs.kind, cs.ts, cs.seq_start, cs.seq_end, cs.last_seq) == \
               (CS_KIND[hdr["kind"]], hdr["ts"], *hdr["seqs"], hdr["last_seq"]), f
        if hdr["kind"] == "empty_set":
            n = cs.change_count
            assert list(zip(ss[cs.change_off:cs.change_off + n], se[cs.change_off:cs.change_off + n])) == \
                   hdr["versions"] and n == len(hdr["versions"]), f
            continue
        assert (cs.version_start, cs.version_end, cs.change_count) == (*hdr["versions"], len(chs)), f
        for k, m in enumerate(chs):
            q = cs.change_off + k
            g = tuple(c[q] for c in cols)
            pk = m["pk"]
            if isinstance(pk, bytes):       # an interned row key: compared by the bytes it names, below
                keyed.setdefault(m["table_cid"] >> 16, []).append((g[0], pk, f, k))
                pk = g[0]
            assert g == (pk, m["table_cid"], m["col_version"], m["db_version"], m["cl"], m["seq"], site[m["site"]],
                         m["val0"], m["val1"], m["val_type"], m["val_len"], m["ts"]), (f, k)
            if m["long"]:
                at, n = m["long"]
                assert (int(arr["val_off"][q]), int(arr["val_size"][q])) == (offs[f] + at, n), (f, k)
                data = dec["changes"]["val_data"]
                data = data[offs[f] + at:offs[f] + at + n]
                assert bytes(data.cpu().numpy() if mode.get("device") else data) == payloads[f][at:at + n], (f, k)
    for t, lst in keyed.items():
        names = eng.pk_bytes(t, np.array([x[0] for x in lst], np.uint64))
        assert names == [x[1] for x in lst], t
    return dec, models


def cuts(p, positions=None):
    return [p[:n] for n in (range(len(p)) if positions is None else positions)]


# ---- a. truncation sweep, LDS path -----------------------------------------------------------------

@pytest.mark.parametrize("kind", W.KINDS)
def test_truncation_sweep_lds(kind):
    """Every cut of a 6-change Full frame, of an Empty with its ts and of an EmptySet of 3 ranges: a cut
    inside a length prefix makes the lane-0 walk read padding as a length, and must still be
    rejected; a uni cut inside the trailing cluster_id is accepted; the Empty cut right after
    `versions` is accepted with ts 0 and the lone option byte 1 after it is rejected."""
    fullp = W.full(kind, W.ACT[0], 3, W.mixed_changes(), ts=44)
    emptyp = W.message(kind, ChangeV1(W.ACT[1], Empty((4, 9), ts=12345)))
    setp = W.message(kind, ChangeV1(W.ACT[2], EmptySet([(1, 2), (4, 5), (7, 9)], ts=99)))
    assert len(fullp) < 600 and len(W.mixed_changes()) == 6
    items = cuts(fullp) + cuts(emptyp) + cuts(setp)
    payloads, good = W.interleave(items, kind, every=40)
    dec, models = check(engine(), payloads, kind, good, f"truncation sweep, LDS path, payload {kind}")
    st = {len(p): m[0] for p, m in zip(payloads, models) if fullp.startswith(p) and len(p) < len(fullp)}
    tail = 2 if kind == UNI else 0
    assert all(st[n] == (0 if n >= len(fullp) - tail else -1) for n in range(len(fullp)))
    after_versions = (8 if kind == SYNC else 12) + 16 + 4 + 16
    f = len(fullp) + after_versions
    f += f // 40                                            # (the interleaved neighbours before it)
    assert payloads[f] == emptyp[:after_versions] and payloads[f + 1] == emptyp[:after_versions + 1]
    assert (int(dec["status"][f]), dec["cs"][f].ts, dec["cs"][f].version_end) == (0, 0, 9)
    assert dec["status"][f + 1] == -1


# ---- b. truncation and corruption, global path ----------------------------------------------------

def big_frame(extra=0):
    ch = [Change("users", 1, "blob", bytes(range(250)) * 68 + bytes(extra), 1, 3, 0, W.ACT[0], 1)] + \
         W.mixed_changes()[1:]
    return W.full(SYNC, W.ACT[0], 3, ch, ts=55)


def test_truncation_and_corruption_global():
    """A frame above 16384 bytes (walked from global memory by the wave window): cut at each of its
    last 400 bytes (the small changes and the tail) and at 64 places in its 17000-byte BLOB; change
    3's table / pk / cid / value length prefixes set to 2^32 - 16, to the frame length, and to the
    value that ends the change one byte past the frame."""
    p = big_frame()
    tr = {}
    assert M.decode(p, SYNC, W.SCHEMA, W.INTERNED, tr)[0] == 0 and len(p) > 16384 + 400
    c0, c3 = tr["changes"][0], tr["changes"][3]
    assert c3["vlen"] is not None and len(p) - 400 > c0["end"]
    blob = np.linspace(c0["vlen"], c0["end"] - 49, 64).astype(int).tolist()
    items = cuts(p, range(len(p) - 400, len(p))) + cuts(p, blob)
    for at in (c3["table"], c3["pk"], c3["cid"], c3["vlen"]):
        true = struct.unpack_from("<I", p, at)[0]
        for v in (0xFFFFFFF0, len(p), true + len(p) + 1 - c3["end"]):
            b = bytearray(p)
            struct.pack_into("<I", b, at, v)
            items.append(bytes(b))
    payloads, good = W.interleave(items, SYNC, every=60)
    payloads.append(p)
    good.append(len(payloads) - 1)
    check(engine(), payloads, SYNC, good, "truncation and corruption, global path")
    assert all(M.decode(x, SYNC, W.SCHEMA, W.INTERNED)[0] == -1 for x in items)


# ---- c. path switches ------------------------------------------------------------------------------

def counted_frame(n):
    """n one-byte-pk changes, the first carrying a BLOB that puts the frame on the global path"""
    ch = [Change("users", 1, "blob", bytes(range(256)) * 65, 1, 3, 0, W.ACT[0], 1)] + \
         [Change("users" if k % 3 else "t2", k % 100 + 1, "age" if k % 3 else "x", k, k % 7 + 1, 3, k,
                 W.ACT[k % 5], 1 + k % 2) for k in range(1, n)]
    return W.full(SYNC, W.ACT[1], 3, ch, ts=n)


def test_lds_global_switch():
    """frames of exactly 16384 (the last staged in LDS) and 16385 bytes (the first walked in global
    memory), and one byte either side"""
    items = []
    base = W.full(SYNC, W.ACT[0], 3, [Change("users", 1, "blob", b"", 1, 3, 0, W.ACT[0], 1)] + W.mixed_changes()[1:])
    for n in (16383, 16384, 16385, 16386):
        ch = [Change("users", 1, "blob", bytes(k % 251 for k in range(n - len(base))), 1, 3, 0, W.ACT[0], 1)] + \
             W.mixed_changes()[1:]
        items.append(W.full(SYNC, W.ACT[0], 3, ch))
    assert [len(p) for p in items] == [16383, 16384, 16385, 16386]
    items += [p[:-1] for p in items]            # and each cut by one byte: rejected on either path
    payloads, good = W.interleave(items, SYNC, every=2)
    _dec, models = check(engine(), payloads, SYNC, good + [0, 1, 3, 4], "LDS / global switch")
    assert [m[0] for m in models].count(-1) == 4


def test_change_count_switches():
    """global-path frames of 63, 64, 65, 127, 128, 1023, 1024 and 1025 changes: the wave walk stores
    offsets 64 at a time with a partial last group, and past 1024 changes they live in global scratch;
    every change of every frame is compared"""
    counts = (63, 64, 65, 127, 128, 1023, 1024, 1025)
    items = [counted_frame(n) for n in counts]
    assert all(len(p) > 16384 for p in items)
    payloads, good = W.interleave(items, SYNC, every=3)
    _dec, models = check(engine(), payloads, SYNC, good, "change count switches")
    assert [len(m[2]) for p, m in zip(payloads, models) if p in items] == list(counts)


def window_offsets(tr, tail):
    """WaveWin::u32 restated over the walk's reads of a frame (per change the table, pk and cid length
    prefixes, the tag word and a TEXT / BLOB length; then the 8 tail words): each read's offset from
    the window base as u32 sees it, `at - base`, before it reloads the window when that exceeds 63"""
    base = tr["changes"][0]["start"]                 # w.load(chg_start)
    seen = []

    def u32(at):
        nonlocal base
        seen.append(at - base)
        if at - base > 63:
            base = at

    for m in tr["changes"]:
        for at in (m["table"], m["pk"], m["cid"], m["tag"]):
            u32(at)
        if m["vlen"] is not None:
            u32(m["vlen"])
    for i in range(8):
        u32(tail + 4 * i)
    return seen


def test_window_reload_offsets():
    """a global-path frame whose changes put a length prefix at window offsets 60, 61, 62, 63 (the
    last lanes of the window) and 64 (the first offset that reloads it)"""
    ch = [Change("users", 1, "blob", bytes(range(256)) * 65, 1, 3, 0, W.ACT[0], 1)]
    for k, n in enumerate((56, 57, 58, 59, 60, 59, 56)):
        ch.append(Change("n" * n, 5 + k, "age", k, 1, 3, k + 1, W.ACT[0], 1))
    p = W.full(SYNC, W.ACT[0], 3, ch)
    tr = {}
    assert M.decode(p, SYNC, W.SCHEMA, W.INTERNED, tr)[0] == 0 and len(p) > 16384
    seen = window_offsets(tr, tr["changes"][-1]["end"])
    assert {60, 61, 62, 63, 64} <= set(seen), sorted(set(seen))
    payloads, good = W.interleave([p, p[:-1]], SYNC, every=1)
    check(engine(), payloads, SYNC, good + [0], "window reload offsets")


def test_lds_walk_prediction_combinations():
    """the lane-0 walk predicts a change's table / pk / cid lengths from the previous change's: a frame
    whose changes give all 8 hit / miss combinations of the three, starting with an empty table name"""
    tables, pks, cids = {0: "", 2: "t2", 5: "users"}, {3: 5, 4: 300}, {3: "age", 4: "name"}
    seq = [(0, 3, 3)]
    for e in range(8):
        for _rep in range(2):
            lt, lp, lc = seq[-1]
            seq.append((lt if e & 1 else (5 if lt != 5 else 2),
                        lp if e & 2 else 7 - lp, lc if e & 4 else 7 - lc))
    ch = [Change(tables[lt], pks[lp], cids[lc], k, 1, 3, k, W.ACT[0], 1) for k, (lt, lp, lc) in enumerate(seq)]
    p = W.full(SYNC, W.ACT[0], 3, ch)
    tr = {}
    assert M.decode(p, SYNC, W.SCHEMA, W.INTERNED, tr)[0] == 0 and len(p) < 16384
    prev, combos = (0, 0, 0), set()
    for k, m in enumerate(tr["changes"]):
        cur = (m["pk"] - m["table"] - 4, m["cid"] - m["pk"] - 4, m["tag"] - m["cid"] - 4)
        combos.add(tuple(a == b for a, b in zip(cur, prev)))
        prev = cur
    assert len(combos) == 8 and tr["changes"][0]["pk"] - tr["changes"][0]["table"] == 4
    payloads, good = W.interleave([p, p[:-1], p], SYNC, every=1)
    check(engine(), payloads, SYNC, good + [0, 4], "LDS walk prediction combinations")


# ---- d. directed header and value cases ------------------------------------------------------------

@pytest.mark.parametrize("kind", W.KINDS)
def test_directed_cases(kind):
    """tests/wire_cases.directed: message tags, changeset variants, Option bytes, EmptySet and Full
    counts, value tags, NaN / inf / -0.0, each CORRO_E_RANGE screen on its own, malformed interned pks
    alone and next to a CORRO_E_RANGE change, unscreened pks of unknown tables: one frame each, every
    one followed by a good frame"""
    cases = W.directed(kind)
    payloads, good = W.interleave([p for _n, p, _w in cases], kind, every=1)
    dec, models = check(engine(), payloads, kind, good, f"directed cases, payload {kind}")
    for i, (name, _p, want) in enumerate(cases):
        assert dec["status"][2 * i] == want, name
    arr = host_arrays(dec)
    by_name = {name: dec["cs"][2 * i].change_off + 1 for i, (name, _p, w) in enumerate(cases) if w == 0}
    for name, q in by_name.items():
        if name.startswith("NaN"):
            assert (arr["val_type"][q], arr["val0"][q], arr["val_len"][q]) == (M.T_NULL, 0, 0), name
    for name, bits in (("+inf", 0x7FF0 << 48), ("-inf", 0xFFF0 << 48), ("-0.0", 1 << 63)):
        assert (arr["val_type"][by_name[name]], int(arr["val0"][by_name[name]])) == (M.T_REAL, bits), name
    assert arr["pk"][by_name["unknown table, malformed pk"]] == 0


# ---- e. host-loop paths ----------------------------------------------------------------------------

def test_more_unknown_sites_than_one_pass_collects():
    """4200 distinct unregistered site ids in one call (the collection holds 4096 per pass, so the host
    loop registers and decodes more than twice); device mode gives the same arrays"""
    sites = [struct.pack("<QQ", 0xABC0000000 + i, ~i & 0xFFFFFFFF) for i in range(4200)]
    items = [W.full(SYNC, W.ACT[0], f + 1, [Change("users", i, "age", i, 1, f + 1, k, sites[60 * f + k], 1)
                                            for k, i in enumerate(range(60 * f, 60 * f + 60))]) for f in range(70)]
    payloads, good = W.interleave(items, SYNC, every=20)
    eng = engine()
    assert eng.site_count() == 0
    dec, models = check(eng, payloads, SYNC, good, "4200 unknown sites")
    assert all(m[0] == 0 for m in models)
    ids = eng.site_ids()
    assert len(ids) == len(set(ids)) and set(sites) <= set(ids)
    got = host_arrays(dec)["site"]
    assert [ids[o] for o in got[:60].tolist()] == sites[:60]
    dev, _ = check(eng, payloads, SYNC, good, "4200 unknown sites, device mode", device=True)
    a, b = host_arrays(dec), host_arrays(dev)
    assert set(a) == set(b)
    long_ = a["val_len"] == M.VAL_LONG              # (val_off / val_size are written for long values only)
    for k in a:
        assert np.array_equal(a[k][long_], b[k][long_]) if k in ("val_off", "val_size") else \
            np.array_equal(a[k], b[k]), k
    assert np.array_equal(dec["status"], dev["status"])


def test_device_headers_with_bad_frames_interleaved():
    """40 frames, every third malformed, out of range or not a changeset: n_dev counts the status-0
    frames and cs_dev holds exactly their headers in order (the compaction map is not the identity).
    An EmptySet header carries change_off / change_count 0 there, as corro_hip.h documents."""
    from corrosion_amd import _lib as L
    bad = [p for _n, p, w in W.directed(SYNC) if w != 0]
    goodp = W.good_frames(SYNC)
    payloads = [bad[(5 * i) % len(bad)] if i % 3 == 1 else goodp[i % 4] for i in range(40)]
    good = [i for i in range(40) if i % 3 != 1]
    dec, models = check(engine(), payloads, SYNC, good, "device headers", device=True, device_headers=True)
    assert {m[0] for m in models} == {0, 1, -1, -6}
    assert dec["n_dev"] == len(good)
    recs = (L.Changeset * 40).from_buffer_copy(dec["cs_dev"].cpu().numpy().tobytes())
    for j, f in enumerate(good):
        h, d = dec["cs"][f], recs[j]
        same = ("site", "kind", "version_start", "version_end", "seq_start", "seq_end", "last_seq", "ts")
        assert [getattr(d, k) for k in same] == [getattr(h, k) for k in same], f
        assert (d.change_off, d.change_count) == ((0, 0) if h.kind == 2 else (h.change_off, h.change_count)), f


# ---- f. seeded mutation differential ---------------------------------------------------------------

def test_mutation_differential():
    """tests/wire_cases.fuzz_frames (2000 frames, 1 to 3 seeded mutations each of 21 base frames; the
    mix is asserted in tests/test_wire_model.py): every frame's status, and every field of every
    accepted frame, equals the model's. One call per payload kind."""
    frames = W.fuzz_frames()
    eng = engine()
    for kind in W.KINDS:
        payloads, good = W.interleave([p for p, k, _b in frames if k == kind], kind, every=50)
        check(eng, payloads, kind, good, f"mutation differential, payload {kind}")
