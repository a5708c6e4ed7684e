"""A plain-Python model of corro_decode_states (include/corro_hip.h): State frames -> statuses and the
need diff's entries, written from the layout alone (not from wire.decode_sync_state), and the frames the
CPU and GPU tests share: seeded random states, the edge shapes and the malformed list."""
import random
import struct

import numpy as np

from corrosion_amd import wire as W
from corrosion_amd.sync import SyncStateV1

INVALID, RANGE, NOT_STATE, DUPLICATE = -1, -6, 1, 3
V63 = 1 << 63
NONE = 0xFFFFFFFF


class _Bad(Exception):
    pass


def parse_frame(fr):
    """One frame (length prefix included) -> dict(status, and for status 0: actor, heads [(actor, head)],
    need [(actor, [(s, e)])], partial [(actor, [(version, [(s, e)])])], has_ts, ts)."""
    fr = bytes(fr)
    n = len(fr)
    pos = 0

    def need(k):
        if n - pos < k:
            raise _Bad

    def u32():
        nonlocal pos
        need(4)
        pos += 4
        return int.from_bytes(fr[pos - 4:pos], "little")

    def u64():
        nonlocal pos
        need(8)
        pos += 8
        return int.from_bytes(fr[pos - 8:pos], "little")

    def actor():
        nonlocal pos
        need(16)
        pos += 16
        return fr[pos - 16:pos]

    def count(least):                       # a count is bounded by the bytes left before it sizes a loop
        c = u32()
        if c * least > n - pos:
            raise _Bad
        return c

    try:
        need(4)
        if int.from_bytes(fr[:4], "big") != n - 4:
            raise _Bad
        pos = 4
        ver, tag = u32(), u32()
        if ver != 0 or tag > 4:
            raise _Bad
        if tag != 0:
            return {"status": NOT_STATE}
        me = actor()
        big = False
        heads = [(actor(), u64()) for _ in range(count(24))]
        nd = []
        for _ in range(count(20)):
            a = actor()
            nd.append((a, [(u64(), u64()) for _ in range(count(16))]))
        part = []
        for _ in range(count(20)):
            a = actor()
            vs = []
            for _ in range(count(12)):
                v = u64()
                vs.append((v, [(u64(), u64()) for _ in range(count(16))]))
            part.append((a, vs))
        has_ts, ts = 0, 0
        if pos != n:
            opt = fr[pos]
            pos += 1
            if opt > 1:
                raise _Bad
            if opt:
                has_ts, ts = 1, u64()
            if pos != n:
                raise _Bad
    except _Bad:
        return {"status": INVALID}
    big = (any(h >= V63 for _, h in heads) or any(s >= V63 or e >= V63 for _, rs in nd for s, e in rs) or
           any(v >= V63 for _, vs in part for v, _ in vs))
    if big:
        return {"status": RANGE}
    for lst in (heads, nd, part):
        if len({a for a, _ in lst}) != len(lst):
            return {"status": DUPLICATE}
    if any(len({v for v, _ in vs}) != len(vs) for _, vs in part):
        return {"status": DUPLICATE}
    return {"status": 0, "actor": me, "heads": heads, "need": nd, "partial": part, "has_ts": has_ts, "ts": ts}


_E = ("their_head", "our_head", "tn_start", "tn_end", "tp_ver", "tps_start", "tps_end", "on_start", "on_end", "op_ver",
      "ops_start", "ops_end")
_O = ("tn_off", "tp_off", "tps_off", "on_off", "op_off", "ops_off")


def decode_model(frames, pairs, site_of=lambda a: NONE):
    """What corro_decode_states returns for `frames` (a list of byte strings) and `pairs` [(ours, theirs)]:
    a dict of numpy arrays keyed like sync.entries_from_state_frames' result."""
    fs = [parse_frame(f) for f in frames]
    F = len(fs)
    out = {"frame_status": np.array([f["status"] for f in fs], np.int32).reshape(F),
           "frame_actor": np.frombuffer(b"".join(f.get("actor", b"\0" * 16) for f in fs), np.uint8).reshape(F, 16),
           "frame_has_ts": np.array([f.get("has_ts", 0) for f in fs], np.uint8).reshape(F),
           "frame_ts": np.array([f.get("ts", 0) for f in fs], np.uint64).reshape(F)}
    E = {k: [] for k in _E}
    off = {k: [0] for k in _O}
    epair, eactor, esite, pstat, peoff = [], [], [], [], [0]
    for p, (io, it) in enumerate(pairs):
        ours, theirs = fs[io], fs[it]
        bad = ours["status"] != 0 or theirs["status"] != 0
        pstat.append(1 if bad else 0)
        if not bad:
            oh, on, op = dict(ours["heads"]), dict(ours["need"]), dict(ours["partial"])
            tn, tp = dict(theirs["need"]), dict(theirs["partial"])
            for a, head in theirs["heads"]:
                if a == ours["actor"] or head == 0:
                    continue
                epair.append(p)
                eactor.append(a)
                esite.append(site_of(a))
                E["their_head"].append(head)
                E["our_head"].append(oh.get(a, -1))
                for side, nmap, pmap in (("t", tn, tp), ("o", on, op)):
                    for s, e in nmap.get(a, []):
                        E[side + "n_start"].append(s)
                        E[side + "n_end"].append(e)
                    off[side + "n_off"].append(len(E[side + "n_start"]))
                    for v, rs in sorted(pmap.get(a, [])):
                        E[side + "p_ver"].append(v)
                        for s, e in rs:
                            E[side + "ps_start"].append(s)
                            E[side + "ps_end"].append(e)
                        off[side + "ps_off"].append(len(E[side + "ps_start"]))
                    off[side + "p_off"].append(len(E[side + "p_ver"]))
        peoff.append(len(epair))
    for k, v in E.items():
        out[k] = np.array(v, np.int64 if k == "our_head" else np.uint64).reshape(len(v))
    for k, v in off.items():
        out[k] = np.array(v, np.uint64)
    n = len(epair)
    out["entry_pair"] = np.array(epair, np.int32).reshape(n)
    out["entry_actor"] = np.frombuffer(b"".join(eactor), np.uint8).reshape(n, 16)
    out["entry_site"] = np.array(esite, np.uint32).reshape(n)
    out["pair_status"] = np.array(pstat, np.uint8).reshape(len(pairs))
    out["pair_ent_off"] = np.array(peoff, np.uint64)
    out["nunregistered"] = sum(1 for s in esite if s == NONE)
    return out


ARRAYS = _E + _O + ("entry_pair", "entry_actor", "entry_site", "pair_status", "pair_ent_off", "frame_status", "frame_actor",
                    "frame_has_ts", "frame_ts")


def assert_same(got, want, what=""):
    """The device's (or host path's) result against the model's, array for array."""
    for k in ARRAYS:
        g = got[k].cpu().numpy() if hasattr(got[k], "cpu") else np.asarray(got[k])
        w = want[k]
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        # (a CUDA tensor is signed where the numpy array is not: the bits are compared)
        bits = {1: np.uint8, 4: np.uint32, 8: np.uint64}
        assert g.dtype.itemsize == w.dtype.itemsize, (what, k, g.dtype, w.dtype)
        assert np.array_equal(np.ascontiguousarray(g).view(bits[g.dtype.itemsize]), w.view(bits[w.dtype.itemsize])), (what, k, g, w)
    assert int(got["nunregistered"]) == want["nunregistered"], what


# ---- frames

def aid(i, lo=None, hi=None):
    """A 16-byte actor id: distinct per i unless a half is pinned."""
    a = struct.pack("<Q", 0x1000 + i if lo is None else lo) + struct.pack("<Q", 0xABCD0000 + 7 * i if hi is None else hi)
    return a


def state_frame(st):
    return W.frame(W.encode_sync_state(st))


def join(frames):
    """(buf bytes, frame_off uint64 array) of frames laid back to back."""
    off = np.zeros(len(frames) + 1, np.uint64)
    off[1:] = np.cumsum([len(f) for f in frames])
    return b"".join(frames), off


def random_state(rng, me, universe, nmax=12):
    """A seeded SyncStateV1 over a small actor universe, so that the maps of two states overlap; each map
    in an order of its own."""
    def ranges(k, top):
        pts = sorted(rng.sample(range(1, top), 2 * k))
        return [(pts[2 * i], pts[2 * i + 1]) for i in range(k)]

    st = SyncStateV1(actor_id=me)
    for a in rng.sample(universe, rng.randint(0, min(nmax, len(universe)))):
        st.heads[a] = rng.choice([0, 0, 1]) * rng.randint(1, 1000) if rng.random() < 0.15 else rng.randint(1, 1000)
    for a in rng.sample(universe, rng.randint(0, min(nmax, len(universe)))):
        st.need[a] = ranges(rng.randint(0, 4), 1200)
    for a in rng.sample(universe, rng.randint(0, min(nmax, len(universe)))):
        vs = rng.sample(range(1, 1200), rng.randint(0, 4))
        st.partial_need[a] = {v: ranges(rng.randint(0, 3), 400) for v in vs}
    st.last_cleared_ts = rng.choice([None, rng.getrandbits(63)])
    return st


def random_pairs(seed, npairs, nactors=24):
    """npairs seeded (ours, theirs) SyncStateV1 pairs over one actor universe."""
    rng = random.Random(seed)
    universe = [aid(i) for i in range(nactors)]
    out = []
    for _ in range(npairs):
        me, peer = rng.sample(universe, 2)
        out.append((random_state(rng, me, universe), random_state(rng, peer, universe)))
    return out


def _good():
    """The state the malformed frames are cut from: every section non-empty, the timestamp present."""
    st = SyncStateV1(actor_id=aid(900))
    st.heads = {aid(1): 10, aid(2): 20}
    st.need = {aid(1): [(1, 2), (5, 6)], aid(3): [(7, 9)]}
    st.partial_need = {aid(2): {4: [(0, 3)], 9: [(1, 1), (5, 8)]}, aid(1): {7: []}}
    st.last_cleared_ts = 77
    return st


def malformed_frames():
    """[(name, frame bytes, status)]: the frames corro_decode_states must refuse, each alone."""
    good = W.encode_sync_state(_good())
    fr = W.frame
    out = []
    # sections of `good` end at: header 8, actor 24, heads count 28, heads 76, need count 80, need 168 (its
    # first range at 100), partial count 172, partial 296 (first version at 192, its seq count at 200), the
    # option byte 297, the timestamp 305
    assert len(good) == 305
    for cut in (3, 8, 20, 24, 26, 28, 52, 76, 80, 100, 104, 168, 172, 192, 200, 204, 297, 301):
        out.append((f"cut_{cut}", fr(good[:cut]), INVALID))
    # a count of 0xFFFFFFFF at each of the six count positions
    for name, at in (("heads", 24), ("need", 76), ("need_ranges", 96), ("partial", 168), ("partial_versions", 188),
                     ("partial_seqs", 200)):
        out.append((f"count_{name}", fr(good[:at] + b"\xff" * 4 + good[at + 4:]), INVALID))
    out.append(("prefix_short", struct.pack(">I", len(good) - 1) + good, INVALID))
    out.append(("prefix_long", struct.pack(">I", len(good) + 1) + good, INVALID))
    out.append(("no_prefix", b"\0\0", INVALID))
    out.append(("trailing", fr(good + b"\0"), INVALID))
    out.append(("trailing_after_none", fr(good[:296] + b"\0\0"), INVALID))
    out.append(("option_2", fr(good[:296] + b"\x02" + good[297:]), INVALID))
    out.append(("version_1", fr(b"\x01\0\0\0" + good[4:]), INVALID))
    for tag in (1, 2, 3, 4):
        out.append((f"tag_{tag}", fr(struct.pack("<II", 0, tag) + good[8:]), NOT_STATE))
    out.append(("tag_5", fr(struct.pack("<II", 0, 5) + good[8:]), INVALID))
    big = struct.pack("<Q", V63)
    out.append(("head_2_63", fr(good[:44] + big + good[52:]), RANGE))
    out.append(("need_start_2_63", fr(good[:100] + big + good[108:]), RANGE))
    out.append(("need_end_2_63", fr(good[:108] + big + good[116:]), RANGE))
    out.append(("partial_version_2_63", fr(good[:192] + big + good[200:]), RANGE))
    out.append(("range_and_truncated", fr((good[:44] + big + good[52:])[:300]), INVALID))
    # duplicates: the second actor of each map renamed to the first, and a version twice
    out.append(("dup_head", fr(good[:52] + good[28:44] + good[68:]), DUPLICATE))
    out.append(("dup_need", fr(good[:132] + good[80:96] + good[148:]), DUPLICATE))
    out.append(("dup_partial", fr(good[:264] + good[172:188] + good[280:]), DUPLICATE))
    out.append(("dup_version", fr(good[:220] + good[192:200] + good[228:]), DUPLICATE))
    out.append(("dup_and_range", fr(good[:44] + big + good[28:44] + good[68:]), RANGE))
    return out
