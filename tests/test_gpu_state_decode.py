"""GPU state decode (corro_decode_states, csrc/state_decode.hip) against the plain-Python model
(tests/state_model.py), from host and from device memory, array for array; then the chain it opens: the
need diff on its entries against batch_compute_available_needs, and requests_from_state_frames against
plan_sync_requests, byte for byte."""
import random

import numpy as np
import pytest

from corrosion_amd import _lib as L
from corrosion_amd import sync as S
from corrosion_amd import wire as W
from tests import state_model as M

pytestmark = pytest.mark.gpu
MEMS = ["host", "device"]
KNOWN = [M.aid(i) for i in range(24)]          # the universe of random_pairs, registered in order
_ENGINE = {}


def engine(name="main"):
    if name not in _ENGINE:
        import corrosion_amd as ca
        e = ca.MergeEngine({"t": ["a"]}, capacity_hint=1024)
        if name == "main":
            assert list(e.register_sites(np.frombuffer(b"".join(KNOWN), np.uint8))) == list(range(len(KNOWN)))
        _ENGINE[name] = e
    return _ENGINE[name]


def site_of(a):
    return KNOWN.index(a) if a in KNOWN else M.NONE


def run(frames, pairs, mem, eng=None):
    buf, off = M.join(frames)
    eng = eng or engine()
    if mem == "device":
        import torch
        res = S.entries_from_state_frames(eng, torch.from_numpy(np.frombuffer(buf, np.uint8).copy()).cuda(), off, pairs, device=True)
        assert res["their_head"].is_cuda and res["entry_site"].is_cuda and res["frame_status"].is_cuda
        return res
    return S.entries_from_state_frames(eng, buf, off, pairs)


def check(frames, pairs, mem, what=""):
    want = M.decode_model(frames, pairs, site_of)
    before = engine().site_count()
    got = run(frames, pairs, mem)
    assert engine().site_count() == before                            # a lookup never inserts
    M.assert_same(got, want, what)
    return got, want


def eof_ts(st):
    """The frame of a state whose Option<Timestamp> is left off the wire (default_on_eof)."""
    assert st.last_cleared_ts is None
    return W.frame(W.encode_sync_state(st)[:-1])


def small_states():
    a = M.aid
    s0 = S.SyncStateV1(actor_id=a(100))                               # zero heads, nothing at all
    s1 = S.SyncStateV1(actor_id=a(101), heads={a(1): 5})              # one head, timestamp 0x00
    s2 = S.SyncStateV1(actor_id=a(1), last_cleared_ts=(1 << 64) - 1)
    s2.heads = {a(2): 0, a(101): 9, a(3): 7, a(4): 1, a(1): 3}        # a head of 0; an actor only in heads (4)
    s2.need = {a(3): [], a(9): [(1, 4)], a(101): [(2, 2), (8, 11)]}   # an empty need vector; an actor not in heads (9)
    s2.partial_need = {a(3): {6: [], 2: [(0, 1)]}, a(8): {}, a(101): {}}   # a version without seq ranges; empty maps
    s3 = S.SyncStateV1(actor_id=a(3), heads={a(101): 4, a(1): 2, a(3): 8}, need={a(101): [(1, 1)]},
                       partial_need={a(1): {5: [(3, 4)]}})
    return [s0, s1, s2, s3]


@pytest.mark.parametrize("mem", MEMS)
def test_smallest_shapes(mem):
    sts = small_states()
    frames = [eof_ts(sts[0]), M.state_frame(sts[1]), M.state_frame(sts[2]), eof_ts(sts[3])]
    pairs = [(i, j) for i in range(4) for j in range(4)]              # every frame on both sides, and with itself
    got, want = check(frames, pairs, mem)
    assert list(want["frame_has_ts"]) == [0, 0, 1, 0] and int(want["frame_ts"][2]) == (1 << 64) - 1
    assert len(want["their_head"]) > 10 and (want["our_head"] == -1).any() and (want["our_head"] > 0).any()
    # ours = s1 (actor 101), theirs = s2: the head of 0 and the head for 101 are skipped
    lo, hi = int(want["pair_ent_off"][6]), int(want["pair_ent_off"][7])
    assert [bytes(x) for x in want["entry_actor"][lo:hi]] == [M.aid(3), M.aid(4), M.aid(1)]
    check([frames[0]], [(0, 0)], mem, "one frame, no entry")
    check(frames, [], mem, "no pair")


def big_state(me, n, seed, tag):
    """n actors whose ids share a half, each map in an order of its own."""
    rng = random.Random(seed)
    ids = [M.aid(i, lo=77) if tag == "lo" else M.aid(i, hi=77) if tag == "hi" else M.aid(1000 + i) for i in range(n)]
    st = S.SyncStateV1(actor_id=me)
    order = ids[:]
    rng.shuffle(order)
    st.heads = {x: rng.randint(1, 500) for x in order}
    rng.shuffle(order)
    st.need = {x: [(k, k + 1) for k in range(1, 1 + 3 * rng.randint(0, 2), 3)] for x in order[: 2 * n // 3]}
    rng.shuffle(order)
    st.partial_need = {x: {v: [(0, v)] * rng.randint(0, 2) for v in rng.sample(range(1, 50), rng.randint(1, 3))}
                       for x in order[: n // 2]}
    return st


@pytest.mark.parametrize("mem", MEMS)
def test_join_over_probe_chains_and_half_equal_ids(mem):
    a = big_state(M.aid(500), 300, 1, "lo")                           # 300 actors: more than one wave per section
    b = big_state(M.aid(501), 300, 2, "lo")
    c = big_state(M.aid(502), 150, 3, "hi")
    d = big_state(M.aid(0, lo=77), 150, 4, "hi")                      # its own id is one of a's and b's heads
    frames = [M.state_frame(s) for s in (a, b, c, d)]
    assert list(a.heads) != list(a.need)[:300] and list(a.need) != list(a.partial_need)
    # frame 1 is `ours` in one pair and `theirs` in another; 0 against 2 shares no actor at all
    got, want = check(frames, [(0, 1), (1, 0), (2, 3), (3, 2), (0, 2), (3, 0), (1, 1)], mem)
    n = np.diff(want["pair_ent_off"].astype(np.int64))
    assert list(n) == [300, 300, 150, 150, 150, 299, 300]
    assert (want["our_head"][:600] >= 0).all() and (want["our_head"][900:1050] == -1).all()


@pytest.mark.parametrize("mem", MEMS)
def test_partial_versions_come_out_ascending(mem):
    top = (1 << 63) - 1
    x, y = M.aid(1), M.aid(2)
    desc = {v: [(v % 7, v % 7 + 1)] * (v % 3) for v in (top, 900, 40, 2, 1)}
    rng = random.Random(9)
    vs = [1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, top, top - 1]
    rng.shuffle(vs)
    shuf = {v: [(i, i + v % 5) for i in range(v % 4)] for v in vs}
    theirs = S.SyncStateV1(actor_id=M.aid(7), heads={x: 4, y: 6}, partial_need={y: desc, x: shuf})
    ours = S.SyncStateV1(actor_id=M.aid(8), heads={y: 1}, partial_need={x: desc, y: shuf})
    got, want = check([M.state_frame(ours), M.state_frame(theirs)], [(0, 1), (1, 0)], mem)
    assert [int(v) for v in want["tp_ver"][:13]] == sorted(vs) and int(want["tp_ver"][17]) == top
    assert list(theirs.partial_need[y]) == [top, 900, 40, 2, 1]       # (descending on the wire)


BAD = M.malformed_frames()


@pytest.mark.parametrize("mem", MEMS)
def test_malformed_frames_between_good_frames(mem):
    ours, theirs = M.random_pairs(77, 1)[0]
    g = [M.state_frame(ours), M.state_frame(theirs)]
    frames, pairs = [], []
    for _name, fr, _st in BAD:                                        # good, bad, good, good, bad, good ...
        k = len(frames)
        frames += [g[0], fr, g[1]]
        pairs += [(k, k + 2), (k + 1, k + 2), (k, k + 1), (k + 2, k)]
    got, want = check(frames, pairs, mem)
    assert list(want["frame_status"]) == [s for b in BAD for s in (0, b[2], 0)]
    assert list(want["pair_status"]) == [0, 1, 1, 0] * len(BAD)
    alone = M.decode_model(g, [(0, 1), (1, 0)], site_of)
    n = len(alone["their_head"])
    assert n > 4 and len(want["their_head"]) == n * len(BAD)          # the neighbours' output is unchanged
    for k in ("their_head", "our_head", "entry_actor", "entry_site"):
        g_k = got[k].cpu().numpy() if hasattr(got[k], "cpu") else got[k]
        assert all(np.array_equal(g_k[i * n:(i + 1) * n].astype(np.int64), alone[k].astype(np.int64)) for i in range(len(BAD))), k
    for (name, fr, st) in BAD[:3]:                                    # and each alone, as the only frame
        check([fr], [(0, 0)], mem, name)


def test_unregistered_actors_get_none_and_stay_unregistered():
    ours, theirs = M.random_pairs(5, 1)[0]
    theirs.heads[M.aid(700)] = 3                                      # two strangers
    theirs.heads[M.aid(701)] = 4
    got, want = check([M.state_frame(ours), M.state_frame(theirs)], [(0, 1)], "device")
    assert want["nunregistered"] == 2 and list(want["entry_site"][-2:]) == [M.NONE, M.NONE]
    assert (want["entry_site"][:-2] < len(KNOWN)).all()


def test_call_failures_on_device_arrays():
    import torch
    ours, theirs = M.random_pairs(6, 1)[0]
    buf, off = M.join([M.state_frame(ours), M.state_frame(theirs)])
    dbuf = torch.from_numpy(np.frombuffer(buf, np.uint8).copy()).cuda()
    for bad_off, pairs in ((off[[1, 0, 2]], [(0, 1)]), (off + np.uint64(1), [(0, 1)]), (off, [(0, 2)]), (off, [(2, 1)])):
        with pytest.raises(L.CorroError) as e:
            S.entries_from_state_frames(engine(), dbuf, bad_off, pairs, device=True)
        assert e.value.code == -1
    for key in ("n", "ntn", "ntp", "ntps", "non", "nop", "nops"):
        for mem in (False, True):
            dec = S._StateFrames(engine(), dbuf if mem else buf, off, [(0, 1)], mem)
            setattr(dec.o, key, getattr(dec.o, key) + 1)             # pass-1 totals that differ from pass 0's
            with pytest.raises(L.CorroError) as e:
                dec.fill()
            assert e.value.code == -1 and "sizes differ" in str(e.value)
    M.assert_same(S.entries_from_state_frames(engine(), dbuf, off, [(0, 1)], device=True),
                  M.decode_model([M.state_frame(ours), M.state_frame(theirs)], [(0, 1)], site_of))


def test_need_diff_on_decoded_entries_equals_the_host_path():
    import torch
    pairs = M.random_pairs(50, 50)
    want = S.batch_compute_available_needs(engine(), pairs)
    frames, idx = [], []
    for ours, theirs in pairs:
        idx.append((len(frames), len(frames) + 1))
        frames += [M.state_frame(ours), M.state_frame(theirs)]
    buf, off = M.join(frames)
    ent = S.entries_from_state_frames(engine(), torch.from_numpy(np.frombuffer(buf, np.uint8).copy()).cuda(), off, idx, device=True)
    res = S._needs_device(engine(), {k: ent[k] for k in S._ENT_KEYS})
    res = {k: v.cpu().numpy() for k, v in res.items()}
    index = [(int(p), bytes(a)) for p, a in zip(ent["entry_pair"].cpu().numpy(), ent["entry_actor"].cpu().numpy())]
    got = S.decode(res, index, len(pairs))
    assert got == want and sum(len(m) for m in want) > 100


def test_requests_from_state_frames_equal_plan_sync_requests():
    import torch
    rng = random.Random(31)
    universe = KNOWN[:12] + [M.aid(800)]                              # one actor the engine has not seen
    frames, sessions, states = [], [], []
    for sn in range(3):
        ours = M.random_state(rng, M.aid(300 + sn), universe)
        servers = [M.random_state(rng, M.aid(310 + 3 * sn + k), universe) for k in range(3)]
        servers[sn].heads[M.aid(800)] = 40 + sn
        for k in range(3):
            servers[k].heads[KNOWN[20 + k]] = 50 + k                  # (something `ours` has never heard of)
        if sn == 1:
            servers[1] = S.SyncStateV1(actor_id=M.aid(399))           # a server with nothing to offer, in the middle
        k = len(frames)
        frames += [M.state_frame(ours)] + [M.state_frame(s) for s in servers]
        sessions.append((k, [k + 1, k + 2, k + 3]))
        states.append((ours, servers))
    ref = engine("reference")                                         # the host path registers what it meets
    needs = [S.batch_compute_available_needs(ref, [(ours, s) for s in servers]) for ours, servers in states]
    assert needs[1][1] == {} and all(needs[sn][k] for sn in range(3) for k in range(3) if (sn, k) != (1, 1))
    want = S.plan_sync_requests(ref, needs)
    eng = engine()
    before = eng.site_count()
    buf, off = M.join(frames)
    res = S.requests_from_state_frames(eng, torch.from_numpy(np.frombuffer(buf, np.uint8).copy()).cuda(), off, sessions)
    assert res["buf"].is_cuda and eng.site_count() == before + 1     # the stranger, and nobody else
    assert eng.site_ids()[-1] == M.aid(800)
    host = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in res.items()}
    got = S.split_requests(host, res["groups"], 3, [3, 3, 3])
    assert got == want
    assert got[1][1] == [] and got[1][0] and got[1][2] and sum(len(x) for s in got for x in s) > 20
