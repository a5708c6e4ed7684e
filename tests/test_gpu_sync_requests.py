"""GPU parity of the sync request planner (corro_plan_requests) against the sequential oracle of
tests/sync_req_util.py: byte-exact frames per group and an equal frame table, from host and from device
memory.

The refusal of a frame payload of 2^32 bytes or more needs gigabytes of input built on the card and
has its own file, tests/test_gpu_sync_requests_payload.py."""
import ctypes as C

import numpy as np
import pytest

from corrosion_amd import _lib as L
from corrosion_amd import sync as S
from tests import sync_req_util as U
from tests.test_sync_requests import KATS, kat_servers

pytestmark = pytest.mark.gpu
MEMS = ["host", "device"]
_ENGINE = []


def engine():
    """One engine for the module, the oracle's four actors registered as sites 0..3."""
    if not _ENGINE:
        import corrosion_amd as ca
        e = ca.MergeEngine({"t": ["a"]}, capacity_hint=1024)
        ords = e.register_sites(np.frombuffer(b"".join(U.ACTORS), np.uint8))
        assert list(ords) == [0, 1, 2, 3]
        _ENGINE.append(e)
    return _ENGINE[0]


SITE_OF = {a: i for i, a in enumerate(U.ACTORS)}
A0 = U.ACTORS[0]


def to_dev(arr):
    import torch
    view = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32, np.dtype(np.uint8): np.uint8}
    return {k: torch.from_numpy(np.ascontiguousarray(v).view(view[v.dtype])).cuda() for k, v in arr.items()}


def plan(arr, chunk, drain, mem, eng=None):
    res = S._plan_requests(eng or engine(), to_dev(arr) if mem == "device" else arr, chunk, drain, mem == "device")
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in res.items()}


def check(res, want, ngroups):
    gfo, fo = res["grp_frame_off"].astype(np.int64), res["frame_off"].astype(np.int64)
    assert len(gfo) == ngroups + 1 and gfo[0] == 0 and gfo[-1] == res["nframes"] == len(want["frame_entry"])
    assert fo[0] == 0 and fo[-1] == res["nbytes"] == sum(len(b) for b in want["group_bytes"])
    buf = res["buf"].tobytes()
    for g, wb in enumerate(want["group_bytes"]):
        assert buf[fo[gfo[g]]:fo[gfo[g + 1]]] == wb, f"group {g}"
    for k in ("frame_entry", "frame_round", "frame_needs", "grp_frame_off"):
        assert res[k].astype(np.int64).tolist() == want[k], k


def run_sessions(sessions, chunk, drain, mem):
    arr, groups = U.flatten(sessions, SITE_OF)
    res = plan(arr, chunk, drain, mem)
    check(res, U.expected(sessions, groups, chunk, drain), len(groups))
    return res


@pytest.mark.parametrize("mem", MEMS)
@pytest.mark.parametrize("kat", KATS["kats"], ids=[k["name"] for k in KATS["kats"]])
def test_kats(kat, mem):
    actor = bytes.fromhex(KATS["actor"])
    assert actor == A0
    run_sessions([kat_servers(kat)], kat["chunk"], kat["drain"], mem)


def test_public_api_k3_and_known_bytes():
    got = S.plan_sync_requests(engine(), [[{A0: [S.Full(14, 16)]}, {}, {A0: [S.Full(1, 25)]}],
                                          [{A0: [S.Full(12, 20)]}]])
    assert [len(s) for s in got] == [3, 1] and got[0][1] == []
    from corrosion_amd import wire as W
    assert [(r, W.decode_sync_request(f[4:])) for r, f in got[0][2]] == [
        (0, [(A0, [S.Full(21, 25)])]), (0, [(A0, [S.Full(11, 13), S.Full(17, 20)])]), (0, [(A0, [S.Full(1, 10)])])]
    assert got[1][0] == [(0, bytes.fromhex(KATS["full_12_20_frame_hex"]))]


@pytest.mark.parametrize("mem", MEMS)
@pytest.mark.parametrize("chunk,drain", [(10, 10), (3, 2), (1, 1), (10, 1), (1, 10)])
def test_random_sessions_in_one_call(chunk, drain, mem):
    run_sessions(U.random_sessions(), chunk, drain, mem)


def test_random_sessions_one_call_equals_one_call_each():
    """Sessions do not leak into each other: 300 sessions in one call give what 300 calls give."""
    sessions = U.random_sessions()
    arr, groups = U.flatten(sessions, SITE_OF)
    one = plan(arr, 3, 2, "host")
    fo, gfo = one["frame_off"].astype(np.int64), one["grp_frame_off"].astype(np.int64)
    buf = one["buf"].tobytes()
    g0 = 0
    for servers in sessions:
        a1, gr1 = U.flatten([servers], SITE_OF)
        if not gr1:
            continue
        r1 = plan(a1, 3, 2, "host")
        lo, hi = gfo[g0], gfo[g0 + len(gr1)]
        assert r1["buf"].tobytes() == buf[fo[lo]:fo[hi]]
        assert np.array_equal(r1["frame_round"], one["frame_round"][lo:hi])
        assert np.array_equal(r1["frame_needs"], one["frame_needs"][lo:hi])
        assert np.array_equal(r1["grp_frame_off"].astype(np.int64), gfo[g0:g0 + len(gr1) + 1] - lo)
        g0 += len(gr1)
    assert g0 == len(groups)


@pytest.mark.parametrize("mem", MEMS)
def test_hot_group_identical_huge_needs(mem):
    """Three servers with the same Full 1..=100000 (30k items), a fourth with 50000..=50004."""
    servers = [[(A0, [("F", 1, 100000)])] for _ in range(3)] + [[(A0, [("F", 50000, 50004)])]]
    res = run_sessions([servers], 10, 10, mem)
    assert res["nframes"] >= 10000


@pytest.mark.parametrize("mem", MEMS)
def test_tile_edges(mem):
    big, many, edge = U.tile_edge_sessions()
    res = run_sessions([big], 10, 10, mem)
    assert res["nbytes"] == 9648 + 4
    res = run_sessions([many], 10, 10, mem)
    assert res["nframes"] == 400 and list(res["frame_needs"]) == [1] * 400
    res = run_sessions([edge], 10, 10, mem)
    assert res["frame_off"][res["grp_frame_off"][1]] == 8192
    run_sessions([big, many, edge, big], 10, 10, mem)


@pytest.mark.parametrize("mem", MEMS)
def test_quirks(mem):
    sessions = U.quirk_sessions()
    res = run_sessions(sessions, 10, 10, mem)
    arr, groups = U.flatten(sessions, SITE_OF)
    gfo = res["grp_frame_off"]
    g = [(a, b) for a, b, _ in groups].index((4, 1))
    assert gfo[g] == gfo[g + 1]
    from corrosion_amd import wire as W
    fo = res["frame_off"].astype(np.int64)
    buf = res["buf"].tobytes()
    first = [W.decode_sync_request(buf[fo[f] + 4:fo[f + 1]])[0][1] for f in range(int(gfo[0]), int(gfo[1]))]
    assert first == [[S.Full(21, 21)], [S.Full(11, 20)], [S.Full(1, 10)]]
    g3 = [(a, b) for a, b, _ in groups].index((3, 0))
    f3 = int(gfo[g3])
    assert W.decode_sync_request(buf[fo[f3] + 4:fo[f3 + 1]]) == [(A0, [S.Partial(5, ((0, 9),))])]


def test_chain_from_the_device_need_diff():
    """corro_compute_needs_onepass on 64 random state pairs, four per session, its device output passed
    straight in; the frames equal the oracle's over sync.decode of the host path's needs."""
    import torch
    from tests.sync_util import entries_from_pairs
    from tests.test_gpu_sync import random_side
    rng = np.random.default_rng(21)
    pairs = [(random_side(rng, with_head=rng.random() < 0.9), random_side(rng)) for _ in range(64)]
    ent = entries_from_pairs(pairs)
    e = engine()
    actor_of = [U.ACTORS[(i // 4) % 3] if i % 4 < 3 else U.ACTORS[3] for i in range(64)]
    host = S.decode(e.compute_needs(ent), [(i, actor_of[i]) for i in range(64)], 64)
    sessions = []
    for sn in range(16):
        servers = []
        for i in range(4 * sn, 4 * sn + 4):
            needs = [("F", n.start, n.end) if isinstance(n, S.Full) else ("P", n.version, tuple(n.seqs))
                     for n in host[i].get(actor_of[i], [])]
            servers.append([(actor_of[i], needs)])
        sessions.append(servers)
    dev_ent = {k: torch.from_numpy(np.ascontiguousarray(v).view(np.int64)).cuda() for k, v in ent.items()}
    needs = S._needs_device_1pass(e, dev_ent)
    site = torch.tensor([SITE_OF[a] for a in actor_of], dtype=torch.int32).cuda()
    geo = torch.arange(65, dtype=torch.int64).cuda()
    ses = (torch.arange(64, dtype=torch.int64) // 4).cuda()
    res = S.plan_requests_device(e, needs, site, geo, ses)
    res = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in res.items()}
    groups = [(i // 4, i % 4, i) for i in range(64)]
    want = U.expected(sessions, groups)
    assert res["nframes"] > 50
    check(res, want, 64)


def _valid():
    sessions = [[[(A0, [("F", 1, 25), ("P", 4, ((0, 3), (8, 9)))]), (U.ACTORS[1], [("F", 3, 4)])],
                 [(A0, [("F", 20, 30)])]]]
    return U.flatten(sessions, SITE_OF)[0]


def _set(arr, key, idx, val):
    arr[key] = arr[key].copy()
    arr[key][idx] = val


def _bad_kind(a): _set(a, "kind", 0, 2)
def _bad_site(a): _set(a, "site", 1, 99)
def _need_off_not_monotone(a): _set(a, "need_off", 1, 4)
def _need_off_past_needs(a): _set(a, "need_off", 3, 9)
def _grp_off_past_entries(a): _set(a, "grp_ent_off", 2, 7)
def _grp_off_not_monotone(a): _set(a, "grp_ent_off", 0, 3)
def _session_decreasing(a): _set(a, "grp_session", 0, 5)
def _seq_span_outside(a): _set(a, "sr_n", 1, 3)
def _seq_start_after_end(a): _set(a, "s_start", 1, 10)
def _full_end_2_63(a): _set(a, "end", 0, 1 << 63)
def _seq_end_max(a): _set(a, "s_end", 1, (1 << 64) - 1)
def _too_many_items(a): _set(a, "end", 0, 1 << 34)


BAD = [(_bad_kind, 10, 10, -1), (_bad_site, 10, 10, -1), (_need_off_not_monotone, 10, 10, -1),
       (_need_off_past_needs, 10, 10, -1), (_grp_off_past_entries, 10, 10, -1), (_grp_off_not_monotone, 10, 10, -1),
       (_session_decreasing, 10, 10, -1), (_seq_span_outside, 10, 10, -1), (_seq_start_after_end, 10, 10, -1),
       (None, 0, 10, -1), (None, 10, 0, -1), (_full_end_2_63, 10, 10, -6), (_seq_end_max, 10, 10, -6),
       (_too_many_items, 1, 10, -6)]


def _raw(arr, chunk, drain, pass_, o, mem, eng=None):
    keep = to_dev(arr) if mem == "device" else arr
    ptr = (lambda a: a.data_ptr() if a.numel() else None) if mem == "device" else (lambda a: a.ctypes.data if a.size else None)
    r = L.RequestIn()
    r.n, r.nneeds, r.nseqs, r.ngroups = len(arr["site"]), len(arr["kind"]), len(arr["s_start"]), len(arr["grp_session"])
    r.chunk_size, r.drain = chunk, drain
    for k in S._REQ_IN:
        setattr(r, k, ptr(keep[k]))
    if mem == "device":
        import torch
        torch.cuda.synchronize()
    return L.lib().corro_plan_requests((eng or engine())._h, C.byref(r), L.CORRO_MEM_DEVICE if mem == "device" else 0, C.byref(o), pass_)


@pytest.mark.parametrize("mem", MEMS)
@pytest.mark.parametrize("mutate,chunk,drain,code", BAD, ids=[(m.__name__ if m else f"chunk{c}_drain{d}") for m, c, d, _ in BAD])
def test_refusals_write_nothing_and_leave_the_context_usable(mutate, chunk, drain, code, mem):
    good = _valid()
    ok = plan(good, 10, 10, mem)
    bad = dict(good)
    if mutate:
        mutate(bad)
    outs = {"grp_frame_off": np.full(3, 0x5A5A5A5A5A5A5A5A, np.uint64), "buf": np.full(ok["nbytes"], 0x5A, np.uint8),
            "frame_off": np.full(ok["nframes"] + 1, 0x5A5A5A5A5A5A5A5A, np.uint64),
            "frame_entry": np.full(ok["nframes"], 0x5A5A5A5A5A5A5A5A, np.uint64),
            "frame_round": np.full(ok["nframes"], 0x5A5A5A5A, np.uint32), "frame_needs": np.full(ok["nframes"], 0x5A5A5A5A, np.uint32)}
    held = to_dev(outs) if mem == "device" else {k: v.copy() for k, v in outs.items()}
    o = L.Requests()
    for k, v in held.items():
        setattr(o, k, v.data_ptr() if mem == "device" else v.ctypes.data)
    for pass_ in (0, 1):
        o.nframes, o.nbytes = (ok["nframes"], ok["nbytes"]) if pass_ else (0, 0)
        assert _raw(bad, chunk, drain, pass_, o, mem) == code
    for k, v in held.items():
        got = v.cpu().numpy() if mem == "device" else v
        assert np.array_equal(got.view(outs[k].dtype), outs[k]), k
    again = plan(good, 10, 10, mem)
    assert again["buf"].tobytes() == ok["buf"].tobytes() and again["nframes"] == ok["nframes"] > 0
