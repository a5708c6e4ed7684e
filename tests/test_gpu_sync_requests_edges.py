"""Directed edges of corro_plan_requests (csrc/req_plan.hip): the widths of its per-call sort keys
(cbits from the largest coordinate + 1, vbits from the largest Partial version, gbits and sbits from
the group and site counts), the two 32-bit halves of every 64-bit frame field, the order of servers,
rounds and pieces, the shapes only the ABI arrays can express, the output writer's tiles and its
byte-store path, and the two-pass protocol.

Every case is built as ABI arrays (tests/req_plan_model.py arrays) and checked byte for byte, with
the frame table and grp_frame_off, against the interval model (tests/req_plan_model.py plan), which
tests/test_req_plan_model.py holds to hand-written answers and to the set oracle. Each case runs from
host and from device memory unless it says otherwise.

Not reached: 1 + gbits + sbits = 64, the full width of the book key, would take 2^31 groups in a call.
"""
import numpy as np
import pytest

from corrosion_amd import _lib as L
from tests import req_plan_model as M
from tests import sync_req_util as U
from tests.test_gpu_sync_requests import MEMS, _raw, check, plan, to_dev

pytestmark = pytest.mark.gpu

SITES = b"".join(U.ACTORS)
W, I63, U64 = 1 << 32, (1 << 63) - 1, (1 << 64) - 1


def F(a, b):
    return ("F", a, b)


def P(v, *seqs):
    return ("P", v, tuple(seqs))


def run(groups, mem, chunk=10, drain=10, eng=None, sites=SITES, lead=(), trail=()):
    """One call against the model; returns (result, model's answer)."""
    arr = M.arrays(groups, lead, trail)
    want = M.plan(arr, chunk, drain, sites)
    res = plan(arr, chunk, drain, mem, eng)
    check(res, want, len(groups))
    return res, want


def rungs(d):
    return pytest.mark.parametrize("rung", list(d.values()), ids=list(d.keys()))


# ---- coordinate width ------------------------------------------------------------------------

def full_trio(B, site=0):
    """Three servers' overlapping needs on one actor from base B, 40 wide."""
    return [[(site, [F(B, B + 40)])], [(site, [F(B + 5, B + 33)])], [(site, [F(B + 12, B + 40), F(B + 2, B + 3)])]]


def seq_trio(B, site=0, v=7):
    return [[(site, [P(v, (B + 30, B + 34), (B + 10, B + 20))])], [(site, [P(v, (B + 5, B + 32))])],
            [(site, [P(v, (B, B + 40))])]]


BASES = {"0": 0, "2^8": 1 << 8, "2^31-20": (1 << 31) - 20, "2^32-20": W - 20, "2^32": W, "2^33+1": (1 << 33) + 1,
         "2^62": 1 << 62, "2^63-1-40": I63 - 40}


@pytest.mark.parametrize("mem", MEMS)
@rungs(BASES)
def test_full_coordinate_width(rung, mem):
    res, want = run([(0, ents) for ents in full_trio(rung)], mem, drain=2)
    assert res["nframes"] == 8 and max(want["frame_round"]) == 2


@pytest.mark.parametrize("mem", MEMS)
def test_full_small_and_top_books_in_one_call(mem):
    """cbits is per call: a book of small coordinates next to the book that ends at 2^63 - 1, as two
    actors of one session and as one actor in two sessions."""
    small, top = full_trio(3), full_trio(I63 - 40, site=1)
    groups = [(0, a + b) for a, b in zip(small, top)] + [(1, ents) for ents in full_trio(I63 - 40)] + \
             [(2, ents) for ents in full_trio(3)]
    res, _ = run(groups, mem, drain=2)
    assert res["nframes"] >= 4 * 5


@pytest.mark.parametrize("mem", MEMS)
@rungs({**BASES, "2^64-2-40": U64 - 1 - 40})
def test_seq_coordinate_width(rung, mem):
    res, _ = run([(0, ents) for ents in seq_trio(rung)], mem)
    assert res["nframes"] == 3 and res["frame_needs"].tolist() == [1, 1, 1]


@pytest.mark.parametrize("mem", MEMS)
def test_seq_ranges_either_side_of_2_32_keep_their_order(mem):
    """No range holds the word line, so only the order of the pieces can go wrong: given high first."""
    groups = [(0, [(0, [P(7, (W + 5, W + 15), (W - 20, W - 10))])]), (0, [(0, [P(7, (W + 10, W + 20), (W - 25, W - 15))])])]
    res, _ = run(groups, mem)
    assert res["nframes"] == 2


@pytest.mark.parametrize("mem", MEMS)
def test_seq_small_and_top_books_in_one_call(mem):
    small, top = seq_trio(3), seq_trio(U64 - 1 - 40, site=1)
    groups = [(0, a + b) for a, b in zip(small, top)] + [(1, ents) for ents in seq_trio(U64 - 1 - 40, v=8)] + \
             [(2, ents) for ents in seq_trio(3, v=8)]
    res, _ = run(groups, mem)
    assert res["nframes"] == 12


# ---- Partial version width -------------------------------------------------------------------

@pytest.mark.parametrize("mem", MEMS)
@rungs({"0": 0, "1": 1, "2^32-1": W - 1, "2^32": W, "2^32+1": W + 1, "2^63": 1 << 63, "2^64-1": U64})
def test_partial_version_width(rung, mem):
    v = rung
    res, _ = run([(0, [(0, [P(v, (0, 9))])]), (0, [(0, [P(v, (5, 14))])])], mem)
    assert res["nframes"] == 2 and res["nbytes"] == 2 * (52 + 16)


@pytest.mark.parametrize("mem", MEMS)
@rungs({"5": 5, "2^31": 1 << 31, "2^32-1": W - 1, "2^63-1": I63})
def test_versions_v_and_v_plus_2_32_do_not_dedupe(rung, mem):
    v = rung
    groups = [(0, [(0, [P(v, (0, 9)), P(v + W, (0, 9))])]), (0, [(0, [P(v + W, (5, 12)), P(v, (5, 12))])])]
    res, _ = run(groups, mem)
    assert res["nframes"] == 4


@pytest.mark.parametrize("mem", MEMS)
def test_version_0_partial_and_full_do_not_interact(mem):
    groups = [(0, [(0, [F(0, 5), P(0, (0, 5))])]), (0, [(0, [P(0, (3, 8)), F(3, 8)])])]
    res, _ = run(groups, mem)
    assert res["nframes"] == 4


# ---- sites -----------------------------------------------------------------------------------

@rungs({str(k): k for k in (1, 2, 3, 4, 5, 255, 256, 257)})
def test_site_count(rung):
    """A fresh engine of `rung` sites with random ids; needs on the lowest, a middle and the highest
    ordinal, and the frames carry that ordinal's registered bytes."""
    import corrosion_amd as ca
    ns = rung
    ids = np.random.default_rng(100 + ns).integers(0, 256, (ns, 16), dtype=np.uint8)
    assert len({bytes(r) for r in ids}) == ns
    e = ca.MergeEngine({"t": ["a"]}, capacity_hint=1024)
    try:
        assert list(e.register_sites(ids.reshape(-1))) == list(range(ns))
        ords = sorted({0, ns // 2, ns - 1})
        groups = [(0, [(o, [F(1, 25), P(2, (0, 9))]) for o in ords]), (0, [(o, [F(5, 30), P(2, (4, 12))]) for o in ords[::-1]])]
        for mem in MEMS:
            res, want = run(groups, mem, eng=e, sites=ids.tobytes())
            assert res["nframes"] >= 6 * len(ords)
            buf = res["buf"].tobytes()
            got = {buf[o + 16:o + 32] for o in res["frame_off"][:-1].tolist()}
            assert got == {bytes(ids[o]) for o in ords}
    finally:
        e.close()


# ---- groups and sessions ---------------------------------------------------------------------

@pytest.mark.parametrize("mem", MEMS)
@rungs({str(k): k for k in (1, 2, 3, 4, 5, 255, 256, 257)})
def test_sessions_of_one_server_each(rung, mem):
    """Every session asks the same actor for the same versions: nothing dedupes across sessions."""
    res, _ = run([(s, [(0, [F(1, 25), P(3, (0, 4))])]) for s in range(rung)], mem)
    assert res["nframes"] == 4 * rung


@pytest.mark.parametrize("mem", MEMS)
@pytest.mark.parametrize("drain", [1, 2])
def test_one_session_of_257_servers(drain, mem):
    """Round-robin over many ranks and many rounds; server i needs i ..= i + 30 and a Partial."""
    res, want = run([(9, [(0, [F(i, i + 30), P(1, (i, i + 3))])]) for i in range(257)], mem, drain=drain)
    assert max(want["frame_round"]) >= 4 // drain and res["nframes"] > 257


@pytest.mark.parametrize("mem", MEMS)
def test_session_values_with_gaps_up_to_2_64_minus_1(mem):
    """Equal needs in neighbouring sessions: a wrong first-group index would dedupe across them."""
    ses = [3, 3, 9, W, W, W + 1, 1 << 63, U64, U64]
    groups = [(s, [(0, [F(1, 25), P(3, (0, 4))]), (1, [F(1, 5)])]) for s in ses]
    res, _ = run(groups, mem, drain=2)
    assert res["nframes"] == 6 * 5


# ---- chunk and drain -------------------------------------------------------------------------

SPAN = [(0, [(0, [F(1000, 1100)])]), (0, [(0, [F(1040, 1060), F(1095, 1105)])])]


@pytest.mark.parametrize("mem", MEMS)
@rungs({"1": 1, "2": 2, "S-1": 99, "S": 100, "S+1": 101, "2^32": W, "2^63": 1 << 63, "2^64-1": U64})
def test_chunk_size(rung, mem):
    res, want = run(SPAN, mem, chunk=rung, drain=7)
    assert res["nframes"] >= 2


@pytest.mark.parametrize("mem", MEMS)
@rungs({"1": 1, "2": 2, "items-1": 10, "items": 11, "items+1": 12, "2^32-1": W - 1})
def test_drain(rung, mem):
    """The first server has 11 items at chunk 10."""
    assert len(M.chunk_range(1000, 1100, 10)) == 11
    res, want = run(SPAN, mem, chunk=10, drain=rung)
    assert max(want["frame_round"]) == (11 - 1) // rung


@pytest.mark.parametrize("mem", MEMS)
@rungs({"0": 0, "2^62": 1 << 62})
def test_wide_chunks(rung, mem):
    """(e - s) a multiple of a 2^36 chunk: 17 chunks, the last one version wide. The second server asks
    for B + c + 5 ..= B + 2c in round 0, before the first reaches that chunk in round 1."""
    B, c = rung, 1 << 36
    groups = [(0, [(0, [F(B, B + (1 << 40))])]), (0, [(0, [F(B + c + 5, B + 2 * c), F(B + (1 << 40), B + (1 << 40) + 1)])])]
    res, _ = run(groups, mem, chunk=c)
    assert res["nframes"] == 17 + 2


# ---- nested and repeated Partial ranges ------------------------------------------------------

def spread(ranges):
    """One Partial need per range, dealt to three servers of one session."""
    return [(0, [(2, [P(5, r) for r in ranges[k::3]])]) for k in range(3)]


NEST = [(k, 600 - k) for k in range(300)]
NESTED = {"one_need": [(0, [(2, [P(5, *NEST)])]), (0, [(2, [P(5, (250, 650))])])],
          "outermost_popped_last": spread(NEST[::-1]),
          "outermost_popped_first": spread(NEST),
          "identical": [(0, [(2, [P(5, *[(5, 50)] * 300)])]), (0, [(2, [P(5, (5, 50))] * 300)])],
          "staircase": spread([(k, k + 300) for k in range(300)])}


@pytest.mark.parametrize("mem", MEMS)
@rungs(NESTED)
def test_nested_partial_ranges(rung, mem):
    res, _ = run(rung, mem)
    assert res["nframes"] >= 1


# ---- shapes ----------------------------------------------------------------------------------

@pytest.mark.parametrize("mem", MEMS)
def test_empty_call(mem):
    res, _ = run([], mem)
    assert res["nframes"] == 0 and res["nbytes"] == 0
    assert res["frame_off"].tolist() == [0] and res["grp_frame_off"].tolist() == [0]


SHAPES = {
    "three_empty_groups": dict(groups=[(0, []), (0, []), (1, [])]),
    "three_empty_groups_among_entries": dict(groups=[(0, []), (0, []), (1, [])], lead=[(0, [F(1, 9)])], trail=[(1, [F(1, 9)])]),
    "empty_group_between_live_ones": dict(groups=[(7, [(0, [F(1, 25)])]), (7, []), (7, [(0, [F(5, 30)])])]),
    "entries_outside_every_group": dict(groups=[(0, [(0, [F(1, 25)])]), (1, [(0, [F(5, 30)])])],
                                        lead=[(0, [F(1, 100), P(4, (0, 9))]), (1, [])], trail=[(0, [F(1, 100), P(4, (0, 9))])]),
    "entry_without_needs": dict(groups=[(0, [(0, [F(1, 5)]), (1, []), (0, [F(3, 9)])]), (0, [(3, [])]), (0, [(0, [F(1, 12)])])]),
    "one_site_in_two_entries": dict(groups=[(0, [(0, [F(1, 15), P(2, (0, 5))]), (1, [F(1, 5)]), (0, [F(10, 30), P(2, (3, 9))])]),
                                            (0, [(0, [F(1, 40)])])]),
    "all_needs_start_after_end": dict(groups=[(0, [(0, [F(1, 25)])]), (0, [(0, [F(9, 3), F(I63, 0)]), (2, [F(8, 2)])]),
                                              (0, [(0, [F(5, 30)])])]),
    "empty_partial_takes_a_drain_slot": dict(groups=[(0, [(0, [F(1, 5)])]), (0, [(0, [P(4, (0, 3)), P(4), F(2, 5)])])], drain=2),
}


@pytest.mark.parametrize("mem", MEMS)
@rungs(SHAPES)
def test_shapes(rung, mem):
    run(mem=mem, **rung)


# ---- output writer ---------------------------------------------------------------------------

BIG = [(0, [(0, [F(1, 3), P(3, *[(20 * k, 20 * k + 7) for k in range(2100)]), F(10, 12)])])]


def raw_outs(nframes, nbytes, ngroups, mem, off=0):
    """0x5A-filled output arrays for the raw ABI, two elements longer than asked; buf starts `off`
    bytes past a 16-byte-aligned address with at least 64 guard bytes either side. Returns
    (corro_requests, the arrays by name, buf's offset in its store)."""
    outs = {"grp_frame_off": np.full(ngroups + 3, 0x5A5A5A5A5A5A5A5A, np.uint64), "buf": np.full(nbytes + 160, 0x5A, np.uint8),
            "frame_off": np.full(nframes + 3, 0x5A5A5A5A5A5A5A5A, np.uint64),
            "frame_entry": np.full(nframes + 2, 0x5A5A5A5A5A5A5A5A, np.uint64),
            "frame_round": np.full(nframes + 2, 0x5A5A5A5A, np.uint32), "frame_needs": np.full(nframes + 2, 0x5A5A5A5A, np.uint32)}
    held = to_dev(outs) if mem == "device" else outs
    o = L.Requests()
    for k, v in held.items():
        setattr(o, k, v.data_ptr() if mem == "device" else v.ctypes.data)
    lead = (-o.buf) % 16 + 64 + off
    assert lead + nbytes + 64 <= nbytes + 160
    o.buf += lead
    assert o.buf % 16 == off
    return o, held, lead


def fetch(held, mem):
    return {k: (v.cpu().numpy().view(np.uint8) if mem == "device" else v.view(np.uint8)) for k, v in held.items()}


def raw_plan(arr, mem, off=0, eng=None, dn=(0, 0), chunk=10, drain=10):
    """Both passes through the raw ABI, pass 1 told pass 0's sizes plus `dn`; returns (pass 1's return
    code, its frame bytes, the output arrays as bytes, buf's offset, (nframes, nbytes))."""
    G = len(arr["grp_session"])
    o, _held, _ = raw_outs(0, 0, G, mem)
    assert _raw(arr, chunk, drain, 0, o, mem, eng) == 0
    nf, nb = o.nframes, o.nbytes
    o, held, lead = raw_outs(nf, nb, G, mem, off)
    o.nframes, o.nbytes = nf + dn[0], nb + dn[1]
    rc = _raw(arr, chunk, drain, 1, o, mem, eng)
    got = fetch(held, mem)
    return rc, got["buf"][lead:lead + nb].tobytes(), got, lead, (nf, nb)


@pytest.mark.parametrize("mem", MEMS)
def test_frame_over_four_tiles(mem):
    """33,652 bytes in one frame, starting 56 bytes into the first tile and followed by a small frame."""
    res, _ = run(BIG, mem)
    assert res["frame_off"].tolist() == [0, 56, 56 + 52 + 16 * 2100, 112 + 52 + 16 * 2100]


@pytest.mark.parametrize("mem", MEMS)
@rungs({"8192": (8192, [P(9, (1, 2), (4, 5)), P(8, (1, 2), (4, 5), (7, 8))] + [F(20 * k, 20 * k + 3) for k in range(143)]),
        "8196": (8196, [P(9, *[(3 * k, 3 * k + 1) for k in range(5)])] + [F(20 * k, 20 * k + 3) for k in range(144)])})
def test_exact_totals(rung, mem):
    """One-piece Full frames are 56 bytes, a Partial of r ranges 52 + 16 r: a last tile that is full,
    and one of a single word."""
    total, needs = rung
    res, _ = run([(0, [(0, needs)])], mem)
    assert res["nbytes"] == total


@pytest.mark.parametrize("mem,off", [("device", 0), ("device", 1), ("device", 4), ("device", 8), ("device", 12), ("host", 1)])
def test_output_buffer_alignment(mem, off):
    """out->buf at `off` bytes past a 16-byte line (the writer's byte-store path on the device): the
    bytes equal the model's, so the aligned call's, and the 64 bytes before and after stay 0x5A."""
    arr = M.arrays(BIG)
    want = M.plan(arr, 10, 10, SITES)
    rc, frames, got, lead, (nf, nb) = raw_plan(arr, mem, off)
    assert rc == 0 and (nf, nb) == (3, len(want["group_bytes"][0]))
    assert frames == want["group_bytes"][0]
    assert bytes(got["buf"][:lead]) == b"\x5a" * lead and lead >= 64 + off
    rest = bytes(got["buf"][lead + nb:])
    assert rest == b"\x5a" * len(rest) and len(rest) >= 64
    assert got["frame_off"].view(np.uint64)[:nf + 1].tolist() == [0, 56, 56 + 33652, 112 + 33652]


# ---- pass protocol and reuse -----------------------------------------------------------------

SMALL = [(0, [(0, [F(1, 25), P(4, (0, 3), (8, 9))]), (1, [F(3, 4)])]), (0, [(0, [F(20, 30)])])]


@pytest.mark.parametrize("mem", MEMS)
@rungs({"nframes+1": (1, 0), "nframes-1": (-1, 0), "nbytes+1": (0, 1), "nbytes-1": (0, -1)})
def test_pass_1_refuses_other_sizes_and_writes_nothing(rung, mem):
    rc, _frames, got, _lead, (nf, nb) = raw_plan(M.arrays(SMALL), mem, dn=rung)
    assert rc == -1 and nf > 1 and nb > 1
    for k, v in got.items():
        assert bytes(v) == b"\x5a" * len(v), k


@pytest.mark.parametrize("mem", MEMS)
def test_pass_1_twice(mem):
    arr = M.arrays(SMALL)
    G = len(arr["grp_session"])
    o, _h, _ = raw_outs(0, 0, G, mem)
    assert _raw(arr, 10, 10, 0, o, mem) == 0
    nf, nb = o.nframes, o.nbytes
    seen = []
    for _ in range(2):
        o, held, lead = raw_outs(nf, nb, G, mem)
        o.nframes, o.nbytes = nf, nb
        assert _raw(arr, 10, 10, 1, o, mem) == 0
        seen.append({k: bytes(v) for k, v in fetch(held, mem).items()})
    assert seen[0] == seen[1]
    want = M.plan(arr, 10, 10, SITES)
    assert seen[0]["buf"][lead:lead + nb] == b"".join(want["group_bytes"])


@pytest.mark.parametrize("mem", MEMS)
def test_small_call_after_large_calls_equals_a_fresh_engine(mem):
    """Stale scratch: the same small call after the 33 KiB frame and after the 257-server session."""
    import corrosion_amd as ca
    small = M.arrays(SMALL)
    fresh = ca.MergeEngine({"t": ["a"]}, capacity_hint=1024)
    try:
        fresh.register_sites(np.frombuffer(SITES, np.uint8))
        first = plan(small, 10, 10, mem, fresh)
    finally:
        fresh.close()
    check(first, M.plan(small, 10, 10, SITES), 2)
    for large, drain in ((BIG, 10), ([(9, [(0, [F(i, i + 30), P(1, (i, i + 3))])]) for i in range(257)], 1)):
        run(large, mem, drain=drain)
        again = plan(small, 10, 10, mem)
        for k, v in first.items():
            assert np.array_equal(np.asarray(v), np.asarray(again[k])), k
