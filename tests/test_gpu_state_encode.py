"""GPU state encode (corro_encode_states, csrc/state_encode.hip) against the plain-Python restatement of
generate_sync and the host codec (tests/state_encode_model.py: W.frame(W.encode_sync_state(state))), byte
for byte, from host and from device memory; a real bookie's frame against Agent.generate_sync(); then the
chain: the encoder's device output through corro_decode_states against tests/state_model.py, and
requests_from_books against requests_from_state_frames on host-encoded frames.

One rule worth saying aloud: a partial with last_seq = 0 and nothing present, or one that misses seq 0 alone,
has the complement (0,0) within [0, last_seq], yet gets no entry. The reference's is_complete() looks at
1..=last_seq (agent.rs:1068-1074) and corro_generate_sync keeps that, so for byte equality with
Agent.generate_sync() such partials count as complete and are left out, on the device as on the host. The
seq cases below include them; their expected bytes are the model's, and SEQ_WANT spells them out."""
import random

import numpy as np
import pytest

from corrosion_amd import _lib as L
from corrosion_amd import sync as S
from corrosion_amd import wire as W
from tests import state_encode_model as EM
from tests import state_model as M

pytestmark = pytest.mark.gpu
MEMS = ["host", "device"]
U64 = (1 << 64) - 1
INVALID, RANGE = -1, -6
_ENGINE = {}
a = M.aid


def engine(name="main"):
    if name not in _ENGINE:
        import corrosion_amd as ca
        _ENGINE[name] = ca.MergeEngine({"t": ["a"]}, capacity_hint=1024)
    return _ENGINE[name]


def host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def encoder(states, me=None, ts=None, max_payload=0, mem="host"):
    me = me or [a(900 + b) for b in range(len(states))]
    return S._StateEnc(engine(), S.concat_books([EM.book_of_rows(r) for r in states]), me, ts, max_payload, mem == "device")


def run(states, me=None, ts=None, max_payload=0, mem="host"):
    """(frames as byte strings, statuses, the three counts) of one call."""
    me = me or [a(900 + b) for b in range(len(states))]
    book = S.concat_books([EM.book_of_rows(r) for r in states])
    res = S.state_frames_from_books(engine(), book, me, ts=ts, max_payload=max_payload, device=mem == "device")
    if mem == "device":
        assert all(res[k].is_cuda for k in ("buf", "frame_off", "state_status", "n_heads", "n_need", "n_partial"))
    buf, off = host(res["buf"]).tobytes(), [int(x) for x in host(res["frame_off"])]
    assert off[0] == 0 and off[-1] == res["total_bytes"] == len(buf) and len(off) == len(states) + 1
    out = {"frames": [buf[off[b]:off[b + 1]] for b in range(len(states))]}
    for k in ("state_status", "n_heads", "n_need", "n_partial"):
        out[k] = [int(x) for x in host(res[k])]
    return out


def check(states, me=None, ts=None, max_payload=0, mem="host", what=""):
    me = me or [a(900 + b) for b in range(len(states))]
    want = EM.encode_model(states, me, ts, max_payload)
    got = run(states, me, ts, max_payload, mem)
    for k in ("state_status", "n_heads", "n_need", "n_partial"):
        assert got[k] == want[k], (what, k)
    for b, (g, w) in enumerate(zip(got["frames"], want["frames"])):
        assert g == w, (what, b, len(g), len(w))
    return got


def head_rows(n, base=0, gaps=lambda i: [], parts=lambda i: []):
    return [(a(base + i), i + 1, gaps(i), parts(i)) for i in range(n)]


@pytest.mark.parametrize("mem", MEMS)
def test_states_without_a_head(mem):
    none = [(a(1), None, [], []), (a(2), None, [(1, 2)], [(3, 5, [(0, 1)])])]       # max = -1: nothing, whatever the row holds
    got = check([[], none], mem=mem)
    assert [len(f) for f in got["frames"]] == [4 + 8 + 16 + 12 + 1] * 2
    assert got["n_heads"] == [0, 0]
    check([[]], mem=mem, what="one state, no row")


@pytest.mark.parametrize("mem", MEMS)
def test_timestamps(mem):
    rows = head_rows(1)
    got = check([rows, rows, rows, []], ts=[None, 0, U64, 5], mem=mem)
    assert [len(f) for f in got["frames"]] == [65, 73, 73, 49]
    assert got["frames"][2][-9:] == b"\x01" + b"\xff" * 8


@pytest.mark.parametrize("mem", MEMS)
def test_need_and_partial_entries_follow_their_rows(mem):
    complete = [(4, 3, [(0, 3)]), (6, 5, [(1, 5)]), (7, 0, [])]                  # whole; missing seq 0 alone; last_seq 0
    rows = [(a(1), 10, [], []),                                                  # a head alone
            (a(2), 10, [(3, 4)], []),                                            # one gap
            (a(3), 10, [], complete),                                            # every partial complete: not in partial_need
            (a(4), 10, [(2, 2), (5, 9)], [(3, 3, [(0, 3)]), (8, 4, [(0, 1)])]),  # its neighbour is, with one of two versions
            (a(5), None, [(1, 1)], [(2, 9, [])])]
    got = check([rows], ts=[17], mem=mem)
    assert (got["n_heads"], got["n_need"], got["n_partial"]) == ([4], [2], [1])
    st = W.decode_sync_state(got["frames"][0][4:])
    assert list(st.heads) == [a(1), a(2), a(3), a(4)] and list(st.need) == [a(2), a(4)]
    assert st.partial_need == {a(4): {8: [(2, 4)]}}


SEQ_CASES = {
    "last_seq 0, nothing present": (0, []),
    "last_seq 0, seq 0 present": (0, [(0, 0)]),
    "last_seq 1, nothing present": (1, []),
    "a gap only at 0": (9, [(1, 9)]),
    "a gap at 0 and 1": (9, [(2, 9)]),
    "a gap only at the end": (9, [(0, 8)]),
    "a gap only in the middle": (9, [(0, 3), (6, 9)]),
    "gaps at 0, in the middle and at the end": (9, [(2, 3), (6, 7)]),
    "a present range clipped by last_seq": (9, [(0, 3), (7, 30)]),
    "a present range wholly past last_seq": (9, [(0, 3), (12, 30)]),
    "a present range that starts at last_seq": (9, [(0, 3), (9, 30)]),
    "one range past last_seq alone": (9, [(20, 30)]),
    "last_seq 2^64-1, present (0, 2^64-2)": (U64, [(0, U64 - 1)]),
    "last_seq 2^64-1, present (1, 2^64-1)": (U64, [(1, U64)]),
    "last_seq 2^64-1, present (2, 2^64-1)": (U64, [(2, U64)]),
    "last_seq 2^64-1, nothing present": (U64, []),
    "last_seq 2^64-1, all present": (U64, [(0, U64)]),
}
SEQ_WANT = {"last_seq 0, nothing present": None, "last_seq 0, seq 0 present": None, "last_seq 1, nothing present": [(0, 1)],
            "a gap only at 0": None, "a gap at 0 and 1": [(0, 1)], "a gap only at the end": [(9, 9)],
            "a gap only in the middle": [(4, 5)], "a present range clipped by last_seq": [(4, 6)],
            "last_seq 2^64-1, present (0, 2^64-2)": [(U64, U64)], "last_seq 2^64-1, present (1, 2^64-1)": None,
            "last_seq 2^64-1, present (2, 2^64-1)": [(0, 1)], "last_seq 2^64-1, all present": None}


@pytest.mark.parametrize("mem", MEMS)
@pytest.mark.parametrize("case", list(SEQ_CASES))
def test_seq_gaps_of_one_partial(case, mem):
    last, present = SEQ_CASES[case]
    # (a second, plainly incomplete version keeps the actor's entry there whatever the first one gives)
    got = check([[(a(1), 9, [], [(5, last, present), (6, 2, [(0, 0)])])]], mem=mem, what=case)
    versions = W.decode_sync_state(got["frames"][0][4:]).partial_need[a(1)]
    assert versions[6] == [(1, 2)]
    if case in SEQ_WANT:                            # the model's answer, said aloud
        assert versions.get(5) == SEQ_WANT[case], case
    check([[(a(1), 9, [], [(5, last, present)])]], mem=mem, what=case + ", alone")


@pytest.mark.parametrize("mem", MEMS)
def test_every_parallel_boundary(mem):
    many_rows = head_rows(300, gaps=lambda i: [(2, 3)] if i % 3 == 0 else [],
                          parts=lambda i: [(7, 9, [(0, i % 9)])] if i % 8 == 0 else [])
    check([many_rows], mem=mem, what="300 rows in one state")
    check([[(a(1), 5000, [(10 * j + 1, 10 * j + 3 + j % 5) for j in range(300)], [])]], mem=mem, what="300 gaps in one row")
    present = [(3 * j + 1, 3 * j + 1 + j % 2) for j in range(299)]
    got = check([[(a(1), 9, [], [(5, 3 * 299 + 5, present)])]], ts=[3], mem=mem, what="300 seq gaps in one partial")
    assert len(W.decode_sync_state(got["frames"][0][4:]).partial_need[a(1)][5]) == 300
    check([[(a(1), 9, [], [(v, 9, [(0, v % 9)]) for v in range(1, 301)])]], mem=mem, what="300 partials in one row")
    ones = [[(a(b), b + 1, [(1, 1)] if b % 2 else [], [(b + 1, 5, [])] if b % 3 == 0 else [])] for b in range(300)]
    got = check(ones, ts=[b if b % 4 == 0 else None for b in range(300)], mem=mem, what="300 one-row states")
    assert {len(f) % 4 for f in got["frames"]} == {1}                # so the frames lie at every alignment
    other = head_rows(257, base=500, gaps=lambda i: [(1, i + 1)], parts=lambda i: [(3, 8, [(2, 4)])] if i % 2 else [])
    got = check([many_rows, [], other], mem=mem, what="an empty state between two large ones")
    assert len(got["frames"][1]) == 41


BAD_ROWS = {
    "a gap inverted": [(a(1), 9, [(4, 3)], [])],
    "gaps unsorted": [(a(1), 9, [(6, 7), (2, 3)], [])],
    "gaps overlapping": [(a(1), 9, [(2, 5), (5, 7)], [])],
    "gaps touching": [(a(1), 9, [(2, 4), (5, 7)], [])],
    "a later row's first gap below the one before it is fine, its second is not": [(a(1), 9, [(5, 6)], []), (a(2), 9, [(1, 2), (3, 3)], [])],
    "a present range inverted": [(a(1), 9, [], [(5, 9, [(3, 2)])])],
    "present ranges unsorted": [(a(1), 9, [], [(5, 9, [(6, 7), (0, 1)])])],
    "present ranges overlapping": [(a(1), 9, [], [(5, 9, [(0, 3), (2, 7)])])],
    "present ranges touching": [(a(1), 9, [], [(5, 9, [(0, 3), (4, 7)])])],
    "a present range behind one that ends at 2^64-1": [(a(1), 9, [], [(5, 9, [(0, U64), (0, 1)])])],
    "partial versions equal": [(a(1), 9, [], [(5, 9, []), (5, 9, [(0, 1)])])],
    "partial versions descending": [(a(1), 9, [], [(6, 9, []), (5, 9, [])])],
    "not canonical in a row without a head": [(a(1), None, [(4, 3)], [])],
}


@pytest.mark.parametrize("mem", MEMS)
@pytest.mark.parametrize("case", list(BAD_ROWS))
def test_a_state_that_is_not_canonical_is_left_out(case, mem):
    first = head_rows(5, gaps=lambda i: [(1, 2), (9, 9)], parts=lambda i: [(4, 9, [(0, 3)])])
    last = head_rows(3, base=50, gaps=lambda i: [(7, 8)], parts=lambda i: [(2, 5, []), (3, 5, [(1, 1)])])
    # (rows of the same forms on both sides: a flag of the middle state must not leak through a scan)
    got = check([first, BAD_ROWS[case], last], ts=[1, 2, 3], mem=mem, what=case)
    assert got["state_status"] == [0, INVALID, 0] and got["frames"][1] == b""
    alone = check([first, last], me=[a(900), a(902)], ts=[1, 3], mem=mem)
    assert [got["frames"][0], got["frames"][2]] == alone["frames"]


def _with_offsets(states, change):
    book = S.concat_books([EM.book_of_rows(r) for r in states])
    change(book)
    return book


@pytest.mark.parametrize("mem", MEMS)
@pytest.mark.parametrize("key", ["gap_off", "part_off", "psr_off"])
def test_an_offset_array_that_decreases_inside_a_state(key, mem):
    rows = lambda base: head_rows(3, base=base, gaps=lambda i: [(1, 2), (5, 6)], parts=lambda i: [(4, 9, [(0, 1), (4, 5)]), (6, 9, [(3, 3)])])
    states, me = [rows(0), rows(10), rows(20)], [a(900), a(901), a(902)]

    def swap(book):                                  # the middle state's second offset passes its third
        at = {"gap_off": 4, "part_off": 4, "psr_off": 7}[key]
        book[key][at] += 3
    book = _with_offsets(states, swap)
    res = S.state_frames_from_books(engine(), book, me, device=mem == "device")
    assert [int(x) for x in host(res["state_status"])] == [0, INVALID, 0]
    off, buf = [int(x) for x in host(res["frame_off"])], host(res["buf"]).tobytes()
    want = EM.encode_model([states[0], states[2]], [me[0], me[2]])["frames"]
    assert off[1] == off[2] and [buf[off[0]:off[1]], buf[off[2]:off[3]]] == want


@pytest.mark.parametrize("mem", MEMS)
def test_max_payload(mem):
    rows = head_rows(7, gaps=lambda i: [(1, 2)] * (i % 2), parts=lambda i: [(4, 9, [(0, 3)])] if i == 3 else [])
    size = len(W.encode_sync_state(EM.generate_sync(rows, a(901), 5)))
    small = head_rows(1)
    got = check([small, rows, small], ts=[None, 5, None], max_payload=size, mem=mem)
    assert got["state_status"] == [0, 0, 0] and len(got["frames"][1]) == size + 4
    got = check([small, rows, small], ts=[None, 5, None], max_payload=size - 1, mem=mem)
    assert got["state_status"] == [0, RANGE, 0] and got["frames"][1] == b"" and len(got["frames"][2]) == 65
    bad = rows + [(a(99), 9, [(4, 3)], [])]                          # both: CORRO_E_INVALID goes first
    got = check([small, bad, small], ts=[None, 5, None], max_payload=40, mem=mem)
    assert got["state_status"] == [RANGE, INVALID, RANGE]
    check([small, rows], ts=[None, 5], max_payload=100 << 20, mem=mem, what="the reference's 100 MiB")
    check([small, rows], ts=[None, 5], max_payload=1 << 40, mem=mem, what="above 2^32 - 1")


@pytest.mark.parametrize("mem", MEMS)
def test_pass_1_with_another_total_is_refused(mem):
    enc = encoder([head_rows(3), head_rows(2, base=9)], mem=mem)
    assert enc.total_bytes == 32 + 3 * 24 + 9 + 32 + 2 * 24 + 9
    for wrong in (enc.total_bytes - 1, enc.total_bytes + 1, 0):
        buf = enc.alloc(enc.total_bytes + 8, np.uint8)
        buf[:] = 7
        enc.o.total_bytes = wrong
        with pytest.raises(L.CorroError) as e:
            enc.write(buf)
        assert e.value.code == -1 and "total_bytes" in str(e.value)
        assert (host(buf) == 7).all()                                # a refused call writes nothing
    enc.o.total_bytes = enc.total_bytes
    buf = enc.alloc(enc.total_bytes + 8, np.uint8)
    buf[:] = 7
    out = host(enc.write(buf)).tobytes()
    assert out == b"".join(EM.encode_model([head_rows(3), head_rows(2, base=9)], [a(900), a(901)])["frames"])
    assert (host(buf)[enc.total_bytes:] == 7).all()                  # and a served one nothing past its bytes


def test_bad_global_offsets_in_device_memory_fail_the_call():
    """Host arrays are screened on the host (tests/test_abi_state_encode.py); device arrays by the check kernel."""
    states = [head_rows(3, gaps=lambda i: [(1, 2)]), head_rows(2, base=9)]
    for key, at, delta in (("state_row_off", 1, 3), ("state_row_off", 2, 1), ("gap_off", 5, 1), ("part_off", 5, 1),
                           ("psr_off", 0, 1)):
        def change(book):
            book[key][at] += delta
        with pytest.raises(L.CorroError) as e:
            S.state_frames_from_books(engine(), _with_offsets(states, change), [a(900), a(901)], device=True)
        assert e.value.code == -1 and "state_row_off" in str(e.value), key


@pytest.mark.parametrize("device", [False, True])
def test_a_real_bookie(device):
    from tests.state_encode_util import mixed_agent
    ag = mixed_agent()
    for ts in (None, 1 << 40):
        st = ag.generate_sync()
        st.last_cleared_ts = ts
        got = ag.generate_sync_frame(last_cleared_ts=ts, device=device)
        assert device == hasattr(got, "is_cuda")
        assert (host(got).tobytes() if device else got) == W.frame(W.encode_sync_state(st))
    assert st.need and st.partial_need and len(st.heads) > len(st.need)


def random_rows(rng, universe):
    rows = []
    for actor in sorted(rng.sample(universe, rng.randint(0, len(universe)))):
        pts = sorted(rng.sample(range(1, 200), 2 * rng.randint(0, 3)))
        gaps = [(pts[2 * i], pts[2 * i + 1]) for i in range(len(pts) // 2) if i == 0 or pts[2 * i] > pts[2 * i - 1] + 1]
        parts = []
        for v in sorted(rng.sample(range(1, 60), rng.randint(0, 3))):
            last = rng.randint(0, 40)
            q = sorted(rng.sample(range(0, 60), 2 * rng.randint(0, 3)))
            present = [(q[2 * i], q[2 * i + 1]) for i in range(len(q) // 2) if i == 0 or q[2 * i] > q[2 * i - 1] + 1]
            parts.append((v, last, present))
        rows.append((actor, None if rng.random() < 0.1 else rng.randint(0, 300), gaps, parts))
    return rows


def random_states(seed, n):
    rng = random.Random(seed)
    universe = [a(i) for i in range(14)]
    states = [random_rows(rng, universe) for _ in range(n)]
    me = [rng.choice(universe) if rng.random() < 0.5 else a(100 + b) for b in range(n)]
    ts = [rng.choice([None, 0, 77, U64]) for _ in range(n)]
    return states, me, ts


@pytest.mark.parametrize("mem", MEMS)
def test_random_states(mem):
    states, me, ts = random_states(11, 40)
    assert all(EM.rows_canonical(r) for r in states)
    got = check(states, me, ts, mem=mem)
    assert sum(got["n_partial"]) > 10 and sum(got["n_need"]) > 10 and 0 in got["n_heads"]


def test_round_trip_through_the_decoder():
    """The encoder's device output, unchanged, into corro_decode_states: the entries the decoder's model gives
    for the host codec's frames (every version below 2^63)."""
    states, me, ts = random_states(5, 12)
    eng = engine("bare")                                             # no site registered: every entry_site is NONE
    fr = S.state_frames_from_books(eng, S.concat_books([EM.book_of_rows(r) for r in states]), me, ts=ts, device=True)
    pairs = [(i, j) for i in range(12) for j in range(12) if (i + j) % 3 != 1]
    got = S.entries_from_state_frames(eng, fr["buf"], fr["frame_off"], pairs, device=True)
    want = M.decode_model(EM.encode_model(states, me, ts)["frames"], pairs)
    assert (want["frame_status"] == 0).all() and len(want["their_head"]) > 50 and len(want["tps_start"]) > 10
    M.assert_same(got, want)


def test_requests_from_books_match_the_host_encoded_chain():
    import torch
    states, me, ts = random_states(21, 9)
    sessions = [(0, [1, 2, 3]), (4, [5]), (6, [7, 8, 0])]
    eng = engine("chain")
    got = S.requests_from_books(eng, [EM.book_of_rows(r) for r in states], me, sessions, ts=ts)
    buf, off = M.join(EM.encode_model(states, me, ts)["frames"])
    want = S.requests_from_state_frames(eng, torch.from_numpy(np.frombuffer(buf, np.uint8).copy()).cuda(), off, sessions)
    assert got["nframes"] == want["nframes"] > 5 and got["nbytes"] == want["nbytes"]
    for k in ("buf", "frame_off", "grp_frame_off", "frame_round", "frame_needs", "pair_status"):
        assert np.array_equal(host(got[k]), host(want[k])), k
    assert got["groups"] == want["groups"] and (host(got["state_status"]) == 0).all()
