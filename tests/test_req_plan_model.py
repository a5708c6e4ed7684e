"""CPU checks of the request planner's interval model (tests/req_plan_model.py) before it judges the
kernel: the hand-derived KATs, equality with the set oracle (tests/sync_req_util.py) wherever that
one can go, and hand-written answers where it cannot (values past 2^32, spans of 2^40, and the shapes
only the ABI arrays can express)."""
import pytest

from tests import req_plan_model as M
from tests import sync_req_util as U
from tests.test_sync_requests import KATS, kat_expect, kat_servers

SITES = b"".join(U.ACTORS)
SITE_OF = {a: i for i, a in enumerate(U.ACTORS)}
A0, A1 = U.ACTORS[0], U.ACTORS[1]
W, U64 = 1 << 32, (1 << 64) - 1


def F(a, b):
    return ("F", a, b)


def P(v, *seqs):
    return ("P", v, tuple(seqs))


def answer(per_group):
    """The model's result written by hand: per group its frames (round, entry, actor, needs)."""
    out = {"group_bytes": [], "frame_entry": [], "frame_round": [], "frame_needs": [], "grp_frame_off": [0]}
    for fr in per_group:
        out["group_bytes"].append(b"".join(U.frame_bytes(a, nds) for _r, _e, a, nds in fr))
        out["frame_entry"] += [e for _r, e, _a, _n in fr]
        out["frame_round"] += [r for r, _e, _a, _n in fr]
        out["frame_needs"] += [len(n) for _r, _e, _a, n in fr]
        out["grp_frame_off"].append(len(out["frame_entry"]))
    return out


def test_ranges():
    r = M.Ranges()
    assert r.minus(3, 9) == [(3, 9)] and r.minus(5, 4) == []
    r.insert(10, 20)
    r.insert(30, 40)
    assert r.minus(0, 50) == [(0, 9), (21, 29), (41, 50)]
    assert r.minus(10, 20) == [] and r.minus(15, 35) == [(21, 29)] and r.minus(20, 21) == [(21, 21)]
    r.insert(21, 28)                                  # touches on the left only
    assert r.items() == [(10, 28), (30, 40)]
    r.insert(29, 29)                                  # bridges
    assert r.items() == [(10, 40)]
    r.insert(0, 8)
    assert r.items() == [(0, 8), (10, 40)]
    r.insert(5, 100)
    assert r.items() == [(0, 100)]
    big = M.Ranges()
    big.insert(0, 1 << 62)
    big.insert((1 << 63), U64 - 1)
    assert big.minus(0, U64 - 1) == [((1 << 62) + 1, (1 << 63) - 1)]


def test_chunk_range_quirk():
    assert M.chunk_range(1, 25, 10) == [(1, 11), (11, 21), (21, 25)]
    assert M.chunk_range(1, 11, 10) == [(1, 11), (11, 11)]
    assert M.chunk_range(5, 4, 10) == []
    assert M.chunk_range(7, 7, U64) == [(7, 7)]
    c = M.chunk_range(0, 1 << 40, 1 << 36)
    assert len(c) == 17 and c[0] == (0, 1 << 36) and c[-1] == (1 << 40, 1 << 40)


@pytest.mark.parametrize("kat", KATS["kats"], ids=[k["name"] for k in KATS["kats"]])
def test_kats(kat):
    servers = kat_servers(kat)
    arr, groups = U.flatten([servers], SITE_OF)
    assert [sv for _sn, sv, _e in groups] == list(range(len(servers)))   # no KAT has an empty server
    assert all(len(ents) == 1 for ents in servers)                       # and each one entry: its server's number
    want = answer([[(r, sv, a, nds) for r, a, nds in fr] for sv, fr in enumerate(kat_expect(kat))])
    assert M.plan(arr, kat["chunk"], kat["drain"], SITES) == want


@pytest.mark.parametrize("chunk,drain", [(10, 10), (3, 2), (1, 1), (10, 1), (1, 10)])
def test_equals_the_set_oracle_on_the_random_sessions(chunk, drain):
    """All 300 sessions in one call, as the GPU file passes them, and each on its own."""
    sessions = U.random_sessions()
    assert len(sessions) == 300
    arr, groups = U.flatten(sessions, SITE_OF)
    assert M.plan(arr, chunk, drain, SITES) == U.expected(sessions, groups, chunk, drain)
    for servers in sessions:
        a1, g1 = U.flatten([servers], SITE_OF)
        assert M.plan(a1, chunk, drain, SITES) == U.expected([servers], g1, chunk, drain)


def test_equals_the_set_oracle_on_the_quirk_and_tile_sessions():
    big, many, edge = U.tile_edge_sessions()
    for sessions in (U.quirk_sessions(), [big], [many], [edge], [big, many, edge, big]):
        arr, groups = U.flatten(sessions, SITE_OF)
        assert M.plan(arr, 10, 10, SITES) == U.expected(sessions, groups, 10, 10)


def test_full_across_the_word_line():
    arr = M.arrays([(0, [(0, [F(W - 2, W + 8)])]), (0, [(0, [F(W - 5, W + 20)])])])
    want = answer([[(0, 0, A0, [F(W + 8, W + 8)]), (0, 0, A0, [F(W - 2, W + 7)])],
                   [(0, 1, A0, [F(W + 15, W + 20)]), (0, 1, A0, [F(W + 9, W + 14)]), (0, 1, A0, [F(W - 5, W - 3)])]])
    assert M.plan(arr, 10, 10, SITES) == want


def test_full_wide_chunks():
    """0 ..= 2^40 at chunk 2^36: 17 chunks, the last the single version 2^40; popped from the back."""
    c = 1 << 36
    arr = M.arrays([(0, [(1, [F(0, 1 << 40)])])])
    frames = [(0, 0, A1, [F(1 << 40, 1 << 40)])]
    frames += [(0 if k >= 7 else 1, 0, A1, [F(k * c, (k + 1) * c - 1)]) for k in range(15, -1, -1)]
    assert [r for r, *_ in frames] == [0] * 10 + [1] * 7
    assert M.plan(arr, c, 10, SITES) == answer([frames])


def test_partial_at_the_top_version_and_seq():
    arr = M.arrays([(0, [(0, [P(U64, (U64 - 12, U64 - 1 - 1), (3, 4))])]), (0, [(0, [P(U64, (U64 - 20, U64 - 6))])])])
    want = answer([[(0, 0, A0, [P(U64, (3, 4), (U64 - 12, U64 - 2))])], [(0, 1, A0, [P(U64, (U64 - 20, U64 - 13))])]])
    assert M.plan(arr, 10, 10, SITES) == want
    with pytest.raises(ValueError):
        M.plan(M.arrays([(0, [(0, [P(1, (0, U64))])])]), 10, 10, SITES)
    with pytest.raises(ValueError):
        M.plan(M.arrays([(0, [(0, [F(0, 1 << 63)])])]), 10, 10, SITES)


def test_versions_that_differ_in_bit_32_keep_their_own_books():
    v = 5
    arr = M.arrays([(0, [(0, [P(v, (0, 9)), P(v + W, (0, 9))])]), (0, [(0, [P(v + W, (5, 12)), P(v, (5, 12))])])])
    want = answer([[(0, 0, A0, [P(v + W, (0, 9))]), (0, 0, A0, [P(v, (0, 9))])],
                   [(0, 1, A0, [P(v, (10, 12))]), (0, 1, A0, [P(v + W, (10, 12))])]])
    assert M.plan(arr, 10, 10, SITES) == want


def test_version_0_partial_and_full_are_different_books():
    arr = M.arrays([(0, [(0, [F(0, 5), P(0, (0, 5))])]), (0, [(0, [P(0, (3, 8)), F(3, 8)])])])
    want = answer([[(0, 0, A0, [P(0, (0, 5))]), (0, 0, A0, [F(0, 5)])],
                   [(0, 1, A0, [F(6, 8)]), (0, 1, A0, [P(0, (6, 8))])]])
    assert M.plan(arr, 10, 10, SITES) == want


def test_abi_only_shapes():
    """Entries outside every group, an empty group between live ones, an entry without needs, one site
    in two entries of a server, needs with start > end, an empty Partial that takes a drain slot, and
    grp_session values that are not 0..k."""
    groups = [(7, [(0, [F(1, 5)]), (1, []), (0, [F(3, 9)])]),          # entries 1, 2, 3
              (7, []),
              (7, [(0, [F(1, 12), F(9, 3)])]),                         # entry 4
              (U64, [(0, [F(1, 5)]), (2, [F(8, 2), F(6, 1)])]),        # entries 5, 6: a new session
              (U64, [(0, [P(4, (0, 3)), P(4), F(2, 5)])])]             # entry 7
    arr = M.arrays(groups, lead=[(0, [F(1, 100)])], trail=[(0, [F(1, 100), P(4, (0, 9))])])
    assert arr["grp_ent_off"].tolist() == [1, 4, 4, 5, 7, 8] and len(arr["site"]) == 9
    want = answer([[(0, 3, A0, [F(3, 9)]), (0, 1, A0, [F(1, 2)])],
                   [],
                   [(0, 4, A0, [F(11, 12)]), (0, 4, A0, [F(10, 10)])],
                   [(0, 5, A0, [F(1, 5)])],
                   [(1, 7, A0, [P(4, (0, 3))])]])
    # drain 2: the last group pops F(2, 5) (all of it requested) and the empty Partial in round 0
    assert M.plan(arr, 10, 2, SITES) == want
    empty = M.arrays([])
    assert M.plan(empty, 10, 10, SITES) == answer([])
    assert M.plan(M.arrays([(0, []), (0, []), (1, [])]), 10, 10, SITES) == answer([[], [], []])
    with pytest.raises(ValueError):
        M.plan(M.arrays([(1, [(0, [F(1, 2)])]), (0, [(0, [F(1, 2)])])]), 10, 10, SITES)
    with pytest.raises(ValueError):
        M.plan(M.arrays([(0, [(4, [F(1, 2)])])]), 10, 10, SITES)


def test_round_robin_ranks_and_rounds():
    """Three servers, drain 1: the ranks take turns, and a server that runs out leaves the rotation."""
    arr = M.arrays([(3, [(0, [F(1, 25)])]), (3, [(0, [F(1, 5)])]), (3, [(0, [F(1, 25)])])])
    want = answer([[(0, 0, A0, [F(21, 25)]), (1, 0, A0, [F(11, 20)]), (2, 0, A0, [F(6, 10)])],
                   [(0, 1, A0, [F(1, 5)])],
                   []])
    assert M.plan(arr, 10, 1, SITES) == want


def test_ten_deep_nested_partial_book():
    inner = [(0, [(0, [P(9, (9 - k, 11 + k))])]) for k in range(10)]
    want = answer([[(0, 0, A0, [P(9, (9, 11))])]] +
                  [[(0, k, A0, [P(9, (9 - k, 9 - k), (11 + k, 11 + k))])] for k in range(1, 10)])
    assert M.plan(M.arrays(inner), 10, 10, SITES) == want
    outer = inner[::-1]
    assert M.plan(M.arrays(outer), 10, 10, SITES) == answer([[(0, 0, A0, [P(9, (0, 20))])]] + [[]] * 9)
    one = M.arrays([(0, [(0, [P(9, *[(9 - k, 11 + k) for k in range(10)])])])])
    assert M.plan(one, 10, 10, SITES) == answer([[(0, 0, A0, [P(9, (0, 20))])]])


def test_wide_values_are_cheap():
    """2^62-wide needs and books of a thousand ranges: nothing is per integer."""
    arr = M.arrays([(0, [(0, [F(0, 1 << 62)])]), (0, [(0, [F(5, (1 << 62) + 5)])])])
    got = M.plan(arr, 1 << 58, 100, SITES)
    assert got["grp_frame_off"] == [0, 17, 19] and got["frame_needs"] == [1] * 19
    seqs = [(k << 40, (k << 40) + (1 << 39)) for k in range(1000)]
    arr = M.arrays([(0, [(0, [P(1, *seqs)])]), (0, [(0, [P(1, (0, 1 << 62))])])])
    got = M.plan(arr, 10, 10, SITES)
    assert got["frame_needs"] == [1, 1] and len(got["group_bytes"][1]) == 4 * 13 + 16 * 1000
