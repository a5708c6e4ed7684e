"""CPU checks of the sync request planner's test oracle (tests/sync_req_util.py) and of the host codec
(wire.encode_sync_request / decode_sync_request): the oracle reproduces the hand-derived answers of
tests/golden/sync_request_kats.json before it is used to judge the kernel."""
import numpy as np
import pytest

from corrosion_amd import sync as S
from corrosion_amd import wire as W
from tests import sync_req_util as U
from tests._util import load_golden

KATS = load_golden("sync_request_kats.json")
A = bytes.fromhex(KATS["actor"])


def kat_need(nd):
    return ("F", nd[1], nd[2]) if nd[0] == "F" else ("P", nd[1], tuple(tuple(r) for r in nd[2]))


def kat_servers(kat):
    return [[(A, [kat_need(nd) for nd in needs]) for _a, needs in ents] for ents in kat["servers"]]


def kat_expect(kat):
    return [[(r, A, [kat_need(nd) for nd in needs]) for r, _a, needs in frames] for frames in kat["expect"]]


@pytest.mark.parametrize("kat", KATS["kats"], ids=[k["name"] for k in KATS["kats"]])
def test_oracle_reproduces_kat(kat):
    got = U.plan_session(kat_servers(kat), kat["chunk"], kat["drain"])
    assert [[(r, a, nds) for r, _e, a, nds in fr] for fr in got] == kat_expect(kat)


def test_chunk_range_quirk():
    assert U.chunk_range(1, 25, 10) == [(1, 11), (11, 21), (21, 25)]
    assert U.chunk_range(1, 11, 10) == [(1, 11), (11, 11)]
    assert U.chunk_range(5, 4, 10) == []


def test_known_frame_bytes():
    want = bytes.fromhex(KATS["full_12_20_frame_hex"])
    assert len(want) == 56
    payload = W.encode_sync_request(A, [S.Full(12, 20)])
    assert len(payload) == 52
    assert W.frame(payload) == want
    assert U.frame_bytes(A, [("F", 12, 20)]) == want


def test_codec_round_trip_random():
    rng = np.random.default_rng(5)
    for _ in range(200):
        needs = []
        for _ in range(int(rng.integers(0, 6))):
            if rng.random() < 0.5:
                s = int(rng.integers(0, 2**63, dtype=np.uint64))
                needs.append(S.Full(s, s + int(rng.integers(0, 1000))))
            else:
                seqs = tuple((int(s), int(s) + int(rng.integers(0, 99))) for s in rng.integers(0, 2**40, int(rng.integers(0, 5))))
                needs.append(S.Partial(int(rng.integers(0, 2**62)), seqs))
        actor = bytes(rng.integers(0, 256, 16, dtype=np.uint8))
        payload = W.encode_sync_request(actor, needs)
        assert W.decode_sync_request(payload) == [(actor, needs)]
        oracle_needs = [("F", n.start, n.end) if isinstance(n, S.Full) else ("P", n.version, n.seqs) for n in needs]
        assert U.frame_bytes(actor, oracle_needs) == W.frame(payload)
    for bad in (b"", b"\0" * 8, W.encode_sync_request(A, [S.Full(1, 2)])[:-1], W.encode_sync_request(A, []) + b"x",
                b"\0\0\0\0\1\0\0\0"):                                   # SyncMessageV1::Changeset
        with pytest.raises(ValueError):
            W.decode_sync_request(bad)


def test_oracle_invariants_random_sessions():
    rng = np.random.default_rng(11)
    sessions = U.random_sessions()
    assert len(sessions) == 300
    for servers in sessions:
        chunk, drain = int(rng.choice([1, 3, 10])), int(rng.choice([1, 2, 10]))
        plan = U.plan_session(servers, chunk, drain)
        want_full, want_part, got_full, got_part = {}, {}, {}, {}
        for ents in servers:
            for actor, needs in ents:
                for nd in needs:
                    if nd[0] == "F":
                        want_full.setdefault(actor, set()).update(range(nd[1], nd[2] + 1))
                    else:
                        for a, b in nd[2]:
                            want_part.setdefault((actor, nd[1]), set()).update(range(a, b + 1))
        for frames in plan:
            rounds = [r for r, _e, _a, _n in frames]
            assert rounds == sorted(rounds)
            for _r, _e, actor, needs in frames:
                assert needs
                for nd in needs:
                    if nd[0] == "F":
                        assert nd[2] - nd[1] + 1 <= chunk + 1           # every Full piece is <= chunk + 1 wide
                        vs = set(range(nd[1], nd[2] + 1))
                        seen = got_full.setdefault(actor, set())
                        assert not (vs & seen)                          # no version in two Full requests
                        seen |= vs
                    else:
                        assert len(needs) == 1
                        for a, b in nd[2]:
                            vs = set(range(a, b + 1))
                            seen = got_part.setdefault((actor, nd[1]), set())
                            assert not (vs & seen)
                            seen |= vs
        assert got_full == {k: v for k, v in want_full.items() if v}    # the union of requests = the union of needs
        assert got_part == {k: v for k, v in want_part.items() if v}


def test_requests_csr_matches_oracle_flatten():
    """The product's flattening of {actor: needs} maps and the oracle's agree on the arrays."""
    sessions = U.random_sessions(20, seed=3)
    site_of = {a: i for i, a in enumerate(U.ACTORS)}
    want, groups = U.flatten(sessions, site_of)
    as_maps = [[{a: [S.Full(n[1], n[2]) if n[0] == "F" else S.Partial(n[1], n[2]) for n in nds] for a, nds in ents}
                for ents in servers] for servers in sessions]
    got, ggroups = S.requests_csr(as_maps, site_of.__getitem__)
    assert ggroups == [(sn, sv) for sn, sv, _e in groups]
    for k in want:
        assert np.array_equal(got[k], want[k]), k
