"""CPU checks of the State wire layout: wire.encode_sync_state / decode_sync_state round-trip, and the
plain-Python model of corro_decode_states (tests/state_model.py) against sync.entries_from_states on the
decoded dataclasses and on the malformed list."""
import random

import numpy as np
import pytest

from corrosion_amd import sync as S
from corrosion_amd import wire as W
from tests import state_model as M

PAIRS = M.random_pairs(20260, 200)


def test_round_trip_on_seeded_states():
    for ours, theirs in PAIRS:
        for st in (ours, theirs):
            back = W.decode_sync_state(W.encode_sync_state(st))
            assert back == st
            assert [list(m) for m in (back.heads, back.need, back.partial_need)] == [
                list(m) for m in (st.heads, st.need, st.partial_need)]           # wire order = dict order
            assert [list(p) for p in back.partial_need.values()] == [list(p) for p in st.partial_need.values()]


def test_layout_by_hand():
    st = S.SyncStateV1(actor_id=bytes(range(16)), heads={b"A" * 16: 3}, need={b"B" * 16: [(1, 2)]},
                       partial_need={b"C" * 16: {9: [(4, 5)]}}, last_cleared_ts=6)
    u32, u64 = (lambda x: x.to_bytes(4, "little")), (lambda x: x.to_bytes(8, "little"))
    want = (u32(0) + u32(0) + bytes(range(16)) + u32(1) + b"A" * 16 + u64(3) + u32(1) + b"B" * 16 + u32(1) + u64(1) + u64(2) +
            u32(1) + b"C" * 16 + u32(1) + u64(9) + u32(1) + u64(4) + u64(5) + b"\x01" + u64(6))
    assert W.encode_sync_state(st) == want
    st.last_cleared_ts = None
    assert W.encode_sync_state(st) == want[:-9] + b"\x00"
    assert W.decode_sync_state(want[:-9]) == st                                # default_on_eof
    assert W.frame(want)[:4] == len(want).to_bytes(4, "big")


def test_decode_refuses_what_is_not_one_state():
    good = W.encode_sync_state(PAIRS[0][1])
    for bad in (good[:-3], good + b"\0", b"\0\0\0\0\x04\0\0\0" + good[8:], good[:-1] + b"\x02" if good[-1:] == b"\0" else
                good[:-9] + b"\x02"):
        with pytest.raises(ValueError):
            W.decode_sync_state(bad)
    with pytest.raises(ValueError):
        W.encode_sync_state(S.SyncStateV1(actor_id=b"short"))


def test_model_entries_equal_entries_from_states():
    frames, pairs = [], []
    for ours, theirs in PAIRS:
        pairs.append((len(frames), len(frames) + 1))
        frames += [M.state_frame(ours), M.state_frame(theirs)]
    got = M.decode_model(frames, pairs)
    decoded = [(W.decode_sync_state(frames[o][4:]), W.decode_sync_state(frames[t][4:])) for o, t in pairs]
    want, index = S.entries_from_states(decoded)
    assert len(index) > 2 * len(PAIRS)                                         # (the sample is not degenerate)
    for k, v in want.items():
        assert np.array_equal(got[k], v), k
    assert [(int(p), bytes(a)) for p, a in zip(got["entry_pair"], got["entry_actor"])] == index
    assert not got["frame_status"].any() and not got["pair_status"].any()
    assert got["pair_ent_off"][-1] == len(index) and got["nunregistered"] == len(index)
    # every shape the entries know is in the sample
    assert (got["our_head"] == -1).any() and (got["our_head"] >= 0).any()
    for k in ("tn_off", "tp_off", "tps_off", "on_off", "op_off", "ops_off"):
        d = np.diff(got[k].astype(np.int64))
        assert (d == 0).any() and (d > 1).any(), k
    for ver, off in (("tp_ver", "tp_off"), ("op_ver", "op_off")):
        for a, b in zip(got[off][:-1], got[off][1:]):
            assert np.all(np.diff(got[ver][int(a):int(b)].astype(np.int64)) > 0)


def test_model_sites_and_frame_fields():
    ours, theirs = PAIRS[3]
    sites = {a: i for i, a in enumerate(theirs.heads) if i % 2}
    got = M.decode_model([M.state_frame(ours), M.state_frame(theirs)], [(0, 1), (1, 0)], lambda a: sites.get(a, M.NONE))
    assert [int(s) for s in got["entry_site"]] == [sites.get(bytes(a), M.NONE) for a in got["entry_actor"]]
    assert got["nunregistered"] == int((got["entry_site"] == M.NONE).sum())
    assert bytes(got["frame_actor"][0]) == ours.actor_id and bytes(got["frame_actor"][1]) == theirs.actor_id
    for i, st in enumerate((ours, theirs)):
        assert got["frame_has_ts"][i] == (st.last_cleared_ts is not None)
        assert got["frame_ts"][i] == (st.last_cleared_ts or 0)


BAD = M.malformed_frames()


@pytest.mark.parametrize("name,fr,status", BAD, ids=[b[0] for b in BAD])
def test_model_statuses_on_malformed_frames(name, fr, status):
    assert M.parse_frame(fr)["status"] == status
    if status == M.INVALID and not name.startswith("prefix_"):
        with pytest.raises(ValueError):                                        # the host decoder refuses it too
            W.decode_sync_state(fr[4:])
    good = M.state_frame(PAIRS[1][0]), M.state_frame(PAIRS[1][1])
    alone = M.decode_model(list(good), [(0, 1)])
    got = M.decode_model([good[0], fr, good[1]], [(0, 2), (1, 2), (0, 1)])
    assert list(got["frame_status"]) == [0, status, 0] and list(got["pair_status"]) == [0, 1, 1]
    for k in M.ARRAYS:
        if not k.startswith(("frame_", "pair_")):
            assert np.array_equal(got[k], alone[k]), k                          # the neighbours' output is unchanged


def test_the_list_covers_what_the_decoder_must_refuse():
    names = {b[0] for b in BAD}
    assert {"count_heads", "count_need", "count_need_ranges", "count_partial", "count_partial_versions",
            "count_partial_seqs", "prefix_short", "prefix_long", "trailing", "option_2", "tag_5", "head_2_63", "dup_head",
            "dup_need", "dup_partial", "dup_version"} <= names
    assert {b[2] for b in BAD} == {M.INVALID, M.RANGE, M.NOT_STATE, M.DUPLICATE}
    assert M.parse_frame(M.state_frame(M._good()))["status"] == 0
    rng = random.Random(5)
    junk = bytes(rng.getrandbits(8) for _ in range(64))
    assert M.parse_frame(junk)["status"] == M.INVALID
