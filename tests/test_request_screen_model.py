"""The plain restatement of process_sync's screen (tests/req_decode_util.keeps, a literal loop over the
versions as corro-agent/src/api/peer/mod.rs:857-870 reads) on hand-written cases, the expected-array
builder on a known frame, and the keep ratio of the seeded random workload the GPU test runs."""
import numpy as np

from corrosion_amd import sync as S
from tests import req_decode_util as U

GAPS = [(5, 9), (20, 20)]


def test_unknown_actor_is_dropped():
    assert not U.keeps(None, S.Full(1, 3))
    assert not U.keeps(None, S.Partial(1, ()))


def test_full_needs():
    assert U.keeps(([], None), S.Full(1, 3))                 # max None, no gaps: nothing answers it
    assert U.keeps((GAPS, None), S.Full(21, 30))             # max None: above-everything is not "above max"
    assert not U.keeps(([], 10), S.Full(11, 15))             # start > max
    assert U.keeps(([], 10), S.Full(10, 15))                 # 10 itself is known
    assert not U.keeps((GAPS, 30), S.Full(5, 9))             # a range that is its gap
    assert not U.keeps((GAPS, 30), S.Full(6, 8))             # inside one gap
    assert U.keeps((GAPS, 30), S.Full(6, 10))                # leaves its gap by one version
    assert U.keeps((GAPS, 30), S.Full(4, 9))
    assert not U.keeps(([(28, 30)], 30), S.Full(28, 40))     # spans a gap and max
    assert U.keeps(([(28, 29)], 30), S.Full(28, 40))         # ... but 30 is known
    assert U.keeps((GAPS, 30), S.Full(9, 20))                # two gaps with known versions between
    assert not U.keeps((GAPS, 30), S.Full(7, 6))             # empty: `all` over nothing
    assert not U.keeps(([], None), S.Full(1, 0))


def test_partial_needs():
    assert not U.keeps((GAPS, 30), S.Partial(7, ((0, 3),)))  # in a gap
    assert not U.keeps((GAPS, 30), S.Partial(31, ()))        # above max
    assert U.keeps((GAPS, 30), S.Partial(30, ((0, 3),)))     # known
    assert U.keeps((GAPS, 30), S.Partial(10, ()))
    assert U.keeps(([], None), S.Partial(99, ()))


def test_expected_arrays_of_a_known_frame():
    a, b = b"\x01" * 16, b"\x02" * 16
    fr = U.request_frame([(a, [S.Full(1, 3), S.Partial(7, ((0, 1), (4, 1 << 32)))]), (b, [S.Full(2, 2)])])
    exp = U.expected([(fr, 0), (b"\0\0", U.E_INVALID)], {a: 0}, {0: (GAPS, 30)})
    assert exp["frame_pair_off"].tolist() == [0, 2, 2] and exp["pair_site"].tolist() == [0, U.NONE]
    assert exp["pair_need_off"].tolist() == [0, 2, 3]
    assert exp["kind"].tolist() == [0, 1, 0] and exp["need_keep"].tolist() == [1, 0, 0]
    assert exp["sr_off"].tolist() == [0, 0, 2] and exp["sr_n"].tolist() == [0, 2, 0]
    assert exp["s_end"].tolist() == [1, 1 << 32]
    assert exp["need_ent_off"].tolist() == [0, 1, 1, 1] and exp["ent_seq_end"].tolist() == [0xFFFFFFFF]
    exp = U.expected([(fr, 0)], {a: 0, b: 1})                # no screen: the registered actors' needs are kept
    assert exp["need_keep"].tolist() == [1, 1, 1]
    assert exp["need_ent_off"].tolist() == [0, 1, 4, 5]
    assert exp["ent_seq_start"].tolist() == [0, 0, 0, 4, 0] and exp["ent_seq_end"].tolist() == [0xFFFFFFFF] * 2 + [
        1, 0xFFFFFFFF, 0xFFFFFFFF]
    assert exp["ent_need"].tolist() == [0, 1, 1, 1, 2]


def test_random_workload_exercises_both_sides_of_the_screen():
    rng = np.random.default_rng(U.SCREEN_SEED)
    actors = [bytes([i + 1]) * 16 for i in range(6)]
    kept = total = 0
    for _ in range(200):
        books, frames = U.random_screen_trial(rng, actors)
        exp = U.expected([(f, 0) for f in frames], {a: i for i, a in enumerate(actors)}, books)
        kept += int(exp["need_keep"].sum())
        total += exp["nneeds"]
        for gaps, _mx in (b for b in books.values() if b):
            assert len(gaps) <= 5 and all(s <= e for s, e in gaps)
            assert all(gaps[i][1] + 1 < gaps[i + 1][0] for i in range(len(gaps) - 1))
    assert total >= 1000 and 0.1 < kept / total < 0.9, (kept, total)
