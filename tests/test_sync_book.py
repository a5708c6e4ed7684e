"""The host half of the state encoder on its own: the bookie's sync book (corro_bookie_sync_book,
Agent.sync_book) under a plain-Python restatement of generate_sync (tests/state_encode_model.py) against
Agent.generate_sync, and the model's own edges. A bookie is filled by process_multiple_changes alone, which
needs the engine: that one case is marked gpu; the empty bookie and the pass-1 refusals are in
tests/test_abi_state_encode.py."""
import pytest

from tests import state_encode_model as EM

U64 = (1 << 64) - 1


def test_seq_gaps_edges():
    assert EM.seq_gaps([], 0) == [(0, 0)]
    assert EM.seq_gaps([(0, 0)], 0) == []
    assert EM.seq_gaps([], U64) == [(0, U64)]
    assert EM.seq_gaps([(0, U64 - 1)], U64) == [(U64, U64)]
    assert EM.seq_gaps([(1, U64)], U64) == [(0, 0)]
    assert EM.seq_gaps([(0, U64)], U64) == []
    assert EM.seq_gaps([(2, 3), (6, 7)], 9) == [(0, 1), (4, 5), (8, 9)]
    # a present range that runs past last_seq is clipped; one that starts past it is not there
    assert EM.seq_gaps([(2, 30)], 9) == [(0, 1)]
    assert EM.seq_gaps([(0, 3), (12, 30)], 9) == [(4, 9)]
    assert EM.seq_gaps([(0, 3), (9, 30)], 9) == [(4, 8)]


def test_is_complete_looks_at_1_to_last_seq():
    """agent.rs:1068-1074: full_range() is 1..=last_seq, so seq 0 alone never makes a partial incomplete."""
    assert EM.is_complete([], 0) and EM.is_complete([(0, 0)], 0)
    assert EM.is_complete([(1, 5)], 5) and EM.is_complete([(0, 5)], 5) and EM.is_complete([(1, U64)], U64)
    assert not EM.is_complete([], 1) and not EM.is_complete([(0, 0)], 1) and not EM.is_complete([(0, U64 - 1)], U64)
    assert not EM.is_complete([(2, 5)], 5) and not EM.is_complete([(0, 1), (3, 5)], 5) and not EM.is_complete([(0, 4)], 5)


def test_model_rows_round_trip_and_rule():
    a, b, c = bytes([1]) * 16, bytes([2]) * 16, bytes([3]) * 16
    rows = [(a, 9, [(3, 4), (6, 8)], [(5, 9, [(2, 3), (6, 7)]), (7, 3, [(0, 3)])]),
            (b, None, [], []),
            (c, 4, [], [(2, 0, []), (4, 5, [(1, 5)])])]
    assert EM.rows_of_book(EM.book_of_rows(rows)) == rows
    st = EM.generate_sync(rows, bytes(16), ts=7)
    assert list(st.heads.items()) == [(a, 9), (c, 4)]
    assert st.need == {a: [(3, 4), (6, 8)]}
    assert st.partial_need == {a: {5: [(0, 1), (4, 5), (8, 9)]}}       # c's partials are both complete
    assert st.last_cleared_ts == 7
    assert EM.rows_canonical(rows)
    for bad in ([(a, 9, [(3, 4), (5, 8)], [])], [(a, 9, [(6, 8), (3, 4)], [])], [(a, 9, [(4, 3)], [])],
                [(a, 9, [], [(5, 9, [(2, 3), (3, 7)])])], [(a, 9, [], [(5, 9, []), (5, 9, [])])],
                [(a, 9, [], [(6, 9, []), (5, 9, [])])]):
        assert not EM.rows_canonical(bad), bad


@pytest.mark.gpu
def test_sync_book_of_a_mixed_bookie_matches_generate_sync():
    from tests.state_encode_util import A, B, C_, D, ME, mixed_agent
    ag = mixed_agent()
    book = ag.sync_book()
    rows = EM.rows_of_book(book)
    assert [r[0] for r in rows] == [A, B, C_, D]                       # the bookie's order, every actor
    want = ag.generate_sync()
    got = EM.generate_sync(rows, ME)
    assert got == want
    for m in ("heads", "need", "partial_need"):                        # dict order included
        assert list(getattr(got, m).items()) == list(getattr(want, m).items()), m
    assert [list(p.items()) for p in got.partial_need.values()] == [list(p.items()) for p in want.partial_need.values()]
    # the mix the case is about
    assert want.need == {A: [(3, 4), (6, 8), (10, 11)]}
    assert want.partial_need == {A: {12: [(0, 1), (4, 5), (8, 9)]}}
    assert list(want.heads) == [A, B, C_, D]
    by = {r[0]: r for r in rows}
    assert by[A][3] == [(12, 9, [(2, 3), (6, 7)])]                     # present ranges as stored, not the gaps
    assert by[B][3] == [(2, 3, [(0, 3)])] and by[B][2] == []           # a complete partial is in the book
    assert by[C_][3] == [(1, 3, [(1, 3)])]                             # complete over 1..=last_seq only
    assert by[D][2] == [] and by[D][3] == []
    assert EM.rows_canonical(rows)
