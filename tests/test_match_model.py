"""The host model of match_changes (tests/match_model.py) pinned on literal cases written out by hand from
corro-types/src/updates.rs:92-121, :270-305, :420-481 and pubsub.rs:294-332."""
from tests import match_model as M

S = M.SENTINEL


def test_first_taken_change_not_first_change_gives_the_cl():
    """A pk whose first change is a column the subscription does not list and whose second is one it does:
    the candidate is the second change, and cl is its."""
    sub = ("sub", {"t": ["b"]})
    changes = [("t", 7, "a", 1), ("t", 7, "b", 3), ("t", 7, "b", 5)]
    (cands, count), = M.match_changes([sub], changes)
    assert cands == {"t": {7: 3}} and count == 1


def test_sentinel_is_taken_by_any_subscription_naming_the_table():
    changes = [("t", 1, S, 2), ("u", 1, S, 2)]
    (c0, _), (c1, _) = M.match_changes([("sub", {"t": []}), ("sub", {"t": ["a"], "v": ["x"]})], changes)
    assert c0 == {"t": {1: 2}} and c1 == {"t": {1: 2}}


def test_update_handle_takes_the_first_change_regardless_of_column():
    changes = [("t", 9, "zz", 1), ("t", 9, S, 2), ("u", 9, "a", 1)]
    (cands, count), = M.match_changes([("update", "t")], changes)
    assert cands == {"t": {9: 1}} and count == 1


def test_one_pk_in_two_tables_gives_two_entries_in_first_appearance_order():
    changes = [("u", 4, "a", 1), ("t", 4, "a", 3), ("u", 5, "a", 1), ("u", 4, "a", 9)]
    (cands, count), = M.match_changes([("sub", {"t": ["a"], "u": ["a"]})], changes)
    assert list(cands) == ["u", "t"] and list(cands["u"]) == [4, 5]
    assert cands == {"u": {4: 1, 5: 1}, "t": {4: 3}} and count == 3


def test_even_cl_is_a_delete_and_odd_an_update():
    assert M.handle_candidates({"t": {1: 2, 2: 3}, "u": {1: 0}}) == [(M.DELETE, 1), (M.UPDATE, 2), (M.DELETE, 1)]
    assert M.handle_candidates({}) == []


def test_no_change_and_no_handle():
    assert M.match_changes([("update", "t")], []) == [None]
    assert M.match_changes([], [("t", 1, "a", 1)]) == []
    assert M.by_handle([("update", "t")], [[], [("u", 1, "a", 1)], [("t", 1, "a", 1)]]) == [[(2, {"t": {1: 1}})]]
    assert M.by_handle([], [[("t", 1, "a", 1)]]) == []


def test_a_change_no_filter_lists_leaves_no_empty_table():
    (cands, count), = M.match_changes([("sub", {"t": ["a"]})], [("t", 1, "b", 1), ("u", 1, S, 1)])
    assert cands == {} and count == 0
