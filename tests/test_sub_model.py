"""The host model of a subscription's result set (tests/sub_model.py) against SQLite's own answers
(tests/golden/sub_kats.json): every round of every sequence, exactly -- event types, rowids, change ids, keys,
cells by storage class and bits, and the whole set after the round."""
import pytest

from tests import sub_model as S

KATS = S.load_kats()


def _cells(vals):
    return [S.dec(v) for v in vals]


def _same_cells(a, b):
    return len(a) == len(b) and all(S.identical(x, y) for x, y in zip(a, b))


def test_the_fixture_covers_what_it_is_to_pin():
    assert KATS["sqlite_version"] == "3.37.2"
    seqs = {s["name"]: s for s in KATS["sequences"]}
    assert sorted(seqs) == ["equality", "orders", "rowids", "transitions"]
    kinds = [e[0] for s in KATS["sequences"] for r in s["rounds"] for e in r["events"]]
    assert {"Insert", "Update", "Delete"} == set(kinds)
    # Insert, Update, Insert, Update, Insert over rowids 1..3: 4, 6, 8, and 9 behind them
    r0, r1 = seqs["rowids"]["rounds"][:2]
    assert [(e[0], e[1]) for e in r0["events"]] == [("Insert", 4), ("Update", 1), ("Insert", 6), ("Update", 2), ("Insert", 8)]
    assert [(e[0], e[1]) for e in r1["events"]] == [("Insert", 9)]
    assert any(k < 0 for r in seqs["orders"]["rounds"] for k in r["keys"])


@pytest.mark.parametrize("seq", KATS["sequences"], ids=[s["name"] for s in KATS["sequences"]])
def test_every_round_equals_sqlites_answer(seq):
    m = S.SubModel([(r[0], _cells(r[1:])) for r in seq["initial"]])

    def check_rows(want):
        got = m.rows()
        assert [(r, S.signed(k)) for r, k, _c in got] == [(w[0], w[1]) for w in want]
        assert all(_same_cells(g[2], _cells(w[2])) for g, w in zip(got, want))

    check_rows(seq["rows"])
    assert [r[0] for r in seq["rows"]] == list(range(1, len(seq["initial"]) + 1))
    for n, rnd in enumerate(seq["rounds"]):
        got = m.update(rnd["keys"], {r[0]: _cells(r[1:]) for r in rnd["fresh"]})
        want = rnd["events"]
        assert [(t, r, c, S.signed(k)) for t, r, c, k, _v in got] == [tuple(e[:4]) for e in want], (seq["name"], n)
        assert all(_same_cells(g[4], _cells(w[4])) for g, w in zip(got, want)), (seq["name"], n)
        check_rows(rnd["rows"])
