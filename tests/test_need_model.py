"""The host model of the need diff (tests/need_model.py) against the oracle, on the KATs, the
inverted-range fixture and every case the GPU edge test runs (tests/need_cases.py): the two share
no technique, so where they agree the GPU test has a witness worth comparing with."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import need_cases as NC
from tests import need_model as M
from tests._util import load_golden
from tests.sync_util import (decode_needs, entries_from_pairs, expected_from_cases, kat_expect,
                             pairs_from_cases)

KEYS = ("need_off", "seq_off", "kind", "start", "end", "sr_off", "sr_n", "s_start", "s_end")


def assert_model_equals_oracle(pairs, ent=None):
    ent = entries_from_pairs(pairs) if ent is None else ent
    exp = O.needs(ent)
    got = M.to_csr(M.needs(pairs))
    if all(np.array_equal(got[k], exp[k].astype(got[k].dtype)) for k in KEYS):
        return
    dec = decode_needs(exp, len(pairs))     # name the first entry that differs
    for i, (our, their) in enumerate(pairs):
        assert M.entry_needs(our, their) == dec[i], (i, our, their)
    raise AssertionError("CSR arrays differ although every entry decodes alike")


def test_have_ranges():
    assert M.have_ranges(1, 10, ()) == ((1, 10),)
    assert M.have_ranges(1, 10, ((3, 5), (6, 8))) == ((1, 2), (9, 10))
    assert M.have_ranges(1, 10, ((5, 9), (3, 7), (0, 1), (10, 12))) == ((2, 2),)
    assert M.have_ranges(1, 10, ((1, 10),)) == ()
    assert M.have_ranges(0, NC.U64, ((NC.U64, NC.U64), (0, 0))) == ((1, NC.U64 - 1),)
    with pytest.raises(ValueError):
        M.have_ranges(1, 10, ((5, 4),))


def test_model_kats():
    for c in load_golden("sync_kats.json")["cases"]:
        assert M.entry_needs(c["our"], c["their"]) == kat_expect(c["expect"]), c["name"]


def test_model_inverted_fixture():
    cases = load_golden("sync_inverted_cases.json")["cases"]
    pairs = pairs_from_cases(cases)
    assert M.needs(pairs) == expected_from_cases(cases)
    assert_model_equals_oracle(pairs)


def test_inverted_seq_range_of_ours_example():
    """A have range of seqs spanning [t, s] overlaps our inverted seq range (s, t): kept as is."""
    our = NC.side(None, [], {5: [(10, 3)]})
    their = NC.side(7, [], {5: [(20, 30)]})
    exp = [("partial", 5, [(10, 3)]), ("full", 1, 7)]
    assert M.entry_needs(our, their) == exp
    assert decode_needs(O.needs(entries_from_pairs([(our, their)])), 1)[0] == exp


@pytest.mark.parametrize("family", list(NC.FAMILIES))
def test_model_equals_oracle_directed(family):
    assert_model_equals_oracle(NC.FAMILIES[family]())


def test_families_hold_inverted_ranges_both_ways():
    """Inverted ranges of ours that a have range spans (kept as is) and that none spans (dropped)."""
    for family, kind in (("holes", "full"), ("seq_diff", "partial")):
        pairs = NC.FAMILIES[family]()
        kept = dropped = 0
        for (our, their), got in zip(pairs, M.needs(pairs)):
            rs = our["need"] if kind == "full" else [r for v in our["partials"].values() for r in v]
            if len(rs) != 1 or rs[0][0] <= rs[0][1]:
                continue
            out = [(x[1], x[2]) for x in got if x[0] == "full"] if kind == "full" else \
                  [r for x in got if x[0] == "partial" for r in x[2]]
            if tuple(rs[0]) in out:
                kept += 1
            else:
                dropped += 1
        assert kept >= 10 and dropped >= 10, (family, kept, dropped)


def test_model_equals_oracle_exhaustive():
    assert_model_equals_oracle(NC.exhaustive_pairs())


@pytest.mark.parametrize("kind", NC.CAP_KINDS)
def test_cap_launches_sit_at_their_caps(kind):
    """cap_launches asserts the input totals of its workgroups itself; the output total of the O
    launches needs the need diff, so it is checked here."""
    launches = NC.cap_launches(kind)
    assert len(launches) == 8
    if kind == "O":
        for _, ent, total, _ in launches:
            off = O.needs(ent)["need_off"]
            assert int(off[2 * NC.NEEDS_T]) - int(off[NC.NEEDS_T]) == total


def test_placements_keep_every_case():
    """take_entries / place: a placed launch holds each directed entry, unchanged, where it says."""
    pairs = NC.our_partials_family()
    alone = O.needs(entries_from_pairs(pairs))
    want = decode_needs(alone, len(pairs))
    for placement in NC.PLACEMENTS:
        seen = 0
        for ent, pos in NC.place(pairs, placement):
            n = len(ent["their_head"])
            if placement == "final":
                assert n % NC.NEEDS_T != 0 and pos[-1] == n - 1
            elif placement != "alone":
                assert n == NC.NEEDS_T * len(pairs)
            dec = decode_needs(O.needs(ent), n)
            for p in pos:
                assert dec[int(p)] == want[seen], (placement, seen)
                seen += 1
        assert seen == len(pairs)
