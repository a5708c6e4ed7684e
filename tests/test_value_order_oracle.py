"""The value ladders of tests/value_ladders.py through the CPU oracle (no GPU): oracle.Fold and
oracle.ShardedFold must give the winners, impact flags and db_versions of the plain Python model
(int / float / bytes comparison under the class order of SURVEY App. A.4). The GPU tests of
test_gpu_value_order.py assert against both; this keeps the two references from drifting apart."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import value_ladders as V
from tests._util import rows_to_tuples

NSITES = 8
SITES, RANK, ORD = V.shuffled_sites(NSITES, 7)
LO_SITE, HI_SITE = int(ORD[NSITES - 1]), int(ORD[0])  # lo is written by the site of higher rank


def folds():
    return [("Fold", O.Fold(SITES)), ("ShardedFold", O.ShardedFold(SITES, nshards=4, nthreads=2))]


def check(case, split):
    """Apply the case (in one apply, or first / second members in two) and compare with the model."""
    held, impact, dbv = V.model_fold(sorted(case.changes, key=lambda c: case.phase[c.seq]) if split else case.changes,
                                     RANK)
    parts = [[c for c in case.changes if case.phase[c.seq] == p] for p in (0, 1)] if split else [case.changes]
    want_imp = [i for i in impact]
    for name, f in folds():
        got_imp = np.concatenate([f.apply(V.batch_of(p)) for p in parts if p])
        rows = rows_to_tuples(f.export(), with_ts=True)
        want = V.model_rows(held, with_ts=True)
        if rows != want:
            bad = [(g, w) for g, w in zip(rows, want) if g != w][:3]
            raise AssertionError(f"{name}: " + "; ".join(
                f"{case.label.get((w[1], w[2]))}: got {g}, model {w}" for g, w in bad) + f" ({len(rows)}/{len(want)} rows)")
        assert list(got_imp) == want_imp, f"{name}: impact flags"
        dv = f.db_versions()
        assert [int(x) for x in dv] == [dbv.get(s, -1) for s in range(NSITES)], name
    return held, impact


def test_ladders_are_strictly_increasing_and_whole():
    for name, ladder in V.LADDERS.items():
        assert len(ladder) == V.LADDER_LEN[name], name
        keys = [V.key(v) for v in ladder]
        assert all(a < b for a, b in zip(keys, keys[1:])), name
    assert len(V.pairs_of(V.INTEGER)) == 373 and 4 * len(V.pairs_of(V.INTEGER)) == 1492
    # every bit position separates some adjacent INTEGER pair at its top differing bit
    tops = {((a ^ b) & 0xFFFFFFFFFFFFFFFF).bit_length() - 1 for a, b in V.pairs_of(V.INTEGER)}
    assert tops == set(range(64))
    assert V.key(-0.0) == V.key(0.0) and V.key(b"a") < V.key(b"a\0") < V.key(b"a" * 7)
    assert V.key(b"\x7f") < V.key(b"\x80") and V.key(b"\0" * 16) < V.key(b"\0" * 17) < V.key(b"\0" * 16 + b"\1")
    assert RANK[LO_SITE] > RANK[HI_SITE] and list(RANK) != sorted(RANK)


@pytest.mark.parametrize("split", [False, True], ids=["one_apply", "two_applies"])
@pytest.mark.parametrize("ladder", list(V.LADDERS))
def test_oracle_duels(ladder, split):
    pairs = V.pairs_of(V.LADDERS[ladder])
    case = V.duel_batch(pairs, LO_SITE, HI_SITE)
    held, impact = check(case, split)
    # what the model must say for a duel: hi wins both cells; flags 1,1 (lo, hi) and 1,0 (hi, lo)
    for k, (lo, hi) in enumerate(pairs):
        for cell in (2 * k, 2 * k + 1):
            assert V.key(held[(1 + cell, 1)].value) == V.key(hi) and held[(1 + cell, 1)].site == HI_SITE
    flags = impact if not split else None
    if flags is not None:
        assert flags == [1, 1, 1, 0] * len(pairs)


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("split", [False, True], ids=["one_apply", "two_applies"])
@pytest.mark.parametrize("ladder", list(V.LADDERS))
def test_oracle_melees(ladder, split, seed):
    vals = V.LADDERS[ladder]
    for cell_size in (None, 48):
        case = V.melee_batch(vals, seed, NSITES, cell_size=cell_size)
        held, _ = check(case, split)
        if cell_size is None:
            assert V.key(held[(1, 1)].value) == V.key(vals[-1])


@pytest.mark.parametrize("split", [False, True], ids=["one_apply", "two_applies"])
def test_oracle_equal_values(split):
    case = V.equal_batch(V.EQUAL_WIDE, LO_SITE, HI_SITE)
    held, impact = check(case, split)
    for (pk, cid), label in case.label.items():
        first, second = [c for c in case.changes if c.pk == pk]
        want = first if RANK[first.site] >= RANK[second.site] else second
        assert held[(pk, cid)] == want, label
    if not split:
        assert impact[6:8] == [1, 0]  # same site: the earlier change keeps the cell


@pytest.mark.parametrize("split", [False, True], ids=["one_apply", "two_applies"])
def test_oracle_col_version_boundaries(split):
    case = V.col_version_batch(V.CV_PAIRS, LO_SITE, HI_SITE)
    held, _ = check(case, split)
    for (pk, cid), label in case.label.items():
        assert held[(pk, cid)].cv == max(c.cv for c in case.changes if c.pk == pk), label
