"""The host model of changeset extraction (tests/extract_model.py) against oracle.extract_changes on
random rows, where both are exact, and against answers written out by hand at the edges where
neither may be taken on trust: db_version 2^63 - 1, bounds up to 2^64 - 1, a seq tie, a seq filter
that misses every row of a version. The oracle is held to the same literal answers (it once found
version 2^63 - 1 for a need starting at 2^63: the u64 bound promoted the comparison to float64)."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import extract_model as M

I63, U64, U32 = (1 << 63) - 1, (1 << 64) - 1, (1 << 32) - 1


def R(pk, site, dbv, seq, ts):
    """One row in ROWF order: (pk, table_cid, col_version, db_version, cl, seq, site, ts, val0, val1, val_type, val_len)."""
    return (pk, 1, 1, dbv, 1, seq, site, ts, 10 * pk, 0, 1, 0)


def rows_of(tuples):
    from corrosion_amd.engine import ROW_FIELDS
    return {k: np.array([t[i] for t in tuples], ROW_FIELDS[k]) for i, k in enumerate(M.ROWF)}


def canon(groups):
    return [(v, last, ts, M.seq_classes(rows)) for v, last, ts, rows in groups]


def needs_of(needs, seq=None):
    nd = {"site": np.array([x[0] for x in needs], np.uint32), "start": np.array([x[1] for x in needs], np.uint64),
          "end": np.array([x[2] for x in needs], np.uint64)}
    if seq is not None:
        nd["seq_start"] = np.array([s[0] for s in seq], np.uint32)
        nd["seq_end"] = np.array([s[1] for s in seq], np.uint32)
    return nd


# ---- literal answers -----------------------------------------------------------------------
# two sites; site 0: version 1 (seqs 0, 1, 1: a tie) and version 5; site 1: version 1 and version
# 2^63 - 1 (seqs 3 and 2^32 - 1, the larger ts on the smaller seq)
A1, A2, A3, A4 = R(1, 0, 1, 0, 10), R(2, 0, 1, 1, 30), R(3, 0, 1, 1, 20), R(4, 0, 5, 0, 7)
A5, A6, A7 = R(5, 1, 1, 4, 9), R(6, 1, I63, U32, 99), R(7, 1, I63, 3, 100)
STATE_A = [A6, A3, A1, A5, A4, A7, A2]

LITERAL = [
    # (need, seq filter or None, expected groups)
    ((0, 0, U64), None, [(5, 0, 7, [A4]), (1, 1, 30, [A1, A2, A3])]),
    ((1, 0, U64), None, [(I63, U32, 100, [A7, A6]), (1, 4, 9, [A5])]),
    ((1, 0, I63), None, [(I63, U32, 100, [A7, A6]), (1, 4, 9, [A5])]),
    ((1, I63, I63), None, [(I63, U32, 100, [A7, A6])]),
    ((1, I63, U64), None, [(I63, U32, 100, [A7, A6])]),
    ((1, I63 + 1, U64), None, []),                      # starts past the largest int64
    ((1, U64, U64), None, []),
    ((1, 2, I63 - 1), None, []),                        # strictly between two present versions
    ((1, 0, 0), None, []),
    ((0, 5, 1), None, []),                              # start > end
    ((0, U64, 0), None, []),
    ((2, 0, U64), None, []),                            # unknown site ordinal
    ((U32, 0, U64), None, []),
    ((0, 1, 1), (1, 1), [(1, 1, 30, [A2, A3])]),        # the tie, cut exactly on it
    ((0, 1, 1), (0, 0), [(1, 1, 30, [A1])]),            # ts 30 comes from a filtered-out row
    ((0, 1, 1), (0, 1), [(1, 1, 30, [A1, A3, A2])]),
    ((0, 1, 1), (2, 9), [(1, 1, 30, [])]),              # misses every row: the version still appears
    ((0, 0, U64), (1, U32), [(5, 0, 7, []), (1, 1, 30, [A2, A3])]),
    ((1, 0, U64), (4, U32), [(I63, U32, 100, [A6]), (1, 4, 9, [A5])]),   # MAX(ts) from the excluded seq 3
    ((1, 0, U64), (U32, U32), [(I63, U32, 100, [A6]), (1, 4, 9, [])]),
    ((1, 0, U64), (5, 4), [(I63, U32, 100, []), (1, 4, 9, [])]),          # seq_start > seq_end: no rows
    ((2, 0, U64), (0, U32), []),
]

# three sites, the middle one empty; versions that differ only in the site
B1, B2, B3, B4 = R(1, 0, 7, 0, 0), R(2, 2, 7, 0, 0), R(3, 2, 8, 2, 0), R(4, 2, 8, 1, 0)
STATE_B = [B4, B1, B3, B2]
LITERAL_B = [
    ((0, 0, U64), None, [(7, 0, 0, [B1])]),
    ((1, 0, U64), None, []),
    ((2, 0, U64), None, [(8, 2, 0, [B4, B3]), (7, 0, 0, [B2])]),
    ((2, 8, 8), (2, 2), [(8, 2, 0, [B3])]),
    ((2, 8, 8), (0, 0), [(8, 2, 0, [])]),
    ((3, 0, U64), None, []),
]


@pytest.mark.parametrize("which", ["model", "oracle"])
@pytest.mark.parametrize("state,cases,nsites", [(STATE_A, LITERAL, 2), (STATE_B, LITERAL_B, 3)])
def test_literal_answers(which, state, cases, nsites):
    rows = rows_of(state)
    for need, seq, exp in cases:
        nd = needs_of([need], None if seq is None else [seq])
        if which == "model":
            got = M.extract(rows, nd, nsites)[0]
            # the model's own row order: seq classes ascending
            seqs = [[r[M.I_SEQ] for r in g[3]] for g in got]
            assert all(s == sorted(s) for s in seqs)
        else:
            got = M.from_oracle(rows, O.extract_changes(rows, nd))[0]
        assert canon(got) == canon(exp), (need, seq)
        assert [g[0] for g in got] == [g[0] for g in exp]


def test_model_without_nsites_finds_no_rows_for_an_unknown_site():
    rows = rows_of(STATE_A)
    assert M.extract(rows, needs_of([(2, 0, U64), (U32, 0, U64)])) == [[], []]


def test_seq_classes_is_the_order_contract():
    assert M.seq_classes([A2, A1, A3]) == [(0, [A1]), (1, [A2, A3])]
    assert M.seq_classes([A3, A2, A1]) == M.seq_classes([A1, A2, A3])
    assert M.seq_classes([]) == []


# ---- model == oracle where both are exact ------------------------------------------------------

def random_rows(rng, m, nsites, nver, nseq):
    from corrosion_amd.engine import ROW_FIELDS
    rows = {k: rng.integers(0, 1 << 20, m).astype(dt) for k, dt in ROW_FIELDS.items()}
    rows["pk"] = np.arange(1, m + 1, dtype=np.uint64)      # distinct rows, so ties are told apart
    rows["site"] = rng.integers(0, nsites, m).astype(np.uint32)
    # versions spread up to 2^61, clustered so that ranges hold several
    base = rng.integers(1, 1 << 61, nver)
    rows["db_version"] = base[rng.integers(0, nver, m)].astype(np.int64)
    rows["seq"] = rng.integers(0, nseq, m).astype(np.uint32)   # few seqs: many ties
    rows["ts"] = rng.integers(0, 1 << 62, m).astype(np.uint64)
    return rows


@pytest.mark.parametrize("seq_filter", [False, True])
def test_model_equals_oracle_on_random_rows(seq_filter):
    rng = np.random.default_rng(11 + seq_filter)
    nsites, m, n = 5, 3000, 300
    rows = random_rows(rng, m, nsites, 40, 12)
    vs = np.unique(rows["db_version"])
    pick = lambda: vs[rng.integers(0, len(vs), n)].astype(np.uint64)  # noqa: E731
    start, end = pick(), pick()
    start[::3] -= np.uint64(1)                                   # bounds on and just off present versions
    end[::4] += np.uint64(1)
    start[::5] = 0
    end[::7] = np.uint64((1 << 62) - 1)                          # open-ended
    swap = (start > end) & (rng.random(n) < 0.8)                 # keep a few start > end
    start[swap], end[swap] = end[swap], start[swap]
    nd = {"site": rng.integers(0, nsites + 2, n).astype(np.uint32), "start": start, "end": end}
    if seq_filter:
        a = rng.integers(0, 14, n).astype(np.uint32)
        b = (a + rng.integers(0, 5, n)).astype(np.uint32)
        b[::13] = a[::13] - np.uint32(1)                         # seq_start > seq_end (wraps at 0 to 2^32 - 1)
        nd["seq_start"], nd["seq_end"] = a, b
    got = M.extract(rows, nd, nsites)
    exp = M.from_oracle(rows, O.extract_changes(rows, nd))
    for e in range(n):
        assert canon(got[e]) == canon(exp[e]), e
    # not vacuous: groups, multi-group needs, multi-row groups, ties and filtered-out groups all occur
    groups = [g for need in got for g in need]
    assert sum(len(need) >= 2 for need in got) >= 10
    assert sum(len(g[3]) >= 2 for g in groups) >= 10
    assert any(len(cls) >= 2 for g in groups for _s, cls in M.seq_classes(g[3]))
    assert sum(need == [] for need in got) >= 10
    if seq_filter:
        assert sum(len(g[3]) == 0 for g in groups) >= 10
