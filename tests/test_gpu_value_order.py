"""The merge's value, site and col_version order at its bit boundaries, through every merge body.

The ladders of tests/value_ladders.py (adjacent values that differ at every INTEGER bit, REAL signs /
zeros / denormals / infinities, TEXT / BLOB bytes >= 0x80, embedded NULs, the 8- / 16-byte word ends
and the inline / long boundary) go through each body as duels (two cells per adjacent pair, both
orders, the lesser value written by the site of higher rank), as melees (a whole ladder in one cell)
and as equal-value cases. Every result -- exported rows, impact flags, db_versions -- is asserted
bit-exact twice: against the plain Python model of value_ladders.py and against oracle.Fold on the
same batches.

No switch forces a body (CORRO_HIP_FORCE_GENERAL, CORRO_GEN_OVF_MIN, CORRO_OVF_REDUCE and
CORRO_TRIAGE are read once per process), so the shape of the batch picks it, by k_triage's
conditions (merge_kernels.h) on a one-bucket engine (capacity_hint <= 1280 gives B = 1):

  fast_packed / fast_three_stage    cl = 1, INTEGER batch into an INTEGER state, no impacts, <= 3072
                                    records; every col_version < 2^15 / one unrelated change at 2^15
  fast_impact_packed / _int         the same with impact flags
  wide / wide_impact                any non-INTEGER value in the batch (one unrelated TEXT change
                                    for the INTEGER ladder): fast_body<true> / fast_body_impact_wide.
                                    A value longer than 16 bytes sends its bucket to the general
                                    body, so cells with one run apart from the inline ones.
  gen_small / gen_mid / gen_large   one sentinel change (cid 0, NULL, col_version == cl == 2) on an
                                    unrelated row, padded with unrelated cl = 1 changes to <= 512,
                                    513..1024, 1025..2048 records; ladders cut into slices that fit
                                    (rows stay under LONG_ROW = 128 records)
  ovf*                              more than 3072 records in the bucket, with and without the
                                    sentinel and impacts: the device-wide fold (ovf_kernels.h),
                                    confirmed by metrics()["overflow_rounds"]; every other route
                                    asserts that the counter did NOT move."""
from collections import namedtuple

import numpy as np
import pytest

from oracle import oracle as O
from tests import value_ladders as V
from tests._util import rows_to_tuples

pytestmark = pytest.mark.gpu

SCHEMA = {"t": ["a", "b", "c"]}
NSITES = 8
SITES, RANK, ORD = V.shuffled_sites(NSITES, 7)
LO_SITE, HI_SITE = int(ORD[NSITES - 1]), int(ORD[0])  # the lesser value is written by the higher rank
CAP_HINT = 1024  # one bucket

# cap: most ladder changes per slice (both applies together); pad_to: records per apply, reached with
# unrelated changes; cell: most values per melee cell (doubled: each value is written twice)
Route = namedtuple("Route", "name impact cap cvbig text sentinel pad_to ovf cell int_only")
ROUTES = [
    Route("fast_packed", False, 3000, False, False, False, 0, False, None, True),
    Route("fast_three_stage", False, 3000, True, False, False, 0, False, None, True),
    Route("fast_impact_packed", True, 3000, False, False, False, 0, False, None, True),
    Route("fast_impact_int", True, 3000, True, False, False, 0, False, None, True),
    Route("wide", False, 3000, False, True, False, 0, False, None, False),
    Route("wide_impact", True, 3000, False, True, False, 0, False, None, False),
    Route("gen_small", True, 200, False, False, True, 0, False, 48, False),
    Route("gen_mid", True, 400, False, False, True, 600, False, 48, False),
    Route("gen_large", True, 800, False, False, True, 1200, False, 48, False),
    Route("ovf", False, 3000, False, False, False, 3200, True, None, False),
    Route("ovf_impact", True, 3000, False, False, False, 3200, True, None, False),
    Route("ovf_sentinel", False, 3000, False, False, True, 3200, True, None, False),
    Route("ovf_sentinel_impact", True, 3000, False, False, True, 3200, True, None, False),
]
BY_NAME = {r.name: r for r in ROUTES}
ROUTE_LADDER = [(r.name, l) for r in ROUTES for l in V.LADDERS if l == "integer" or not r.int_only]
EXTRA_PK, EXTRA_DBV, EXTRA_SEQ = 1_000_000, 1_000_000, 1_000_000


@pytest.fixture(scope="module")
def engines():
    """One engine per (site table, INTEGER-only or not), reset between uses: a state that has held a
    non-INTEGER value keeps its buckets off the INTEGER fast bodies even after a reset."""
    import corrosion_amd as ca
    cache = {}

    def get(wide, sites=SITES, tag="std"):
        e = cache.get((tag, wide))
        if e is None:
            e = cache[(tag, wide)] = ca.MergeEngine(SCHEMA, capacity_hint=CAP_HINT)
            e.register_sites(sites)
        else:
            e.reset()
        return e
    yield get
    for e in cache.values():
        e.close()


def extras(route, k, n):
    """The unrelated changes that steer apply k (of n ladder changes) to the route's body."""
    out = []
    pk0 = EXTRA_PK * (k + 1)

    def add(pk, cid, value, cv, cl=1):
        i = len(out)
        out.append(V.Change(pk0 + pk, cid, value, cv, EXTRA_DBV * (k + 1) + i, i % NSITES, cl, EXTRA_SEQ * (k + 1) + i))
    if route.cvbig:
        add(0, 2, 11, 1 << 15)
    if route.text:
        add(1, 2, "x", 1)
    if route.sentinel:
        add(2, 0, None, 2, cl=2)
    j = 0
    while n + len(out) < route.pad_to:
        add(10 + j // 3, 1 + j % 3, j, 1)
        j += 1
    return out


def slices(case, route):
    """Whole cells of the case, at most route.cap changes a slice. On the wide routes the cells that
    hold a long value are kept apart (they take the general body)."""
    cells, order = {}, []
    for c in case.changes:
        if c.pk not in cells:
            cells[c.pk] = []
            order.append(c.pk)
        cells[c.pk].append(c)
    groups = [order]
    if route.text:
        has_long = {pk: any(V.is_long(c.value) for c in cells[pk]) for pk in order}
        groups = [[pk for pk in order if not has_long[pk]], [pk for pk in order if has_long[pk]]]
    for g in groups:
        cur = []
        for pk in g:
            assert len(cells[pk]) <= route.cap
            if len(cur) + len(cells[pk]) > route.cap:
                yield cur
                cur = []
            cur = cur + cells[pk]
        if cur:
            yield cur


def explain(got, want, labels, who):
    if got == want:
        return None
    gk, wk = {r[:3]: r for r in got}, {r[:3]: r for r in want}
    lines = [f"rows differ from {who}: got {len(got)}, expected {len(want)}"]
    for k in sorted(set(gk) | set(wk)):
        if gk.get(k) != wk.get(k):
            lines.append(f"  {labels.get((k[1], k[2]), f'pk {k[1]} cid {k[2]}')}: got {gk.get(k)}, expected {wk.get(k)}")
        if len(lines) > 6:
            break
    return "\n".join(lines)


def run(get_engine, route, case, split, sites=SITES, rank=RANK, tag="std"):
    nsl = 0
    for part in slices(case, route):
        nsl += 1
        phases = [[c for c in part if case.phase[c.seq] == p] for p in (0, 1)] if split else [part]
        applies = [p + extras(route, k, len(p)) for k, p in enumerate(phases) if p]
        everything = [c for a in applies for c in a]
        wide = any(not isinstance(c.value, int) for c in everything)
        assert not (route.int_only and wide)
        held, m_imp, m_dbv = V.model_fold(everything, rank)
        eng = get_engine(wide, sites, tag)
        fold = O.Fold(sites)
        dv0 = np.array(eng.db_versions()[:len(sites)], np.int64)
        ovf0 = eng.metrics()["overflow_rounds"]
        g_imp, f_imp = [], []
        for a in applies:
            b = V.batch_of(a)
            assert route.ovf or len(a) <= 3072
            gi = eng.apply(b, impact=route.impact)
            f_imp += [int(x) for x in fold.apply(b)]
            if route.impact:
                g_imp += [int(x) for x in gi]
        where = f"route={route.name} slice={nsl} applies={len(applies)}"
        # the route was the one meant
        ovf = eng.metrics()["overflow_rounds"] - ovf0
        assert ovf == (len(applies) if route.ovf else 0), f"{where}: overflow_rounds grew by {ovf}"
        # rows
        got = rows_to_tuples(eng.export(), with_ts=True)
        bad = explain([r for r in got if r[2] != 0], V.model_rows(held, with_ts=True), case.label, "the model")
        assert bad is None, f"{where}\n{bad}"
        bad = explain(got, rows_to_tuples(fold.export(), with_ts=True), case.label, "oracle.Fold")
        assert bad is None, f"{where}\n{bad}"
        # impact flags
        if route.impact:
            for i, c in enumerate(everything):
                lab = case.label.get((c.pk, c.cid), "steering change")
                assert m_imp[i] is None or g_imp[i] == m_imp[i], f"{where}: impact of change {i} ({lab}, value {c.value!r}): got {g_imp[i]}, model {m_imp[i]}"
                assert g_imp[i] == f_imp[i], f"{where}: impact of change {i} ({lab}, value {c.value!r}): got {g_imp[i]}, oracle {f_imp[i]}"
        # db_versions (a reset keeps them: the engine's are the maximum over all it has merged)
        dv = np.array(eng.db_versions()[:len(sites)], np.int64)
        want = dv0.copy()
        for s, v in m_dbv.items():
            want[s] = max(want[s], v)
        assert np.array_equal(dv, want), f"{where}: db_versions differ from the model"
        assert np.array_equal(dv, np.maximum(dv0, fold.db_versions())), f"{where}: db_versions differ from oracle.Fold"
    assert nsl > 0


@pytest.mark.parametrize("split", [False, True], ids=["one_apply", "two_applies"])
@pytest.mark.parametrize("route,ladder", ROUTE_LADDER, ids=[f"{r}-{l}" for r, l in ROUTE_LADDER])
def test_duels(engines, route, ladder, split):
    """Adjacent ladder values against each other, both orders; across two applies the first member
    of each cell is the prior state (prior_cmp_int, prior_cmp_packed, the wide prior compare)."""
    run(engines, BY_NAME[route], V.duel_batch(V.pairs_of(V.LADDERS[ladder]), LO_SITE, HI_SITE), split)


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("route,ladder", ROUTE_LADDER, ids=[f"{r}-{l}" for r, l in ROUTE_LADDER])
def test_melees(engines, route, ladder, seed):
    """A whole ladder (each value twice, random sites, shuffled) in one cell, and cut into cells of 48
    values so that values inside the ladder win too; in one apply and in two."""
    r = BY_NAME[route]
    vals = V.LADDERS[ladder]
    def melee(ladder, sd):  # the whole ladder in one cell where the body holds it, and cut into cells
        whole = None if r.cell else V.melee_batch(ladder, sd, NSITES)
        return V.melee_batch(ladder, sd + 50, NSITES, pk0=1000, cell_size=r.cell or 48, into=whole)
    run(engines, r, melee(vals, seed), False)
    run(engines, r, melee(vals, seed + 100), True)
    inline = [v for v in vals if not V.is_long(v)]
    if r.text and len(inline) != len(vals):  # the melee the mixed-class fast bodies can hold
        run(engines, r, melee(inline, seed), False)
        run(engines, r, melee(inline, seed + 100), True)


@pytest.mark.parametrize("split", [False, True], ids=["one_apply", "two_applies"])
@pytest.mark.parametrize("route", [r.name for r in ROUTES])
def test_equal_values(engines, route, split):
    """Equal values at equal col_version: the higher site rank wins in either order; the same site
    twice leaves the earlier change in place (flags 1,0). -0.0 and 0.0 are equal."""
    r = BY_NAME[route]
    run(engines, r, V.equal_batch(V.EQUAL_INTEGER if r.int_only else V.EQUAL_WIDE, LO_SITE, HI_SITE), split)


@pytest.mark.parametrize("split", [False, True], ids=["one_apply", "two_applies"])
@pytest.mark.parametrize("route", ["fast_packed", "fast_impact_packed", "gen_small", "wide", "ovf_impact"])
def test_col_version_boundaries(engines, route, split):
    """Duels on col_version around 2^15, 2^31, 2^32 and 2^62 with the value and the site rank
    reversed. One pair per apply: a batch with a col_version of 2^15 or more leaves the packed forms
    (the first pair stays in them, the others take the three-stage / three-word forms)."""
    for pair in V.CV_PAIRS:
        run(engines, BY_NAME[route], V.col_version_batch([pair], LO_SITE, HI_SITE), split)


@pytest.fixture(scope="module", params=[65536, 65537])
def many_sites(request):
    n = request.param
    return (n,) + V.shuffled_sites(n, 11)


@pytest.mark.parametrize("split", [False, True], ids=["one_apply", "two_applies"])
@pytest.mark.parametrize("route", ["fast_packed", "fast_impact_packed"])
def test_site_rank_bit_boundaries(engines, many_sites, route, split):
    """Equal values between sites whose ranks differ across the byte and word ends of the packed
    keys' 16-bit rank field, sites registered in shuffled order (ordinal != rank). With 65537 sites
    the packed forms are off (ranks no longer fit 16 bits) and rank 0x10000 must beat 0xFFFF."""
    n, sites, rank, ordinal = many_sites
    ranks = [(0, 1), (0xFF, 0x100), (0x7FFF, 0x8000), (0xFFFE, 0xFFFF)] + ([(0xFFFF, 0x10000)] if n > 65536 else [])
    contests = []
    for lo, hi in ranks:
        a, b = (7, 1, int(ordinal[lo])), (7, 1, int(ordinal[hi]))
        contests.append((a, b, f"site ranks lo={lo:#x} hi={hi:#x} order=lo,hi"))
        contests.append((b, a, f"site ranks lo={lo:#x} hi={hi:#x} order=hi,lo"))
    run(engines, BY_NAME[route], V.contest_batch(contests), split, sites=sites, rank=rank, tag=n)
