"""Directed edges of corro_extract_changes (csrc/extract.hip): the widths at which the index key
(site, db_version, seq) stops packing into 64 bits, the order and tiling of what comes out, and the
shapes at which the lane-per-need and thread-per-row kernels change blocks.

Every state is a hand-built batch of plain inserts on a small INTEGER-pk table, so its clock rows
carry exactly the (site, db_version, seq, ts) the case names; every extraction is checked by
tests/extract_util.py check_extract against the brute-force model (tests/extract_model.py) over
the engine's exported rows, once with host needs and once with the same needs as CUDA tensors.
Outside the deliberate tie cases every (site, db_version, seq) is unique (asserted), so the order
check binds every row."""
import collections
import ctypes as C

import numpy as np
import pytest

import synth
from tests import extract_model as M
from tests.extract_util import SCHEMA, batch, check_extract, device_needs, host_result, needs_arrays, triples

pytestmark = pytest.mark.gpu

U32, U64, I63 = (1 << 32) - 1, (1 << 64) - 1, (1 << 63) - 1


def new_engine(nsites):
    import corrosion_amd as ca
    e = ca.MergeEngine(SCHEMA, capacity_hint=1 << 16)
    e.register_sites(synth.site_ids(nsites, 21))
    assert e.site_count() == nsites
    return e


def state_rows(e, built, ties=None):
    """The engine's exported rows, which must be the clock rows the case built: `built` triples, each
    once, except the deliberately tied ones ({triple: count})."""
    rows = e.export()
    want = collections.Counter(built)
    assert collections.Counter(triples(rows)) == want
    assert {t: c for t, c in want.items() if c > 1} == (ties or {})
    return rows


def run_both(e, rows, nd, nsites):
    """One need set through both memory kinds, against the model; returns the model's answer."""
    exp = M.extract(rows, nd, nsites)
    check_extract(e.extract_changes(nd), exp, nd)
    dev = e.extract_changes(device_needs(nd))
    assert dev["version"].is_cuda and all(v.is_cuda for v in dev["rows"].values())
    check_extract(dev, exp, nd)
    return exp


def bits(v):
    return max(1, int(v).bit_length())


# ---- key-width ladder ------------------------------------------------------------------------

def ladder_changes(nsites, md, ms):
    """Per site: versions 1, 4, about md / 2, md - 3 and md; the version at md holds seqs up to ms."""
    ch, ts = [], 100
    for s in range(nsites):
        layout = [(1, [2, 0]), (4, [3]), (md // 2 + s, [ms, 0]), (md - 3, [7]), (md, [ms, 5, 0, ms - 1, 1])]
        for v, seqs in layout:
            for q in seqs:                   # applied out of seq order on purpose
                ch.append((s, v, q, ts))
                ts += 1
    return ch


def ladder_needs(nsites, md):
    per = [(0, md), (0, md + 1), (0, 1 << 62), (0, I63), (0, U64), (md, md), (md + 1, U64), (5, 4), (md, 1),
           (5, md // 2 - 1), (1, 1), (2, md - 1), (0, 0)]
    nd = [(s, a, b) for s in range(nsites) for a, b in per]
    return nd + [(nsites, 0, U64), (nsites + 1, 0, U64), (U32, 0, U64)]


# seq filters: on a present seq (5: only in the version at md), on an absent one (6: misses every row
# of every version), up to 2^32 - 1, from 0, a single class, inverted
SEQ_FILTERS = [(5, 5), (6, 6), (2, U32), (0, 3), (0, 0), (9, 8), (0, U32)]

# (nsites, max db_version, max seq, total key bits, db + stb, E_RANGE)
RUNGS = [
    (2, (1 << 30) - 1, U32, 63, 31),          # composite
    (2, (1 << 31) - 1, U32, 64, 32),          # the last composite width
    (2, (1 << 31) - 1, 1 << 31, 64, 32),
    (2, (1 << 32) - 1, U32, 65, 33),          # the first two-sort width
    (2, (1 << 62) - 1, U32, 95, 63),
    (2, I63, U32, 96, 64),                    # the last legal width; site 1 at 2^63 - 1 is the all-ones key
    (4, (1 << 61) - 1, U32, 95, 63),
    (4, (1 << 62) - 2, U32, 96, 64),
    (4, (1 << 62) - 1, U32, 96, 64),          # site 3 at 2^62 - 1: all ones again
    (3, (1 << 62) - 1, U32, 96, 64),          # stb steps at 3 sites (highest ordinal 0b10)
    (5, (1 << 61) - 1, U32, 96, 64),          # and at 5
    (5, (1 << 60) - 1, 9, 67, 63),            # two sorts with a narrow seq
]


@pytest.mark.parametrize("nsites,md,ms,total,dbstb", RUNGS)
def test_key_width_ladder(nsites, md, ms, total, dbstb):
    db, sb, stb = bits(md), bits(ms), bits(nsites - 1)
    assert (db + sb + stb, db + stb) == (total, dbstb) and dbstb <= 64
    ch = ladder_changes(nsites, md, ms)
    e = new_engine(nsites)
    e.apply(batch(ch))
    rows = state_rows(e, [c[:3] for c in ch])
    assert int(rows["db_version"].max()) == md and int(rows["seq"].max()) == ms
    needs = ladder_needs(nsites, md)
    exp = run_both(e, rows, needs_arrays(needs), nsites)
    per = (len(needs) - 3) // nsites
    for s in range(nsites):                    # not vacuous, and the literal shape of the open-ended need
        mine = exp[s * per:(s + 1) * per]
        for k in (0, 1, 3, 4):                 # (0, open) for every open >= md
            assert [g[0] for g in mine[k]] == [md, md - 3, md // 2 + s, 4, 1]
            assert [len(g[3]) for g in mine[k]] == [5, 1, 2, 1, 2]
        assert [g[0] for g in mine[5]] == [md] and mine[6] == [] and mine[7] == [] and mine[9] == []
    assert exp[-3:] == [[], [], []]
    for f in SEQ_FILTERS:
        expf = run_both(e, rows, needs_arrays(needs, [f] * len(needs)), nsites)
        top = expf[(nsites - 1) * per]         # highest ordinal, (0, md)
        assert top[0][:2] == (md, ms)
        assert len(top[0][3]) == {(5, 5): 1, (6, 6): 0, (2, U32): 3, (0, 3): 2, (0, 0): 1, (9, 8): 0, (0, U32): 5}[f]
    e.close()


@pytest.mark.parametrize("nsites,md", [(3, I63), (5, (1 << 62) - 1)])
def test_key_wider_than_64_bits_is_refused_and_the_engine_recovers(nsites, md):
    from corrosion_amd import _lib as L
    assert bits(md) + bits(nsites - 1) == 65
    e = new_engine(nsites)
    e.apply(batch(ladder_changes(nsites, md, 9)))
    nd = needs_arrays(ladder_needs(nsites, md))
    for form in (nd, device_needs(nd)):
        with pytest.raises(L.CorroError) as err:
            e.extract_changes(form)
        assert err.value.code == -6            # CORRO_E_RANGE
    e.reset()
    md2 = (1 << 40) - 1
    ch = ladder_changes(nsites, md2, 9)
    e.apply(batch(ch))
    rows = state_rows(e, [c[:3] for c in ch])
    exp = run_both(e, rows, needs_arrays(ladder_needs(nsites, md2)), nsites)
    assert [g[0] for g in exp[0]] == [md2, md2 - 3, md2 // 2, 4, 1]
    e.close()


# ---- need and row shapes ---------------------------------------------------------------------

def small_state():
    ch = [(s, v, q, 1000 * s + 10 * v + q) for s in range(2) for v in (1, 2, 6) for q in range(v)]
    e = new_engine(2)
    e.apply(batch(ch))
    return e, state_rows(e, [c[:3] for c in ch])


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_only_the_last_need_is_not_empty(n):
    e, rows = small_state()
    empties = [(2, 0, U64), (0, 7, U64), (1, 6, 2), (0, 3, 5), (U32, 1, 6), (1, 0, 0)]
    needs = [empties[i % len(empties)] for i in range(n - 1)] + [(1, 0, U64)]
    for seq in (None, [(0, U32)] * n, [(1, 4)] * n):
        exp = run_both(e, rows, needs_arrays(needs, seq), 2)
        assert all(g == [] for g in exp[:-1]) and [g[0] for g in exp[-1]] == [6, 2, 1]
    e.close()


def test_output_of_exactly_256_and_257_rows():
    sizes = {1: 100, 2: 100, 3: 56, 4: 1}
    ch = [(0, v, (q * 37) % c, v * 1000 + q) for v, c in sizes.items() for q in range(c)]   # seqs permuted
    ch += [(1, 2, q, 7) for q in range(3)]
    e = new_engine(2)
    e.apply(batch(ch))
    rows = state_rows(e, [c[:3] for c in ch])
    for needs, total in (([(0, 1, 3)], 256), ([(0, 1, 4)], 257), ([(0, 1, 2), (1, 9, 9), (0, 3, 3)], 256),
                         ([(0, 4, 4), (0, 1, 3)], 257), ([(0, 1, 3), (0, 1, 4)], 513)):
        exp = run_both(e, rows, needs_arrays(needs), 2)
        assert sum(len(g[3]) for need in exp for g in need) == total
    e.close()


def test_one_version_of_300_rows_under_seq_filters():
    order = [(q * 131) % 300 for q in range(300)]               # a permutation: 131 and 300 are coprime
    assert sorted(order) == list(range(300))
    ch = [(0, 3, q, 5000 + q) for q in order] + [(0, 2, 0, 1), (0, 4, 300, 2), (1, 3, 150, 3)]
    e = new_engine(2)
    e.apply(batch(ch))
    rows = state_rows(e, [c[:3] for c in ch])
    filters = [(0, 0), (299, 299), (1, 298), (300, 400), (0, 299), (150, 150), (255, 256), (0, U32)]
    exp = run_both(e, rows, needs_arrays([(0, 3, 3)] * len(filters), filters), 2)
    assert [len(need[0][3]) for need in exp] == [1, 1, 298, 0, 300, 1, 2, 300]
    assert all(need[0][:3] == (3, 299, 5299) for need in exp)
    exp = run_both(e, rows, needs_arrays([(0, 3, 3), (0, 0, U64)]), 2)                      # no filter
    assert len(exp[0][0][3]) == 300 and [len(g[3]) for g in exp[1]] == [1, 300, 1]
    e.close()


def test_seq_ties_on_the_filter_boundary():
    """A resurrecting column change (cl 3 on a row at cl 1) also writes the row's sentinel clock with
    its own site / db_version / seq: two rows on one (version, seq), twice over."""
    first = [(0, 1, q, 10 + q) for q in range(4)]                # rows pk 1..4 at cl 1
    second = [(0, 2, 4, 24), (0, 2, 5, 25), (0, 2, 6, 26), (0, 2, 7, 27), (0, 2, 8, 28)]
    b2 = batch(second, pk_base=100, cid=2)
    for i, pk in ((1, 1), (3, 2)):                               # seq 5 resurrects pk 1, seq 7 pk 2
        b2["pk"][i], b2["cl"][i] = pk, 3
    e = new_engine(2)
    e.apply(batch(first))
    e.apply(b2)
    tied = {(0, 2, 5): 2, (0, 2, 7): 2}
    rows = state_rows(e, [c[:3] for c in first + second] + list(tied), ties=tied)
    filters = [(5, 5), (4, 5), (5, 6), (5, 7), (6, 6), (7, 7), (6, 7), (0, 4), (8, 9), (0, U32)]
    exp = run_both(e, rows, needs_arrays([(0, 2, 2)] * len(filters), filters), 2)
    assert [len(need[0][3]) for need in exp] == [2, 3, 3, 5, 1, 2, 3, 1, 1, 7]
    run_both(e, rows, needs_arrays([(0, 0, U64), (0, 2, 2), (1, 0, U64)]), 2)
    e.close()


def test_an_empty_site_between_two_neighbours_and_unknown_ordinals():
    ch = [(0, 7, 0, 1), (0, 9, 1, 2), (2, 7, 0, 3), (2, 8, 2, 4), (2, 8, 1, 5), (0, 8, 3, 6)]
    e = new_engine(3)
    e.apply(batch(ch))
    rows = state_rows(e, [c[:3] for c in ch])
    needs = [(s, a, b) for s in (0, 1, 2, 3, 4, U32) for a, b in ((0, U64), (7, 9), (8, 8), (0, 9), (9, U64))]
    for seq in (None, [(0, 2)] * len(needs)):
        exp = run_both(e, rows, needs_arrays(needs, seq), 3)
        assert [g[0] for g in exp[0]] == [9, 8, 7] and [g[0] for g in exp[10]] == [8, 7]
        assert all(need == [] for need in exp[5:10] + exp[15:])
    e.close()


# ---- timestamps ------------------------------------------------------------------------------

def test_ts_is_zero_when_never_tracked():
    ch = [(s, v, q, 0) for s in range(2) for v in (1, 5) for q in range(3)]
    e = new_engine(2)
    e.apply(batch(ch, ts=False))
    rows = state_rows(e, [c[:3] for c in ch])
    nd = needs_arrays([(0, 0, U64), (1, 5, 5), (1, 0, 4)])
    for form in (nd, device_needs(nd)):
        res = host_result(e.extract_changes(form))
        assert len(res["ts"]) == 4 and not res["ts"].any() and len(res["rows"]["ts"]) == 12
        assert not res["rows"]["ts"].any()
    run_both(e, rows, nd, 2)
    run_both(e, rows, needs_arrays([(0, 0, U64), (1, 5, 5)], [(1, 1), (0, 9)]), 2)
    e.close()


def test_ts_tracked_from_the_second_apply_on():
    first = [(0, 3, 0, 0), (0, 3, 1, 0), (0, 2, 0, 0), (1, 3, 0, 0)]
    second = [(0, 3, 2, 50), (0, 3, 3, 40), (0, 4, 0, 9), (1, 3, 1, 77)]
    e = new_engine(2)
    e.apply(batch(first, ts=False))
    e.extract_changes(needs_arrays([(0, 0, U64)]))               # an index built before ts existed
    e.apply(batch(second, pk_base=100))
    rows = state_rows(e, [c[:3] for c in first + second])
    exp = run_both(e, rows, needs_arrays([(0, 0, U64), (1, 0, U64)]), 2)
    assert [(g[0], g[2], [r[M.I_TS] for r in g[3]]) for g in exp[0]] == \
        [(4, 9, [9]), (3, 50, [0, 0, 50, 40]), (2, 0, [0])]
    assert [(g[0], g[2], [r[M.I_TS] for r in g[3]]) for g in exp[1]] == [(3, 77, [0, 77])]
    # MAX(ts) is over the whole version: the filters leave out the row that carries it
    exp = run_both(e, rows, needs_arrays([(0, 3, 3), (0, 3, 3), (1, 3, 3)], [(0, 1), (3, 3), (0, 0)]), 2)
    assert [(need[0][2], [r[M.I_TS] for r in need[0][3]]) for need in exp] == [(50, [0, 0]), (50, [40]), (77, [0])]
    e.close()


# ---- index lifecycle -------------------------------------------------------------------------

def test_index_is_rebuilt_after_reset_with_a_smaller_state_and_another_width():
    e = new_engine(3)
    stages = [
        # composite, 240 rows; two sorts (40 + 32 + 2 bits), 36 rows; composite again, 9 rows
        [(s, v, q, v * 100 + q) for s in range(3) for v in range(1, 21) for q in range(4)],
        [(s, (1 << 40) - 1 - 5 * v, (1 << 31) + q, v + q + 1) for s in range(3) for v in range(4) for q in range(3)],
        [(s, v, 0, 7) for s in range(3) for v in (2, 3, 11)],
    ]
    needs = [(s, a, b) for s in range(3) for a, b in ((0, U64), (1, 20), (12, 20), (3, 11), ((1 << 40) - 11, 1 << 40),
                                                      (21, (1 << 40) - 17), (0, 1))]
    widths = []
    for ch in stages:
        e.apply(batch(ch))
        rows = state_rows(e, [c[:3] for c in ch])
        widths.append(bits(int(rows["db_version"].max())) + bits(int(rows["seq"].max())) + 2)
        exp = run_both(e, rows, needs_arrays(needs), 3)
        assert len(exp[0]) == len({c[1] for c in ch}) and len(exp[0]) >= 3
        run_both(e, rows, needs_arrays(needs, [(0, 1 << 31)] * len(needs)), 3)
        e.reset()
        assert int(e.extract_changes(needs_arrays(needs))["grp_off"][-1]) == 0
    assert widths[0] <= 64 < widths[1] and widths[2] <= 64
    e.close()


def test_output_scratch_regrows_between_two_extractions_of_one_state():
    ch = [(s, v, (q * 7) % 25, v + q) for s in range(2) for v in range(1, 31) for q in range(25)]     # 1500 rows
    e = new_engine(2)
    e.apply(batch(ch))
    rows = state_rows(e, [c[:3] for c in ch])
    few = needs_arrays([(0, 3, 3), (1, 30, 30), (1, 31, 40)], [(24, 24), (0, 1), (0, 9)])
    exp = run_both(e, rows, few, 2)
    assert sum(len(g[3]) for need in exp for g in need) == 3
    many = needs_arrays([(s, a, 30) for s in range(2) for a in range(1, 21)])
    exp = run_both(e, rows, many, 2)
    assert sum(len(g[3]) for need in exp for g in need) == 2 * 25 * sum(range(11, 31))
    run_both(e, rows, few, 2)
    e.close()


# ---- a subset of the row arrays, through the C ABI -----------------------------------------------

def _extract_subset(e, nd, fields, on_dev):
    """corro_extract_changes with only `fields` of out->rows non-NULL; returns those arrays (numpy)."""
    import torch
    from corrosion_amd import _lib as L
    from corrosion_amd.engine import ROW_FIELDS
    lib = L.lib()
    n = len(nd["site"])
    src = device_needs(nd) if on_dev else {k: np.ascontiguousarray(v) for k, v in nd.items()}
    mem = L.CORRO_MEM_DEVICE if on_dev else L.CORRO_MEM_HOST
    tdt = {8: torch.int64, 4: torch.int32}

    def alloc(cnt, dt):
        if on_dev:
            return torch.zeros(max(cnt, 1), dtype=tdt[np.dtype(dt).itemsize], device="cuda")
        return np.zeros(max(cnt, 1), dt)

    def ptr(a):
        return a.data_ptr() if on_dev else a.ctypes.data
    s = L.ExtractIn()
    s.n = n
    for k in ("site", "start", "end", "seq_start", "seq_end"):
        setattr(s, k, ptr(src[k]) if k in src else None)
    o = L.ExtractOut()
    gc, rc = alloc(n, np.uint64), alloc(n, np.uint64)
    o.grp_count, o.row_count = ptr(gc), ptr(rc)
    if on_dev:
        torch.cuda.synchronize()
    L.check(lib.corro_extract_changes(e._h, C.byref(s), mem, C.byref(o), 0))
    gcount = (gc.cpu().numpy() if on_dev else gc)[:n].astype(np.int64)
    rcount = (rc.cpu().numpy() if on_dev else rc)[:n].astype(np.int64)
    go, ro = alloc(n + 1, np.uint64), alloc(n + 1, np.uint64)
    offs = [np.concatenate([[0], np.cumsum(c)]).astype(np.int64) for c in (gcount, rcount)]
    for dst, off in zip((go, ro), offs):
        if on_dev:
            dst.copy_(torch.from_numpy(off))
        else:
            dst[:] = off.astype(np.uint64)
    G, R = int(offs[0][-1]), int(offs[1][-1])
    grp = {k: alloc(G, np.uint64) for k in ("version", "last_seq", "ts", "grp_row_off", "grp_rows")}
    out = {k: alloc(R, ROW_FIELDS[k]) for k in fields}
    o.grp_off, o.row_off = ptr(go), ptr(ro)
    for k, a in grp.items():
        setattr(o, k, ptr(a))
    for k, a in out.items():
        setattr(o.rows, k, ptr(a))                               # every other field of o.rows stays NULL
    if on_dev:
        torch.cuda.synchronize()
    L.check(lib.corro_extract_changes(e._h, C.byref(s), mem, C.byref(o), 1))
    return {k: (a.cpu().numpy().view(ROW_FIELDS[k]) if on_dev else a)[:R] for k, a in out.items()}, R


@pytest.mark.parametrize("on_dev", [False, True])
def test_pass_1_with_only_seq_db_version_and_site(on_dev):
    ch = [(s, v, (q * 3) % 10, v + q) for s in range(3) for v in (1, 2, 50) for q in range(10)]
    e = new_engine(3)
    e.apply(batch(ch))
    rows = state_rows(e, [c[:3] for c in ch])
    nd = needs_arrays([(2, 0, U64), (0, 2, 50), (1, 3, 49), (1, 1, 1)], [(0, 9), (2, 7), (0, 9), (9, 9)])
    exp = run_both(e, rows, nd, 3)
    full = host_result(e.extract_changes(nd))
    got, R = _extract_subset(e, nd, ("seq", "db_version", "site"), on_dev)
    assert R == sum(len(g[3]) for need in exp for g in need) == 30 + 12 + 0 + 1
    for k in ("seq", "db_version", "site"):
        assert np.array_equal(got[k], full["rows"][k]), k
    e.close()
