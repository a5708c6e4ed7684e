"""corro_query_rows on the device: a table's live rows selected by column predicates, against SQLite's
recorded answers (tests/golden/query_kats.json) and against the host model (tests/query_model.py) over the
engine's own export(). The tests run in file order; the first is the shape whose host code once crashed.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import corrosion_amd as ca
import synth
from corrosion_amd import _lib as L
from corrosion_amd import engine as E
from corrosion_amd._twopass import TwoPass
from tests import query_gen as G
from tests import query_model as M
from tests.test_query_gen import KEYED_SEED, TABLE_SEED
from tests.test_query_model import dec, same

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
E_INVALID, E_DEVICE, E_UNKNOWN_TABLE, E_RANGE = -1, -3, -4, -6


def py_batch(changes):
    """changes: (table, pk, cid, col_version, db_version, cl, seq, site, Python value) -> a host batch"""
    cells = [E.value_cell(c[8]) for c in changes]
    a = np.array([[int(x) for x in c[:8]] for c in changes], dtype=object).reshape(-1, 8)
    data, off, size = b"", [], []
    for _ty, _ln, _w0, _w1, b in cells:
        off.append(len(data))
        size.append(len(b) if b else 0)
        data += b or b""
    batch = {"pk": np.array([int(x) & M.M64 for x in a[:, 1]], np.uint64),
             "table_cid": np.array([(int(t) << 16) | int(c) for t, c in zip(a[:, 0], a[:, 2])], np.uint32),
             "col_version": a[:, 3].astype(np.int64), "db_version": a[:, 4].astype(np.int64), "cl": a[:, 5].astype(np.uint32),
             "seq": a[:, 6].astype(np.uint32), "site": a[:, 7].astype(np.uint32),
             "val_type": np.array([c[0] for c in cells], np.uint8), "val_len": np.array([c[1] for c in cells], np.uint8),
             "val0": np.array([c[2] for c in cells], np.uint64), "val1": np.array([c[3] for c in cells], np.uint64)}
    if data:
        batch.update(val_off=np.array(off, np.uint64), val_size=np.array(size, np.uint32), val_data=np.frombuffer(data, np.uint8))
    return batch


def int_rows(table, rows, dbv=1, site=0):
    """INTEGER rows {pk: [values]} of one table as changes (a row without values: its sentinel alone)"""
    ch = []
    for pk, vals in rows.items():
        if not vals:
            ch.append((table, pk, 0, 1, dbv, 1, len(ch), site, None))
        ch += [(table, pk, c + 1, 1, dbv, 1, len(ch) + k, site, v) for k, (c, v) in enumerate(enumerate(vals))]
    return ch


_DTS = {"pk": np.uint64, "cl": np.int64, "val_type": np.uint8, "val_len": np.uint8, "val0": np.uint64, "val1": np.uint64,
        "val_off": np.uint64, "val_size": np.uint32, "val_data": np.uint8, "key_status": np.uint8, "key_index": np.uint32}


def to_host(res):
    """a device result as the host result: numpy arrays of its dtypes, long_values from val_data"""
    out = {k: (np.ascontiguousarray(a.cpu().numpy()).view(_DTS[k]) if hasattr(a, "cpu") else a) for k, a in res.items()}
    if "val_data" in out:
        raw, off, size = out["val_data"].tobytes(), out["val_off"].reshape(-1), out["val_size"].reshape(-1)
        out["long_values"] = {int(i): raw[int(off[i]):int(off[i]) + int(size[i])] for i in np.nonzero(size)[0]}
    return out


def query(eng, table, where=(), columns=(), keys=None, device=False, values=True):
    if keys is not None:
        keys = np.array([int(k) & M.M64 for k in keys], np.uint64)
        if device:
            import torch
            keys = torch.from_numpy(keys.view(np.int64).copy()).to(f"cuda:{eng.device}")
    res = eng.query_rows(table, where, columns, keys=keys, values=values, device=device)
    return to_host(res) if device else res


def query_both(eng, table, where=(), columns=(), keys=None):
    """the query with host arrays and with device arrays; the results must be identical. Returns the host one."""
    h, d = query(eng, table, where, columns, keys), query(eng, table, where, columns, keys, device=True)
    assert sorted(h) == sorted(d)
    for k in h:
        assert h[k] == d[k] if isinstance(h[k], (int, dict)) else np.array_equal(h[k], d[k]), k
    return h


def signed(pks):
    return [int(p) - (1 << 64) if int(p) >> 63 else int(p) for p in pks]


def check_model(eng, table, where, columns, keys=None, live=None, dead=None, types=None):
    """query_both against the model over materialise(export()): pks, cl, the cells as values, key_status, key_index"""
    t = eng.table_index(table)
    name, cols = eng.schema[t]
    if live is None:
        live, dead = M.materialise(eng.export(), eng.schema)
    want = M.query(live.get(t, {}), where, columns, keys=keys, col_names=cols, decl_types=types, dead=dead.get(t, {}),
                   int_pk=name not in eng.interned)
    got = query_both(eng, table, where, columns, keys)
    assert got["nrows"] == len(want["pk"]) and got["pk"].tolist() == want["pk"] and got["cl"].tolist() == want["cl"]
    vals = E.query_values(got)
    assert got["val_type"].shape == (len(want["pk"]), len(columns))
    for r, cells in enumerate(want["cells"]):
        for j, c in enumerate(cells):
            assert same(vals[r][j], M.py_value(c)), (where, r, j)
    if keys is not None:
        assert got["key_status"].tolist() == want["key_status"] and got["key_index"].tolist() == want["key_index"]
    return got


# ---- 1. the shape that crashed --------------------------------------------------------------------

def test_a_fresh_context_that_never_made_a_pk_call_is_queried():
    """INTEGER-pk tables only, one apply, then the query: corro_ctx::pk is still empty (it is sized by the pk
    calls), which is what the removed implementation indexed."""
    eng = ca.MergeEngine({"t0": ["a", "b"], "t1": ["a"]}, capacity_hint=1 << 10)
    eng.register_sites(synth.site_ids(1, 3))
    eng.apply(py_batch(int_rows(0, {1: [10, 20], 2: [30, 40], 3: [50, 60]}) + int_rows(1, {1: [7]})))
    for device in (False, True):
        res = query(eng, "t0", [[("a", ">=", 30)]], ["pk", "b"], device=device)
        assert res["pk"].tolist() == [2, 3] and E.query_values(res) == [[2, 40], [3, 60]]
        res = query(eng, "t1", [[("pk", "=", 1)]], ["a"], keys=[1, 2], device=device)
        assert res["key_status"].tolist() == [1, 0] and E.query_values(res) == [[7]]
    eng.close()


def test_an_interned_table_that_is_marked_and_holds_no_key_is_queried():
    eng = ca.MergeEngine({"tb": ["a"], "ti": ["a"]}, capacity_hint=1 << 10, interned=("tb",))
    eng.register_sites(synth.site_ids(1, 3))
    eng.apply(py_batch(int_rows(1, {5: [50], 6: [60]})))
    for device in (False, True):
        assert query(eng, "tb", [[("a", "=", 1)]], ["a"], device=device)["nrows"] == 0
        assert query(eng, "tb", [], ["pk"], keys=[0, L.CORRO_PK_ABSENT], device=device)["key_status"].tolist() == [0, 0]
        assert query(eng, "ti", [[("a", "<", 60)]], ["pk"], device=device)["pk"].tolist() == [5]
    assert eng.pk_count("tb") == 0
    eng.close()


# ---- 2. every fixture case ------------------------------------------------------------------------

@pytest.fixture(scope="module")
def kats():
    with open(os.path.join(HERE, "golden", "query_kats.json")) as f:
        k = json.load(f)
    eng = ca.MergeEngine({k["table"]: [c[0] for c in k["columns"]]}, capacity_hint=1 << 10)
    eng.register_sites(synth.site_ids(1, 3))
    eng.set_column_types(k["table"], [c[1] for c in k["columns"]])
    eng.set_affinity_policy(k["affinity_policy"])
    ch = []
    for r in k["rows"]:
        ch += [(0, r[0], c + 1, 1, 1, 1, len(ch) + c, 0, dec(v)) for c, v in enumerate(r[1:])]
    eng.apply(py_batch(ch))
    yield k, eng
    eng.close()


@pytest.mark.parametrize("device", [False, True])
def test_every_fixture_case_equals_sqlites_answer(kats, device):
    k, eng = kats
    assert len(k["rows"]) == 18
    ran = 0
    for n, case in enumerate(k["cases"]):
        where = [[tuple([t[0], t[1]] + [dec(v) for v in t[2:]]) for t in g] for g in case["where"]]
        res = query(eng, k["table"], where, case["columns"], device=device)
        assert signed(res["pk"]) == case["pks"], (n, case["where"])
        vals = E.query_values(res)
        assert len(vals) == len(case["values"])
        for got, want in zip(vals, case["values"]):
            assert len(got) == len(want)
            for g, w in zip(got, want):
                assert same(g, dec(w)), (n, case["where"], g, w)
        ran += 1
    assert ran == len(k["cases"]) and ran > 900


# ---- 3. random parity against the model ------------------------------------------------------------

@pytest.fixture(scope="module")
def rnd():
    from tests.test_gpu_pk import _pack
    eng = ca.MergeEngine(G.SCHEMA, capacity_hint=1 << 12, interned=G.INTERNED)
    eng.register_sites(synth.site_ids(1, 3))
    eng.set_column_types("ta", G.TYPES["ta"])
    ids = eng.pk_keys("tc", [_pack([b"key-%d" % k]) for k in range(G.N_ROWS["tc"])])
    assert ids.tolist() == list(range(G.N_ROWS["tc"]))           # pk_of's keys of tc are these ids
    batches, rows = G.history()
    for b in batches:
        eng.apply(py_batch(b))
    live, dead = M.materialise(eng.export(), eng.schema)
    assert {t: sorted(live.get(t, {})) for t in range(3)} == \
        {t: sorted(pk for pk, (s, _v) in rows[n].items() if s == "live") for t, n in enumerate(G.SCHEMA)}
    assert all(len(dead.get(t, {})) > 30 for t in range(3)) and eng.metrics()["arena_bytes"] > 0
    yield eng, rows, live, dead
    eng.close()


def _parity(rnd, queries):
    eng, rows, live, dead = rnd
    assert G.interesting_share(rows, queries) >= 0.5
    hit = 0
    for t, where, columns, keys in queries:
        got = check_model(eng, t, where, columns, keys, live, dead, G.TYPES[t])
        asked = len(live[eng.table_index(t)]) if keys is None else int((got["key_status"] % 2 == 1).sum())
        hit += 0 < got["nrows"] < asked
    assert hit >= len(queries) / 2                               # the device answers are not degenerate either


def test_200_random_predicates_in_the_table_form(rnd):
    _parity(rnd, G.predicates(rnd[1], 200, TABLE_SEED))


def test_100_random_predicates_in_the_keyed_form(rnd):
    _parity(rnd, G.predicates(rnd[1], 100, KEYED_SEED, keyed=True))


# ---- 4. directed shapes ---------------------------------------------------------------------------

WIDE = [f"c{k}" for k in range(1, 128)]


@pytest.fixture(scope="module")
def shapes():
    """t0: pks 1..300 with a = pk; t1: the same pks with a = -pk; none: no rows; wide: 127 columns; ext: the pk extremes"""
    eng = ca.MergeEngine({"t0": ["a", "b"], "t1": ["a"], "none": ["a"], "wide": WIDE, "ext": ["a"]}, capacity_hint=1 << 12)
    eng.register_sites(synth.site_ids(1, 3))
    ch = int_rows(0, {pk: [pk, pk % 3] for pk in range(1, 301)}) + int_rows(1, {pk: [-pk] for pk in range(1, 301)})
    ch += int_rows(3, {pk: [1000 * pk + c for c in range(1, 128)] for pk in (5, 6, 7)})
    ch += int_rows(4, {pk: [k] for k, pk in enumerate((-2**63, -2, -1, 0, 1, 2**63 - 1))})
    eng.apply(py_batch(ch))
    yield eng
    eng.close()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257])
def test_match_counts_and_key_counts_around_the_wave_and_block_sizes(shapes, n):
    res = check_model(shapes, "t0", [[("a", "<=", n)]], ["pk", "a"])
    assert res["nrows"] == n
    keys = [(k * 7) % 320 + 1 for k in range(n)]                 # some past 300: absent
    res = check_model(shapes, "t0", [[("b", "!=", 0)]], ["a"], keys=keys)
    assert len(res["key_status"]) == n


def test_every_row_no_row_the_other_table_and_a_table_without_rows(shapes):
    assert check_model(shapes, "t0", [], ["pk"])["nrows"] == 300
    assert check_model(shapes, "t0", [[("a", ">", 0)]], [])["nrows"] == 300
    assert check_model(shapes, "t0", [[("a", "<", 0)]], ["a"])["nrows"] == 0
    assert check_model(shapes, "t1", [[("a", "<", 0)]], ["a"])["nrows"] == 300      # the same pks, the other tag
    assert check_model(shapes, "t1", [[("a", "=", -7)]], ["pk"])["pk"].tolist() == [7]
    assert check_model(shapes, "none", [], ["pk", "a"])["nrows"] == 0
    assert check_model(shapes, "none", [], ["a"], keys=[1, 2])["key_status"].tolist() == [0, 0]


def test_cids_on_both_sides_of_the_presence_words(shapes):
    for c in (1, 63, 64, 127):
        res = check_model(shapes, "wide", [[(f"c{c}", "=", 6000 + c)]], ["c1", "c63", "c64", "c127", f"c{c}"])
        assert res["pk"].tolist() == [6] and E.query_values(res) == [[6001, 6063, 6064, 6127, 6000 + c]]
    res = check_model(shapes, "wide", [[("c63", ">", 5063), ("c64", "<", 7064)], [("c127", "=", 5127)]], ["c127"])
    assert res["pk"].tolist() == [5, 6]


def test_table_form_order_is_signed_for_an_integer_pk(shapes):
    res = check_model(shapes, "ext", [], ["pk", "a"])
    assert signed(res["pk"]) == [-2**63, -2, -1, 0, 1, 2**63 - 1]
    assert check_model(shapes, "ext", [[("pk", "<", 0)]], ["a"])["nrows"] == 3
    assert signed(check_model(shapes, "ext", [[("pk", ">=", -1.5)], [("pk", "=", "-9223372036854775808")]], [])["pk"]) == \
        [-2**63, -1, 0, 1, 2**63 - 1]


def test_interned_table_order_is_by_id(rnd):
    eng, _rows, live, dead = rnd
    res = check_model(eng, "tc", [], ["pk"], None, live, dead)
    assert res["pk"].tolist() == sorted(live[2]) and res["nrows"] > 300


def test_the_empty_state_answers_nothing():
    eng = ca.MergeEngine({"t0": ["a", "b"]}, capacity_hint=1 << 10)
    for device in (False, True):
        res = query(eng, "t0", [[("a", "=", 1)]], ["pk", "a"], device=device)
        assert res["nrows"] == 0 and res["val_data_len"] == 0 and res["val0"].shape == (0, 2)
        res = query(eng, "t0", [], ["a"], keys=[1, 1, 2], device=device)
        assert res["nrows"] == 0 and res["key_status"].tolist() == [0, 0, 0]
        assert query(eng, "t0", [], ["a"], keys=[], device=device)["nrows"] == 0
    eng.close()


def test_rows_are_found_before_and_after_region_growth():
    """the store of test_rows_whose_probe_wraps_the_regions_end_are_found_before_and_after_growth: one region,
    rows whose probe wraps its end, then a growth that rehashes them"""
    from tests.test_gpu_read_rows import WRAP_PKS, hand_batch
    eng = ca.MergeEngine({"t": ["a", "b", "c", "d"]}, capacity_hint=1 << 10)
    eng.register_sites(synth.site_ids(4, 9))
    first = synth.uniform_batch(3000, 4, 2000, 4, 21)
    wrap = hand_batch([(0, pk, 1 + k % 4, 1, 900, 1, k, k % 4, 7000 + k) for k, pk in enumerate(WRAP_PKS)])
    eng.apply({k: np.concatenate([first[k], wrap[k]]) for k in first})
    where, cols = [[("a", ">=", 7000)], [("b", ">=", 7000)], [("c", ">=", 7000)], [("d", ">=", 7000)]], ["pk", "a", "d"]
    before = check_model(eng, "t", where, cols)
    assert set(WRAP_PKS) <= set(before["pk"].tolist())
    keyed0 = check_model(eng, "t", where, cols, keys=list(WRAP_PKS) + [1, 2, 3])
    m0 = eng.metrics()
    eng.apply(synth.uniform_batch(200000, 4, 60000, 4, 22, pk_base=10**6))
    assert eng.metrics()["region_growths"] > m0["region_growths"]
    after = query_both(eng, "t", where + [[("pk", "<", 0)]], cols, keys=list(WRAP_PKS) + [1, 2, 3])
    assert np.array_equal(after["key_status"], keyed0["key_status"]) and np.array_equal(after["val0"], keyed0["val0"])
    live, dead = M.materialise(eng.export(), eng.schema)
    res = check_model(eng, "t", [[("pk", "<", 10**6), ("a", ">=", 7000)]], cols, None, live, dead)
    assert set(res["pk"].tolist()) <= set(before["pk"].tolist()) and res["nrows"] > 0
    assert check_model(eng, "t", [[("a", "is null"), ("b", "is not null")]], ["b"], None, live, dead)["nrows"] > 1000
    eng.close()


def test_long_values_before_and_after_compaction(rnd):
    eng, _rows, live, dead = rnd
    longs = [[("s", ">", "long-text-value-0003"), ("s", "<=", G.LONG_T[9])], [("b", ">=", G.LONG_B[2])], [("s", "=", G.LONG_T[12])]]
    a = check_model(eng, "ta", longs, ["s", "b", "pk", "s"], None, live, dead, G.TYPES["ta"])
    assert a["val_data_len"] > 0 and (a["val_len"] == E.VAL_LONG).any()
    assert a["val_data_len"] == int(a["val_size"].sum()) == len(a["val_data"])
    plain = query(eng, "ta", longs, ["s", "b", "pk", "s"], values=False)
    assert plain["val_data_len"] == 0 and "val_data" not in plain and np.array_equal(plain["val1"], a["val1"])
    twin = ca.MergeEngine(G.SCHEMA, capacity_hint=1 << 12)      # garbage for the compaction: overwritten long values
    twin.register_sites(synth.site_ids(1, 3))
    twin.apply(py_batch([(1, 1, 1, v, v, 1, 0, 0, "an overwritten long value %d" % v) for v in range(1, 40)]))
    before = check_model(twin, "tb", [[("x", ">", "an overwritten")]], ["x"])
    c = twin.compact_values()
    assert c["arena_after"] < c["arena_before"]
    after = check_model(twin, "tb", [[("x", ">", "an overwritten")]], ["x"])
    assert E.query_values(before) == E.query_values(after) == [["an overwritten long value 39"]]
    twin.close()


# ---- 5. errors and atomicity ----------------------------------------------------------------------

def _code(fn, *a, **kw):
    with pytest.raises(ca.CorroError) as err:
        fn(*a, **kw)
    return err.value.code


_IN_DTS = {"keys": np.uint64, "group_off": np.uint32, "term_col": np.uint32, "term_op": np.uint8, "val_type": np.uint8,
           "val_len": np.uint8, "val0": np.uint64, "val1": np.uint64, "const_off": np.uint64, "const_size": np.uint32,
           "const_data": np.uint8, "proj": np.uint32}
CANARY = 0x5A


class Bound:
    """A keyed query of eight keys over a live context, bound by hand to output arrays of both passes that are
    filled with a canary: every refusal is sent through it and must leave every array as it was. One good
    pass 0 on arrays of its own gives the totals the bound pass 1 needs."""

    def __init__(self, eng, table, where, columns, device, keys=range(1, 9)):
        keys = np.array(list(keys), np.uint64)
        if device:
            import torch
            keys = torch.from_numpy(keys.view(np.int64)).to(f"cuda:{eng.device}")
        self.eng = eng
        self.s, self.keep, self.mem, self.nkeys, self.nproj = eng.query_prepare(table, where, columns, keys=keys)
        self.tp = tp = TwoPass(L.lib().corro_query_rows, (eng._h, C.byref(self.s), self.mem.const), self.mem, L.QueryOut())
        tp.run(0, (("key_status", np.uint8, self.nkeys),))
        self.tot = tp.totals(("nrows", "val_data_len"))
        self.status = np.asarray(tp.result()["key_status"].tolist())
        self.tot["ncells"] = self.tot["nrows"] * self.nproj
        tp.bind((("key_status", np.uint8, self.nkeys), ("key_index", np.uint32, "nrows")) + E._QUERY_ROWS + E._QUERY_CELLS
                + E._QUERY_LONG, self.tot)
        for a, _n in tp.out.values():
            a[...] = CANARY

    def array(self, name, values):
        a = np.ascontiguousarray(values, _IN_DTS[name])
        if self.mem.on_dev:
            import torch
            a = torch.from_numpy(a.view({1: np.uint8, 4: np.int32, 8: np.int64}[a.dtype.itemsize]).copy()).to(self.mem.dev)
        self.keep.append(a)
        return self.mem.ptr(a)

    def untouched(self):
        self.mem.sync()
        for name, (a, _n) in self.tp.out.items():
            assert bool((a == CANARY).all()), name

    def refused(self, code, passes=(0, 1), what=None, **patch):
        """with the input members of `patch` replaced (an array, or None for NULL) and the struct members of
        `what` set, the passes fail with `code` and write nothing; everything is put back afterwards"""
        s, o = self.s, self.tp.o
        old = {k: getattr(s, k) for k in patch}
        scalars = {k: getattr(o if k in ("nrows", "val_data_len") else s, k) for k in (what or {})}
        for k, v in patch.items():
            setattr(s, k, None if v is None else self.array(k, v))
        for k, v in (what or {}).items():
            setattr(o if k in ("nrows", "val_data_len") else s, k, v)
        try:
            for which in passes:
                self.mem.sync()
                assert _code(self.tp.call, which) == code, (which, patch, what)
                self.untouched()
        finally:
            for k, v in {**old, **scalars}.items():
                setattr(o if k in ("nrows", "val_data_len") else s, k, v)


@pytest.mark.parametrize("device", [False, True])
def test_every_refusal_leaves_the_outputs_alone(shapes, rnd, kats, device):
    eng = shapes
    b = Bound(eng, "t0", [[("a", ">", 4), ("b", ">=", 0)]], ["pk", "b"], device)
    assert b.tot == {"nrows": 4, "val_data_len": 0, "ncells": 8} and b.status.tolist() == [3, 3, 3, 3, 1, 1, 1, 1]
    fn, o = L.lib().corro_query_rows, b.tp.o
    # the host's screen, with a live context
    for which in (0, 1):
        for mem in (2, 7, -1):
            assert fn(eng._h, C.byref(b.s), mem, C.byref(o), which) == E_INVALID
        b.untouched()
    for which in (2, -1):
        assert fn(eng._h, C.byref(b.s), b.mem.const, C.byref(o), which) == E_INVALID
    b.untouched()
    for name in ("keys", "group_off", "term_col", "term_op", "val_type", "val_len", "val0", "val1", "proj"):
        b.refused(E_INVALID, **{name: None})
    saved = {k: getattr(o, k) for k in ("key_status", "val_off", "val_size", "val_data")}
    o.key_status = None
    assert _code(b.tp.call, 0) == E_INVALID
    o.key_status = saved["key_status"]
    for k in ("val_off", "val_size"):
        setattr(o, k, None)
        assert _code(b.tp.call, 1) == E_INVALID
        setattr(o, k, saved[k])
    o.val_data, o.val_data_len = None, 5
    assert _code(b.tp.call, 1) == E_INVALID
    o.val_data, o.val_data_len = saved["val_data"], 0
    b.untouched()
    b.refused(E_INVALID, what={"flags": b.s.flags | 8})
    b.refused(E_RANGE, what={"nproj": 257})
    b.refused(E_RANGE, what={"nterms": 65})
    b.refused(E_RANGE, what={"ngroups": 65})
    b.refused(E_RANGE, what={"nkeys": 1 << 31})
    b.refused(E_UNKNOWN_TABLE, what={"table": 5})
    b.refused(E_RANGE, passes=(1,), what={"nrows": 1 << 32})
    b.refused(E_RANGE, passes=(1,), what={"nrows": 1 << 31})                     # times two projected columns
    for wrong in (3, 5):                                                          # a pass 1 given another nrows
        b.refused(E_INVALID, passes=(1,), what={"nrows": wrong})
    b.refused(E_INVALID, passes=(1,), what={"val_data_len": 1})
    # the device's screen: the error word is read before key_status or anything else is written
    b.refused(E_INVALID, term_op=[8, 5])
    b.refused(E_INVALID, val_type=[0, 1])
    b.refused(E_INVALID, val_type=[1, 6])
    b.refused(E_INVALID, val_type=[3, 1], val_len=[17, 0])
    b.refused(E_INVALID, val_len=[255, 0])                                        # a long INTEGER
    b.refused(E_INVALID, val_type=[3, 1], val_len=[255, 0])                       # a long constant, no const_ arrays
    long3 = dict(val_type=[3, 1], val_len=[255, 0], const_off=[0, 0])
    b.refused(E_INVALID, what={"const_data_len": 16}, const_size=[16, 0], const_data=np.zeros(16, np.uint8), **long3)
    b.refused(E_INVALID, what={"const_data_len": 20}, const_size=[21, 0], const_data=np.zeros(20, np.uint8), **long3)
    b.refused(E_INVALID, what={"const_data_len": 20}, const_size=[20, 0], const_data=np.zeros(20, np.uint8),
              **{**long3, "const_off": [1, 0]})
    b.refused(E_INVALID, term_col=[3, 2])                                         # a cid past the table's columns
    b.refused(E_INVALID, proj=[0, 3])
    b.refused(E_INVALID, group_off=[0, 3])                                        # passes nterms
    b.refused(E_INVALID, what={"ngroups": 2}, group_off=[0, 2, 1])                # decreases
    b.refused(E_INVALID, val_type=[2, 1], val0=[0x7FF8000000000000, 0])           # a NaN
    # after all that the bound call itself still answers, into the same arrays
    b.mem.sync()
    b.tp.call(1)
    assert np.asarray(b.tp.out["key_index"][0].tolist()).tolist() == [4, 5, 6, 7]
    assert np.asarray(b.tp.out["pk"][0].tolist()).tolist() == [5, 6, 7, 8]
    # and a good long constant passes the same screen: numbers sort below TEXT, so a > 'zz...' rejects every row
    b.s.const_data_len = 20
    for k, v in dict(const_size=[20, 0], const_data=np.frombuffer(b"z" * 20, np.uint8), **long3).items():
        setattr(b.s, k, b.array(k, v))
    b.mem.sync()
    b.tp.call(0)
    assert (b.tp.o.nrows, np.asarray(b.tp.out["key_status"][0].tolist()).tolist()) == (0, [3] * 8)
    # a term on the key of an interned table, and the portable policy's refusal
    bi = Bound(rnd[0], "tc", [[("u", "is not null"), ("v", "is null")]], ["u"], device, keys=range(8))
    bi.refused(E_INVALID, term_col=[0, 2])
    bi.refused(E_INVALID, term_col=[1, 0])
    _k, keng = kats
    bp = Bound(keng, "t", [[("r", "<", "0.1234567890123456789012345"), ("i", "is not null")]], ["pk", "r"], device)
    keng.set_affinity_policy("portable")                                          # digits past the 19th are dropped
    try:
        bp.refused(E_RANGE)
        bp.refused(E_RANGE, term_col=[1, 1])                                      # any affinity that converts it
        bp.mem.sync()
        bp.s.term_col = bp.array("term_col", [4, 1])                              # a BLOB column converts nothing
        bp.tp.call(0)
    finally:
        keng.set_affinity_policy("sqlite-3.37.2")


def test_malformed_queries_through_the_engine_call(shapes, rnd):
    q = shapes.query_rows
    assert _code(q, "t0", [[("a", "=", float("nan"))]], ["a"]) == E_INVALID
    assert _code(q, 5, [], []) == E_UNKNOWN_TABLE
    assert _code(rnd[0].query_rows, "tc", [[("pk", "=", 1)]], ["u"]) == E_INVALID              # the key of an interned table
    assert _code(rnd[0].query_rows, "tc", [[("u", "=", 1), ("pk", "is null")]], ["u"], keys=np.array([1], np.uint64)) == E_INVALID
    assert _code(rnd[0].query_rows, "tc", [[("pk", "=", 1)]], ["u"], device=True) == E_INVALID


def test_the_caps_are_refused_at_cap_plus_one_and_accepted_at_the_cap(shapes):
    q = shapes.query_rows
    term = ("a", "=", 1)
    assert q("t0", [[term] * 64], ["a"])["pk"].tolist() == [1]
    assert _code(q, "t0", [[term] * 65], ["a"]) == E_RANGE
    assert q("t0", [[("a", "=", k)] for k in range(1, 65)], [])["nrows"] == 64
    assert _code(q, "t0", [[]] * 65, []) == E_RANGE
    res = q("t0", [[("a", "<=", 2)]], ["a", "pk"] * 128)
    assert res["val0"].shape == (2, 256) and res["val0"][1].tolist() == [2] * 256
    assert _code(q, "t0", [], ["a"] * 257) == E_RANGE


def test_the_portable_policy_refuses_a_version_sensitive_constant(kats):
    _k, eng = kats
    sens = "0.1234567890123456789012345"                          # digits past the 19th are dropped
    assert eng.query_rows("t", [[("r", "<", sens)]], ["pk"])["nrows"] >= 0
    eng.set_affinity_policy("portable")
    try:
        assert _code(eng.query_rows, "t", [[("r", "<", sens)]], ["pk"]) == E_RANGE
        assert eng.query_rows("t", [[("r", "<", "0.5")], [("b", "<", sens)]], ["pk"])["nrows"] >= 0   # nothing to convert
    finally:
        eng.set_affinity_policy("sqlite-3.37.2")


def test_a_poisoned_context_is_refused_until_it_is_reset():
    eng = ca.MergeEngine({"t": ["a", "b", "c", "d"]}, capacity_hint=1 << 12)
    eng.register_sites(synth.site_ids(4, 7))
    eng.set_store_limit(1)                    # no heap growth at all
    with pytest.raises(ca.CorroError, match="poisoned"):
        eng.apply(synth.uniform_batch(200000, 4, 150000, 4, 9))
    assert _code(eng.query_rows, "t", [], ["a"]) == E_DEVICE
    eng.reset()
    eng.set_store_limit(0)
    assert query_both(eng, "t", [], ["a"])["nrows"] == 0
    eng.apply(py_batch(int_rows(0, {1: [1, 2, 3, 4]})))
    assert E.query_values(query_both(eng, "t", [[("d", "=", 4)]], ["a", "d"])) == [[1, 4]]
    eng.close()


def test_a_query_leaves_the_state_as_it_was(rnd):
    eng, rows, live, dead = rnd
    m0, c0, n0 = eng.metrics(), eng.count(), eng.pk_count("tc")
    for t, where, columns, keys in G.predicates(rows, 10, 99) + G.predicates(rows, 10, 98, keyed=True):
        query_both(eng, t, where, columns, keys)
    assert M.materialise(eng.export(), eng.schema) == (live, dead)
    m1 = eng.metrics()
    assert (m1["state_rows"], m1["state_records"], m1["arena_bytes"]) == (m0["state_rows"], m0["state_records"], m0["arena_bytes"])
    assert eng.count() == c0 and eng.pk_count("tc") == n0 == G.N_ROWS["tc"]


# ---- 6. behind match_changes ----------------------------------------------------------------------

def test_query_candidates_tells_which_changed_rows_still_satisfy_the_where():
    from corrosion_amd import updates as U, wire
    from corrosion_amd.agent import Agent, Change, ChangeV1, Full
    a = bytes([1] * 16)
    ages = {1: 30, 2: 5, 3: 41, 4: 17, 5: 18}
    changes = [Change("users", pk, "age", age, 1, 1, 0, a, 1) for pk, age in ages.items()]
    changes += [Change("users", 1, "name", "ann", 1, 1, 0, a, 1), Change("posts", 1, "title", "x", 1, 1, 0, a, 1)]
    for k, c in enumerate(changes):
        c.seq = k
    ag = Agent({"users": ["name", "age"], "posts": ["title", "likes"]}, capacity_hint=1 << 12)
    ag.site(a)
    pr, st = ag.process_frames(wire.frames([ChangeV1(a, Full(1, changes, (0, len(changes) - 1), len(changes) - 1, ts=1))]))
    assert (st == 0).all()
    filters = U.MatchFilters(ag.engine, subs=[{"users": ["age"]}])
    res = ag.match_changes(pr, pr.dec, filters)
    got = U.query_candidates(ag.engine, res, "users", [[("age", ">=", 18)]], ["pk", "age", "name"])
    idx = got.pop("cand_index").cpu().numpy()
    assert got["pk"].is_cuda
    got = to_host(got)
    pks = res["cand_pk"].cpu().numpy().view(np.uint64)[idx].tolist()
    assert sorted(pks) == sorted(ages) and len(pks) == len(got["key_status"])
    for pk, status in zip(pks, got["key_status"].tolist()):
        assert status == (1 if ages[pk] >= 18 else 3), pk
    sel = [pks[i] for i in got["key_index"].tolist()]
    assert got["pk"].tolist() == sel
    assert E.query_values(got) == [[pk, ages[pk], "ann" if pk == 1 else None] for pk in sel]
    ag.engine.close()
