"""A subscription's result set on the device (corro_sub_create / _update / _rows, updates.Subscription) against
the host model (tests/sub_model.py), exactly: events, rowids, change ids, cells by storage class and bits, long
values by their bytes. The engine's state is set by local writes; the model reads it through export()."""
import ctypes as C
import random

import numpy as np
import pytest

from corrosion_amd import _lib as L
from corrosion_amd import engine as E
from corrosion_amd import updates as U
from corrosion_amd.agent import Agent
from tests import query_model as M
from tests import sub_model as S

pytestmark = pytest.mark.gpu
ACTOR = bytes(range(1, 17))
E_INVALID = -1
KATS = S.load_kats()
LONG = "a long value, more than sixteen bytes"
_DTS = {"type": np.uint8, "rowid": np.uint64, "change_id": np.uint64, "pk": np.uint64, "val_type": np.uint8,
        "val_len": np.uint8, "val0": np.uint64, "val1": np.uint64, "val_off": np.uint64, "val_size": np.uint32,
        "val_data": np.uint8}


OTHER = bytes(range(31, 47))


def make_agent(schema=None, interned=(), actor=ACTOR):
    ag = Agent(schema or {"t": ["a", "b", "c"], "u": ["a"]}, capacity_hint=1 << 12, actor_id=actor, interned=list(interned))
    for s in (ACTOR, OTHER):                            # (the same site ordinals on every agent)
        ag.site(s)
    return ag


def packed(raw):
    """A BLOB pk's packed column, as Agent.row_keys takes the pk of an interned table."""
    return bytes([1, (1 << 3) | 4, len(raw)]) + raw


def to_host(res):
    out = {k: (np.ascontiguousarray(a.cpu().numpy()).view(_DTS[k]).reshape(tuple(a.shape)) if hasattr(a, "cpu") else a)
           for k, a in res.items()}
    if "long_values" not in out:
        raw, off, size = out["val_data"].tobytes(), out["val_off"].reshape(-1), out["val_size"].reshape(-1)
        out["long_values"] = {int(i): raw[int(off[i]):int(off[i]) + int(size[i])] for i in np.nonzero(size)[0]}
    return out


def cells_of(res):
    n, m = res["val_type"].shape
    lv = res["long_values"]
    return [[E.cell_value(res["val_type"][r, j], res["val_len"][r, j], res["val0"][r, j], res["val1"][r, j], lv.get(r * m + j))
             for j in range(m)] for r in range(n)]


def key_array(keys, device):
    a = np.array([int(k) & M.M64 for k in keys], np.uint64)
    if device:
        import torch
        return torch.from_numpy(a.view(np.int64).copy()).cuda()
    return a


def same_cells(a, b):
    return len(a) == len(b) and all(S.identical(x, y) for x, y in zip(a, b))


class Pair:
    """A device subscription and the model of it, advanced side by side."""

    def __init__(self, ag, table, where=(), columns=("pk", "a", "b"), **caps):
        self.eng, self.where, self.columns = ag.engine, where, list(columns)
        self.t = self.eng.table_index(table)
        self.cols = self.eng.schema[self.t][1]
        self.int_pk = table not in self.eng.interned
        live, _dead = self.state()
        self.model = S.SubModel(S.selected(live, where, self.columns, col_names=self.cols, int_pk=self.int_pk), int_pk=self.int_pk)
        self.sub = U.Subscription(self.eng, table, where, self.columns, **caps)

    def state(self):
        live, dead = M.materialise(self.eng.export(), self.eng.schema)
        return live.get(self.t, {}), dead.get(self.t, {})

    def check_events(self, got, want):
        got = to_host(got)
        assert got["nevents"] == len(want)
        assert [S.TYPES[x] for x in got["type"].tolist()] == [w[0] for w in want]
        assert got["rowid"].tolist() == [w[1] for w in want]
        assert got["change_id"].tolist() == [w[2] for w in want]
        assert got["pk"].tolist() == [w[3] for w in want]
        assert all(same_cells(g, w[4]) for g, w in zip(cells_of(got), want)), (cells_of(got), want)
        assert (got["ninsert"], got["nupdate"], got["ndelete"]) == tuple(sum(w[0] == k for w in want) for k in S.TYPES)
        assert got["val_data_len"] == sum(len(b) for b in got["long_values"].values())

    def update(self, keys, device=False):
        live, dead = self.state()
        want = self.model.update(keys, S.fresh_of(live, keys, self.where, self.columns, col_names=self.cols, dead=dead,
                                                  int_pk=self.int_pk))
        self.check_events(self.sub.update(key_array(keys, device)), want)
        return want

    def check_rows(self, device=False):
        got, want = to_host(self.sub.rows(device=device)), self.model.rows()
        assert got["nrows"] == len(want)
        assert got["rowid"].tolist() == [w[0] for w in want] and got["pk"].tolist() == [w[1] for w in want]
        assert all(same_cells(g, w[2]) for g, w in zip(cells_of(got), want))
        return want

    def close(self):
        self.sub.close()


def kinds(events):
    return [e[0] for e in events]


# ---- create ------------------------------------------------------------------------------------------

def test_an_empty_table_gives_no_rows_and_a_no_op_update():
    ag = make_agent()
    p = Pair(ag, "t")
    assert p.check_rows() == [] and p.check_rows(device=True) == []
    assert p.update([]) == [] and p.update([1, 2, 2]) == [] and p.update([], device=True) == []
    p.close()


def test_create_fills_the_set_in_query_order_with_rowids_from_one():
    ag = make_agent()
    ag.local_write([("insert", "t", k, {"a": k % 7, "b": LONG + str(k) if k % 3 == 0 else "s%d" % k, "c": 1})
                    for k in (5, -3, 900, 17, -2**63, 2**63 - 1, 0, 44, 45, 46)])
    ag.local_write([("delete", "t", 44, {})])
    where = [[("a", ">=", 2)], [("pk", "<", 0)]]
    p = Pair(ag, "t", where, ["b", "pk", "a"])
    for device in (False, True):
        rows = p.check_rows(device)
        q = ag.engine.query_rows("t", where, ["b", "pk", "a"])
        assert [r[1] for r in rows] == q["pk"].tolist() and [r[0] for r in rows] == list(range(1, q["nrows"] + 1))
        assert len(rows) >= 6 and any(isinstance(r[2][0], str) and len(r[2][0]) > 16 for r in rows)
    p.close()


def test_create_over_an_interned_table_orders_by_id():
    ag = make_agent(interned=("u",))
    ag.local_write([("insert", "u", packed(b"key-%d" % k), {"a": k}) for k in (3, 1, 2, 9, 4)])
    p = Pair(ag, "u", [[("a", "!=", 9)]], ["a", "pk"])
    rows = p.check_rows()
    assert [r[1] for r in rows] == [0, 1, 2, 4] and [r[2][0] for r in rows] == [3, 1, 2, 4]
    ag.local_write([("delete", "u", packed(b"key-1"), {}), ("update", "u", packed(b"key-9"), {"a": 8}),
                    ("insert", "u", packed(b"key-77"), {"a": 77})])
    assert kinds(p.update([1, 3, 5, 0], device=True)) == ["Insert", "Insert", "Delete"]
    p.check_rows(device=True)
    p.close()


def test_create_screens_its_query():
    ag = make_agent()
    eng = ag.engine
    h = C.c_void_p()
    for columns, keys in (((), None), (("a",), np.zeros(1, np.uint64))):      # no projection; the keyed form
        s, keep, mem, _n, _m = eng.query_prepare("t", (), columns, keys=keys, values=False)
        assert L.lib().corro_sub_create(eng._h, C.byref(s), mem.const, 0, 0, C.byref(h)) == E_INVALID and h.value is None
    s, keep, mem, _n, _m = eng.query_prepare("t", (), ("a",), values=False)
    assert L.lib().corro_sub_create(eng._h, C.byref(s), 7, 0, 0, C.byref(h)) == E_INVALID
    s.table = 9
    assert L.lib().corro_sub_create(eng._h, C.byref(s), mem.const, 0, 0, C.byref(h)) == -4


# ---- the fixture -------------------------------------------------------------------------------------

@pytest.mark.parametrize("seq", KATS["sequences"], ids=[s["name"] for s in KATS["sequences"]])
@pytest.mark.parametrize("device", [False, True])
def test_every_fixture_round_replays_through_the_engine(seq, device):
    cols = seq["columns"]
    ag = make_agent({"q": cols})
    ag.local_write([("insert", "q", r[0], {c: S.dec(v) for c, v in zip(cols, r[1:])}) for r in seq["initial"]])
    sub = U.Subscription(ag.engine, "q", (), ["pk"] + cols)

    def check_rows(want):
        got = to_host(sub.rows(device=device))
        assert got["rowid"].tolist() == [w[0] for w in want] and [S.signed(k) for k in got["pk"].tolist()] == [w[1] for w in want]
        assert all(same_cells(g, [w[1]] + [S.dec(v) for v in w[2]]) for g, w in zip(cells_of(got), want))

    check_rows(seq["rows"])
    for n, rnd in enumerate(seq["rounds"]):
        fresh = {r[0] for r in rnd["fresh"]}
        stmts = [("upsert", "q", r[0], {c: S.dec(v) for c, v in zip(cols, r[1:])}) for r in rnd["fresh"]]
        stmts += [("delete", "q", k, {}) for k in dict.fromkeys(rnd["keys"]) if k not in fresh]
        if stmts:
            ag.local_write(stmts)
        got = to_host(sub.update(key_array(rnd["keys"], device)))
        want = rnd["events"]
        assert [(S.TYPES[t], r, c, S.signed(k)) for t, r, c, k in zip(got["type"].tolist(), got["rowid"].tolist(),
                                                                   got["change_id"].tolist(), got["pk"].tolist())] == \
            [tuple(e[:4]) for e in want], (seq["name"], n)
        assert all(same_cells(g, [w[3]] + [S.dec(v) for v in w[4]]) for g, w in zip(cells_of(got), want)), (seq["name"], n)
        check_rows(rnd["rows"])
    sub.close()


# ---- transitions and equality ------------------------------------------------------------------------

@pytest.fixture()
def five():
    ag = make_agent()
    ag.local_write([("insert", "t", k, {"a": 10 * k, "b": "v%d" % k, "c": 0}) for k in (1, 2, 3)])
    p = Pair(ag, "t", [[("a", ">", 0)]])
    yield ag, p
    p.close()


def test_nothing_to_a_row_is_an_insert(five):
    ag, p = five
    ag.local_write([("insert", "t", 4, {"a": 40, "b": "v4"})])
    assert [(e[0], e[1], e[2]) for e in p.update([4])] == [("Insert", 4, 1)]
    p.check_rows()


def test_the_same_cells_make_no_event(five):
    ag, p = five
    assert p.update([1, 2, 3]) == []
    p.check_rows()


def test_a_differing_cell_is_an_update_with_the_rows_rowid(five):
    ag, p = five
    ag.local_write([("update", "t", 2, {"b": "other"})])
    assert [(e[0], e[1]) for e in p.update([2])] == [("Update", 2)]
    p.check_rows()


def test_a_row_to_nothing_is_a_delete_with_the_old_cells(five):
    ag, p = five
    ag.local_write([("delete", "t", 1, {}), ("update", "t", 3, {"a": -1, "b": "rejected now"})])
    ev = p.update([1, 3])
    assert [(e[0], e[1], e[4]) for e in ev] == [("Delete", 1, [1, 10, "v1"]), ("Delete", 3, [3, 30, "v3"])]
    p.check_rows()


def test_nothing_to_nothing_makes_no_event(five):
    ag, p = five
    ag.local_write([("insert", "t", 8, {"a": -5}), ("insert", "t", 9, {"a": 5}), ("delete", "t", 9, {})])
    assert p.update([7, 8, 9]) == []


def test_a_change_to_an_unprojected_column_makes_no_event(five):
    ag, p = five
    ag.local_write([("update", "t", 2, {"c": 99})])
    assert p.update([2]) == []
    p.check_rows()


EQUALITY = [  # (stored, written over it, the event)
    (None, None, None), (None, 0, "Update"), (1, 1.0, None), (2**53 + 1, float(2**53), "Update"), (2**53, float(2**53), None),
    (0.0, -0.0, None), ("abc", b"abc", "Update"), (b"abc", b"abc", None), ("abc", "abd", "Update"), ("", b"", "Update"),
    (LONG, LONG, None), (LONG + "x", LONG + "y", "Update"), (LONG, LONG.encode(), "Update"),
    ("abcdefghijklmnop", "abcdefghijklmnopq", "Update"), ("abcdefghijklmnopq", "abcdefghijklmnop", "Update"),
    ("abcdefgh", "abcdefgi", "Update"), ("abcdefghi", "abcdefghj", "Update"), (5.5, 5.5, None), (5.5, 5.25, "Update"),
]


@pytest.mark.parametrize("case", EQUALITY, ids=[repr(c[:2])[:48] for c in EQUALITY])
def test_cell_equality_is_sqlites_is(case):
    old, new, event = case
    ag = make_agent()
    ag.local_write([("insert", "t", 1, {"a": old, "b": 1})])
    p = Pair(ag, "t", (), ["a"])
    ag.local_write([("update", "t", 1, {"a": new, "b": 2})])
    assert kinds(p.update([1])) == ([event] if event else [])
    # the store keeps the old cell of a row that made no event, and gives it back when the row leaves
    ag.local_write([("delete", "t", 1, {})])
    ev = p.update([1], device=True)
    assert kinds(ev) == ["Delete"] and S.identical(ev[0][4][0], new if event else old)
    p.close()


def test_a_long_value_rewritten_with_the_same_bytes_makes_no_event():
    ag = make_agent()
    ag.local_write([("insert", "t", 1, {"a": LONG, "b": 1})])
    p = Pair(ag, "t", (), ["a"])
    h0 = int(ag.engine.query_rows("t", (), ["a"])["val1"][0, 0])
    ag.local_write([("update", "t", 1, {"a": "x" * 40})])
    ag.local_write([("update", "t", 1, {"a": LONG})])
    assert int(ag.engine.query_rows("t", (), ["a"])["val1"][0, 0]) != h0      # (a new arena handle)
    assert p.update([1]) == []
    p.close()


# ---- duplicates, empties, sizes ----------------------------------------------------------------------

def test_duplicate_keys_count_once_and_unknown_keys_make_nothing(five):
    ag, p = five
    ag.local_write([("insert", "t", 4, {"a": 40}), ("delete", "t", 2, {}), ("update", "t", 3, {"b": "new"})])
    ev = p.update([4, 2, 4, 3, 2, 999, 3, 4, -7, 999])
    assert kinds(ev) == ["Update", "Insert", "Delete"]
    assert p.update([]) == [] and p.update([999, -7]) == []
    p.check_rows()


@pytest.mark.parametrize("n", [63, 64, 65, 255, 256, 257])
def test_calls_of_all_inserts_all_updates_and_all_deletes_at_the_wave_and_workgroup_edges(n):
    ag = make_agent()
    p = Pair(ag, "t", (), ["a", "b"])
    keys = [k * 3 - 300 for k in range(n)]
    ag.local_write([("insert", "t", k, {"a": k, "b": LONG + str(k) if k % 5 == 0 else k}) for k in keys])
    assert kinds(p.update(keys + keys[:7], device=True)) == ["Insert"] * n
    ag.local_write([("update", "t", k, {"a": k + 1}) for k in keys])
    assert kinds(p.update(keys)) == ["Update"] * n
    p.check_rows()
    ag.local_write([("delete", "t", k, {}) for k in keys])
    assert kinds(p.update(list(reversed(keys)), device=True)) == ["Delete"] * n
    assert p.check_rows() == []
    p.close()


# ---- growth ------------------------------------------------------------------------------------------

def test_the_table_and_the_arena_grow_from_the_smallest_store():
    ag = make_agent()
    p = Pair(ag, "t", (), ["a", "b"], row_cap=4, val_cap=64)
    keys = list(range(-150, 150))
    ag.local_write([("insert", "t", k, {"a": (LONG + str(k)) * (1 + k % 3), "b": k}) for k in keys])
    assert kinds(p.update(keys)) == ["Insert"] * 300
    rows = p.check_rows()
    assert [r[0] for r in rows] == list(range(1, 301))
    p.check_rows(device=True)
    p.close()


def test_a_long_value_rewritten_until_the_arena_compacts():
    ag = make_agent()
    ag.local_write([("insert", "t", k, {"a": "keep-%d-" % k + "k" * 30, "b": k}) for k in (1, 2, 3)])
    p = Pair(ag, "t", (), ["a", "b"], val_cap=256)
    for n in range(24):
        ag.local_write([("update", "t", 2, {"a": ("round %d " % n) * (3 + n % 4)})])
        assert kinds(p.update([2], device=bool(n % 2))) == ["Update"]
        p.check_rows()
    p.close()


def test_compacting_the_engines_arena_between_two_updates_changes_nothing():
    ag = make_agent()
    ag.local_write([("insert", "t", k, {"a": LONG + str(k), "b": k}) for k in range(20)])
    p = Pair(ag, "t", (), ["a", "b"])
    ag.local_write([("update", "t", k, {"a": "rewritten " + LONG + str(k)}) for k in range(0, 20, 2)])
    assert len(p.update(range(0, 20, 2))) == 10
    before = ag.engine.compact_values()
    assert before["arena_after"] < before["arena_before"]
    assert p.update(range(20)) == []
    p.check_rows()
    ag.local_write([("delete", "t", 4, {})])
    assert kinds(p.update([4])) == ["Delete"]
    p.close()


# ---- the pass protocol -------------------------------------------------------------------------------

TOTALS = ("nevents", "ninsert", "nupdate", "ndelete", "val_data_len")


def test_pass_0_changes_nothing_and_a_wrong_total_is_invalid(five):
    ag, p = five
    ag.local_write([("insert", "t", 4, {"a": 40, "b": LONG}), ("delete", "t", 2, {}), ("update", "t", 3, {"b": "new"})])
    keys = key_array([1, 2, 3, 4], False)
    tp, keep = p.sub.two_pass(keys)
    tp.run(0)
    first = tp.totals(TOTALS)
    tp.run(0)
    assert tp.totals(TOTALS) == first == {"nevents": 3, "ninsert": 1, "nupdate": 1, "ndelete": 1, "val_data_len": len(LONG)}
    p.check_rows()                                      # (the model has not been advanced either)
    for name in TOTALS:
        tp, keep = p.sub.two_pass(keys)
        tp.run(0)
        tot = tp.totals(TOTALS)
        tot["ncells"] = tot["nevents"] * p.sub.nproj
        tp.bind(U._SUB_EVENTS + U._SUB_CELLS + U._SUB_DATA, tot)
        setattr(tp.o, name, getattr(tp.o, name) + 1)
        assert L.lib().corro_sub_update(*tp.lead, C.byref(tp.o), 1) == E_INVALID
        p.check_rows()
    assert kinds(p.update([1, 2, 3, 4])) == ["Update", "Insert", "Delete"]
    p.check_rows()
    o = L.SubRowsOut()
    assert L.lib().corro_sub_rows(p.sub._h, L.CORRO_MEM_HOST, C.byref(o), 0) == 0 and o.nrows == 3
    o.nrows = 4
    assert L.lib().corro_sub_rows(p.sub._h, L.CORRO_MEM_HOST, C.byref(o), 1) == E_INVALID
    assert L.lib().corro_sub_update(p.sub._h, None, 1, L.CORRO_MEM_HOST, C.byref(L.SubEvents()), 0) == E_INVALID
    assert L.lib().corro_sub_update(p.sub._h, keys.ctypes.data, 1 << 31, L.CORRO_MEM_HOST, C.byref(L.SubEvents()), 0) == -6
    # the rest of the screen: a bad pass, a bad mem, pass-1 totals of 2^32 cells or more
    ev, rows = L.SubEvents(), L.SubRowsOut()
    for which in (-1, 2):
        assert L.lib().corro_sub_update(p.sub._h, keys.ctypes.data, 4, L.CORRO_MEM_HOST, C.byref(ev), which) == E_INVALID
        assert L.lib().corro_sub_rows(p.sub._h, L.CORRO_MEM_HOST, C.byref(rows), which) == E_INVALID
    assert L.lib().corro_sub_update(p.sub._h, keys.ctypes.data, 4, 2, C.byref(ev), 0) == E_INVALID
    assert L.lib().corro_sub_rows(p.sub._h, 7, C.byref(rows), 0) == E_INVALID
    for nevents in ((1 << 32) // p.sub.nproj + 1, 1 << 32, 1 << 63):
        ev.nevents = nevents
        assert L.lib().corro_sub_update(p.sub._h, keys.ctypes.data, 4, L.CORRO_MEM_HOST, C.byref(ev), 1) == -6
    p.check_rows()


def test_a_poisoned_context_is_refused_until_it_is_reset():
    import synth
    ag = make_agent({"t": ["a", "b", "c", "d"]})
    ag.engine.register_sites(synth.site_ids(4, 7))
    ag.local_write([("insert", "t", 1, {"a": 1})])
    sub = U.Subscription(ag.engine, "t", (), ["a"])
    ag.engine.set_store_limit(1)                        # no heap growth at all
    with pytest.raises(L.CorroError, match="poisoned"):
        ag.engine.apply(synth.uniform_batch(200000, 4, 150000, 4, 9))
    keys = key_array([1], False)
    for fn in (lambda: sub.update(keys), sub.rows, lambda: U.Subscription(ag.engine, "t", (), ["a"])):
        with pytest.raises(L.CorroError, match="poisoned") as e:
            fn()
        assert e.value.code == -3
    ag.engine.reset()
    ag.engine.set_store_limit(0)
    got = to_host(sub.update(keys))                     # (the set outlives the reset: its row is gone from the state)
    assert [S.TYPES[x] for x in got["type"].tolist()] == ["Delete"] and sub.rows()["nrows"] == 0
    sub.close()


def test_long_values_of_a_hundred_kilobytes_compare_by_all_their_bytes():
    big = "x" * 100_000
    ag = make_agent()
    ag.local_write([("insert", "t", 1, {"a": big + "a", "b": big}), ("insert", "t", 2, {"a": big, "b": 2})])
    p = Pair(ag, "t", (), ["a", "b"], val_cap=64)
    ag.local_write([("update", "t", 1, {"a": "y"}), ("update", "t", 2, {"a": "y"})])
    ag.local_write([("update", "t", 1, {"a": big + "b"}), ("update", "t", 2, {"a": big})])
    ev = p.update([1, 2], device=True)                  # row 1 differs in its last byte, row 2 in nothing
    assert [(e[0], e[3]) for e in ev] == [("Update", 1)]
    p.check_rows()
    p.close()


def test_the_stage_times_of_an_update_are_reported_while_profiling_is_on(five):
    ag, p = five
    ag.local_write([("insert", "t", 4, {"a": 40}), ("delete", "t", 2, {})])
    assert p.sub.last_timings() == {0: {}, 1: {}}
    ag.engine.set_profiling(True)
    p.update([2, 4])
    t = p.sub.last_timings()
    assert list(t[0]) == list(U.Subscription.STAGES[:4]) and list(t[1]) == list(U.Subscription.STAGES)
    assert all(v > 0 for which in t.values() for v in which.values())
    ag.engine.set_profiling(False)


def test_update_subscription_without_a_match_result_says_so(five):
    ag, p = five
    with pytest.raises(ValueError, match="match_changes"):
        ag.update_subscription(p.sub, 0)


# ---- differential ------------------------------------------------------------------------------------

def _value(rng):
    k = rng.randrange(8)
    if k == 0:
        return None
    if k == 1:
        return rng.random() * 100
    if k == 2:
        return "".join(rng.choice("abcxyz") for _ in range(rng.randrange(17, 60)))
    if k == 3:
        return bytes(rng.randrange(256) for _ in range(rng.randrange(0, 24)))
    return rng.randrange(-50, 50)


@pytest.mark.parametrize("device", [False, True], ids=["numpy", "cuda"])
def test_random_transactions_through_match_changes_and_handle_candidates(device):
    rng = random.Random(20261021 + device)
    ag = make_agent()
    eng = ag.engine
    live = set(rng.sample(range(2600), 2000))
    ag.local_write([("insert", "t", k, {"a": rng.randrange(-50, 50), "b": _value(rng), "c": 0}) for k in sorted(live)])
    where = [[("a", ">=", 0), ("a", "<", 40)], [("a", "is null")]]
    p = Pair(ag, "t", where, ["pk", "a", "b"], row_cap=64, val_cap=1024)
    assert 500 < len(p.check_rows()) < 2000
    filters = U.MatchFilters(eng, subs=[{"t": ["a", "b"]}])
    seen = set()
    for rnd in range(20):
        stmts, used = [], set()
        for _ in range(60):
            k = rng.randrange(2600)
            if k in used:
                continue
            used.add(k)
            op = rng.choice(("insert", "update", "upsert", "delete", "c"))
            if op == "c":
                stmts.append(("update", "t", k, {"c": rnd + 1}))
            elif op == "delete":
                stmts.append(("delete", "t", k, {}))
                live.discard(k)
            elif op == "insert" and k in live:
                stmts.append(("update", "t", k, {"a": rng.randrange(-50, 50) if rng.random() < 0.8 else None}))
            else:
                cells = {"a": rng.randrange(-50, 50)} if rng.random() < 0.5 else {"a": rng.randrange(-50, 50), "b": _value(rng)}
                stmts.append((op, "t", k, cells))
                if op != "update":
                    live.add(k)
        ag.local_write(stmts, device=device)
        res = ag.last_local
        n = res["nrows"]
        changes = {k: res[k][:n].contiguous() if device else res[k][:n] for k in ("pk", "table_cid", "cl")}
        if device:
            import torch
            changes["cl"] = changes["cl"].to(torch.int32)            # (corro_rows carries cl as int64)
            imp, cs = torch.ones(n, dtype=torch.uint8, device="cuda"), torch.tensor([[0, n]], dtype=torch.int64, device="cuda")
        else:
            imp, cs = np.ones(n, np.uint8), np.array([[0, n]], np.uint64)
        match = U.match_changes(eng, changes, imp, cs, filters)
        cand = match["cand_pk"].cpu().numpy().view(np.uint64).tolist() if device else match["cand_pk"].tolist()
        state, dead = p.state()
        want = p.model.update(cand, S.fresh_of(state, cand, where, p.columns, col_names=p.cols, dead=dead))
        p.check_events(p.sub.handle_candidates(match, 0), want)
        p.check_rows(device)
        seen.update(kinds(want))
    assert seen == {"Insert", "Update", "Delete"}
    p.close()


# ---- end to end --------------------------------------------------------------------------------------

def test_frames_through_process_frames_match_changes_and_update_subscription():
    a, b = make_agent(), make_agent(actor=OTHER)
    a.local_write([("insert", "t", k, {"a": k, "b": LONG + str(k) if k % 2 else k, "c": 0}) for k in range(1, 9)])
    buf = a.broadcast_frames(cluster_id=3)["buf"]
    b.process_frames(buf.cpu().numpy().tobytes() if hasattr(buf, "is_cuda") else buf.tobytes(), payload=1)
    where = [[("a", "<", 6)]]
    p = Pair(b, "t", where, ["pk", "a", "b"])
    assert len(p.check_rows()) == 5
    filters = U.MatchFilters(b.engine, subs=[{"t": ["a", "b"]}])
    a.local_write([("update", "t", 1, {"b": "changed"}), ("update", "t", 2, {"a": 50}), ("update", "t", 7, {"a": 0}),
                   ("delete", "t", 3, {}), ("update", "t", 4, {"c": 5}), ("insert", "t", -4, {"a": -4, "b": LONG})])
    buf = a.broadcast_frames(cluster_id=3)["buf"]
    res, status = b.process_frames(buf.cpu().numpy().tobytes() if hasattr(buf, "is_cuda") else buf.tobytes(), payload=1)
    assert all(int(s) == 0 for s in status)
    match = b.match_changes(res, res.dec, filters)
    cand = match["cand_pk"].cpu().numpy().view(np.uint64).tolist()
    state, dead = p.state()
    want = p.model.update(cand, S.fresh_of(state, cand, where, p.columns, col_names=p.cols, dead=dead))
    assert kinds(want) == ["Insert", "Update", "Insert", "Delete", "Delete"]
    got = b.update_subscription(p.sub, 0)
    assert got["type"].is_cuda
    p.check_events(got, want)
    p.check_rows(device=True)
    p.close()
