"""corro_local_write on the device against the cr-sqlite-generated fixtures (tests/golden/local_write_kats.json),
against the host model (tests/local_write_model.py) on random and directed shapes, its failure atomicity, and the
round trip local write -> broadcast frames -> another node's process_frames."""
import random
import struct

import numpy as np
import pytest

import local_write_model as M
from corrosion_amd import _lib as L
from corrosion_amd.agent import Agent, Change, encode_value, value_bytes
from corrosion_amd.sync import Full as NeedFull

pytestmark = pytest.mark.gpu

KATS = M.load_kats()
SITES = [bytes.fromhex(h) for h in KATS["sites"]]
KINDS = M.KIND_NAMES
TS = 0x1234_0000_0001


def make_agent(tables, actor=SITES[0]):
    ag = Agent({t["name"]: [c for c, _ in t["cols"]] for t in tables}, capacity_hint=1 << 12, actor_id=actor,
               interned=[t["name"] for t in tables if t["pk"] == "blob"])
    for t in tables:
        if any(ty for _, ty in t["cols"]):
            ag.engine.set_column_types(t["name"], [ty for _, ty in t["cols"]])
    for s in SITES:                                   # ordinals = the fixtures' site indices
        ag.site(s)
    return ag


def pk_of(tables, t, pk, vals):
    """The fixture's pk as Agent.row_keys takes it: an int, or a BLOB pk's packed column."""
    if tables[t]["pk"] != "blob":
        return pk
    raw = M.dec(vals[pk])
    return bytes([1, (1 << 3) | 4, len(raw)]) + raw


def apply_remote(ag, tables, rows, vals):
    """Rows (table, pk, cid, value, cv, dbv, site, cl, seq) merged in order with one apply."""
    ch = [Change(tables[t]["name"], pk_of(tables, t, pk, vals), "-1" if c == 0 else tables[t]["cols"][c - 1][0], v, cv, dbv,
                 seq, SITES[site], cl) for t, pk, c, v, cv, dbv, site, cl, seq in rows]
    n = len(ch)
    b = {k: np.zeros(n, dt) for k, dt in (("table_cid", np.uint32), ("col_version", np.int64), ("db_version", np.int64),
                                           ("cl", np.uint32), ("seq", np.uint32), ("site", np.uint32), ("val0", np.uint64),
                                           ("val1", np.uint64), ("val_type", np.uint8), ("val_len", np.uint8),
                                           ("val_off", np.uint64), ("val_size", np.uint32))}
    b["pk"] = ag.row_keys(ch)
    data = b""
    for j, c in enumerate(ch):
        b["table_cid"][j] = ag.engine.lookup(c.table, c.cid)
        b["col_version"][j], b["db_version"][j], b["cl"][j], b["seq"][j] = c.col_version, c.db_version, c.cl, c.seq
        b["site"][j] = SITES.index(c.site_id)
        b["val_type"][j], b["val0"][j], b["val1"][j], b["val_len"][j] = encode_value(c.val)
        if b["val_len"][j] == L.CORRO_VAL_LONG:
            raw = value_bytes(c.val)
            b["val_off"][j], b["val_size"][j] = len(data), len(raw)
            data += raw
    if data:
        b["val_data"] = np.frombuffer(data, np.uint8)
    else:
        del b["val_off"], b["val_size"]
    ag.engine.apply(b)


def value_of(rows, k, longs):
    ty, ln, w0, w1 = int(rows["val_type"][k]), int(rows["val_len"][k]), int(rows["val0"][k]), int(rows["val1"][k])
    if ty == 5:
        return None
    if ty == 1:
        return w0 - (1 << 64) if w0 >> 63 else w0
    if ty == 2:
        return struct.unpack("<d", struct.pack("<Q", w0))[0]
    b = longs[k] if ln == L.CORRO_VAL_LONG else (w0.to_bytes(8, "big") + w1.to_bytes(8, "big"))[:ln]
    return b.decode() if ty == 3 else bytes(b)


def exported(ag, tables, pk_index=None):
    """export() as sorted (table, pk, cid, value, cv, dbv, site, cl, seq, ts) with Python values; an interned
    table's pk as its BLOB bytes."""
    rows = ag.engine.export()
    out = []
    for k in range(len(rows["pk"])):
        tc = int(rows["table_cid"][k])
        t, pk = tc >> 16, int(rows["pk"][k])
        if tables[t]["pk"] == "blob":
            packed = ag.engine.pk_bytes(tables[t]["name"], np.array([pk], np.uint64))[0]
            pk = packed[3:]
        out.append((t, pk, tc & 0xFFFF, value_of(rows, k, rows["long_values"]), int(rows["col_version"][k]),
                    int(rows["db_version"][k]), int(rows["site"][k]), int(rows["cl"][k]), int(rows["seq"][k]),
                    int(rows["ts"][k])))
    return sorted(out, key=lambda r: (r[0], repr(r[1]), r[2]))


def snapshot(ag, tables):
    """Everything a failed call must leave as it was."""
    return (exported(ag, tables), [int(x) for x in ag.engine.db_versions()], ag.bookie.last(ag.actor_id),
            ag.bookie.needed(ag.actor_id), int(ag.engine.metrics()["arena_bytes"]),
            [ag.engine.pk_count(t["name"]) for t in tables if t["pk"] == "blob"])


def to_statements(tables, stmts, vals=None):
    """Model statements (kind, t, pk, [(cid, value)]) -> Agent.local_write tuples."""
    out = []
    for kind, t, pk, cells in stmts:
        p = pk_of(tables, t, pk, vals) if vals is not None else pk
        out.append((KINDS[kind], tables[t]["name"], p, {tables[t]["cols"][c - 1][0]: v for c, v in cells}))
    return out


def change_tuple(ag, tables, c):
    t = [x["name"] for x in tables].index(c.table)
    cid = 0 if c.cid == "-1" else [n for n, _ in tables[t]["cols"]].index(c.cid) + 1
    pk = c.pk[3:] if tables[t]["pk"] == "blob" else c.pk
    return (t, pk, cid, c.val, c.col_version, c.db_version, SITES.index(c.site_id), c.cl, c.seq)


def same_rows(a, b):
    return len(a) == len(b) and all(x[:3] == y[:3] and M.same(x[3], y[3]) and x[4:] == y[4:] for x, y in zip(a, b))


@pytest.mark.parametrize("sc", KATS["scenarios"], ids=[s["name"][:40] for s in KATS["scenarios"]])
def test_fixture_scenario(sc):
    tables, vals = sc["tables"], sc["vals"]
    ag = make_agent(tables)
    fix_pk = lambda t, pk: M.dec(vals[pk]) if tables[t]["pk"] == "blob" else pk
    last_v = None
    for k, st in enumerate(sc["steps"]):
        where = (sc["name"], k)
        if "remote" in st:
            rows = [(tc >> 7, pk, tc & 127, M.dec(vals[v]), cv, dbv, site, cl, seq)
                    for tc, pk, v, cv, dbv, site, cl, seq in M.chunks(st["remote"], 8)]
            apply_remote(ag, tables, rows, vals)
        else:
            stmts = [(kind, t, pk, [(cid, M.dec(vals[v])) for cid, v in cells]) for kind, t, pk, cells in M.statements(st["tx"])]
            v, last_seq, changes = ag.local_write(to_statements(tables, stmts, vals), ts=TS)
            want = [(tc >> 7, fix_pk(tc >> 7, pk), tc & 127, M.dec(vals[x]), cv, st["v"], 0, cl, seq)
                    for tc, pk, x, cv, cl, seq in M.chunks(st["ch"], 6)]
            got = [change_tuple(ag, tables, c) for c in changes]
            print(where, "v", v, "last_seq", last_seq, "rows", len(got))
            assert v == st["v"], where
            assert same_rows(got, want), (where, got, want)
            raw = ag.last_local
            assert all(int(x) == TS for x in raw["ts"]) and all(int(x) == 0 for x in raw["site"]), where
            if v:
                # (nothing supersedes the transaction's last clock write, so it is among the survivors)
                assert last_seq == max(r[8] for r in want), where
                last_v = v
            else:
                assert last_seq == 0 and changes == [], where
            assert ag.bookie.last(ag.actor_id) == last_v, where
        if "state" in st or "dg" in st:
            got = exported(ag, tables)
            dbv = [None if x < 0 else int(x) for x in ag.engine.db_versions()][:len(SITES)]
            at = {repr(M.enc(M.dec(v))): i for i, v in enumerate(vals)}
            flat = []
            for t, pk, cid, val, cv, dbvv, site, cl, seq, _ts in got:
                p = at.get(repr(M.enc(pk)), -1) if tables[t]["pk"] == "blob" else pk
                flat.append((t * 128 + cid, p, at.get(repr(M.enc(val)), -1), cv, dbvv, site, cl, seq))
            flat.sort(key=lambda r: (r[0] >> 7, r[1], r[0] & 127))
            flat = [x for r in flat for x in r]
            if "state" in st:
                assert flat == st["state"], where
                assert dbv == st["dbv"], where
            if "dg" in st:
                assert M.digest(flat, dbv) == st["dg"], where


def test_last_seq_counts_superseded_writes():
    """insert + delete of a fresh row: the sentinel alone, seq 3, and last_seq = MAX(seq) = 3."""
    tables = KATS["scenarios"][0]["tables"]
    ag = make_agent(tables)
    v, last_seq, ch = ag.local_write([("insert", "t", 1, {"a": 1, "b": 2, "c": 3}), ("delete", "t", 1, {})], ts=TS)
    assert (v, last_seq) == (1, 3) and [(c.cid, c.col_version, c.cl, c.seq) for c in ch] == [("-1", 2, 2, 3)]
    v, last_seq, ch = ag.local_write([("insert", "t", 2, {"a": 1, "b": 2, "c": 3}), ("update", "t", 2, {"a": 5}),
                                      ("delete", "t", 2, {}), ("insert", "t", 2, {"a": 7, "b": 8, "c": 9}),
                                      ("update", "t", 2, {"c": 9, "b": 0})], ts=TS)
    assert (v, last_seq) == (2, 9)
    assert [(c.cid, c.val, c.col_version, c.cl, c.seq) for c in ch] == [
        ("-1", None, 3, 3, 5), ("a", 7, 1, 3, 6), ("c", 9, 1, 3, 8), ("b", 0, 2, 3, 9)]


WIDE = [{"name": "w", "pk": "integer", "cols": [["c%d" % i, "integer" if i == 3 else ""] for i in range(5)]},
        {"name": "x", "pk": "integer", "cols": [["y", ""]]}]


def run_both(ag, model, tables, stmts, device=False):
    """One transaction through the agent and the model; asserts they agree and returns the agent's result."""
    v, last_seq, changes = ag.local_write(to_statements(tables, stmts), ts=TS, device=device)
    mv, mlast, rows, result = model.local_write(stmts)
    raw = ag.last_local_ops
    assert ag.engine.local_bound(raw["kind"], raw["table"], raw["cell_off"]) == M.bound(tables, stmts) >= len(rows)
    got = [change_tuple(ag, tables, c)[:5] + change_tuple(ag, tables, c)[7:] for c in changes]
    want = [r[:5] + r[5:] for r in rows]
    assert (v, last_seq) == (mv, mlast), (stmts, v, last_seq, mv, mlast)
    diff = [(a, b) for a, b in zip(got, want) if not (a[:3] == b[:3] and M.same(a[3], b[3]) and a[4:] == b[4:])]
    assert len(got) == len(want) and not diff, (len(got), len(want), diff[:4], [s for s in stmts if diff and s[2] == diff[0][1][1]])
    res = ag.last_local["op_result"]
    assert [int(x) for x in (res.cpu() if device else res)] == result
    assert all(c.db_version == v for c in changes)
    return v, last_seq, changes


def model_state(model):
    return sorted(((t, pk, cid, val, cv, dbv, site, cl, seq) for t, pk, cid, val, cv, dbv, site, cl, seq in model.export()),
                  key=lambda r: (r[0], repr(r[1]), r[2]))


def assert_state(ag, model, tables):
    got = [r[:9] for r in exported(ag, tables)]
    want = model_state(model)
    assert len(got) == len(want) and all(a[:3] == b[:3] and M.same(a[3], b[3]) and a[4:] == b[4:] for a, b in zip(got, want)), \
        [(a, b) for a, b in zip(got, want) if not (a[:3] == b[:3] and M.same(a[3], b[3]) and a[4:] == b[4:])][:5]


def test_differential_against_the_model():
    """2,000 statements in transactions of 1-64 over 64 rows x 5 columns, host and device arrays alternating."""
    rng = random.Random(11)
    ag, model = make_agent(WIDE), M.Model(WIDE)
    pool = [None, 0, 1, -1, 1.0, 2.5, "x", "1", "01", "seventeen bytes !!", "seventeen bytes !?", b"\x00", 1 << 62]
    left, k = 2000, 0
    while left:
        n = min(left, rng.randint(1, 64))
        left -= n
        stmts, alive = [], {}
        for _ in range(n):
            pk = rng.randrange(64)
            if pk not in alive:
                r = model.rows.get((0, pk))
                alive[pk] = bool(r) and r["L"] % 2 == 1
            kind = rng.choice([M.UPDATE, M.UPDATE, M.UPSERT, M.UPSERT, M.DELETE] + ([] if alive[pk] else [M.INSERT]))
            cells = [] if kind == M.DELETE else [(c, rng.choice(pool)) for c in rng.sample(range(1, 6), rng.randint(1, 5))]
            stmts.append((kind, 0, pk, cells))
            alive[pk] = kind != M.DELETE and (alive[pk] or kind != M.UPDATE)
        run_both(ag, model, WIDE, stmts, device=k % 2 == 1)
        k += 1
    assert_state(ag, model, WIDE)
    assert ag.bookie.last(ag.actor_id) == model.dbv[0] and ag.bookie.needed(ag.actor_id) == []


def test_directed_shapes():
    ag, model = make_agent(WIDE), M.Model(WIDE)
    assert ag.local_write([], ts=TS) == (0, 0, [])                                    # nops = 0
    run_both(ag, model, WIDE, [(M.INSERT, 0, 1, [(1, 5)])])                           # one op
    before = snapshot(ag, WIDE)
    v, last_seq, ch = run_both(ag, model, WIDE, [(M.UPDATE, 0, 1, [(1, 5)]), (M.UPDATE, 0, 1, [(2, None)]),
                                                 (M.DELETE, 0, 9, []), (M.UPDATE, 0, 9, [(1, 1)])])
    assert (v, ch) == (0, []) and snapshot(ag, WIDE) == before                        # only no-ops
    for n in (65, 300):                                                               # many ops on one row
        rng = random.Random(n)
        stmts = []
        for i in range(n):
            kind = rng.choice([M.UPDATE, M.UPSERT, M.UPSERT, M.DELETE])
            stmts.append((kind, 0, 7, [] if kind == M.DELETE else [(c, rng.randrange(3)) for c in rng.sample(range(1, 6), 2)]))
        run_both(ag, model, WIDE, stmts, device=n == 300)
    run_both(ag, model, WIDE, [(M.UPSERT, 0, 1000 + i, [(1 + i % 5, i)]) for i in range(257)])     # 257 one-op rows
    run_both(ag, model, WIDE, [(M.UPDATE, 0, 1000 + i, [(1 + i % 5, i + (i % 3 == 0))]) for i in range(257)], device=True)
    run_both(ag, model, WIDE, [(M.UPDATE, 0, 1, [(5, 1), (4, "2"), (3, "3"), (1, 4)])])             # descending SET list
    run_both(ag, model, WIDE, [(M.INSERT, 1, 1, [(1, 1)]), (M.UPDATE, 0, 1, [(2, 2)]), (M.UPDATE, 1, 1, [(1, 2)]),
                               (M.DELETE, 0, 1, []), (M.UPSERT, 1, 1, [(1, 3)])])                  # one key, two tables
    assert_state(ag, model, WIDE)


def test_127_columns_cross_the_presence_word():
    tables = [{"name": "big", "pk": "integer", "cols": [["c%d" % i, ""] for i in range(127)]}]
    ag, model = make_agent(tables), M.Model(tables)
    v, last_seq, ch = run_both(ag, model, tables, [(M.INSERT, 0, 1, [(63, 1), (64, 2), (65, 3), (127, 4)])])
    assert len(ch) == 127 and last_seq == 126
    run_both(ag, model, tables, [(M.UPDATE, 0, 1, [(127, 5), (65, 3), (64, 9), (63, 9), (1, 0)]), (M.DELETE, 0, 1, []),
                                 (M.UPSERT, 0, 1, [(64, 1)]), (M.UPDATE, 0, 1, [(64, 2), (126, 1)])], device=True)
    assert_state(ag, model, tables)


def raw_ops(kind, table, pk, cell_off, cid, val0):
    n = len(cid)
    return {"kind": np.array(kind, np.uint8), "table": np.array(table, np.uint32), "pk": np.array(pk, np.uint64),
            "cell_off": np.array(cell_off, np.uint64), "cid": np.array(cid, np.uint32), "val0": np.array(val0, np.uint64),
            "val1": np.zeros(n, np.uint64), "val_type": np.ones(n, np.uint8), "val_len": np.zeros(n, np.uint8)}


def test_errors_leave_everything_untouched():
    tables = KATS["scenarios"][9]["tables"]            # t(a, b, c) and the BLOB-pk table bl(x, y)
    assert tables[1]["pk"] == "blob"
    ag = make_agent(tables)
    ag.local_write([("insert", "t", i, {"a": i}) for i in range(50)] + [("insert", "bl", bytes([1, 12, 1, 1]), {"x": "a long value of more than 16 bytes"})], ts=TS)
    before = snapshot(ag, tables)
    stmts = [("upsert", "t", 100 + i, {"a": "another value longer than 16 bytes", "b": i}) for i in range(99)] + [("insert", "t", 7, {"a": 1})]
    with pytest.raises(L.CorroError) as e:
        ag.local_write(stmts, ts=TS)
    assert e.value.code == L.CORRO_E_CONSTRAINT and "op 99" in str(e.value)
    assert snapshot(ag, tables) == before
    assert before[-1] == [1]
    # updates and deletes of unknown BLOB pks only look the keys up: the intern table does not grow, whether
    # the transaction fails or writes nothing (an insert's or upsert's pk is interned before the call:
    # Agent.local_write states the exception)
    unknown = [("update", "bl", bytes([1, 12, 1, 9]), {"x": 1}), ("delete", "bl", bytes([1, 12, 2, 9, 9]), {})]
    with pytest.raises(L.CorroError) as e:
        ag.local_write(unknown + [("insert", "t", 7, {"a": 1})], ts=TS)
    assert e.value.code == L.CORRO_E_CONSTRAINT and "op 2" in str(e.value)
    assert snapshot(ag, tables) == before
    assert ag.local_write(unknown, ts=TS) == (0, 0, []) and snapshot(ag, tables) == before
    site = ag.site(ag.actor_id)
    dup = raw_ops([1], [0], [7], [0, 2], [2, 2], [1, 2])
    bad = [dup, raw_ops([1], [0], [7], [0, 1], [0], [1]), raw_ops([1], [0], [7], [0, 1], [4], [1]),
           raw_ops([3], [0], [7], [0, 1], [1], [1]), raw_ops([4], [0], [7], [0, 0], [], []),
           raw_ops([1], [2], [7], [0, 0], [], [])]
    for ops in bad:
        with pytest.raises(L.CorroError) as e:
            ag.engine.local_write(ops, TS, site, bookie=ag.bookie, actor_id=ag.actor_id)
        assert e.value.code == -1
        assert snapshot(ag, tables) == before
    with pytest.raises(L.CorroError) as e:
        ag.engine.local_write(raw_ops([1], [0], [7], [0, 1], [1], [1]), TS, 99, bookie=ag.bookie, actor_id=ag.actor_id)
    assert e.value.code == -1
    ops = raw_ops([2, 1], [0, 0], [500, 7], [0, 1, 3], [1, 2, 3], [1, 2, 3])           # 3 + 2 rows survive, the bound is 4 + 2
    assert ag.engine.local_bound(ops["kind"], ops["table"], ops["cell_off"]) == 6
    with pytest.raises(L.CorroError) as e:
        ag.engine.local_write(ops, TS, site, bookie=ag.bookie, actor_id=ag.actor_id, cap=4)
    assert e.value.code == -6
    assert snapshot(ag, tables) == before
    res = ag.engine.local_write(ops, TS, site, bookie=ag.bookie, actor_id=ag.actor_id, cap=5)
    assert res["nrows"] == 5 and res["version"] == 2 and ag.bookie.last(ag.actor_id) == 2


def test_broadcast_round_trip_and_serving():
    tables = KATS["scenarios"][9]["tables"]
    a, b = make_agent(tables, SITES[0]), make_agent(tables, SITES[1])
    txs = [[("insert", "t", i, {"a": i, "b": "x" * (i % 40), "c": None}) for i in range(120)] +
           [("insert", "bl", bytes([1, 12, 2, 0, 255]), {"x": b"\x00" * 20, "y": 1.5})],
           [("update", "t", 3, {"a": "y" * 30}), ("delete", "t", 4, {}), ("upsert", "bl", bytes([1, 12, 2, 0, 255]), {"y": 2})],
           [("delete", "t", 3, {}), ("insert", "t", 3, {"b": 1})]]
    for k, stmts in enumerate(txs):
        v, last_seq, changes = a.local_write(stmts, ts=TS + k, device=k == 1)
        enc = a.broadcast_frames(max_buf_size=2048 if k == 0 else None, cluster_id=3)
        buf = enc["buf"]
        assert enc["nframes"] >= (2 if k == 0 else 1)
        res, status = b.process_frames(buf.cpu().numpy().tobytes() if hasattr(buf, "is_cuda") else buf.tobytes(), payload=1)
        assert all(int(s) == 0 for s in status)
        print("round trip", k, "frames", enc["nframes"], "known", res.known, "status", list(status), "ready", res.ready)
        if enc["nframes"] > 1:          # chunks of one version are buffered as partials, then applied once complete
            assert res.ready == [(SITES[0], v)] and [r for _a, _v, r in b.process_ready(res.ready)] == [2]
        assert [r[:9] for r in exported(b, tables)] == [r[:9] for r in exported(a, tables)], (res.known, list(status))
        assert b.bookie.last(SITES[0]) == v
        answers = a.handle_needs([(SITES[0], NeedFull(v, v))], max_buf_size=1 << 30)[0]
        served = [c for m in answers for c in m.changeset.changes]
        key = lambda c: (c.table, bytes(c.pk) if isinstance(c.pk, (bytes, bytearray)) else c.pk, c.cid, c.val, c.col_version,
                         c.db_version, c.seq, c.site_id, c.cl)
        assert [key(c) for c in served] == [key(c) for c in changes]
