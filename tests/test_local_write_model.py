"""The host model of corro_local_write (tests/local_write_model.py) against every cr-sqlite-generated
fixture (tests/golden/local_write_kats.json), and live against the cr-sqlite extension where the reference
tree is present."""
import importlib.util
import os
import random

import pytest

import local_write_model as M

KATS = M.load_kats()
EXT = os.path.join(M.HERE, "..", "..", "reference", "crates", "corro-types", "crsqlite-linux-x86_64.so")


def flat_state(model, vals):
    """The model's state in the fixtures' "state" notation."""
    at = {repr(M.enc(M.dec(v))): k for k, v in enumerate(vals)}
    rows = []
    for t, pk, cid, val, cv, dbv, site, cl, seq in model.export():
        rows.append((t * 128 + cid, pk, at.get(repr(M.enc(val)), -1), cv, dbv, site, cl, seq))
    rows.sort(key=lambda r: (r[0] >> 7, r[1], r[0] & 127))
    return [x for r in rows for x in r]


def unflat(rows8, vals):
    return [(tc >> 7, pk, tc & 127, M.dec(vals[v]), cv, dbv, site, cl, seq) for tc, pk, v, cv, dbv, site, cl, seq in rows8]


def replay(sc, on_tx):
    vals = sc["vals"]
    model = M.Model(sc["tables"])
    for k, st in enumerate(sc["steps"]):
        if "remote" in st:
            rem = M.chunks(st["remote"], 8)
            for tc, pk, v, cv, dbv, site, cl, seq in rem:
                model.dbv[site] = max(model.dbv[site] or 0, dbv)
            if "state" in st and "after" not in st:
                model.replace_rows(unflat(M.chunks(st["state"], 8), vals))
            else:
                model.replace_rows(unflat(M.chunks(st["after"], 8), vals), keys={(tc >> 7, pk) for tc, pk, *_ in rem})
        else:
            on_tx(model, k, st, vals)
        state = flat_state(model, vals)
        if "state" in st:
            assert state == st["state"], (sc["name"], k)
            assert model.dbv == st["dbv"], (sc["name"], k)
        if "dg" in st:
            assert M.digest(state, model.dbv) == st["dg"], (sc["name"], k)


@pytest.mark.parametrize("sc", KATS["scenarios"], ids=[s["name"][:40] for s in KATS["scenarios"]])
def test_model_matches_fixture(sc):
    def on_tx(model, k, st, vals):
        stmts = [(kind, t, pk, [(cid, M.dec(vals[v])) for cid, v in cells]) for kind, t, pk, cells in M.statements(st["tx"])]
        v, last_seq, rows, _ = model.local_write(stmts)
        want = [(tc >> 7, pk, tc & 127, M.dec(vals[x]), cv, cl, seq) for tc, pk, x, cv, cl, seq in M.chunks(st["ch"], 6)]
        assert v == st["v"], (sc["name"], k)
        assert len(rows) == len(want) and all(
            a[:3] == b[:3] and M.same(a[3], b[3]) and a[4:] == b[4:] for a, b in zip(rows, want)), (sc["name"], k, rows, want)
        assert last_seq == (max(r[6] for r in want) if want else 0) or v == 0
        assert len(rows) <= M.bound(sc["tables"], stmts)
    replay(sc, on_tx)


def test_fixture_covers_the_listed_cases():
    names = " | ".join(s["name"] for s in KATS["scenarios"])
    for word in ("pk-only", "BLOB-pk", "affinity", "long values", "K13", "descending", "upserts", "random"):
        assert word in names
    rnd = KATS["scenarios"][-1]
    ntx = sum("tx" in st for st in rnd["steps"])
    assert ntx >= 200 and any("remote" in st for st in rnd["steps"])
    assert max(len(M.statements(st["tx"])) for st in rnd["steps"] if "tx" in st) == 12
    assert os.path.getsize(M.KATS) <= max(os.path.getsize(os.path.join(M.HERE, "golden", f))
                                          for f in os.listdir(os.path.join(M.HERE, "golden")) if f != "local_write_kats.json")


def test_constraint_error_leaves_the_model_untouched():
    model = M.Model(KATS["scenarios"][0]["tables"])
    model.local_write([(M.INSERT, 0, 1, [(1, 5)])])
    before = (sorted(model.export()), list(model.dbv))
    with pytest.raises(M.ConstraintError) as e:
        model.local_write([(M.UPDATE, 0, 1, [(1, 6)]), (M.INSERT, 0, 1, [])])
    assert e.value.op == 1 and (sorted(model.export()), list(model.dbv)) == before


@pytest.mark.skipif(not os.path.exists(EXT), reason="live cross-check needs the reference tree's cr-sqlite extension")
def test_model_matches_the_extension_live():
    spec = importlib.util.spec_from_file_location("make_local_writes", os.path.join(M.HERE, "golden", "make_local_writes.py"))
    G = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(G)
    tables = [{"name": "r", "pk": "integer", "cols": [["a", ""], ["b", "integer"], ["c", "text"], ["d", "real"]]}]
    db = G.Db(EXT, G.SITES[0], tables)
    model = M.Model(tables)
    rng = random.Random(7)
    pool = [None, 0, 1, 1.0, 2.5, "x", "1", "2.50", G.LONG_A, b"\x01"]
    names = ["a", "b", "c", "d"]
    for _ in range(150):
        stmts = []
        alive = {pk: db.live("r", pk) for pk in range(6)}
        for _ in range(rng.randint(1, 12)):
            pk = rng.randrange(6)
            kind = rng.choice([M.UPDATE, M.UPSERT, M.UPSERT, M.DELETE] + ([] if alive[pk] else [M.INSERT]))
            cells = [] if kind == M.DELETE else [(c, rng.choice(pool)) for c in rng.sample([1, 2, 3, 4], rng.randint(1, 4))]
            stmts.append((kind, 0, pk, cells))
            alive[pk] = kind != M.DELETE and (alive[pk] or kind != M.UPDATE)
        v, ch = db.tx([["iusd"[k], "r", pk, [[names[c - 1], G.enc(x)] for c, x in cells]] for k, _, pk, cells in stmts])
        mv, _, rows, _ = model.local_write(stmts)
        want = [(0, pk, 0 if cid == "-1" else names.index(cid) + 1, G.dec(val), cv, cl, seq)
                for _, pk, cid, val, cv, _, _, cl, seq in ch]
        assert mv == v
        assert len(rows) == len(want) and all(a[:3] == b[:3] and M.same(a[3], b[3]) and a[4:] == b[4:]
                                              for a, b in zip(rows, want)), (stmts, rows, want)
