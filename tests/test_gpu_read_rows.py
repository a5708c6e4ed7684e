"""corro_read_rows on the device: rows read by (table, pk) against the engine's own export(), grouped by
(table, pk) on the host and ordered sentinel first, then by cid. Every read runs with host arrays and
with device arrays and the two results must be equal bit for bit. A long value compares by its bytes
wherever two engines (or two arena generations) are compared, by its handle inside one state.
"""
import ctypes as C

import numpy as np
import pytest

import corrosion_amd as ca
import synth
from corrosion_amd import _lib as L
from corrosion_amd._twopass import Mem, TwoPass
from corrosion_amd import engine as E

pytestmark = pytest.mark.gpu

ROW_KEYS = ("table_cid", "pk", "val_type", "val0", "val1", "val_len", "col_version", "db_version", "site", "cl",
            "seq", "ts")
ABSENT = L.CORRO_PK_ABSENT


def _tuples(rows, by_bytes):
    """one tuple per row in ROW_KEYS order; by_bytes: a long value's val1 is its bytes, not its handle"""
    cols = [np.asarray(rows[k]).tolist() for k in ROW_KEYS]
    if by_bytes:
        for i, b in rows.get("long_values", {}).items():
            cols[4][i] = b
    return list(zip(*cols))


def by_key(rows, by_bytes=False):
    """{(table, pk): the key's rows, sentinel first then by cid} of an export"""
    out = {}
    for t in _tuples(rows, by_bytes):
        out.setdefault((t[0] >> 16, t[1]), []).append(t)
    return {k: sorted(v, key=lambda t: t[0] & 0xFFFF) for k, v in out.items()}


def to_host(res):
    """a device result as numpy arrays of the host result's dtypes (long_values from val_data)"""
    dts = {"status": np.uint8, "key_cl": np.int64, "row_off": np.uint64, "val_off": np.uint64, "val_size": np.uint32,
           "val_data": np.uint8, **E.ROW_FIELDS}
    out = {}
    for k, a in res.items():
        out[k] = np.ascontiguousarray(a.cpu().numpy()).view(dts[k]) if hasattr(a, "cpu") else a
    return out


def read_both(eng, tables, pks, values=True):
    """read_rows with host arrays and with device arrays; the results must be identical. Returns the host one."""
    import torch
    tables, pks = np.asarray(tables, np.uint32), np.asarray(pks, np.uint64)
    h = eng.read_rows(tables, pks, values=values)
    dev = f"cuda:{eng.device}"
    d = to_host(eng.read_rows(torch.from_numpy(tables.view(np.int32).copy()).to(dev),
                              torch.from_numpy(pks.view(np.int64).copy()).to(dev), values=values))
    assert sorted(k for k in h if k != "long_values") == sorted(d)
    for k in d:
        assert np.array_equal(np.asarray(h[k]), np.asarray(d[k])), k
    return h


def check_read(eng, tables, pks, want=None, values=True, by_bytes=False):
    """The read of the keys against `want` (by_key of an export; taken from eng when None): each key's rows
    in order, status and cl from the rows' cl, row_off the scan of the counts, absent keys empty."""
    res = read_both(eng, tables, pks, values)
    if want is None:
        want = by_key(eng.export(), by_bytes)
    n = len(pks)
    got = _tuples(res, by_bytes)
    off = res["row_off"].tolist()
    assert len(off) == n + 1 and off[0] == 0 and off[n] == res["nrows"] == len(got)
    for i, (t, p) in enumerate(zip(np.asarray(tables).tolist(), np.asarray(pks).tolist())):
        rows = want.get((t, p), [])
        assert got[off[i]:off[i + 1]] == rows, (i, t, p)
        cl = rows[0][9] if rows else 0
        assert int(res["key_cl"][i]) == cl
        assert int(res["status"][i]) == (0 if not rows else 1 if cl % 2 else 2)
        if rows and cl % 2 == 0:
            assert len(rows) == 1 and rows[0][0] & 0xFFFF == 0     # a deleted row keeps its sentinel alone
    return res


def hand_batch(changes):
    """changes: (table, pk, cid, col_version, db_version, cl, seq, site, value) with INTEGER values"""
    a = np.array([c[:8] + (c[8] & (2**64 - 1),) for c in changes], dtype=object).reshape(-1, 9)
    return {"pk": a[:, 1].astype(np.uint64), "table_cid": ((a[:, 0].astype(np.int64) << 16) | a[:, 2].astype(np.int64)).astype(np.uint32),
            "col_version": a[:, 3].astype(np.int64), "db_version": a[:, 4].astype(np.int64), "cl": a[:, 5].astype(np.uint32),
            "seq": a[:, 6].astype(np.uint32), "site": a[:, 7].astype(np.uint32), "val0": a[:, 8].astype(np.uint64)}


# ---- 1. parity on an adversarial state ------------------------------------------------------------

@pytest.fixture(scope="module")
def adv():
    eng = ca.MergeEngine(synth.adversarial_schema(8), capacity_hint=1 << 16)
    eng.register_sites(synth.site_ids(16, 5))
    for k in range(3):
        eng.apply(synth.adversarial_batch(60000, 16, 8, 3000, 70 + k))
    yield eng, by_key(eng.export())
    eng.close()


def test_parity_on_an_adversarial_state(adv):
    eng, want = adv
    assert any(r[0][9] % 2 == 0 for r in want.values())                          # deleted rows
    assert any(r[0][9] > 1 and r[0][9] % 2 for r in want.values())               # resurrected rows
    assert any(r[0][0] & 0xFFFF for r in want.values())                          # rows without a sentinel
    keys = list(want)
    absent = [(t, p + 10**6) for t, p in keys]
    assert not set(absent) & set(keys)
    allk = keys + absent
    order = np.random.default_rng(1).permutation(len(allk))
    tables = np.array([allk[i][0] for i in order], np.uint32)
    pks = np.array([allk[i][1] for i in order], np.uint64)
    res = check_read(eng, tables, pks, want)
    assert res["nrows"] == sum(len(r) for r in want.values()) == eng.count()


# ---- 2. shape edges -------------------------------------------------------------------------------

EDGE_SCHEMA = {"t0": ["a", "b"], "t1": ["a", "b"], "t2": ["a"], "wide": [f"c{k}" for k in range(1, 128)]}


@pytest.fixture(scope="module")
def edge():
    eng = ca.MergeEngine(EDGE_SCHEMA, capacity_hint=1 << 12)
    eng.register_sites(synth.site_ids(2, 3))
    ch = [(0, 0, 1, 1, 1, 1, 0, 0, 11), (0, 2**63, 2, 1, 1, 1, 1, 0, 12),           # pk 0 and pk 2^63
          (0, 7, 1, 1, 2, 1, 0, 0, 70), (0, 7, 2, 2, 2, 1, 1, 0, 71), (1, 7, 1, 1, 2, 1, 2, 1, -5),   # pk 7: t0, t1, not t2
          (0, 9, 1, 1, 3, 1, 0, 0, 90), (0, 9, 0, 2, 3, 2, 1, 0, 0),                # deleted: sentinel alone
          (0, 10, 1, 1, 4, 1, 0, 1, 100), (0, 10, 0, 2, 4, 2, 1, 1, 0), (0, 10, 0, 3, 4, 3, 2, 1, 0),
          (0, 10, 2, 1, 4, 3, 3, 1, 101)]                                            # resurrected at cl 3
    for pk in (5, 6):                                                                # 127 columns and a sentinel
        ch.append((3, pk, 0, 1, 5, 1, 0, 0, 0))
        ch += [(3, pk, c, c, 5, 1, c, pk % 2, 1000 * pk + c) for c in range(1, 128)]
    eng.apply(hand_batch(ch))
    yield eng, by_key(eng.export())
    eng.close()


EDGE_KEYS = [(0, 7), (3, 5), (3, 6), (3, 5), (1, 7), (2, 7), (0, 0), (0, 2**63), (0, 9), (0, 10), (0, 8), (4, 7),
             (0xFFFFFFFF, 7), (0xFFFF, 0)]


def test_edge_state_is_what_the_cases_need(edge):
    _eng, want = edge
    assert len(want[(3, 5)]) == 128 and [r[0] & 0xFFFF for r in want[(3, 5)]] == list(range(128))
    assert len(want[(0, 9)]) == 1 and want[(0, 9)][0][9] == 2
    assert want[(0, 10)][0][9] == 3 and len(want[(0, 10)]) == 2
    assert (2, 7) not in want and (0, 7) in want and (1, 7) in want


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_key_counts_around_the_wave_and_block_sizes(edge, n):
    eng, want = edge
    keys = [EDGE_KEYS[i % len(EDGE_KEYS)] for i in range(n)]
    res = check_read(eng, [k[0] for k in keys], [k[1] for k in keys], want)
    if n >= 4:      # a 128-record row lies across the first output block's end: rows [2, 130), [130, 258), ...
        assert res["row_off"][:4].tolist() == [0, 2, 130, 258]


def test_tag_compare_edges_deleted_and_resurrected_rows(edge):
    eng, want = edge
    res = check_read(eng, [k[0] for k in EDGE_KEYS], [k[1] for k in EDGE_KEYS], want)
    st = dict(zip(EDGE_KEYS, res["status"].tolist()))
    assert st[(0, 7)] == st[(1, 7)] == 1 and st[(2, 7)] == 0                  # one pk, three tables
    assert st[(0, 0)] == st[(0, 2**63)] == 1
    assert st[(4, 7)] == st[(0xFFFFFFFF, 7)] == st[(0xFFFF, 0)] == 0           # tables past the schema
    assert st[(0, 9)] == 2 and st[(0, 10)] == 1
    assert int(res["key_cl"][EDGE_KEYS.index((0, 10))]) == 3


def test_all_keys_absent_and_one_key_a_thousand_times(edge):
    eng, want = edge
    res = check_read(eng, [0, 1, 2, 3, 9] * 20, list(range(1000, 1100)), want)
    assert res["nrows"] == 0 and not res["status"].any() and not res["row_off"].any()
    res = check_read(eng, [3] * 1000, [6] * 1000, want)
    assert res["nrows"] == 128000 and (res["status"] == 1).all()


def test_empty_state_answers_every_key_with_status_0():
    eng = ca.MergeEngine(EDGE_SCHEMA, capacity_hint=1 << 12)
    res = check_read(eng, [k[0] for k in EDGE_KEYS], [k[1] for k in EDGE_KEYS], {})
    assert res["nrows"] == 0 and res["val_data_len"] == 0
    eng.close()


# ---- 3. after growth ------------------------------------------------------------------------------

_M64 = 2**64 - 1
# pks of table 0 whose region hash (rowhash.h mix64, rowstore.h region_slot) has bits 40..59 all set: their
# home slot is the LAST slot of the region at every region size up to 2^20 slots (found by a host search)
WRAP_PKS = (2000603744, 2001450288, 2001892904, 2005690369, 2005716372, 2007445592)


def _mix64(x):
    x ^= x >> 33
    x = x * 0xff51afd7ed558ccd & _M64
    x ^= x >> 33
    x = x * 0xc4ceb9fe1a85ec53 & _M64
    return x ^ x >> 33


def region_slot(pk, table, log2s):
    """rowstore.h region_slot on the host"""
    return (_mix64((pk * 0xA0761D6478BD642F + table + 0x51) & _M64) >> 40) & ((1 << log2s) - 1)


def test_rows_whose_probe_wraps_the_regions_end_are_found_before_and_after_growth():
    """capacity_hint 2^10 is below the 1280 records that earn a second bucket (corro_ctx_create), so the store
    is ONE region and bucket_of is 0 for every key. The WRAP_PKS all have the region's last slot as their home
    at every size S <= 2^20, so whatever S is, at most one of them lies there and the probe of every other one
    runs over the region's end into slots 0, 1, ...: the occupied run S - 1, 0, 1, ... crosses it. A region
    never has more than 4 slots per row after a growth (it grows to the least size at most half full), so
    S <= 2^20 holds while the state has at most 2^18 rows, which the test asserts."""
    for pk in WRAP_PKS:
        assert all(region_slot(pk, 0, lg) == (1 << lg) - 1 for lg in range(4, 21)), pk
    eng = ca.MergeEngine({"t": ["a", "b", "c", "d"]}, capacity_hint=1 << 10)
    eng.register_sites(synth.site_ids(4, 9))
    first = synth.uniform_batch(3000, 4, 2000, 4, 21)
    wrap = hand_batch([(0, pk, 1 + k % 4, 1, 900, 1, k, k % 4, 7000 + k) for k, pk in enumerate(WRAP_PKS)])
    eng.apply({k: np.concatenate([first[k], wrap[k]]) for k in first})
    keys = np.concatenate([np.unique(first["pk"]), np.array(WRAP_PKS, np.uint64)])
    tables = np.zeros(len(keys), np.uint32)
    before = check_read(eng, tables, keys)
    assert (before["status"][-len(WRAP_PKS):] == 1).all()          # the wrapping rows are found
    m0 = eng.metrics()
    eng.apply(synth.uniform_batch(200000, 4, 60000, 4, 22, pk_base=10**6))
    m1 = eng.metrics()
    assert m1["region_growths"] > m0["region_growths"] and m1["heap_growths"] > m0["heap_growths"]
    assert m1["state_rows"] <= 1 << 18
    after = check_read(eng, tables, keys)                          # rehashed: they wrap at the new size too
    assert (after["status"][-len(WRAP_PKS):] == 1).all()
    for k in ROW_KEYS + ("status", "key_cl", "row_off"):
        assert np.array_equal(before[k], after[k]), k
    # and every key of the grown state
    want = by_key(eng.export())
    allk = list(want)
    res = check_read(eng, [k[0] for k in allk], [k[1] for k in allk], want)
    assert (res["status"] == 1).all() and res["nrows"] == eng.count()
    eng.close()


# ---- 4. long values -------------------------------------------------------------------------------

def _long_engine(seeds):
    eng = ca.MergeEngine(synth.adversarial_schema(8), capacity_hint=1 << 14)
    eng.register_sites(synth.site_ids(16, 5))
    for s in seeds:
        eng.apply(synth.with_long_values(synth.adversarial_batch(8000, 16, 8, 500, s), s + 100))
    return eng


def _check_long(eng):
    exp = eng.export()
    want = by_key(exp)
    keys = list(want) + [(0, 10**7)]
    tables, pks = [k[0] for k in keys], [k[1] for k in keys]
    res = check_read(eng, tables, pks, want, values=True)
    is_long = res["val_len"] == E.VAL_LONG
    assert is_long.any() and (res["val_size"][~is_long] == 0).all()
    idx = np.nonzero(is_long)[0]
    assert (res["val_size"][idx] == (res["val1"][idx] & np.uint64(0xFFFFFF))).all()
    assert res["val_data_len"] == int(res["val_size"].sum()) == len(res["val_data"])
    assert res["long_values"] == dict(zip(idx.tolist(), eng.value_bytes(res["val1"][idx])))
    plain = check_read(eng, tables, pks, want, values=False)
    assert plain["val_data_len"] == 0 and "val_data" not in plain
    assert np.array_equal(plain["val1"], res["val1"])                 # the handle, as in exports
    return by_key(exp, by_bytes=True)


def test_long_values_come_with_their_bytes_before_and_after_compaction():
    eng = _long_engine((31, 32, 33))
    a = _check_long(eng)
    c = eng.compact_values()
    assert c["arena_after"] < c["arena_before"]
    assert _check_long(eng) == a
    eng.close()


# ---- 5. round trip into another engine ------------------------------------------------------------

def test_a_device_read_applies_unchanged_into_an_empty_engine():
    import torch
    a = _long_engine((41, 42))
    want = by_key(a.export(), by_bytes=True)
    keys = list(want)
    dev = f"cuda:{a.device}"
    tables = torch.tensor([k[0] for k in keys], dtype=torch.int32, device=dev)
    pks = torch.from_numpy(np.array([k[1] for k in keys], np.uint64).view(np.int64)).to(dev)
    res = a.read_rows(tables, pks, values=True)
    assert res["val_data_len"] > 0 and res["val_data"].is_cuda
    b = ca.MergeEngine(synth.adversarial_schema(8), capacity_hint=1 << 14)
    b.register_sites(synth.site_ids(16, 5))
    b.apply(E.rows_as_batch(res))
    assert by_key(b.export(), by_bytes=True) == want
    a.close()
    b.close()


# ---- 6. interned pks ------------------------------------------------------------------------------

def _pk_engine(known):
    e = ca.MergeEngine({"tb": ["a"], "ti": ["a"]}, capacity_hint=1 << 12, interned=("tb",))
    e.register_sites(synth.site_ids(2, 4))
    return e, e.pk_keys("tb", known)


@pytest.mark.parametrize("device", [False, True])
def test_pk_find_looks_without_interning(device):
    import torch
    from tests.test_gpu_pk import _pack
    known = [_pack([bytes([k, 3 * k % 256]) * (1 + k % 30)]) for k in range(200)] + [_pack([1])]
    unknown = [_pack([b"no such key %d" % k]) for k in range(40)] + [_pack([2]), _pack(["a text key that is long enough"])]
    e, ids = _pk_engine(known)
    twin, twin_ids = _pk_engine(known)
    assert np.array_equal(ids, twin_ids) and sorted(ids.tolist()) == list(range(len(known)))

    def find(packed):
        if not device:
            return e.pk_find("tb", packed)
        data = torch.frombuffer(bytearray(b"".join(packed)), dtype=torch.uint8).cuda()
        off = torch.tensor(np.cumsum([0] + [len(p) for p in packed]), dtype=torch.int64).cuda()
        return e.pk_find("tb", (data, off)).cpu().numpy().view(np.uint64)
    noncanon = b"\x01\x21\x00\x00\x00\x01"                              # Integer(1) in four bytes
    got = find(known + [noncanon] + unknown)
    assert np.array_equal(got[:len(known)], ids)
    assert got[len(known)] == ids[-1]                                   # found under its canonical form
    assert (got[len(known) + 1:] == np.uint64(ABSENT)).all()
    with pytest.raises(ca.CorroError) as err:
        find([b"\x01\x0b\x05ab"])                                       # malformed: a length past the end
    assert err.value.code == -1
    # the table is as it was: the last key looked up gets the id it gets in a twin that never ran a find
    assert np.array_equal(e.pk_keys("tb", unknown[-1:]), twin.pk_keys("tb", unknown[-1:]))
    assert int(e.pk_keys("tb", unknown[-1:])[0]) == len(known)
    # a table keyed by its INTEGER pk gives the integer back
    assert e.pk_find("ti", [_pack([7]), _pack([-1])]).tolist() == [7, 2**64 - 1]
    e.apply(hand_batch([(0, int(ids[5]), 1, 1, 1, 1, 0, 0, 55)]))
    res = read_both(e, [0, 0, 0], [int(ids[5]), ABSENT, int(ids[6])])
    assert res["status"].tolist() == [1, 0, 0] and res["row_off"].tolist() == [0, 1, 1, 1]
    e.close()
    twin.close()


# ---- 7. behind match_changes ----------------------------------------------------------------------

def test_read_matched_gives_every_candidate_its_current_rows():
    from corrosion_amd import updates as U, wire
    from corrosion_amd.agent import Agent, Change, ChangeV1, Full
    acts = [bytes([k + 1] * 16) for k in range(2)]

    def full(actor, v, changes):
        for k, c in enumerate(changes):
            c.seq = k
        return ChangeV1(actor, Full(v, changes, (0, len(changes) - 1), len(changes) - 1, ts=v))
    a, b = acts
    msgs = [full(a, 1, [Change("users", 1, "name", "ann", 1, 1, 0, a, 1), Change("users", 1, "age", 30, 1, 1, 0, a, 1),
                        Change("users", 2, "age", 5, 3, 1, 0, a, 1), Change("posts", 1, "title", "x", 1, 1, 0, a, 1)]),
            full(b, 1, [Change("users", 2, "name", "bob", 1, 1, 0, b, 1), Change("posts", 1, "-1", None, 2, 1, 0, b, 2),
                        Change("users", 3, "-1", None, 1, 1, 0, b, 1)])]
    ag = Agent({"users": ["name", "age"], "posts": ["title", "likes"]}, capacity_hint=1 << 12)
    for act in acts:
        ag.site(act)
    pr, st = ag.process_frames(wire.frames(msgs))
    assert (st == 0).all()
    filters = U.MatchFilters(ag.engine, subs=[{"users": ["age"]}], updates=["posts", "users"])
    res, rd = ag.read_matched(pr, pr.dec, filters)
    assert res["ncand"] > 0 and rd["pk"].is_cuda
    assert np.array_equal(to_host(U.read_candidates(ag.engine, res))["row_off"], to_host(rd)["row_off"])
    rd = to_host(rd)
    want = by_key(ag.engine.export())
    got = _tuples(rd, False)
    off = rd["row_off"].tolist()
    tables = res["cand_table"].cpu().numpy().view(np.uint32)
    pks = res["cand_pk"].cpu().numpy().view(np.uint64)
    cls = res["cand_cl"].cpu().numpy().view(np.uint32)
    even = 0
    for j in range(res["ncand"]):
        assert got[off[j]:off[j + 1]] == want[(int(tables[j]), int(pks[j]))]
        if cls[j] % 2 == 0:
            even += 1
            assert rd["status"][j] == 2
    assert even
    ag.engine.close()


# ---- 8. refusals ----------------------------------------------------------------------------------

@pytest.mark.parametrize("device", [False, True])
def test_pass_1_with_another_nrows_writes_nothing(edge, device):
    import torch
    eng, _want = edge
    mem = Mem(torch.device(f"cuda:{eng.device}")) if device else Mem()
    tables, pks = np.array([0, 3], np.uint32), np.array([7, 5], np.uint64)
    if device:
        tables = torch.from_numpy(tables.view(np.int32)).to(mem.dev)
        pks = torch.from_numpy(pks.view(np.int64)).to(mem.dev)
    s = L.ReadIn()
    s.n, s.flags = 2, L.CORRO_READ_VALUES
    keep = mem.fill(s, {"table": tables, "pk": pks}, (("table", np.uint32, 2), ("pk", np.uint64, 2)))
    tp = TwoPass(L.lib().corro_read_rows, (eng._h, C.byref(s), mem.const), mem, L.ReadOut())
    tp.run(0, tuple((k, dt, 2, *me) for k, dt, _n, *me in E._READ_PRE))
    tot = tp.totals(("nrows", "val_data_len"))
    assert tot == {"nrows": 130, "val_data_len": 0}
    tp.result()
    tp.bind(E._READ_ROWS + E._READ_LONG[:2], tot)
    for a, _n in tp.out.values():
        a[...] = 0x5A
    for wrong in (129, 131):
        tp.o.nrows = wrong
        mem.sync()
        with pytest.raises(ca.CorroError) as err:
            tp.call(1)
        assert err.value.code == -1
        mem.sync()
        for name, (a, _n) in tp.out.items():
            assert bool((a == 0x5A).all()), name
    tp.o.nrows = 130
    tp.call(1)
    assert not bool((tp.out["rows.pk"][0] == 0x5A).all())
    del keep


def test_unknown_flag_bits_are_refused(edge):
    eng, _want = edge
    for flags in (2, 3, 1 << 31):
        with pytest.raises(ca.CorroError) as err:
            eng.read_rows(np.array([0], np.uint32), np.array([7], np.uint64), flags=flags)
        assert err.value.code == -1


def test_poisoned_context_is_refused_until_reset():
    sites = synth.site_ids(4, 7)
    eng = ca.MergeEngine({"t": ["a", "b", "c", "d"]}, capacity_hint=1 << 12)
    eng.register_sites(sites)
    eng.set_store_limit(1)                    # no heap growth at all
    with pytest.raises(ca.CorroError, match="poisoned"):
        eng.apply(synth.uniform_batch(200000, 4, 150000, 4, 9))
    with pytest.raises(ca.CorroError, match="poisoned") as err:
        eng.read_rows(np.array([0], np.uint32), np.array([1], np.uint64))
    assert err.value.code == -3
    eng.reset()
    eng.set_store_limit(0)
    assert read_both(eng, [0], [1])["status"].tolist() == [0]
    small = synth.uniform_batch(1000, 4, 100, 4, 11)
    eng.apply(small)
    keys = np.unique(small["pk"])
    check_read(eng, np.zeros(len(keys), np.uint32), keys)
    eng.close()


def test_a_read_leaves_the_state_as_it_was(adv):
    eng, want = adv
    rows0, m0 = eng.metrics()["state_rows"], eng.count()
    keys = list(want)[:500]
    read_both(eng, [k[0] for k in keys] * 2, [k[1] for k in keys] * 2)
    assert by_key(eng.export()) == want
    assert eng.metrics()["state_rows"] == rows0 and eng.count() == m0
