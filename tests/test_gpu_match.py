"""corro_match_changes on the device against the host model of match_changes (tests/match_model.py):
exact equality of class_off and the five candidate columns, and of candidates_by_handle against the model's
insertion-ordered dicts. The impact flags are synthetic arrays fed straight in, so the kernels are tested
apart from the merge -- except in the two chain tests at the end.

A case is a list of changesets; a changeset is a list of changes (table, pk, cid, cl, flag). `table` may be
a raw table_cid (an int) for changes the schema does not know. An item ("gap", [changes]) occupies batch rows
that no changeset header covers.
"""
import ctypes as C

import numpy as np
import pytest

from tests import match_model as M

pytestmark = pytest.mark.gpu

SCHEMA = {"t1": ["a"], "t4": ["a", "b", "c", "d"], "t9": [f"c{k}" for k in range(9)]}
TABLES = list(SCHEMA)
S = M.SENTINEL
UNKNOWN = 0xFFFFFFFF


@pytest.fixture(scope="module")
def eng():
    import corrosion_amd as ca
    e = ca.MergeEngine(SCHEMA, capacity_hint=1 << 12)
    yield e
    e.close()


def tcid_of(table, cid):
    if isinstance(table, int):
        return table
    return TABLES.index(table) << 16 | (0 if cid == S else 1 + SCHEMA[table].index(cid))


def layout(case):
    """The batch arrays, the (change_off, change_count) pairs, and per changeset its (batch index, change)
    list."""
    rows, pairs, per_cs = [], [], []
    for item in case:
        if isinstance(item, tuple) and item and item[0] == "gap":
            rows.extend(item[1])
            continue
        pairs.append((len(rows) if item else 0, len(item)))
        per_cs.append([(len(rows) + k, ch) for k, ch in enumerate(item)])
        rows.extend(item)
    arr = {"pk": np.array([r[1] for r in rows], np.uint64),
           "table_cid": np.array([tcid_of(r[0], r[2]) for r in rows], np.uint32),
           "cl": np.array([r[3] for r in rows], np.uint32)}
    imp = np.array([r[4] for r in rows], np.uint8)
    return arr, imp, np.array(pairs, np.uint64).reshape(-1, 2), per_cs


def expected(filters, arr, per_cs):
    """From the model: class_off and the candidate columns, and the per-handle dicts. The candidate's batch
    index is found by running the model a second time with the index in the place of cl."""
    live = [[(i, ch) for i, ch in cs if ch[4] and not isinstance(ch[0], int)] for cs in per_cs]
    by_handle = M.by_handle(filters.handles, [[ch[:4] for _i, ch in cs] for cs in live])
    rep = {}
    for h, c in enumerate(filters.handle_class):
        rep.setdefault(c, filters.handles[h])
    reps = [rep[c] for c in range(filters.nclasses)]
    idx = M.by_handle(reps, [[(ch[0], ch[1], ch[2], i) for i, ch in cs] for cs in live])
    off, change, cs_col = [0], [], []
    for per in idx:
        for s, cands in per:
            won = sorted(i for pks in cands.values() for i in pks.values())
            change += won
            cs_col += [s] * len(won)
        off.append(len(change))
    change = np.array(change, np.int64)
    cols = {"cand_change": change.astype(np.uint32), "cand_cs": np.array(cs_col, np.uint32),
            "cand_table": (arr["table_cid"][change] >> 16).astype(np.uint32), "cand_pk": arr["pk"][change],
            "cand_cl": arr["cl"][change]}
    return np.array(off, np.uint64), cols, by_handle


def ordered(by_handle):
    """dicts as nested lists, so that a comparison sees the insertion order"""
    return [[(s, [(t, list(pks.items())) for t, pks in cands.items()]) for s, cands in per] for per in by_handle]


def to_dev(a):
    import torch
    a = np.ascontiguousarray(a)
    view = {8: np.int64, 4: np.int32, 1: np.uint8}[a.dtype.itemsize]
    return torch.from_numpy(a.view(view).copy()).cuda()


def host(a, dt):
    return (a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)).view(dt)


def run(eng, filters, arr, imp, pairs, device):
    from corrosion_amd import updates
    if device:
        arr, imp = {k: to_dev(a) for k, a in arr.items()}, to_dev(imp)
        pairs = to_dev(pairs).reshape(-1, 2)
    return updates.match_changes(eng, arr, imp, pairs, filters, device=device)


def check(eng, case, subs=(), updates=(), device=True):
    from corrosion_amd import updates as U
    filters = U.MatchFilters(eng, subs=subs, updates=updates)
    arr, imp, pairs, per_cs = layout(case)
    off, cols, by_handle = expected(filters, arr, per_cs)
    res = run(eng, filters, arr, imp, pairs, device)
    assert host(res["class_off"], np.uint64).tolist() == off.tolist()
    assert res["ncand"] == int(off[-1])
    for k, want in cols.items():
        assert host(res[k], want.dtype).tolist() == want.tolist(), k
    assert ordered(U.candidates_by_handle(res, filters)) == ordered(by_handle)
    events = [[(s, M.handle_candidates(c)) for s, c in per] for per in by_handle]
    assert U.notify_events(res, filters) == events
    return res, filters


# ---- the model's literal cases ---------------------------------------------------------------------------

def test_first_taken_change_gives_the_cl(eng):
    res, _ = check(eng, [[("t4", 7, "a", 1, 1), ("t4", 7, "b", 3, 1), ("t4", 7, "b", 5, 1)]], subs=[{"t4": ["b"]}])
    assert host(res["cand_change"], np.uint32).tolist() == [1] and host(res["cand_cl"], np.uint32).tolist() == [3]


def test_sentinel_passes_any_subscription_naming_the_table(eng):
    res, _ = check(eng, [[("t4", 1, S, 2, 1), ("t9", 1, S, 2, 1)]], subs=[{"t4": []}, {"t4": ["a"], "t1": ["a"]}])
    assert host(res["class_off"], np.uint64).tolist() == [0, 1, 2]


def test_update_handle_takes_the_first_change_of_any_column(eng):
    res, _ = check(eng, [[("t4", 9, "d", 1, 1), ("t4", 9, S, 2, 1), ("t9", 9, "c0", 1, 1)]], updates=["t4"])
    assert host(res["cand_change"], np.uint32).tolist() == [0]


def test_one_pk_in_two_tables_gives_two_entries(eng):
    case = [[("t9", 4, "c0", 1, 1), ("t4", 4, "a", 3, 1), ("t9", 5, "c0", 1, 1), ("t9", 4, "c0", 9, 1)]]
    res, f = check(eng, case, subs=[{"t4": ["a"], "t9": ["c0"]}])
    from corrosion_amd import updates as U
    (s, cands), = U.candidates_by_handle(res, f)[0]
    assert s == 0 and list(cands) == ["t9", "t4"] and cands == {"t9": {4: 1, 5: 1}, "t4": {4: 3}}


def test_cl_parity_gives_delete_and_update(eng):
    from corrosion_amd import updates as U
    res, f = check(eng, [[("t1", 1, "a", 2, 1), ("t1", 2, "a", 3, 1)]], updates=["t1"])
    assert U.notify_events(res, f) == [[(0, [(U.DELETE, 1), (U.UPDATE, 2)])]]


# ---- directed ----------------------------------------------------------------------------------------------

def test_changes_without_a_flag_do_not_exist(eng):
    """Non-impactful changes before the first impactful one of a pk: the candidate is the impactful one."""
    case = [[("t4", 3, "a", 1, 0), ("t4", 3, "a", 5, 0), ("t4", 3, "a", 7, 1), ("t4", 3, "a", 9, 1)]]
    res, _ = check(eng, case, updates=["t4"])
    assert host(res["cand_change"], np.uint32).tolist() == [2] and host(res["cand_cl"], np.uint32).tolist() == [7]


def test_dedup_is_per_changeset_and_per_class(eng):
    """The same pk in two changesets: two candidates. The same pk under two classes whose first taken changes
    differ: two different cand_change."""
    case = [[("t4", 1, "a", 1, 1), ("t4", 1, "b", 1, 1)], [("t4", 1, "b", 3, 1)]]
    res, _ = check(eng, case, subs=[{"t4": ["a"]}, {"t4": ["b"]}])
    assert host(res["class_off"], np.uint64).tolist() == [0, 1, 3]
    assert host(res["cand_change"], np.uint32).tolist() == [0, 1, 2]
    assert host(res["cand_cs"], np.uint32).tolist() == [0, 0, 1]


def test_pk_edges_are_ordinary_keys(eng):
    """0, 1, 2^32, 2^64 - 1, and pks equal in their low 32 bits, in one changeset, each twice."""
    pks = [0, 1, 1 << 32, (1 << 64) - 1, 5, (1 << 32) + 5, (7 << 32) + 5, (1 << 63), 0xFFFFFFFF]
    case = [[("t1", p, "a", 1, 1) for p in pks] + [("t1", p, S, 3, 1) for p in reversed(pks)]]
    res, _ = check(eng, case, updates=["t1"])
    assert res["ncand"] == len(pks)


def test_seventy_classes_cross_the_bit_words(eng):
    """70 classes; 31, 32, 63 and 64 (and others) take t9.c3."""
    cols = SCHEMA["t9"]
    rest = [c for c in cols if c != "c3"]             # k + 1 in binary over the other 8 columns: 70 distinct filters
    subs = [{"t9": [rest[b] for b in range(8) if (k + 1) >> b & 1] + (["c3"] if k in (31, 32, 63, 64) else []),
             "t4": ["abcd"[k % 4]] if k % 3 else []} for k in range(70)]
    from corrosion_amd import updates as U
    f = U.MatchFilters(SCHEMA, subs=subs)
    assert f.nclasses == 70 and f.words == 3
    c3 = 1 + len(SCHEMA["t1"]) + 1 + len(SCHEMA["t4"]) + 1 + 3
    for c in (31, 32, 63, 64):
        assert f.bits[c3, c // 32] >> (c % 32) & 1
    rng = np.random.default_rng(5)
    case = [[("t9", int(rng.integers(0, 6)), cols[int(rng.integers(0, 9))], 1 + k, 1) for k in range(40)],
            [("t9", 2, "c3", 1, 1), ("t4", 2, "b", 1, 1)]]
    check(eng, case, subs=subs)


def test_classes_that_take_nothing_are_empty_ranges(eng):
    """A class whose columns no change carries, and one whose table is absent from the batch, in the middle."""
    res, _ = check(eng, [[("t4", 1, "a", 1, 1)]], subs=[{"t4": ["a"]}, {"t4": ["d"]}, {"t9": ["c1"]}, {"t4": ["a", "b"]}])
    assert host(res["class_off"], np.uint64).tolist() == [0, 1, 1, 1, 2]


def test_a_version_of_5000_changes_between_small_and_empty_changesets(eng):
    rng = np.random.default_rng(9)
    tabs = ["t1", "t4", "t9"]

    def change(k):
        t = tabs[int(rng.integers(0, 3))]
        cid = S if rng.random() < 0.1 else SCHEMA[t][int(rng.integers(0, len(SCHEMA[t])))]
        return (t, int(rng.integers(0, 100)), cid, int(rng.integers(1, 9)), int(rng.random() < 0.7))
    big = [change(k) for k in range(5000)]
    case = [[], [], [("t4", 17, "a", 1, 1)], [], big, [], [("t4", 17, "a", 2, 1)], [], []]
    res, _ = check(eng, case, subs=[{"t4": ["a", "c"], "t9": ["c8"]}, {"t1": []}, {"t9": ["c0", "c1"]}], updates=["t4", "t9"])
    assert 4 in host(res["cand_cs"], np.uint32).tolist()


def test_one_key_under_maximal_contention(eng):
    """600 changes that share one (table, pk) under one class: one candidate, the lowest impactful index."""
    case = [[("t4", 42, "abcd"[k % 4], k + 1, int(k >= 3)) for k in range(600)]]
    res, _ = check(eng, case, updates=["t4"])
    assert host(res["cand_change"], np.uint32).tolist() == [3] and host(res["cand_cl"], np.uint32).tolist() == [4]


def test_4096_distinct_pks_fill_the_table_to_its_minimum_load(eng):
    case = [[("t1", (k * 0x9E3779B97F4A7C15) % (1 << 64), "a", 1, 1) for k in range(4096)]]
    res, _ = check(eng, case, updates=["t1"])
    assert res["ncand"] == 4096


def test_changes_the_schema_does_not_know_are_never_candidates(eng):
    """CORRO_TCID_UNKNOWN, a table index past the schema and a cid above its table's, with flag 1, as the last
    changes of the batch: an unchecked index would leave the bit matrix."""
    case = [[("t9", 1, "c8", 1, 1), (2 << 16 | 10, 1, None, 1, 1), (0 << 16 | 2, 1, None, 1, 1),
             (3 << 16, 1, None, 1, 1), (0xFFFF << 16 | 0xFFFF - 1, 1, None, 1, 1), (UNKNOWN, 1, None, 1, 1)]]
    res, _ = check(eng, case, subs=[{"t9": ["c8"]}], updates=["t9", "t1"])
    assert host(res["cand_change"], np.uint32).tolist() == [0, 0]


def test_changes_outside_every_changeset_are_never_candidates(eng):
    case = [("gap", [("t4", 1, "a", 1, 1)]), [("t4", 1, "b", 3, 1)], ("gap", [("t4", 2, "a", 1, 1)] * 3),
            [("t4", 2, "a", 5, 1)], ("gap", [("t4", 9, "a", 1, 1)])]
    res, _ = check(eng, case, updates=["t4"])
    assert host(res["cand_change"], np.uint32).tolist() == [1, 5]


class Raw:
    """One direct call with every output array present and filled with a sentinel."""

    def __init__(self, eng, filters, arr, imp, pairs):
        import torch
        from corrosion_amd import _lib as L
        from corrosion_amd import updates as U
        self.eng, self.L = eng, L
        self.keep = [to_dev(arr["pk"]), to_dev(arr["table_cid"]), to_dev(arr["cl"]), to_dev(imp), filters.device_bits("cuda")]
        rec, ncs, p = U._cs_records(to_dev(pairs).reshape(-1, 2), None, True, "cuda")
        self.keep.append(rec)
        r = L.MatchIn()
        r.n, r.ncs, r.nclasses, r.nslots = len(imp), ncs, filters.nclasses, filters.nslots
        r.pk, r.table_cid, r.cl, r.impactful, r.col_class_bits = (t.data_ptr() for t in self.keep[:5])
        r.cs = p
        self.r = r
        self.o = L.MatchOut()
        self.out = {}
        for name, t in L.MatchOut._fields_:
            if t is C.c_void_p:
                self.out[name] = torch.full((4096,), 7, dtype=torch.uint8, device="cuda")
                setattr(self.o, name, self.out[name].data_ptr())
        torch.cuda.synchronize()

    def __call__(self, which):
        return self.L.lib().corro_match_changes(self.eng._h, C.byref(self.r), self.L.CORRO_MEM_DEVICE, C.byref(self.o), which)

    def untouched(self):
        return all(bool((t == 7).all().item()) for t in self.out.values())


@pytest.mark.parametrize("pairs", [[(2, 2), (0, 2)], [(0, 3), (2, 2)], [(0, 3), (0, 0), (2, 1)], [(0, 5)], [(5, 1)],
                                   [(0, 2), (3, (1 << 64) - 2)]], ids=str)
def test_device_ranges_that_descend_overlap_or_leave_the_batch_are_refused(eng, pairs):
    from corrosion_amd import updates as U
    f = U.MatchFilters(eng, updates=["t4"])
    arr, imp, _p, _ = layout([[("t4", k, "a", 1, 1) for k in range(4)]])
    call = Raw(eng, f, arr, imp, np.array(pairs, np.uint64))
    for which in (0, 1):
        assert call(which) == -1 and b"ranges" in call.L.lib().corro_last_error()
        assert call.untouched() and call.o.ncand == 0


def test_pass_1_with_another_ncand_is_refused(eng):
    from corrosion_amd import updates as U
    f = U.MatchFilters(eng, updates=["t4"])
    arr, imp, pairs, _ = layout([[("t4", k, "a", 1, 1) for k in range(4)]])
    for wrong in (3, 5, 0):
        call = Raw(eng, f, arr, imp, pairs)
        call.o.ncand = wrong
        assert call(1) == -1 and b"ncand" in call.L.lib().corro_last_error()
        assert call.untouched() and call.o.ncand == wrong
    call = Raw(eng, f, arr, imp, pairs)
    assert call(0) == 0 and call.o.ncand == 4
    assert call(1) == 0 and not call.untouched()


def test_nslots_that_is_not_the_schemas_is_refused(eng):
    from corrosion_amd import updates as U
    f = U.MatchFilters(eng, updates=["t4"])
    arr, imp, pairs, _ = layout([[("t4", 1, "a", 1, 1)]])
    call = Raw(eng, f, arr, imp, pairs)
    call.r.nslots = f.nslots - 1
    assert call(0) == -1 and b"nslots" in call.L.lib().corro_last_error() and call.untouched()


@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
def test_zero_counts(eng, device):
    """n = 0, ncs = 0 and nclasses = 0, each alone: no candidate and a closed class_off."""
    one = [[("t4", 1, "a", 1, 1)]]
    res, _ = check(eng, [[], []], updates=["t4"], device=device)                     # n = 0
    assert res["ncand"] == 0 and host(res["class_off"], np.uint64).tolist() == [0, 0]
    res, _ = check(eng, [("gap", one[0])], updates=["t4"], device=device)            # ncs = 0
    assert res["ncand"] == 0 and host(res["class_off"], np.uint64).tolist() == [0, 0]
    res, _ = check(eng, one, device=device)                                          # nclasses = 0
    assert res["ncand"] == 0 and host(res["class_off"], np.uint64).tolist() == [0]


def random_case(seed):
    rng = np.random.default_rng(seed)
    ncs = int(rng.integers(1, 41))
    total = int(rng.integers(1, 2001))
    cuts = np.sort(rng.integers(0, total + 1, ncs - 1)).tolist()
    sizes = np.diff([0] + cuts + [total]).tolist()
    pks = rng.integers(0, 1 << 63, 50).tolist()
    case = []
    for size in sizes:
        cs = []
        for _ in range(size):
            t = TABLES[int(rng.integers(0, 3))]
            cid = S if rng.random() < 0.15 else SCHEMA[t][int(rng.integers(0, len(SCHEMA[t])))]
            cs.append((t, pks[int(rng.integers(0, 50))], cid, int(rng.integers(1, 7)), int(rng.random() < 0.5)))
        case.append(cs)
        if rng.random() < 0.1:
            case.append(("gap", [("t4", pks[0], "a", 1, 1)]))
    subs, updates = [], []
    for _ in range(int(rng.integers(1, 71))):
        if rng.random() < 0.2:
            updates.append(TABLES[int(rng.integers(0, 3))])
            continue
        sub = {}
        for t in rng.permutation(3)[:int(rng.integers(1, 4))]:
            cols = SCHEMA[TABLES[t]]
            sub[TABLES[t]] = [c for c in cols if rng.random() < 0.4]
        subs.append(sub)
    return case, subs, updates


@pytest.mark.parametrize("seed", range(20))
def test_random(eng, seed):
    case, subs, updates = random_case(seed)
    check(eng, case, subs=subs, updates=updates)


def test_host_and_device_memory_give_the_same_arrays(eng):
    case, subs, updates = random_case(101)
    a, _ = check(eng, case, subs=subs, updates=updates, device=True)
    b, _ = check(eng, case, subs=subs, updates=updates, device=False)
    for k in ("class_off", "cand_change", "cand_cs", "cand_table", "cand_pk", "cand_cl"):
        assert host(a[k], b[k].dtype).tolist() == b[k].tolist(), k


# ---- chained behind the merge ------------------------------------------------------------------------------

WIRE_SCHEMA = {"users": ["name", "age"], "posts": ["title", "likes"]}
ACT = [bytes([k + 1] * 16) for k in range(3)]


def test_process_frames_then_match_changes():
    """Frames holding a re-sent version (every flag 0), an Empty and a losing change (the last one), matched on the device
    behind Agent.process_frames; the model runs over Processed.impactful of a twin fed the same ChangeV1s
    through the host path."""
    import corrosion_amd as ca
    from corrosion_amd import updates as U, wire
    from corrosion_amd.agent import Change, ChangeV1, Empty, Full

    def full(actor, v, changes, ts=1):
        for k, c in enumerate(changes):
            c.seq = k
        return ChangeV1(actor, Full(v, changes, (0, len(changes) - 1), len(changes) - 1, ts=ts))
    a, b, c = ACT
    first = full(a, 1, [Change("users", 1, "name", "ann", 1, 1, 0, a, 1), Change("users", 1, "age", 30, 1, 1, 0, a, 1),
                        Change("users", 2, "age", 5, 3, 1, 0, a, 1), Change("posts", 1, "title", "x", 1, 1, 0, a, 1)])
    msgs = [first,
            ChangeV1(b, Empty((1, 2))),
            full(b, 3, [Change("users", 2, "age", 4, 1, 3, 0, b, 1),              # an older col_version
                        Change("users", 2, "name", "bob", 1, 3, 0, b, 1),
                        Change("posts", 1, "-1", None, 2, 3, 0, b, 2),               # deletes the post
                        Change("users", 3, "-1", None, 1, 3, 0, b, 1)]),
            first,                                                                    # re-sent: skipped
            full(c, 1, [Change("posts", 2, "likes", 7, 2, 1, 0, c, 1), Change("posts", 2, "title", "y", 1, 1, 0, c, 1),
                        Change("posts", 2, "likes", 6, 1, 1, 0, c, 1)])]                   # loses to col_version 2
    x = ca.agent.Agent(WIRE_SCHEMA, capacity_hint=1 << 12)
    y = ca.agent.Agent(WIRE_SCHEMA, capacity_hint=1 << 12)
    for act in ACT:
        x.site(act)
        y.site(act)
    rx = x.process_multiple_changes(msgs)
    assert rx.known[0] == "current" and rx.known[2:] == ["current", "skipped", "current"]
    assert [ch.val for ch in rx.impactful[4]] == [7, "y"]                             # without the losing change
    ry, st = y.process_frames(wire.frames(msgs))
    assert (st == 0).all() and ry.known == rx.known
    filters = U.MatchFilters(y.engine, subs=[{"users": ["age"]}, {"posts": ["title"], "users": ["name"]}, {"users": ["age"]}],
                             updates=["posts", "users"])
    res = y.match_changes(ry, ry.dec, filters)
    want = M.by_handle(filters.handles, [[(ch.table, ch.pk, ch.cid, ch.cl) for ch in imp] for imp in rx.impactful])
    assert ordered(U.candidates_by_handle(res, filters)) == ordered(want)
    assert any(per for per in want) and all(s in (0, 2, 4) for per in want for s, _ in per)
    assert U.notify_events(res, filters)[3] == [(s, M.handle_candidates(cands)) for s, cands in want[3]]
    x.engine.close()
    y.engine.close()


def test_match_extracted_after_process_fully_buffered_changes():
    """A version that arrives in two halves, is buffered, then applied: match_extracted over its extracted
    rows against the model over the same rows in seq order."""
    import corrosion_amd as ca
    import torch
    from corrosion_amd import updates as U
    from corrosion_amd.agent import Change, ChangeV1, Full
    a = ACT[0]
    changes = [Change("users", 1, "name", "ann", 1, 1, 0, a, 1), Change("users", 1, "age", 3, 1, 1, 1, a, 1),
               Change("posts", 1, "likes", 2, 1, 1, 2, a, 1), Change("users", 2, "-1", None, 1, 1, 3, a, 1),
               Change("users", 2, "age", 9, 1, 1, 4, a, 1), Change("posts", 1, "title", "t", 1, 1, 5, a, 1)]
    ag = ca.agent.Agent(WIRE_SCHEMA, capacity_hint=1 << 12)
    r = ag.process_multiple_changes([ChangeV1(a, Full(1, changes[:3], (0, 2), 5, ts=1))])
    assert r.known == ["partial"]
    r = ag.process_multiple_changes([ChangeV1(a, Full(1, changes[3:], (3, 5), 5, ts=1))])
    assert r.ready == [(a, 1)] and ag.process_fully_buffered_changes(a, 1)
    dev = lambda v, dt: torch.tensor(v, dtype=dt, device="cuda")     # noqa: E731
    ext = ag.engine.extract_changes({"site": dev([ag.site(a)], torch.int32), "start": dev([1], torch.int64),
                                     "end": dev([1], torch.int64)})
    rows = ext["rows"]
    seq = rows["seq"].cpu().tolist()
    assert len(seq) > 0 and seq == sorted(seq)
    filters = U.MatchFilters(ag.engine, subs=[{"users": ["age"]}, {"posts": ["title"]}], updates=["users", "posts"])
    res = U.match_extracted(ag.engine, rows, filters)
    names = {(t << 16) | k: (tn, "-1" if k == 0 else cols[k - 1]) for t, (tn, cols) in enumerate(WIRE_SCHEMA.items())
             for k in range(len(cols) + 1)}
    model_rows = [names[tc] + (pk, cl) for tc, pk, cl in zip(rows["table_cid"].cpu().tolist(), rows["pk"].cpu().tolist(),
                                                             rows["cl"].cpu().tolist())]
    want = M.by_handle(filters.handles, [[(t, pk, cid, cl) for t, cid, pk, cl in model_rows]])
    assert ordered(U.candidates_by_handle(res, filters)) == ordered(want)
    assert [len(per) for per in want] == [1, 1, 1, 1]
    ag.engine.close()
