"""Compaction of the long-value arena (corro_values_compact / MergeEngine.compact_values, and the
auto-compaction policy): the arena shrinks to the union of the live byte spans, every row keeps its
bytes, the merge reads the moved bytes, and every consumer of handles (export, touched export,
extraction) sees the rewritten ones."""
import numpy as np
import pytest

import synth
from oracle import oracle as O
from tests._util import rows_to_tuples

pytestmark = pytest.mark.gpu

SCHEMA = {"t": ["a", "b", "c", "d"]}


def _engine(schema, sites, cap=1 << 16):
    import corrosion_amd as ca
    e = ca.MergeEngine(schema, capacity_hint=cap)
    e.register_sites(sites)
    return e


def _r8(x):
    return (int(x) + 7) & ~7


def _compare(e, f, with_ts=False):
    got, exp = e.export(), f.export()
    assert rows_to_tuples(got, with_ts) == rows_to_tuples(exp, with_ts)
    assert O.rows_digest(got) == O.rows_digest(exp)
    return got


def _batch(changes, data):
    """changes: (pk, cid, col_version, value) with value an int or an (offset, size) span of `data`
    (a long BLOB); table 0, site 0, cl 1, db_version 1, seq = index."""
    n = len(changes)
    b = {"pk": np.zeros(n, np.uint64), "table_cid": np.zeros(n, np.uint32), "col_version": np.zeros(n, np.int64),
         "db_version": np.ones(n, np.int64), "cl": np.ones(n, np.uint32), "seq": np.arange(n, dtype=np.uint32),
         "site": np.zeros(n, np.uint32), "val0": np.zeros(n, np.uint64), "val1": np.zeros(n, np.uint64),
         "val_type": np.ones(n, np.uint8), "val_len": np.zeros(n, np.uint8), "ts": np.full(n, 5, np.uint64),
         "val_off": np.zeros(n, np.uint64), "val_size": np.zeros(n, np.uint32),
         "val_data": np.frombuffer(bytes(data), np.uint8)}
    for i, (pk, cid, cv, v) in enumerate(changes):
        b["pk"][i], b["table_cid"][i], b["col_version"][i] = pk, cid, cv
        if isinstance(v, tuple):
            off, size = v
            b["val_type"][i], b["val_len"][i] = 4, 255
            b["val0"][i] = int.from_bytes(bytes(data[off:off + 8]), "big")
            b["val_off"][i], b["val_size"][i] = off, size
        else:
            b["val0"][i] = v
    return b


def _cells(rows):
    """{(pk, cid): long value bytes} of an export"""
    return {(int(rows["pk"][i]), int(rows["table_cid"][i]) & 0xFFFF): v for i, v in rows["long_values"].items()}


def _union_size(spans):
    """bytes covered by the union of (offset, size) spans"""
    iv = np.array(sorted((o, o + s) for o, s in spans), np.int64)
    prev_end = np.concatenate(([0], np.maximum.accumulate(iv[:, 1])[:-1]))
    return int(np.maximum(iv[:, 1] - np.maximum(iv[:, 0], prev_end), 0).sum())


def test_compaction_shrinks_and_keeps_the_state():
    sites = synth.site_ids(8, 5)
    e, f = _engine(SCHEMA, sites), O.Fold(sites)
    for k in range(4):
        b = synth.with_long_values(synth.uniform_batch(20000, 8, 3000, 4, 60 + k, cv_max=2, tie_frac=0.5), 70 + k, frac=0.3)
        e.apply(b)
        f.apply(b)
    rows = e.export()
    before = rows_to_tuples(rows)
    live = sum(len(v) for v in rows["long_values"].values())
    assert live > 0
    r = e.compact_values()
    assert r["arena_after"] < r["arena_before"]
    assert r["live_bytes"] == live and r["arena_after"] == _r8(live)
    assert e.metrics()["arena_bytes"] == r["arena_after"]
    assert rows_to_tuples(e.export()) == before
    _compare(e, f)
    # a fifth batch whose long values tie against the stored (moved) ones
    b = synth.with_long_values(synth.uniform_batch(20000, 8, 3000, 4, 64, cv_max=2, tie_frac=0.5), 74, frac=0.3)
    assert np.array_equal(e.apply(b, impact=True), f.apply(b))
    _compare(e, f)


def test_aliased_and_overlapping_spans_are_kept_once():
    rng = np.random.default_rng(11)
    data = rng.integers(0, 256, 1000, dtype=np.uint8)
    live = {1: (10, 40), 2: (10, 40), 3: (10, 40),   # one span named three times
            4: (100, 200), 5: (150, 30),            # a strict sub-span
            6: (400, 100), 7: (450, 100),           # a partial overlap
            8: (800, 33)}
    changes = [(pk, 1, 2, span) for pk, span in live.items()]
    changes.insert(3, (8, 1, 1, (700, 77)))         # dead: beaten in this batch by the higher col_version
    e = _engine(SCHEMA, synth.site_ids(2, 3))
    e.apply(_batch(changes, data))
    want = {(pk, 1): data[o:o + s].tobytes() for pk, (o, s) in live.items()}
    assert _cells(e.export()) == want
    union = _union_size(live.values())
    assert union == 40 + 200 + 150 + 33
    r = e.compact_values()
    assert r["arena_before"] == 1000 and r["live_bytes"] == union and r["arena_after"] == _r8(union)
    assert _cells(e.export()) == want
    r = e.compact_values()                          # already compact: nothing moves
    assert r["arena_before"] == r["arena_after"] == _r8(union)
    assert _cells(e.export()) == want


def test_sizes_and_alignments():
    """Every copy path: head / 16-byte body / tail, sources and destinations of different
    misalignments, pieces of one and of many chunks."""
    rng = np.random.default_rng(12)
    sizes = [17, 18, 31, 33, 4095, 4097, 100003]
    dead_sizes = [19, 21, 25, 37, 45, 43, 47]
    data, changes, spans, shifts = bytearray(), [], {}, []
    for i, (s, d) in enumerate(zip(sizes, dead_sizes)):
        if (len(data) + d) % 2 == 0:
            data += b"\xEE"                          # (a byte no change names: the value starts at an odd offset)
        changes.append((i + 1, 1, 1, (len(data), d)))
        data += rng.integers(0, 256, d, dtype=np.uint8).tobytes()
        changes.append((i + 1, 1, 2, (len(data), s)))
        spans[i + 1] = (len(data), s)
        shifts.append(len(data) - sum(sizes[:i]))
        data += rng.integers(0, 256, s, dtype=np.uint8).tobytes()
    assert all(o % 2 == 1 for o, _ in spans.values())
    assert all(x % 16 for x in shifts) and len({x % 16 for x in shifts}) == len(shifts)
    e = _engine(SCHEMA, synth.site_ids(2, 3))
    e.apply(_batch(changes, data))
    want = {(pk, 1): bytes(data[o:o + s]) for pk, (o, s) in spans.items()}
    assert _cells(e.export()) == want
    r = e.compact_values()
    assert r["live_bytes"] == sum(sizes) and r["arena_after"] == _r8(sum(sizes))
    assert _cells(e.export()) == want


def test_nothing_live_and_empty_engine():
    sites = synth.site_ids(2, 3)
    e, f = _engine(SCHEMA, sites), O.Fold(sites)
    assert e.compact_values() == {"live_bytes": 0, "arena_before": 0, "arena_after": 0}
    assert e.compact_values(dry_run=True) == {"live_bytes": 0, "arena_before": 0, "arena_after": 0}
    data = np.random.default_rng(13).integers(0, 256, 50 * 40, dtype=np.uint8)
    b1 = _batch([(pk, 1 + pk % 4, 1, (40 * (pk - 1), 40)) for pk in range(1, 51)], data)
    b2 = _batch([(pk, 1 + pk % 4, 2, pk) for pk in range(1, 51)], b"\0")
    for b in (b1, b2):
        e.apply(b)
        f.apply(b)
    assert e.metrics()["arena_bytes"] >= 2000
    r = e.compact_values()
    assert r["live_bytes"] == 0 and r["arena_after"] == 0 and e.metrics()["arena_bytes"] == 0
    _compare(e, f)
    b3 = _batch([(pk, 1 + pk % 4, 3, (40 * (pk - 1), 40)) for pk in range(1, 51)], data)  # the arena starts over
    e.apply(b3)
    f.apply(b3)
    assert len(_compare(e, f)["long_values"]) == 50


def test_dry_run_measures_and_moves_nothing():
    sites = synth.site_ids(8, 5)
    e = _engine(SCHEMA, sites)
    for k in range(2):
        e.apply(synth.with_long_values(synth.uniform_batch(5000, 8, 500, 4, 20 + k, cv_max=2), 30 + k, frac=0.3))
    rows = e.export()
    idx = sorted(rows["long_values"])
    handles = np.asarray(rows["val1"])[idx]
    arena = e.metrics()["arena_bytes"]
    d = e.compact_values(dry_run=True)
    assert d["arena_before"] == d["arena_after"] == arena == e.metrics()["arena_bytes"]
    assert e.value_bytes(handles) == [rows["long_values"][i] for i in idx]
    r = e.compact_values()
    assert 0 < d["live_bytes"] < arena
    assert d["live_bytes"] == r["live_bytes"] and r["arena_after"] == _r8(d["live_bytes"])


def test_general_and_overflow_bodies_read_the_moved_bytes():
    seed = 91
    sites = synth.site_ids(8, seed)
    b = synth.with_long_values(synth.adversarial_batch(60000, 8, 1, 60, seed, zipf=1.1), seed, frac=0.4)
    e, f = _engine(synth.adversarial_schema(1), sites, cap=64), O.Fold(sites)
    assert np.array_equal(e.apply(b, impact=True), f.apply(b))
    r = e.compact_values()
    assert r["arena_after"] < r["arena_before"]
    b2 = synth.with_long_values(synth.adversarial_batch(60000, 8, 1, 60, seed + 1, zipf=1.1), seed + 1, frac=0.4)
    assert np.array_equal(e.apply(b2, impact=True), f.apply(b2))
    _compare(e, f, with_ts=True)


def test_touched_export_and_extraction_see_the_rewritten_handles():
    sites = synth.site_ids(8, 5)
    e, f = _engine(SCHEMA, sites), O.Fold(sites)
    e.track_touched()
    b = synth.with_long_values(synth.uniform_batch(8000, 8, 800, 4, 40, cv_max=2, tie_frac=0.5), 41, frac=0.3)
    e.apply(b)
    f.apply(b)
    nd = {"site": np.arange(8, dtype=np.uint32), "start": np.ones(8, np.uint64),
          "end": np.full(8, int(b["db_version"].max()), np.uint64)}

    def extracted():
        res = e.extract_changes(nd)
        rows = dict(res["rows"])
        rows["long_values"] = e.long_values(rows)
        return [int(x) for x in res["row_off"]], rows_to_tuples(rows), np.asarray(rows["val1"]).copy()
    off0, rows0, h0 = extracted()                    # (builds the extraction index)
    assert any(isinstance(t[5], bytes) for t in rows0)
    r = e.compact_values()
    assert r["arena_after"] < r["arena_before"]
    off1, rows1, h1 = extracted()
    assert off1 == off0 and rows1 == rows0
    assert not np.array_equal(h0, h1)                # the index was rebuilt from the rewritten handles
    delta = e.export_touched()                       # every row of the state: all were addressed
    assert rows_to_tuples(delta) == rows_to_tuples(f.export())


def test_stale_handle_is_refused():
    import corrosion_amd as ca
    e = _engine(SCHEMA, synth.site_ids(8, 5))
    for k in range(3):
        e.apply(synth.with_long_values(synth.uniform_batch(5000, 8, 300, 4, 50 + k, cv_max=2), 55 + k, frac=0.4))
    rows = e.export()
    h = np.asarray(rows["val1"])[sorted(rows["long_values"])]
    last = int(h[np.argmax((h >> np.uint64(24)) + (h & np.uint64(0xFFFFFF)))])
    assert len(e.value_bytes([last])[0]) == last & 0xFFFFFF
    r = e.compact_values()
    assert (last >> 24) + (last & 0xFFFFFF) > r["arena_after"]
    with pytest.raises(ca.CorroError) as err:
        e.value_bytes([last])
    assert err.value.code == -1                      # CORRO_E_INVALID


def test_autocompaction_bounds_the_arena():
    sites = synth.site_ids(2, 3)
    floor, ncell = 1 << 16, 2000
    auto, plain, f = _engine(SCHEMA, sites), _engine(SCHEMA, sites), O.Fold(sites)
    auto.set_values_autocompact(floor)
    rng = np.random.default_rng(14)
    over = False
    for k in range(12):
        sizes = rng.integers(180, 221, ncell)
        offs = np.concatenate(([0], np.cumsum(sizes)[:-1]))
        data = rng.integers(0, 256, int(sizes.sum()), dtype=np.uint8)
        b = _batch([(pk + 1, 1, k + 1, (int(offs[pk]), int(sizes[pk]))) for pk in range(ncell)], data)
        for x in (auto, plain, f):
            x.apply(b)
        live = int(sizes.sum())                      # every cell now holds this batch's value
        bound = 2 * live + len(data) + floor
        assert auto.metrics()["arena_bytes"] <= bound, k
        over = plain.metrics()["arena_bytes"] > bound
    assert over                                      # (without the policy the same loop ends above the bound)
    _compare(auto, f)
    _compare(plain, f)


def test_poisoned_context_refuses_compaction(monkeypatch):
    import corrosion_amd as ca
    from tests.test_gpu_agent_atomicity import _pieces, _run, _side
    ids = synth.site_ids(3, 23)
    eng, bk, ords = _side(ids)
    first, _second, full = _pieces(ids, ords, 3, 5)
    monkeypatch.setenv("CORRO_FAULT", "bufpool_reserve")
    with pytest.raises(ca.CorroError, match="poisoned"):
        _run(eng, bk, ords, full + first, "headers")  # complete versions merge, then the commit fails
    monkeypatch.delenv("CORRO_FAULT")
    for dry in (False, True):
        with pytest.raises(ca.CorroError, match="poisoned") as err:
            eng.compact_values(dry_run=dry)
        assert err.value.code == -3                  # CORRO_E_DEVICE
