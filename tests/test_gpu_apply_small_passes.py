"""The small passes around an apply: the bucket-offset scan inside k_colscan (a ticket and a look-back
across its workgroups), the one-kernel tail (db_version fold, region fill sum, the host's copy of the
counters), the launch of the mixed-type body only when it can have work, and the one-kernel reset.
Every case is compared with the oracle fold row for row, and in its crsql_db_versions."""
import math

import numpy as np
import pytest

import synth
from oracle import oracle as O
from tests._util import rows_to_tuples

pytestmark = pytest.mark.gpu

SCHEMA = {"t": ["a", "b", "c", "d"]}
NSITES = 8
SITES = synth.site_ids(NSITES, 5)
# The engine takes 2^ceil(log2(hint / 1280)) buckets, at most 2^15: one bucket (k_colscan's scan
# with a single workgroup and nothing to look back at), and 2^15 (128 workgroups of 256 buckets).
CAP_B1 = 1
CAP_B32K = 1280 * ((1 << 14) + 1)
SIZES = (1, 2, 511, 512, 513, 4097)   # one tile; around a 512-change tile boundary; an odd tile tail

_engines = {}
_dbv_kept = {}   # per shared engine: the db_versions its applies have left (a reset keeps them)
_refs = {}


def _engine(cap):
    import corrosion_amd as ca
    if cap not in _engines:
        e = ca.MergeEngine(SCHEMA, capacity_hint=cap)
        e.register_sites(SITES)
        _engines[cap] = e
    return _engines[cap]


def _batch(n, seed=3):
    return synth.uniform_batch(n, NSITES, max(1, n // 3), 4, seed)


def _ref(n):
    """The oracle's rows and db_versions for _batch(n) into an empty state (computed once)."""
    if n not in _refs:
        f = O.Fold(SITES)
        f.apply(_batch(n))
        _refs[n] = (rows_to_tuples(f.export()), list(f.db_versions()))
    return _refs[n]


def _check(eng, rows, dbv):
    got = rows_to_tuples(eng.export())
    assert len(got) == len(rows)
    assert got == rows
    assert eng.count() == len(rows)
    assert list(eng.db_versions()[:len(dbv)]) == list(dbv)


def _check_shared(cap, n):
    """_check for a shared engine: crsql_db_versions are a running maximum that a reset leaves alone,
    so the expected ones are the maximum over the batches the engine has taken."""
    rows, dbv = _ref(n)
    kept = _dbv_kept[cap] = np.maximum(_dbv_kept.get(cap, np.full(len(dbv), -1, np.int64)), np.array(dbv, np.int64))
    _check(_engines[cap], rows, kept.tolist())


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for e in _engines.values():
        e.close()
    _engines.clear()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("cap", [CAP_B1, CAP_B32K], ids=["B1", "B32768"])
def test_sizes_and_bucket_counts(cap, n):
    eng = _engine(cap)
    eng.reset()
    eng.apply(_batch(n))
    _check_shared(cap, n)


def test_two_applies_reset_first_again():
    """Everything the reset clears, and k_colscan's ticket and status words being reusable: after two
    applies and a reset, the first apply gives what it gives a fresh engine. crsql_db_versions are a
    running maximum that a reset leaves alone; the second batch carries the same (site, db_version)
    pairs as the first, so they equal a fresh engine's too."""
    import corrosion_amd as ca
    n = 4097
    a, b = _batch(n), _batch(n, seed=4)
    assert np.array_equal(a["site"], b["site"]) and np.array_equal(a["db_version"], b["db_version"])
    f = O.Fold(SITES)
    f.apply(a)
    f.apply(b)
    eng = ca.MergeEngine(SCHEMA, capacity_hint=n)
    eng.register_sites(SITES)
    eng.track_touched(True)        # (the reset also clears the touched-row count)
    eng.apply(a)
    eng.apply(b)
    _check(eng, rows_to_tuples(f.export()), list(f.db_versions()))
    eng.reset()
    assert eng.count() == 0
    assert len(eng.export()["pk"]) == 0
    eng.apply(a)
    fresh = ca.MergeEngine(SCHEMA, capacity_hint=n)
    fresh.register_sites(SITES)
    fresh.apply(a)
    rows, dbv = _ref(n)
    _check(fresh, rows, dbv)
    _check(eng, rows, dbv)
    assert list(eng.db_versions()) == list(fresh.db_versions())
    eng.close()
    fresh.close()


def test_failed_validation_then_good_apply():
    """The tail kernel's error gate: a batch with an unknown column id is refused as before, folds
    nothing into the db_versions and leaves the state as it was; a good apply afterwards merges."""
    import corrosion_amd as ca
    n = 2000
    a, b = _batch(n), _batch(n, seed=9)
    b["db_version"] = b["db_version"] + 1000      # (would raise every site's db_version)
    f = O.Fold(SITES)
    f.apply(a)
    eng = ca.MergeEngine(SCHEMA, capacity_hint=n)
    eng.register_sites(SITES)
    eng.apply(a)
    before, dbv = rows_to_tuples(eng.export()), list(eng.db_versions())
    bad = {k: v.copy() for k, v in b.items()}
    bad["table_cid"][-1] = 7                      # cid 7 of table 0 does not exist
    with pytest.raises(ca.CorroError) as ex:
        eng.apply(bad)
    assert ex.value.code == -5
    assert rows_to_tuples(eng.export()) == before
    assert list(eng.db_versions()) == dbv
    assert eng.count() == len(before)
    eng.apply(b)
    f.apply(b)
    _check(eng, rows_to_tuples(f.export()), list(f.db_versions()))
    eng.close()


@pytest.mark.parametrize("impact", [False, True])
def test_mixed_batch_through_the_queued_bodies(impact):
    """Sentinels, cl != 1 and non-INTEGER values: the general and mixed-type bodies work through the
    queues k_triage fills; a second batch meets a state that already holds non-INTEGER values."""
    import corrosion_amd as ca
    seed = 41
    sites = synth.site_ids(8, seed)
    eng = ca.MergeEngine(synth.adversarial_schema(2), capacity_hint=4000)
    eng.register_sites(sites)
    f = O.Fold(sites)
    for k in range(2):
        b = synth.adversarial_batch(4000, 8, 2, 300, seed + k)
        imp = eng.apply(b, impact=impact)
        ref = f.apply(b)
        if impact:
            assert np.array_equal(imp, ref)
        got, exp = rows_to_tuples(eng.export(), with_ts=True), rows_to_tuples(f.export(), with_ts=True)
        assert got == exp
        assert list(eng.db_versions()[:f.nsites]) == list(f.db_versions())
    # an INTEGER-only batch into the state that holds wide values (the mixed-type body must still launch)
    u = synth.uniform_batch(3000, 8, 300, 2, seed)
    eng.apply(u, impact=impact)
    f.apply(u)
    assert rows_to_tuples(eng.export()) == rows_to_tuples(f.export())
    assert list(eng.db_versions()[:f.nsites]) == list(f.db_versions())
    eng.close()


def test_stage_timings_keep_their_six_slots():
    eng = _engine(CAP_B32K)
    eng.reset()
    eng.set_profiling(True)
    eng.apply(_batch(4097))
    t = eng.last_timings()
    eng.set_profiling(False)
    assert list(t) == ["k_hist", "k_colscan", "k_plan", "k_scatter", "k_merge", "k_merge_ovf"]
    assert all(math.isfinite(v) and v >= 0 for v in t.values())
    assert t["k_hist"] > 0 and t["k_scatter"] > 0 and t["k_merge"] > 0
    _check_shared(CAP_B32K, 4097)
