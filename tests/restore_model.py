"""Host model of the restart path (TEST INFRASTRUCTURE): BookedVersions::from_conn
(corro-types/src/agent.rs:1282-1351) per actor and the startup loop that calls it
(corro-agent/src/agent/run_root.rs:139-201), plus helpers that build a corro_bookie_image by hand and
read a bookie back for comparison. The product path is corro_bookie_load (csrc/agent.cpp +
bookie_image.hip)."""
import numpy as np

from oracle.agent import Partial, _rs_gaps, _rs_insert


class LoadedActor:
    """What from_conn returns: max (None or int), needed gaps, partials by version."""

    def __init__(self, mx):
        self.max, self.needed, self.partials = mx, [], {}


def from_conn(mx, seq_rows, gaps):
    """mx: the crsql_db_versions value or None; seq_rows: (version, start_seq, end_seq, last_seq, ts) in
    table order; gaps: (start, end) in table order."""
    bv = LoadedActor(mx)
    for version, s, e, last_seq, ts in seq_rows:               # insert_partial (agent.rs:1414-1432)
        cur = bv.partials.get(version)
        if cur is None:
            bv.max = version if bv.max is None else max(bv.max, version)
            bv.partials[version] = Partial([(s, e)], last_seq, ts)
        else:
            cur.seqs = _rs_insert(cur.seqs, s, e)
    for s, e in gaps:                                           # max does not come from gaps (:1338-1342)
        bv.needed = _rs_insert(bv.needed, s, e)
    return bv


def startup(actors):
    """actors: [(actor_id, max, seq_rows, gaps)] in the order loaded. Returns ({actor: LoadedActor},
    ready = [(actor, version)] of the partials with no gap over 0 ..= last_seq, run_root.rs:181-193)."""
    books, ready = {}, []
    for actor, mx, seq_rows, gaps in actors:
        bv = from_conn(mx, seq_rows, gaps)
        for version in sorted(bv.partials):
            p = bv.partials[version]
            if not _rs_gaps(p.seqs, 0, p.last_seq):
                ready.append((bytes(actor), version))
        books[bytes(actor)] = bv
    return books, ready


ROW_FIELDS = (("pk", np.uint64), ("table_cid", np.uint32), ("col_version", np.int64), ("db_version", np.int64),
              ("cl", np.uint32), ("seq", np.uint32), ("site", np.uint32), ("val0", np.uint64), ("val1", np.uint64),
              ("val_type", np.uint8), ("val_len", np.uint8), ("ts", np.uint64))


def make_image(actors, site_ids=(), rows=None):
    """A corro_bookie_image as the Python mirror takes it. actors: [(actor_id, max or None, seq_rows,
    gaps)]; site_ids: 16-byte ids by ordinal; rows: dict of row arrays (or None)."""
    gap_off, seq_off, gaps, seqs = [0], [0], [], []
    for _a, _m, sr, g in actors:
        seqs += list(sr)
        gaps += list(g)
        seq_off.append(len(seqs))
        gap_off.append(len(gaps))
    u64 = lambda x: np.array(x, np.uint64).reshape(-1)
    ids = lambda x: np.frombuffer(b"".join(bytes(i) for i in x), np.uint8).reshape(-1, 16).copy()
    return {
        "actor_ids": ids([a for a, *_ in actors]), "max": np.array([-1 if m is None else m for _a, m, *_ in actors], np.int64),
        "gap_off": u64(gap_off), "gap_start": u64([g[0] for g in gaps]), "gap_end": u64([g[1] for g in gaps]),
        "seq_off": u64(seq_off), "seq_version": u64([s[0] for s in seqs]), "seq_start": u64([s[1] for s in seqs]),
        "seq_end": u64([s[2] for s in seqs]), "seq_last": u64([s[3] for s in seqs]), "seq_ts": u64([s[4] for s in seqs]),
        "site_ids": ids(site_ids), "rows": rows or {},
    }


def make_rows(keys, ts=7):
    """Canonical INTEGER rows for (site, db_version, seq) keys, in the order given: every other field is
    a function of the key, so a row can be recognised wherever it ends up."""
    n = len(keys)
    site = np.array([k[0] for k in keys], np.uint32)
    dbv = np.array([k[1] for k in keys], np.int64)
    seq = np.array([k[2] for k in keys], np.uint32)
    mix = (site.astype(np.uint64) * np.uint64(1000003)) ^ (dbv.astype(np.uint64) * np.uint64(7919)) ^ seq.astype(np.uint64)
    return {"pk": mix + np.uint64(1), "table_cid": np.full(n, (0 << 16) | 1, np.uint32), "col_version": (seq % 5 + 1).astype(np.int64),
            "db_version": dbv, "cl": np.ones(n, np.uint32), "seq": seq, "site": site, "val0": mix * np.uint64(3),
            "val1": np.zeros(n, np.uint64), "val_type": np.ones(n, np.uint8), "val_len": np.zeros(n, np.uint8),
            "ts": np.full(n, ts, np.uint64)}


def image_equal(a, b):
    """Two images array by array (rows included; CUDA tensors are brought to the host)."""
    def host(x):
        return x.cpu().numpy() if type(x).__module__.startswith("torch") else np.asarray(x)
    keys = [k for k in a if k not in ("rows", "stamp")]        # (the stamp covers where the rows lie, too)
    assert sorted(keys) == sorted(k for k in b if k not in ("rows", "stamp"))
    for k in keys:
        x, y = host(a[k]), host(b[k])
        assert x.shape == y.shape and np.array_equal(x, y), k
    assert sorted(a["rows"]) == sorted(b["rows"])
    for k in a["rows"]:
        x, y = host(a["rows"][k]), host(b["rows"][k])
        assert x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8)), "rows." + k
    return True


def check_bookie(bookie, books):
    """A loaded bookie against startup()'s books: last, needed and every partial, per actor."""
    for actor, bv in books.items():
        assert bookie.last(actor) == bv.max, actor
        assert bookie.needed(actor) == bv.needed, actor
        for version, p in bv.partials.items():
            assert bookie.partial(actor, version) == (p.seqs, p.last_seq), (actor, version)
