"""A brute-force host model of handle_need's two queries (corro-agent/src/api/peer/mod.rs:385-394 and
:423-431 / :603-611) over exported crsql_changes rows (engine.export() form), independent of the
kernel (which binary-searches packed 64-bit keys) and of oracle.extract_changes (which sorts and
searches numpy arrays).

Every need builds a mask over ALL rows by comparing site, db_version and seq as Python ints: no
sorted search, no packed key, no numpy comparison, so a bound of 2^64 - 1 is like any other.

    SELECT db_version, MAX(seq), MAX(ts) ... WHERE site_id = :actor AND db_version BETWEEN :start
      AND :end GROUP BY db_version ORDER BY db_version DESC
    SELECT ... WHERE site_id = :actor AND db_version = :version [AND seq BETWEEN :s AND :e]
      ORDER BY seq ASC

The result has the shape of oracle.extract_changes: per need a list of (version, last_seq, ts, rows),
versions DESCENDING, MAX(seq) / MAX(ts) over all rows of the version (not the seq-filtered ones; a
version whose rows the filter all misses still appears, with no rows), rows as tuples of the twelve
row fields (ROWF order). The order contract is stated by seq_classes(): the rows of a group fall
into classes of equal seq, the classes ascend, and inside a class the rows are a multiset (the SQL
leaves the order of ties open).

Empty results: a site ordinal nobody registered (>= nsites) and start > end match no version, so
the need has no groups. seq_start > seq_end matches no row: like any filter that misses, it leaves
the first query's versions in place, each with no rows.
"""
ROWF = ("pk", "table_cid", "col_version", "db_version", "cl", "seq", "site", "ts", "val0", "val1", "val_type",
        "val_len")
I_DBV, I_SEQ, I_SITE, I_TS = ROWF.index("db_version"), ROWF.index("seq"), ROWF.index("site"), ROWF.index("ts")


def row_tuples(rows, idx=None):
    """Rows (a dict of arrays) as tuples of Python ints in ROWF order, all of them or those at idx."""
    cols = [rows[k].tolist() if hasattr(rows[k], "tolist") else list(rows[k]) for k in ROWF]
    n = len(cols[0])
    return [tuple(int(c[i]) for c in cols) for i in (range(n) if idx is None else idx)]


def seq_classes(group_rows):
    """[(seq, sorted rows of that seq)], seq ascending: the canonical form of one group's rows."""
    by = {}
    for r in group_rows:
        by.setdefault(r[I_SEQ], []).append(r)
    return [(s, sorted(by[s])) for s in sorted(by)]


def extract(rows, needs, nsites=None):
    """needs: {"site", "start", "end", optional "seq_start" / "seq_end"} as sequences of ints (numpy
    arrays included). nsites: the number of registered site ordinals (a need for an ordinal >= nsites
    is empty whatever the rows hold)."""
    all_rows = row_tuples(rows)
    n = len(needs["site"])
    has_seq = needs.get("seq_start") is not None
    out = []
    for e in range(n):
        site, start, end = int(needs["site"][e]), int(needs["start"][e]), int(needs["end"][e])
        if (nsites is not None and site >= nsites) or start > end:
            out.append([])
            continue
        hit = [r for r in all_rows if r[I_SITE] == site and start <= r[I_DBV] <= end]
        groups = []
        for v in sorted({r[I_DBV] for r in hit}, reverse=True):
            of_v = [r for r in hit if r[I_DBV] == v]
            last, ts = max(r[I_SEQ] for r in of_v), max(r[I_TS] for r in of_v)
            if has_seq:
                a, b = int(needs["seq_start"][e]), int(needs["seq_end"][e])
                of_v = [r for r in of_v if a <= r[I_SEQ] <= b] if a <= b else []
            groups.append((v, last, ts, [r for _s, cls in seq_classes(of_v) for r in cls]))
        out.append(groups)
    return out


def from_oracle(rows, oracle_groups):
    """oracle.extract_changes' result (row index arrays) in this model's shape (row tuples)."""
    all_rows = row_tuples(rows)
    return [[(int(v), int(last), int(ts), [all_rows[int(i)] for i in g]) for v, last, ts, g in need]
            for need in oracle_groups]
