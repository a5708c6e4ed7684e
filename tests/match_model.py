"""A plain-Python restatement of corrosion's match_changes, the yardstick of corro_match_changes.

A change is a (table, pk, cid, cl) tuple: table a name, pk any hashable row key, cid a column name with
SENTINEL for the row sentinel. A handle is ("sub", {table: [columns]}) or ("update", table). Candidates
are real insertion-ordered dicts {table: {pk: cl}}, the MatchCandidates = IndexMap<TableName,
IndexMap<pk, cl>> of the reference:

  filter_sub      Subscription's filter_matchable_change (corro-types/src/pubsub.rs:294-332)
  filter_update   UpdateHandle's filter_matchable_change (corro-types/src/updates.rs:92-121)
  match_changes   updates.rs:420-481: per handle, one walk over one changeset's changes
  handle_candidates  updates.rs:270-305: the (Update | Delete, pk) events by cl parity
"""
SENTINEL = "-1"
UPDATE, DELETE = "Update", "Delete"


def _insert(cands, table, pk, cl):
    pks = cands.get(table)
    if pks is None:
        cands[table] = {pk: cl}
        return True
    fresh = pk not in pks
    pks[pk] = cl
    return fresh


def filter_sub(table_columns, cands, change):
    table, pk, cid, cl = change
    if pk in cands.get(table, ()):              # don't double process the same pk
        return False
    cols = table_columns.get(table)
    if cols is None or not (cid == SENTINEL or cid in cols):
        return False
    return _insert(cands, table, pk, cl)


def filter_update(name, cands, change):
    table, pk, _cid, cl = change
    if table != name:
        return False
    if pk in cands.get(table, ()):
        return False
    return _insert(cands, table, pk, cl)


def filter_change(handle, cands, change):
    kind, what = handle
    return filter_sub(what, cands, change) if kind == "sub" else filter_update(what, cands, change)


def match_changes(handles, changes):
    """One changeset's changes against every handle: per handle (candidates, matched_count), or None for
    every handle when the reference returns before its walk (no change, or no handle)."""
    if not changes or not handles:
        return [None] * len(handles)
    out = []
    for h in handles:
        cands = {}
        for ch in changes:
            filter_change(h, cands, ch)
        out.append((cands, sum(len(p) for p in cands.values())))
    return out


def handle_candidates(cands):
    """The NotifyEvent stream of one MatchCandidates: (Update | Delete, pk), tables then pks in map order."""
    return [(DELETE if cl % 2 == 0 else UPDATE, pk) for pks in cands.values() for pk, cl in pks.items()]


def by_handle(handles, changesets):
    """changesets: per changeset the list of its impactful changes. Per handle the list of (changeset
    index, candidates) for the changesets that gave it at least one candidate: what
    corrosion_amd.updates.candidates_by_handle returns."""
    out = [[] for _ in handles]
    for s, changes in enumerate(changesets):
        for k, r in enumerate(match_changes(handles, changes)):
            if r is not None and r[0]:
                out[k].append((s, r[0]))
    return out
