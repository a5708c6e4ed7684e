"""A second host model of SyncStateV1::compute_available_needs (sync.rs:127-249), independent of the
oracle (which edits a range set) and of the kernel (which sweeps over holes).

The have ranges are found by classification: every bound b of the entry and b + 1 is a breakpoint,
membership ("in the universe and in no hole") is constant on each elementary interval between two
consecutive breakpoints, and maximal runs of member intervals are the have ranges. The reference's
clauses are then applied literally: overlapping(range) yields every have range with
end >= range.start and start <= range.end (an inverted range s > t included: rangemap compares the
bounds as given), and the need is max(start) ..= min(end). All arithmetic is on Python ints, so a
bound of 2^64 - 1 is like any other.

Sides are the dicts of tests.sync_util.entries_from_pairs; the result has the shape of
tests.sync_util.decode_needs.
"""
from functools import lru_cache

import numpy as np


@lru_cache(maxsize=1 << 16)
def have_ranges(lo, hi, holes):
    """Maximal runs of {lo..=hi} minus the union of `holes` (a tuple of (s, e), s <= e, any order)."""
    if hi < lo:
        return ()
    bounds = {lo, hi}
    for s, e in holes:
        if s > e:
            raise ValueError("RangeInclusiveSet::remove asserts start <= end")
        bounds.add(s)
        bounds.add(e)
    points = sorted(bounds | {b + 1 for b in bounds})
    runs = []
    for p, nxt in zip(points, points[1:]):
        # [p, nxt - 1] is elementary: no set changes membership inside it
        member = lo <= p <= hi and not any(s <= p <= e for s, e in holes)
        if not member:
            continue
        if runs and runs[-1][1] == p - 1:
            runs[-1][1] = nxt - 1
        else:
            runs.append([p, nxt - 1])
    return tuple((a, b) for a, b in runs)


def overlapping(haves, s, t):
    """rangemap's overlapping(s..=t), inverted ranges included, then the reference's max / min."""
    return [(max(s, a), min(t, b)) for a, b in haves if b >= s and a <= t]


def entry_needs(our, their):
    head = their["head"]
    tparts = {int(v): r for v, r in their.get("partials", {}).items()}
    holes = tuple((s, e) for s, e in their.get("need", [])) + tuple((v, v) for v in sorted(tparts))
    haves = have_ranges(1, head, holes)
    out = []
    for s, t in our.get("need", []):
        out.extend(("full", a, b) for a, b in overlapping(haves, s, t))
    oparts = {int(v): r for v, r in our.get("partials", {}).items()}
    for v in sorted(oparts):
        seqs = [tuple(r) for r in oparts[v]]
        if any(a <= v <= b for a, b in haves):
            out.append(("partial", v, seqs))
        elif v in tparts:
            tseqs = tuple(tuple(r) for r in tparts[v])
            ends = [e for _, e in tseqs] + [e for _, e in seqs]
            if not ends:
                continue
            shaves = have_ranges(0, max(ends), tseqs)
            got = [p for s, t in seqs for p in overlapping(shaves, s, t)]
            if got:
                out.append(("partial", v, got))
    ours = our.get("head")
    if ours is None:
        out.append(("full", 1, head))
    elif head > ours:
        out.append(("full", ours + 1, head))
    return out


def needs(pairs):
    return [entry_needs(our, their) for our, their in pairs]


def to_csr(lists):
    """Decoded needs (per entry) -> the CSR arrays of corro_compute_needs."""
    need_off, seq_off = [0], [0]
    kind, start, end, sr_off, sr_n, s_start, s_end = [], [], [], [], [], [], []
    for lst in lists:
        for x in lst:
            sr_off.append(len(s_start))
            if x[0] == "full":
                kind.append(0); start.append(x[1]); end.append(x[2]); sr_n.append(0)
            else:
                kind.append(1); start.append(x[1]); end.append(x[1]); sr_n.append(len(x[2]))
                for s, e in x[2]:
                    s_start.append(s); s_end.append(e)
        need_off.append(len(kind))
        seq_off.append(len(s_start))
    u = lambda a: np.array(a, dtype=np.uint64)
    return {"need_off": u(need_off), "seq_off": u(seq_off), "kind": np.array(kind, dtype=np.uint8),
            "start": u(start), "end": u(end), "sr_off": u(sr_off), "sr_n": u(sr_n),
            "s_start": u(s_start), "s_end": u(s_end)}
