"""Interval model of the sync request planner, on the ABI arrays of corro_request_in.

A plain-Python restatement of parallel_sync's request loop (reference
crates/corro-agent/src/api/peer/mod.rs:1202-1318) and of chunk_range (:907-915). It judges
corro_plan_requests where tests/sync_req_util.py cannot: that oracle keeps one Python int per
requested version, this one keeps sorted lists of disjoint inclusive ranges of Python ints, so a
need 2^62 wide or ending at 2^64 - 2 costs what a need of three versions costs. Subtracting a range
from a book and inserting one cost time in the number of ranges they touch. It shares no code with
the product nor with sync_req_util.plan_session; only sync_req_util.frame_bytes (struct alone) is
reused to write the frames.

It reads the flat arrays (the dict sync_req_util.flatten returns), not nested session lists, and so
fixes what only the arrays can say:

* Sessions. Groups with equal grp_session form one session, whatever the value (the ABI wants the
  values non-decreasing, so they are neighbours). A session is named by its first group's index.
* Ranks. A server is a group; its rank in the round-robin is its group's order in the call.
* Books. What was already requested is kept per (first group index of the session, site ordinal)
  for Full needs and per (first group index, site ordinal, version) for Partial needs: the
  reference's HashMap<ActorId, ..> and HashMap<(ActorId, Version), ..>, made anew per sync. A
  version-0 Partial and a Full need of the same actor are different books.
* No items. An entry that no group covers (before grp_ent_off[0] or from grp_ent_off[G] on), a
  group with no entries, an entry with no needs and a Full need with start > end all yield no
  items, no frames and take no place in any round.
* A Partial with no seq ranges is one item (it takes a drain slot) and no frame.
* Two entries of one server with the same site share their books, since books are per actor, but
  each frame names its own entry in frame_entry.

chunk_range (:907-915): block starts are start, start + chunk, ... while <= end, and a block runs to
min(block start + chunk, end) inclusive. Neighbouring blocks so share an endpoint, and when chunk
divides end - start the last block is the single version `end`.

The loop (:1202-1318): every server's items (chunks of its Full needs and its Partials, in entry
and need order) form a deque; each round visits the servers that still hold items in rank order and
pops up to `drain` items from the back of each. A Full item asks for its range minus the actor's
Full book, one SyncNeedV1::Full per remaining run in ascending order, and adds them to the book. A
Partial item asks for the union of its seq ranges (overlapping and adjacent ones merged, as
RangeInclusiveSet does) minus the (actor, version) book, as one SyncNeedV1::Partial, and adds that.
An item with nothing left sends no frame. A frame's round is the round it was popped in.
"""
import bisect

import numpy as np

from tests.sync_req_util import frame_bytes


class Ranges:
    """A set of integers as a sorted list of disjoint, non-adjacent inclusive ranges."""

    def __init__(self):
        self.lo, self.hi = [], []

    def minus(self, a, b):
        """The parts of [a, b] outside the set, ascending."""
        out = []
        i = bisect.bisect_left(self.hi, a)           # first range that ends at or after a
        while a <= b:
            if i == len(self.lo) or self.lo[i] > b:
                out.append((a, b))
                break
            if self.lo[i] > a:
                out.append((a, self.lo[i] - 1))
            a = self.hi[i] + 1
            i += 1
        return out

    def insert(self, a, b):
        """Add [a, b], merging every range it overlaps or touches."""
        i = bisect.bisect_left(self.hi, a - 1)       # first range that ends at or after a - 1
        j = bisect.bisect_right(self.lo, b + 1)      # first range that starts after b + 1
        if i < j:
            a, b = min(a, self.lo[i]), max(b, self.hi[j - 1])
        self.lo[i:j] = [a]
        self.hi[i:j] = [b]

    def items(self):
        return list(zip(self.lo, self.hi))


def arrays(groups, lead=(), trail=()):
    """The corro_request_in arrays (numpy, as sync_req_util.flatten gives them) of `groups`, a list of
    (grp_session value, [entry, ...]); an entry is (site ordinal, [need, ...]) and a need is
    ("F", start, end) or ("P", version, [(s, e), ...]). `lead` and `trail` are entries laid out
    before the first group's and after the last group's: no group covers them."""
    A = {k: [] for k in ("site", "kind", "start", "end", "sr_off", "sr_n", "s_start", "s_end", "grp_session")}
    need_off = [0]

    def entries(ents):
        for site, needs in ents:
            A["site"].append(site)
            for nd in needs:
                full = nd[0] == "F"
                A["kind"].append(0 if full else 1)
                A["start"].append(nd[1])
                A["end"].append(nd[2] if full else nd[1])
                A["sr_off"].append(len(A["s_start"]))
                A["sr_n"].append(0 if full else len(nd[2]))
                for a, b in (() if full else nd[2]):
                    A["s_start"].append(a)
                    A["s_end"].append(b)
            need_off.append(len(A["kind"]))

    entries(lead)
    geo = [len(A["site"])]
    for session, ents in groups:
        A["grp_session"].append(session)
        entries(ents)
        geo.append(len(A["site"]))
    entries(trail)
    arr = {k: np.array(v, dtype=np.uint32 if k == "site" else np.uint8 if k == "kind" else np.uint64) for k, v in A.items()}
    arr["need_off"] = np.array(need_off, np.uint64)
    arr["grp_ent_off"] = np.array(geo, np.uint64)
    return arr


def chunk_range(s, e, chunk):
    """:907-915; empty when s > e."""
    return [(b, min(b + chunk, e)) for b in range(s, e + 1, chunk)]


def plan(arr, chunk, drain, sites):
    """What corro_plan_requests must return for the arrays `arr` and the registered site table
    `sites` (16 bytes per ordinal): group_bytes (per group its frames joined), frame_entry,
    frame_round and frame_needs over all frames in group order, and grp_frame_off."""
    A = {k: [int(x) for x in v] for k, v in arr.items()}
    sites = bytes(sites)
    n, G, T = len(A["site"]), len(A["grp_session"]), len(A["kind"])
    geo, noff, ses = A["grp_ent_off"], A["need_off"], A["grp_session"]
    if chunk < 1 or drain < 1 or len(geo) != G + 1 or len(noff) != n + 1 or len(sites) % 16:
        raise ValueError("bad call")
    if sorted(geo) != geo or geo[-1] > n or sorted(noff) != noff or noff[-1] > T or sorted(ses) != ses:
        raise ValueError("offsets or sessions out of order")
    if any(s >= len(sites) // 16 for s in A["site"]):
        raise ValueError("unregistered site")

    first = {}
    for g in range(G):
        first.setdefault(ses[g], g)
    deques = []
    for g in range(G):
        dq = []
        for ent in range(geo[g], geo[g + 1]):
            for t in range(noff[ent], noff[ent + 1]):
                if A["kind"][t] == 0:
                    if A["start"][t] <= A["end"][t] and A["end"][t] >= 1 << 63:
                        raise ValueError("Full end of 2^63 or more")
                    dq += [(ent, None, c) for c in chunk_range(A["start"][t], A["end"][t], chunk)]
                elif A["kind"][t] == 1:
                    o, m = A["sr_off"][t], A["sr_n"][t]
                    if o + m > len(A["s_start"]):
                        raise ValueError("seq ranges outside their array")
                    seqs = list(zip(A["s_start"][o:o + m], A["s_end"][o:o + m]))
                    if any(a > b or b >= (1 << 64) - 1 for a, b in seqs):
                        raise ValueError("bad seq range")
                    dq.append((ent, A["start"][t], seqs))
                else:
                    raise ValueError("bad need kind")
        deques.append(dq)

    frames = [[] for _ in range(G)]                  # per group: (round, entry, site, needs)
    for g0 in sorted(set(first.values())):
        live = [g for g in range(g0, G) if ses[g] == ses[g0]]
        full, part = {}, {}
        rnd = 0
        while live:
            nxt = []
            for g in live:
                dq = deques[g]
                for _ in range(min(drain, len(dq))):
                    ent, ver, what = dq.pop()
                    site = A["site"][ent]
                    if ver is None:
                        book = full.setdefault((g0, site), Ranges())
                        new = book.minus(*what)
                        needs = [("F", a, b) for a, b in new]
                    else:
                        book = part.setdefault((g0, site, ver), Ranges())
                        mine = Ranges()
                        for a, b in what:
                            mine.insert(a, b)
                        new = [p for a, b in mine.items() for p in book.minus(a, b)]
                        needs = [("P", ver, tuple(new))] if new else []
                    for a, b in new:
                        book.insert(a, b)
                    if needs:
                        frames[g].append((rnd, ent, site, needs))
                if dq:
                    nxt.append(g)
            live = nxt
            rnd += 1

    out = {"group_bytes": [], "frame_entry": [], "frame_round": [], "frame_needs": [], "grp_frame_off": [0]}
    for fr in frames:
        out["group_bytes"].append(b"".join(frame_bytes(sites[16 * s:16 * s + 16], nds) for _r, _e, s, nds in fr))
        out["frame_entry"] += [e for _r, e, _s, _n in fr]
        out["frame_round"] += [r for r, _e, _s, _n in fr]
        out["frame_needs"] += [len(nds) for _r, _e, _s, nds in fr]
        out["grp_frame_off"].append(len(out["frame_entry"]))
    return out
