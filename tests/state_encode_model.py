"""A plain-Python restatement of generate_sync (corro-types/src/sync.rs:284-333) over a sync book, the
model of corro_encode_states (include/corro_hip.h): rows of (actor, max, needed gaps, partials with the seq
ranges they hold) -> sync.SyncStateV1, its frame through the host codec, and the status rules. Written from
the header's statement; it shares no code with corro_generate_sync or the kernels.

A row here is (actor, max or None, [(gap start, gap end)], [(version, last_seq, [(present start, end)])])."""
import numpy as np

from corrosion_amd import wire as W
from corrosion_amd.sync import SyncStateV1

INVALID, RANGE = -1, -6
U64 = (1 << 64) - 1
MAX32 = (1 << 32) - 1
KEYS = ("actor", "max", "gap_off", "gap_start", "gap_end", "part_off", "part_version", "part_last_seq", "psr_off",
        "psr_start", "psr_end")


def seq_gaps(present, last_seq):
    """The complement of the present ranges (ascending, disjoint), clipped to last_seq, within [0, last_seq].
    Python integers: no step can wrap."""
    out, x = [], 0                                  # x: the first seq not yet accounted for
    for s, e in present:
        if s > last_seq:
            break
        if s > x:
            out.append((x, s - 1))
        x = e + 1
        if x > last_seq:
            return out
    out.append((x, last_seq))
    return out


def is_complete(present, last_seq):
    """PartialVersion::is_complete (agent.rs:1068-1074): no gap over 1..=last_seq -- seq 0 is not looked at, and
    last_seq = 0 gives an empty range."""
    return not any(e >= 1 for _s, e in seq_gaps(present, last_seq))


def canonical(ranges):
    """Ascending, each start <= end, and no two ranges overlapping or touching."""
    return all(s <= e for s, e in ranges) and all(b[0] > a[1] + 1 for a, b in zip(ranges, ranges[1:]))


def rows_canonical(rows):
    for _actor, _mx, gaps, parts in rows:
        if not canonical(gaps) or any(not canonical(pr) for _v, _l, pr in parts):
            return False
        if any(b[0] <= a[0] for a, b in zip(parts, parts[1:])):
            return False
    return True


def generate_sync(rows, self_actor, ts=None):
    """generate_sync over the rows: the three maps in row order, one actor's versions ascending."""
    st = SyncStateV1(actor_id=bytes(self_actor), last_cleared_ts=ts)
    for actor, mx, gaps, parts in rows:
        if mx is None:
            continue
        actor = bytes(actor)
        if gaps:
            st.need[actor] = [(int(s), int(e)) for s, e in gaps]
        for v, last, present in parts:
            if not is_complete(present, last):
                st.partial_need.setdefault(actor, {})[int(v)] = seq_gaps(present, last)
        st.heads[actor] = int(mx)
    return st


def rows_of_book(book, lo=0, hi=None):
    """Rows [lo, hi) of a book of arrays (Agent.sync_book(), sync.concat_books) as this model's rows."""
    I = lambda a: [int(x) for x in a]
    go, po, so = I(book["gap_off"]), I(book["part_off"]), I(book["psr_off"])
    gs, ge, pv, pl = I(book["gap_start"]), I(book["gap_end"]), I(book["part_version"]), I(book["part_last_seq"])
    ss, se = I(book["psr_start"]), I(book["psr_end"])
    actor = np.asarray(book["actor"], np.uint8).reshape(-1, 16)
    rows = []
    for r in range(lo, len(book["max"]) if hi is None else hi):
        mx = int(book["max"][r])
        parts = [(pv[p], pl[p], list(zip(ss[so[p]:so[p + 1]], se[so[p]:so[p + 1]]))) for p in range(po[r], po[r + 1])]
        rows.append((bytes(actor[r]), None if mx == -1 else mx & U64, list(zip(gs[go[r]:go[r + 1]], ge[go[r]:go[r + 1]])), parts))
    return rows


def book_of_rows(rows):
    """The rows as a sync book's arrays (what Agent.sync_book() returns for a bookie holding them)."""
    b = {k: [] for k in KEYS}
    b["gap_off"], b["part_off"], b["psr_off"] = [0], [0], [0]
    for actor, mx, gaps, parts in rows:
        b["actor"].append(np.frombuffer(bytes(actor), np.uint8))
        b["max"].append(-1 if mx is None else mx - (1 << 64) if mx >= 1 << 63 else mx)
        for s, e in gaps:
            b["gap_start"].append(s)
            b["gap_end"].append(e)
        b["gap_off"].append(len(b["gap_start"]))
        for v, last, present in parts:
            b["part_version"].append(v)
            b["part_last_seq"].append(last)
            for s, e in present:
                b["psr_start"].append(s)
                b["psr_end"].append(e)
            b["psr_off"].append(len(b["psr_start"]))
        b["part_off"].append(len(b["part_version"]))
    out = {k: np.array(v, np.int64 if k == "max" else np.uint64) for k, v in b.items() if k != "actor"}
    out["actor"] = np.concatenate(b["actor"]).reshape(-1, 16) if rows else np.zeros((0, 16), np.uint8)
    return out


def encode_model(states, self_actors, ts=None, max_payload=0):
    """What corro_encode_states returns for `states` (a list of row lists): dict(frames, a list of byte strings,
    empty for a state with a status; state_status; n_heads, n_need, n_partial)."""
    ts = ts or [None] * len(states)
    limit = MAX32 if max_payload == 0 or max_payload > MAX32 else max_payload
    out = {"frames": [], "state_status": [], "n_heads": [], "n_need": [], "n_partial": []}
    for rows, me, t in zip(states, self_actors, ts):
        st, payload = generate_sync(rows, me, t), b""
        status = 0 if rows_canonical(rows) else INVALID
        if status == 0:
            payload = W.encode_sync_state(st)
            if len(payload) > limit:
                status = RANGE
        ok = status == 0
        out["frames"].append(W.frame(payload) if ok else b"")
        out["state_status"].append(status)
        out["n_heads"].append(len(st.heads) if ok else 0)
        out["n_need"].append(len(st.need) if ok else 0)
        out["n_partial"].append(len(st.partial_need) if ok else 0)
    return out
