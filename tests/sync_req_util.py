"""Test oracle of the sync request planner: a sequential restatement of parallel_sync's request loop
(reference crates/corro-agent/src/api/peer/mod.rs:1131-1318, chunk_range :907-915), deliberately
naive. Requested versions and seqs are Python sets of ints, runs are rebuilt by sorting, and the
frames are written with struct alone. It shares no code with the product.

A need is ("F", start, end) or ("P", version, ((s, e), ...)). A server is its entries in order:
[(actor bytes, [need, ...]), ...]. A session is its servers in order; servers without entries are
skipped as :1135-1138 does.
"""
import struct

import numpy as np


def chunk_range(s, e, chunk):
    """:907-915: range.step_by(chunk) block starts, each block ending at min(start + chunk, end)."""
    return [(b, min(b + chunk, e)) for b in range(s, e + 1, chunk)]


def runs(values):
    out = []
    for v in sorted(values):
        if out and out[-1][1] + 1 == v:
            out[-1][1] = v
        else:
            out.append([v, v])
    return [tuple(r) for r in out]


def plan_session(servers, chunk=10, drain=10):
    """Per server (empty ones included, with no frames) the list of (round, entry index, actor,
    [need, ...]) in sending order."""
    out = [[] for _ in servers]
    live = []
    for sv, ents in enumerate(servers):
        if not ents:
            continue
        dq = []
        for ei, (actor, needs) in enumerate(ents):
            for nd in needs:
                if nd[0] == "F":
                    dq += [(ei, actor, ("F", a, b)) for a, b in chunk_range(nd[1], nd[2], chunk)]
                else:
                    dq.append((ei, actor, nd))
        live.append((sv, dq))
    req_full, req_partials = {}, {}
    rnd = 0
    while live:
        nxt = []
        for sv, dq in live:
            if not dq:
                continue
            drained = 0
            while drained < drain and dq:
                ei, actor, nd = dq.pop()
                drained += 1
                if nd[0] == "F":
                    book = req_full.setdefault(actor, set())
                    new = [v for v in range(nd[1], nd[2] + 1) if v not in book]
                    if not new:
                        continue
                    book.update(new)
                    actual = [("F", a, b) for a, b in runs(new)]
                else:
                    book = req_partials.setdefault((actor, nd[1]), set())
                    mine = set()
                    for a, b in nd[2]:
                        mine.update(range(a, b + 1))
                    new = mine - book
                    if not new:
                        continue
                    book |= new
                    actual = [("P", nd[1], tuple(runs(new)))]
                out[sv].append((rnd, ei, actor, actual))
            if dq:
                nxt.append((sv, dq))
        live = nxt
        rnd += 1
    return out


def frame_bytes(actor, needs):
    """The LengthDelimitedCodec frame of SyncMessage::V1(SyncMessageV1::Request(vec![(actor, needs)]))."""
    p = struct.pack("<III", 0, 4, 1) + bytes(actor) + struct.pack("<I", len(needs))
    for nd in needs:
        if nd[0] == "F":
            p += struct.pack("<IQQ", 0, nd[1], nd[2])
        else:
            p += struct.pack("<IQI", 1, nd[1], len(nd[2])) + b"".join(struct.pack("<QQ", a, b) for a, b in nd[2])
    return struct.pack(">I", len(p)) + p


def flatten(sessions, site_of):
    """Sessions -> the host arrays of corro_request_in (numpy) and, per group, (session, server,
    first entry index)."""
    A = {k: [] for k in ("site", "kind", "start", "end", "sr_off", "sr_n", "s_start", "s_end", "grp_session")}
    need_off, geo, groups = [0], [0], []
    for sn, servers in enumerate(sessions):
        for sv, ents in enumerate(servers):
            if not ents:
                continue
            groups.append((sn, sv, len(A["site"])))
            A["grp_session"].append(sn)
            for actor, needs in ents:
                A["site"].append(site_of[actor])
                for nd in needs:
                    A["kind"].append(0 if nd[0] == "F" else 1)
                    A["start"].append(nd[1])
                    A["end"].append(nd[2] if nd[0] == "F" else nd[1])
                    A["sr_off"].append(len(A["s_start"]))
                    A["sr_n"].append(0 if nd[0] == "F" else len(nd[2]))
                    if nd[0] == "P":
                        for a, b in nd[2]:
                            A["s_start"].append(a)
                            A["s_end"].append(b)
                need_off.append(len(A["kind"]))
            geo.append(len(A["site"]))
    arr = {k: np.array(v, dtype=np.uint32 if k == "site" else np.uint8 if k == "kind" else np.uint64) for k, v in A.items()}
    arr["need_off"] = np.array(need_off, np.uint64)
    arr["grp_ent_off"] = np.array(geo, np.uint64)
    return arr, groups


def expected(sessions, groups, chunk=10, drain=10):
    """What corro_plan_requests must return for flatten()'s arrays: per group the joined frame bytes,
    the frame table columns over all groups, and the groups' frame offsets."""
    plans = [plan_session(s, chunk, drain) for s in sessions]
    bufs, entry, rnd, needs, gfo = [], [], [], [], [0]
    for sn, sv, e0 in groups:
        fr = plans[sn][sv]
        bufs.append(b"".join(frame_bytes(a, nds) for _r, _e, a, nds in fr))
        entry += [e0 + e for _r, e, _a, _n in fr]
        rnd += [r for r, _e, _a, _n in fr]
        needs += [len(n) for _r, _e, _a, n in fr]
        gfo.append(len(entry))
    return {"group_bytes": bufs, "frame_entry": entry, "frame_round": rnd, "frame_needs": needs, "grp_frame_off": gfo}


ACTORS = [bytes([16 * k + i for i in range(16)]) for k in range(4)]


def random_session(rng, max_ver=150):
    """<= 4 servers, <= 4 actors, versions <= max_ver; partials with a few small seq ranges that may
    overlap, touch or come out of order; some servers empty."""
    servers = []
    for _ in range(int(rng.integers(1, 5))):
        ents = []
        for a in rng.permutation(4)[: int(rng.integers(0, 5))]:
            needs = []
            for _ in range(int(rng.integers(1, 4))):
                if rng.random() < 0.65:
                    s = int(rng.integers(1, max_ver + 1))
                    needs.append(("F", s, min(max_ver, s + int(rng.integers(0, 40)))))
                else:
                    seqs = []
                    for _ in range(int(rng.integers(1, 4))):
                        s = int(rng.integers(0, 30))
                        seqs.append((s, s + int(rng.integers(0, 8))))
                    needs.append(("P", int(rng.integers(1, 6)), tuple(seqs)))
            ents.append((ACTORS[int(a)], needs))
        servers.append(ents)
    return servers


def random_sessions(count=300, seed=20240):
    rng = np.random.default_rng(seed)
    return [random_session(rng) for _ in range(count)]


def tile_edge_sessions():
    """The sessions of the output-tile test: one Partial of 600 shuffled disjoint ranges (a 9,652-byte
    frame), 400 one-need Full frames, and a server whose frames fill 8192 bytes exactly."""
    A0 = ACTORS[0]
    rng = np.random.default_rng(9)
    ranges = [(20 * k, 20 * k + 7) for k in range(600)]
    shuffled = tuple(ranges[i] for i in rng.permutation(600))
    big = [[(A0, [("P", 3, shuffled)])]]
    many = [[(A0, [("F", 20 * k, 20 * k + 3) for k in range(400)])]]
    # 143 one-piece Full frames (56 bytes) and Partials of two and three ranges (84 and 100 bytes) fill
    # 8192 bytes exactly: the second group's first frame starts on the tile edge
    edge = [[(A0, [("P", 9, ((1, 2), (4, 5))), ("P", 8, ((1, 2), (4, 5), (7, 8)))] +
              [("F", 20 * k, 20 * k + 3) for k in range(143)])],
            [(ACTORS[1], [("F", 1, 5), ("P", 2, ((0, 0),))])]]
    return big, many, edge


def quirk_sessions():
    """The sessions of the quirk test, one oddity of the reference's loop each."""
    A0 = ACTORS[0]
    return [
        [[(A0, [("F", 1, 21)])]],                                   # (e - s) % chunk == 0: a trailing one-version chunk
        [[(A0, [("F", 9, 3), ("F", 4, 4)])], [(A0, [("F", 7, 2)])]],  # s > e: no item; a server left without items
        [[(A0, [("P", 5, ()), ("P", 6, ((3, 3),))])]],               # an empty seq list: no frame
        [[(A0, [("P", 5, ((0, 4), (5, 9)))])]],                       # adjacent seqs merge
        [[(A0, [("F", 1, 30), ("P", 2, ((0, 9),))])], [(A0, [("F", 5, 25), ("P", 2, ((2, 3), (9, 9)))])],
         [(ACTORS[2], [("F", 1, 3)])]],                            # a server all of whose items are deduped away
    ]
