"""Host restatements for the request decode tests: process_sync's screen of a need against the bookie
as the reference writes it (a loop over the versions, corro-agent/src/api/peer/mod.rs:857-870), frame
builders for SyncMessageV1::Request with any number of pairs, and the arrays corro_decode_requests must
produce for a list of frames."""
import struct

import numpy as np

from corrosion_amd import sync as S
from corrosion_amd import wire as W

NONE = 0xFFFFFFFF
E_INVALID, E_RANGE = -1, -6
SEQ_ALL = (0, 0xFFFFFFFF)


# ---- the screen ---------------------------------------------------------------------------------

def keeps(book, need):
    """True when process_sync hands the need to handle_need. book: None (the bookie has no such actor:
    `None => continue`) or (needed, max) with needed a list of inclusive ranges and max an int or None."""
    if book is None:
        return False
    needed, mx = book

    def answered(v):    # booked_read.needed().contains(&v) || booked_read.last().is_some_and(|max| v > max)
        return any(s <= v <= e for s, e in needed) or (mx is not None and v > mx)

    if isinstance(need, S.Full):
        if all(answered(v) for v in range(need.start, need.end + 1)):
            return False
    elif answered(need.version):
        return False
    return True


# ---- frames -------------------------------------------------------------------------------------

def need_bytes(nd):
    if isinstance(nd, S.Full):
        return struct.pack("<IQQ", 0, nd.start, nd.end)
    return struct.pack("<IQI", 1, nd.version, len(nd.seqs)) + b"".join(struct.pack("<QQ", s, e) for s, e in nd.seqs)


def request_payload(pairs):
    """SyncMessage::V1(SyncMessageV1::Request(pairs)), pairs = [(actor, [need, ...]), ...]."""
    out = [struct.pack("<III", 0, 4, len(pairs))]
    for actor, needs in pairs:
        out.append(bytes(actor) + struct.pack("<I", len(needs)) + b"".join(need_bytes(n) for n in needs))
    return b"".join(out)


def request_frame(pairs):
    return W.frame(request_payload(pairs))


def cat(frames):
    """Frames back to back -> (buf uint8, frame_off uint64), corro_requests' layout."""
    off = np.zeros(len(frames) + 1, np.uint64)
    off[1:] = np.cumsum([len(f) for f in frames], dtype=np.uint64) if frames else []
    return np.frombuffer(b"".join(frames), np.uint8), off


# ---- expected outputs ---------------------------------------------------------------------------

FIELDS = {"frame_status": np.int32, "frame_pair_off": np.uint64, "pair_actor": np.uint8, "pair_site": np.uint32,
          "pair_need_off": np.uint64, "kind": np.uint8, "start": np.uint64, "end": np.uint64, "sr_off": np.uint64,
          "sr_n": np.uint64, "s_start": np.uint64, "s_end": np.uint64, "need_site": np.uint32, "need_keep": np.uint8,
          "need_ent_off": np.uint64, "ent_site": np.uint32, "ent_start": np.uint64, "ent_end": np.uint64,
          "ent_seq_start": np.uint32, "ent_seq_end": np.uint32, "ent_need": np.uint64}


def expected(frames, site_of, books=None):
    """frames: [(frame bytes, expected status)]; a status-0 frame is parsed with wire.decode_sync_request.
    site_of: actor -> ordinal (absent = not registered). books: None = no screen, else {site: (needed,
    max)} (absent = the bookie has no such actor). Entries are built as serve.handle_needs_frames builds
    them: a Full need one every-seq entry, a Partial one every-seq entry and one per seq range (clamped)."""
    A = {k: [] for k in FIELDS}
    A["frame_pair_off"].append(0)
    for fb, st in frames:
        A["frame_status"].append(st)
        if st == 0:
            for actor, needs in W.decode_sync_request(fb[4:]):
                site = site_of.get(actor, NONE)
                A["pair_actor"] += list(actor)
                A["pair_site"].append(site)
                A["pair_need_off"].append(len(A["kind"]))
                for nd in needs:
                    part = isinstance(nd, S.Partial)
                    t = len(A["kind"])
                    A["kind"].append(1 if part else 0)
                    A["start"].append(nd.version if part else nd.start)
                    A["end"].append(nd.version if part else nd.end)
                    A["sr_off"].append(len(A["s_start"]))
                    A["sr_n"].append(len(nd.seqs) if part else 0)
                    A["need_site"].append(site)
                    keep = site != NONE and (books is None or keeps(books.get(site), nd))
                    A["need_keep"].append(1 if keep else 0)
                    A["need_ent_off"].append(len(A["ent_site"]))
                    for s, e in (nd.seqs if part else ()):
                        A["s_start"].append(s)
                        A["s_end"].append(e)
                    if keep:
                        for s, e in [SEQ_ALL] + ([tuple(r) for r in nd.seqs] if part else []):
                            A["ent_site"].append(site)
                            A["ent_start"].append(A["start"][t])
                            A["ent_end"].append(A["end"][t])
                            A["ent_seq_start"].append(max(0, min(s, 0xFFFFFFFF)))
                            A["ent_seq_end"].append(max(0, min(e, 0xFFFFFFFF)))
                            A["ent_need"].append(t)
        A["frame_pair_off"].append(len(A["pair_site"]))
    A["pair_need_off"].append(len(A["kind"]))
    A["need_ent_off"].append(len(A["ent_site"]))
    out = {k: np.array(v, dtype=FIELDS[k]) for k, v in A.items()}
    out.update(nframes=len(frames), npairs=len(A["pair_site"]), nneeds=len(A["kind"]), nseqs=len(A["s_start"]),
               nents=len(A["ent_site"]))
    return out


def book_arrays(books, nsites):
    """{site: (needed, max)} -> the CSR book decode_requests takes, over ordinals [0, nsites)."""
    known, mx, off, gs, ge = [], [], [0], [], []
    for s in range(nsites):
        b = books.get(s)
        known.append(0 if b is None else 1)
        mx.append(-1 if b is None or b[1] is None else b[1])
        for a, z in (b[0] if b else ()):
            gs.append(a)
            ge.append(z)
        off.append(len(gs))
    return {"known": np.array(known, np.uint8), "max": np.array(mx, np.int64), "gap_off": np.array(off, np.uint64),
            "gap_start": np.array(gs, np.uint64), "gap_end": np.array(ge, np.uint64)}


# ---- the random screen workload -----------------------------------------------------------------

SCREEN_SEED = 20241
VMAX = 64


def random_screen_trial(rng, actors):
    """One trial: a book for up to 6 actors (up to 5 canonical gaps each, versions below 64) and one
    frame per actor of Full and Partial needs. Returns ({actor index: (needed, max) | None}, frames)."""
    books, frames = {}, []
    for a in range(int(rng.integers(1, len(actors) + 1))):
        if rng.random() < 0.1:
            books[a] = None
        else:
            cuts = sorted(rng.choice(np.arange(1, VMAX - 4), size=2 * int(rng.integers(0, 6)), replace=False).tolist())
            gaps = []
            for s, e in zip(cuts[::2], cuts[1::2]):
                e -= 1                                     # the next gap starts past e + 1: non-touching
                if gaps and s <= gaps[-1][1] + 1:
                    continue
                if s <= e:
                    gaps.append((s, e))
            top = gaps[-1][1] + 1 if gaps else 1
            mx = None if rng.random() < 0.15 else int(rng.integers(top, VMAX))
            books[a] = (gaps, mx)
        needs = []
        for _ in range(int(rng.integers(1, 7))):
            if rng.random() < 0.6:
                s = int(rng.integers(0, VMAX))
                w = int(rng.integers(-1, 8)) if rng.random() < 0.7 else int(rng.integers(0, VMAX))
                needs.append(S.Full(s, max(0, min(VMAX - 1, s + w)) if w >= 0 else max(0, s - 1)))
            else:
                needs.append(S.Partial(int(rng.integers(0, VMAX)),
                                       tuple((int(q), int(q) + 2) for q in range(int(rng.integers(0, 3))))))
        frames.append(request_frame([(actors[a], needs)]))
    return books, frames
