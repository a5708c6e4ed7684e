"""Saving and restoring the bookie and its device row pool: corro_bookie_save / corro_bookie_load next to
the only routes there were before them.

An agent buffers --rows partial rows through process_frames: --actors actors, every version arriving as
two pieces of --piece changes with a one-seq hole between them (seqs 0 .. piece-1 and piece+1 .. 2*piece,
last_seq = 2*piece + 1), so every version stays partial, holds two pool segments and two
__corro_seq_bookkeeping rows, and no row ever visits the host. Then, alternating, after --warmup rounds,
--steps rounds of:

  save_device   corro_bookie_save, rows to CORRO_MEM_DEVICE (both passes, output allocation included)
  save_host     corro_bookie_save, rows to CORRO_MEM_HOST
  load_device   corro_bookie_load of the device image into a fresh bookie
  load_host     corro_bookie_load of the host image into a fresh bookie
  old_save      every buffered version read back with corro_bookie_buffered, one call per version (what a
                caller had to do to persist the rows); it reads a key out of the pool for good, so each
                round runs on a bookie freshly loaded from the image
  old_load      the rows re-fed as partial changesets, one per segment, through
                corro_process_multiple_changes (device rows, host headers) into a fresh bookie. This
                rebuilds the rows and the seq books but NOT the needed gaps or max of an actor whose
                versions were cleared or applied: it is not a complete restore

Every entry point synchronises its stream before it returns, so the figures are wall-clock times around
the calls. Prints one JSON line: min / max ms per route, and the shape (versions, segments). No threshold
is asserted. --versions-scan R1,R2,... repeats the four new routes at the same row count with other
piece sizes (fewer, longer versions), to show what does and does not scale with the number of versions.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--actors", type=int, default=1000)
    ap.add_argument("--piece", type=int, default=4, help="changes per piece; a version holds two pieces")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--versions-scan", default="", help="comma-separated piece sizes to repeat the new routes at")
    ap.add_argument("--no-old", action="store_true", help="skip the two old routes")
    args = ap.parse_args()

    import numpy as np
    import torch
    import corrosion_amd as ca
    from corrosion_amd import _lib as L
    from corrosion_amd import serve, wire
    from corrosion_amd.agent import Bookie, Change, ChangeV1, Full

    actors = [bytes([k & 255, k >> 8] + [9] * 14) for k in range(args.actors)]

    def make_agent(piece):
        per_actor = max(1, args.rows // (2 * piece * args.actors))
        agent = ca.agent.Agent({"t": ["c"]}, capacity_hint=1 << 16, actor_id=b"\xA0" * 16)
        for a in actors:
            agent.site(a)
        last = 2 * piece + 1
        batch, nb = [], 0
        for ai, a in enumerate(actors):
            for v in range(1, per_actor + 1):
                pk0 = (ai * per_actor + v) * (last + 1)
                for s0 in (0, piece + 1):
                    ch = [Change("t", pk0 + s, "c", v * 31 + s, 1, v, s, a, 1) for s in range(s0, s0 + piece)]
                    batch.append(ChangeV1(a, Full(v, ch, (s0, s0 + piece - 1), last, ts=1000 + v)))
                    nb += piece
            if nb >= 200_000 or ai == len(actors) - 1:
                res, status = agent.process_frames(wire.frames(batch))
                assert not np.asarray(status).any() and all(k == "partial" for k in res.known)
                print(f"piece {piece}: buffered actor {ai + 1} of {len(actors)}", file=sys.stderr, flush=True)
                batch, nb = [], 0
        return agent, per_actor * args.actors

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def fresh_load(agent, image):
        bk = Bookie()
        bk.load(image, agent.engine)
        return bk

    def old_save(agent, bk, versions):
        n = 0
        for a in actors:
            for v in versions:
                _r, m = serve._buffered_rows(bk, a, v, 0, 0xFFFFFFFF)
                n += m
        return n

    def old_load_inputs(agent, image):
        """One partial changeset per segment of the image's (sorted) rows: host headers over the device rows."""
        r = image["rows"]
        site, dbv, seq = (r[k].cpu().numpy() for k in ("site", "db_version", "seq"))
        n = len(seq)
        head = np.ones(n, bool)
        head[1:] = (site[1:] != site[:-1]) | (dbv[1:] != dbv[:-1]) | (seq[1:].astype(np.int64) != seq[:-1].astype(np.int64) + 1)
        start = np.flatnonzero(head)
        count = np.diff(np.append(start, n))
        ids = np.frombuffer(b"".join(agent.engine.site_ids()), np.uint8).copy()
        hdr = np.zeros(len(start), np.dtype([("actor_id", "<u8"), ("site", "<u4"), ("kind", "<u4"), ("version_start", "<u8"),
                                             ("version_end", "<u8"), ("seq_start", "<u8"), ("seq_end", "<u8"),
                                             ("last_seq", "<u8"), ("ts", "<u8"), ("change_off", "<u8"), ("change_count", "<u8")]))
        assert hdr.dtype.itemsize == C.sizeof(L.Changeset)
        hdr["actor_id"] = ids.ctypes.data + 16 * site[start].astype(np.uint64)
        hdr["site"], hdr["kind"] = site[start], L.CORRO_CS_FULL
        hdr["version_start"] = hdr["version_end"] = dbv[start]
        hdr["seq_start"], hdr["seq_end"] = seq[start], seq[start] + count - 1
        hdr["last_seq"] = 2 * image["piece"] + 1
        hdr["ts"] = r["ts"].cpu().numpy()[start]
        hdr["change_off"], hdr["change_count"] = start, count
        s = L.Changes()
        s.n = n
        for k in ("pk", "table_cid", "col_version", "db_version", "cl", "seq", "site", "val0", "val1", "val_type", "val_len", "ts"):
            setattr(s, k, r[k].data_ptr())
        return hdr, s, ids

    def old_load(agent, hdr, s):
        bk = Bookie()
        known = np.zeros(len(hdr), np.int32)
        imp = torch.zeros(max(1, s.n), dtype=torch.uint8, device="cuda")
        out = L.ProcessOut()
        out.known, out.impactful = known.ctypes.data, imp.data_ptr()
        torch.cuda.synchronize()
        L.check(L.lib().corro_process_multiple_changes(agent.engine._h, bk._h, hdr.ctypes.data, len(hdr), C.byref(s),
                                                       L.CORRO_MEM_DEVICE, C.byref(out)))
        assert (known == 3).all()                               # every piece buffered as a partial
        return bk

    def measure(piece, old):
        agent, nversions = make_agent(piece)
        per_actor = nversions // args.actors
        t = {}

        def add(name, ms):
            t.setdefault(name, []).append(ms)
        img_d = img_h = None
        for step in range(args.warmup + args.steps):
            rec = step >= args.warmup
            print(f"piece {piece}: round {step + 1} of {args.warmup + args.steps}", file=sys.stderr, flush=True)
            ms, img_d = wall(lambda: agent.save_bookie(device=True))
            rec and add("save_device", ms)
            ms, img_h = wall(lambda: agent.save_bookie())
            rec and add("save_host", ms)
            ms, bk = wall(lambda: fresh_load(agent, img_d))
            rec and add("load_device", ms)
            if old:
                ms, nread = wall(lambda: old_save(agent, bk, range(1, per_actor + 1)))
                assert nread == img_d["nrows"]
                rec and add("old_save", ms)
            del bk
            ms, bk = wall(lambda: fresh_load(agent, img_h))
            rec and add("load_host", ms)
            del bk
            if old:
                img_d["piece"] = piece
                hdr, s, keep = old_load_inputs(agent, img_d)
                ms, bk = wall(lambda: old_load(agent, hdr, s))
                rec and add("old_load", ms)
                del bk
        return {"piece": piece, "rows": int(img_d["nrows"]), "versions": nversions, "segments": 2 * nversions,
                "ms": {k: {"min": min(v), "max": max(v)} for k, v in t.items()}}

    main_run = measure(args.piece, not args.no_old)
    scan = [measure(int(p), False) for p in args.versions_scan.split(",") if p]
    line = {"metric": "bookie save to device memory, ms (min)", "value": main_run["ms"]["save_device"]["min"], "unit": "ms",
            "higher_is_better": False, "steps": args.steps, "warmup": args.warmup, "data": "synthetic",
            "config": {"rows": args.rows, "actors": args.actors, "piece": args.piece},
            "run": main_run, "versions_scan": scan,
            "note": "old_load rebuilds rows and seq books only: not the needed gaps or max of cleared / applied versions"}
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
