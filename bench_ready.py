"""Draining the ready versions: corro_process_fully_buffered_batch (Agent.process_ready) next to the
one-by-one call it is equivalent to, and to the floor under both.

An agent buffers --rows partial rows through process_frames the way bench_restore.py does: --actors
actors, every version arriving as two pieces of --piece changes -- here adjacent (seqs 0 .. piece-1 and
piece .. 2*piece-1, last_seq = 2*piece-1), so every version is complete, holds two pool segments and is
listed as ready; no row ever visits the host. The bookie is saved once (device image); every route of
every round runs on a bookie freshly loaded from that image (the load is not timed) and on a state reset
just before (not timed either), so each route merges the same rows into the same empty state.
Alternating in one process, after --warmup rounds, --steps rounds of:

  batch        corro_process_fully_buffered_batch over every ready version (the arrays of the pairs built
               before the clock starts: the figure is the call's)
  one_by_one   corro_process_fully_buffered, one call per version, over a fixed sample of the list (every
               k-th pair, at most --sample of them); reported per version, and extrapolated to the whole
               list under that label
  floor        corro_apply_batch of the same rows as one device batch with impact flags (the image's rows,
               already on the device): what the drain costs when nothing is gathered or booked

Every entry point synchronises its stream before it returns, so the figures are wall-clock times around
the calls. Prints one JSON line: min / max ms per route and the shape. No threshold is asserted.
--versions-scan P1,P2,... repeats the routes at the same row count with other piece sizes (fewer, longer
versions), to show which route follows the rows and which the versions. --versions N sets the row count
from a number of versions (rows = N * 2 * piece).
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
    ap.add_argument("--versions", type=int, default=0, help="ready versions (overrides --rows: rows = versions * 2 * piece)")
    ap.add_argument("--actors", type=int, default=1000)
    ap.add_argument("--piece", type=int, default=4, help="changes per piece; a version holds two pieces")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--sample", type=int, default=512, help="versions the one-by-one route runs (at most)")
    ap.add_argument("--versions-scan", default="", help="comma-separated piece sizes to repeat the routes at")
    args = ap.parse_args()
    rows_target = args.versions * 2 * args.piece if args.versions else args.rows

    import numpy as np
    import torch
    import corrosion_amd as ca
    from corrosion_amd import _lib as L
    from corrosion_amd import wire
    from corrosion_amd.agent import Bookie, Change, ChangeV1, Full

    actors = [bytes([k & 255, k >> 8] + [9] * 14) for k in range(args.actors)]
    lib = L.lib()

    def make_agent(piece):
        per_actor = max(1, rows_target // (2 * piece * args.actors))
        agent = ca.agent.Agent({"t": ["c"]}, capacity_hint=max(1 << 16, rows_target), actor_id=b"\xA0" * 16)
        for a in actors:
            agent.site(a)
        last = 2 * piece - 1
        batch, nb, nready = [], 0, 0
        for ai, a in enumerate(actors):
            for v in range(1, per_actor + 1):
                pk0 = (ai * per_actor + v) * (last + 1)
                for s0 in (0, piece):
                    ch = [Change("t", pk0 + s, "c", v * 31 + s, 1, v, s, a, 1) for s in range(s0, s0 + piece)]
                    batch.append(ChangeV1(a, Full(v, ch, (s0, s0 + piece - 1), last, ts=1000 + v)))
                    nb += piece
            if nb >= 200_000 or ai == len(actors) - 1:
                res, status = agent.process_frames(wire.frames(batch))
                assert not np.asarray(status).any() and all(k == "partial" for k in res.known)
                nready += len(res.ready)
                print(f"piece {piece}: buffered actor {ai + 1} of {len(actors)}", file=sys.stderr, flush=True)
                batch, nb = [], 0
        assert nready == per_actor * args.actors
        return agent, nready

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def fresh(agent, image):
        """a bookie loaded from the image, its ready list as the C arrays of the pairs, and an empty state"""
        bk = Bookie()
        bk.load(image, agent.engine)
        pairs = bk.take_ready()
        ids = np.frombuffer(b"".join(a for a, _v in pairs), np.uint8).copy()
        ver = np.array([v for _a, v in pairs], np.uint64)
        agent.engine.reset()
        return bk, pairs, ids, ver

    def batch_route(agent, bk, ids, ver):
        res = np.zeros(len(ver), np.int32)
        L.check(lib.corro_process_fully_buffered_batch(agent.engine._h, bk._h, ids.ctypes.data, ver.ctypes.data, len(ver),
                                                       res.ctypes.data))
        return res

    def one_by_one(agent, bk, sample):
        r, hits = C.c_int(), 0
        for a, v in sample:
            L.check(lib.corro_process_fully_buffered(agent.engine._h, bk._h, a, v, C.byref(r)))
            hits += r.value
        return hits

    def measure(piece):
        agent, nversions = make_agent(piece)
        image = agent.save_bookie(device=True)
        rows = {k: image["rows"][k] for k in ("pk", "table_cid", "col_version", "db_version", "cl", "seq", "site", "val0",
                                               "val1", "val_type", "val_len", "ts")}
        nrows = int(image["nrows"])
        stride = max(1, -(-nversions // args.sample))
        t = {}

        def add(name, ms):
            t.setdefault(name, []).append(ms)
        nsample = 0
        for step in range(args.warmup + args.steps):
            rec = step >= args.warmup
            print(f"piece {piece}: round {step + 1} of {args.warmup + args.steps}", file=sys.stderr, flush=True)
            bk, pairs, ids, ver = fresh(agent, image)
            assert len(pairs) == nversions
            ms, res = wall(lambda: batch_route(agent, bk, ids, ver))
            merged = agent.engine.count()
            assert (res == 2).all(), np.unique(res, return_counts=True)
            assert bk.take_ready() == []
            rec and add("batch", ms)
            del bk
            bk, pairs, ids, ver = fresh(agent, image)
            sample = pairs[::stride]
            nsample = len(sample)
            ms, hits = wall(lambda: one_by_one(agent, bk, sample))
            assert hits == nsample
            rec and add("one_by_one", ms)
            del bk
            agent.engine.reset()
            prep = agent.engine.prepare(rows, impact=True)
            ms, imp = wall(lambda: agent.engine.apply_prepared(prep))
            assert agent.engine.count() == merged and bool(imp.any())   # the same cells as the batch route
            rec and add("floor", ms)
        ms = {k: {"min": min(v), "max": max(v)} for k, v in t.items()}
        per = {"min": 1e3 * ms["one_by_one"]["min"] / nsample, "max": 1e3 * ms["one_by_one"]["max"] / nsample}
        agent.engine.close()
        return {"piece": piece, "rows": nrows, "versions": nversions, "segments": 2 * nversions, "ms": ms,
                "one_by_one_sample": nsample, "one_by_one_us_per_version": per,
                "one_by_one_extrapolated_ms": {k: v * nversions / 1e3 for k, v in per.items()},
                "batch_over_floor": ms["batch"]["min"] / ms["floor"]["min"]}

    main_run = measure(args.piece)
    scan = [measure(int(p)) for p in args.versions_scan.split(",") if p]
    line = {"metric": "ready drain in one batch, ms (min)", "value": main_run["ms"]["batch"]["min"], "unit": "ms",
            "higher_is_better": False, "steps": args.steps, "warmup": args.warmup, "data": "synthetic",
            "config": {"rows": rows_target, "actors": args.actors, "piece": args.piece, "sample": args.sample},
            "run": main_run, "versions_scan": scan,
            "note": "one_by_one_extrapolated_ms = the sample's per-version time times the list's versions: not measured"}
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
