"""Serving sync requests benchmark: request bytes in, response bytes out.

A populated agent (--actors actors x --versions versions of --changes column changes each, applied
through process_multiple_changes) answers the requests of --peers peers that hold nothing: every peer's
need diff is Full(1 ..= versions) per actor, plan_sync_requests cuts them into the reference's chunks of
10 and encodes one SyncMessageV1::Request frame per chunk, and the frames of all peers, back to back,
are the one request buffer both paths answer.

  device  serve.handle_request_frames: corro_decode_requests (decode + screen + extraction entries),
          corro_extract_changes, corro_need_spans, corro_encode_changesets, corro_need_tails (the
          "tails" stage: the Empty frames that end a need's answer), then the join per frame and the
          host bookie's walk for the needs that touch a buffered version (none here). With
          --assembled: serve.handle_request_frames_assembled, the same stages and then
          corro_assemble_answers (the "assemble" stage: every frame's answer in one device buffer),
          one read-back of that buffer and one slice per frame
          With --path buffered: serve.handle_request_frames_buffered, which adds the "buffered" stage
          (corro_buffered_spans over the bookie's device row pool and a second encoder call) and
          assembles three pieces per need
  host    the path as it stood before: wire.decode_sync_request per frame, process_sync's screen in
          Python (bisect over the bookie's gaps), then serve.handle_needs_frames over the kept needs
          (its per-need Python loops around the same extraction and encoder)

With --buffered FRACTION that share of each actor's top versions arrives as its first half only, as wire
frames through process_frames, so their rows lie in the bookie's device row pool and every peer's
request runs into them. The host walk reads such a version out of the pool for good, so the host path
then answers from a second, identically fed agent, and the device path's first call (for the device
and assembled paths: the call that materialises) is timed apart from the steady state after it.

Both must give the same bytes; the run fails otherwise. Prints one JSON line with both times and the
device path's stage split (taken in a separate step with a device synchronisation after every stage);
no threshold is asserted.
"""
import argparse
import bisect
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--actors", type=int, default=16)
    ap.add_argument("--versions", type=int, default=200)
    ap.add_argument("--changes", type=int, default=4, help="column changes per version")
    ap.add_argument("--peers", type=int, default=8, help="peers asking for everything, one session each")
    ap.add_argument("--chunk", type=int, default=10)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--assembled", action="store_true",
                    help="time serve.handle_request_frames_assembled as the device path")
    ap.add_argument("--path", choices=("device", "assembled", "buffered"), default=None,
                    help="the device path to time (default: device, or assembled with --assembled)")
    ap.add_argument("--buffered", type=float, default=0.0,
                    help="share of each actor's top versions that arrives as one half through process_frames")
    args = ap.parse_args()
    path = args.path or ("assembled" if args.assembled else "device")

    import numpy as np
    import torch
    import corrosion_amd as ca
    from corrosion_amd import serve, wire
    from corrosion_amd import sync as S
    from corrosion_amd.agent import Change, ChangeV1, Full

    cols = [f"c{k}" for k in range(args.changes)]
    actors = [bytes([k & 255, k >> 8] + [7] * 14) for k in range(args.actors)]
    nbuf = int(round(args.versions * args.buffered))           # top versions per actor that arrive in part
    half = max(1, args.changes // 2)
    if nbuf and args.changes < 2:
        raise SystemExit("--buffered needs --changes >= 2: a version of one change has no half")

    def make_agent():
        agent = ca.agent.Agent({"t": cols}, capacity_hint=1 << 20, actor_id=b"\xA0" * 16)
        for a in actors:
            agent.site(a)
        partial = []
        for ai, a in enumerate(actors):
            msgs = []
            for v in range(1, args.versions + 1):
                pk = 1000 + ai * args.versions + v
                ch = [Change("t", pk, c, v * 31 + k, 1, v, k, a, 1) for k, c in enumerate(cols)]
                if v > args.versions - nbuf:
                    partial.append(ChangeV1(a, Full(v, ch[:half], (0, half - 1), args.changes - 1, ts=1000 + v)))
                else:
                    msgs.append(ChangeV1(a, Full(v, ch, (0, args.changes - 1), args.changes - 1, ts=1000 + v)))
            res = agent.process_multiple_changes(msgs)
            assert all(k == "current" for k in res.known)
        if partial:
            res, status = agent.process_frames(wire.frames(partial))
            assert not np.asarray(status).any() and all(k == "partial" for k in res.known)
        return agent

    agent = make_agent()
    ref_agent = make_agent() if nbuf else agent                # the host walk materialises: it gets its own agent
    needs = {a: [S.Full(1, args.versions)] for a in actors}
    planned = S.plan_sync_requests(agent.engine, [[needs] for _ in range(args.peers)], chunk=args.chunk)
    frames = [f for session in planned for server in session for _round, f in server]
    buf = b"".join(frames)
    off = np.zeros(len(frames) + 1, np.uint64)
    off[1:] = np.cumsum([len(f) for f in frames])
    dev = torch.device("cuda", agent.engine.device)
    dbuf = torch.from_numpy(np.frombuffer(buf, np.uint8).copy()).to(dev)
    doff = torch.from_numpy(off.view(np.int64)).to(dev)

    def device_path(timings=None):
        serve_frames = {"device": serve.handle_request_frames, "assembled": serve.handle_request_frames_assembled,
                        "buffered": serve.handle_request_frames_buffered}[path]
        return serve_frames(agent, dbuf, doff, timings=timings)[1]

    def host_path():
        agent = ref_agent
        sites = {a: i for i, a in enumerate(agent.engine.site_ids())}
        book, kept, owner = {}, [], []
        for f in range(len(frames)):
            for actor, nds in wire.decode_sync_request(buf[int(off[f]) + 4:int(off[f + 1])]):
                if actor not in sites:
                    continue
                if actor not in book:
                    gaps = agent.bookie.needed(actor)
                    book[actor] = ([s for s, _ in gaps], [e for _, e in gaps], agent.bookie.last(actor))
                gs, ge, mx = book[actor]
                if mx is None and not gs:
                    continue
                for nd in nds:
                    s, e = (nd.start, nd.end) if isinstance(nd, S.Full) else (nd.version, nd.version)
                    if s > e or (mx is not None and s > mx):
                        continue
                    hi = e if mx is None else min(e, mx)
                    k = bisect.bisect_right(gs, s)
                    if k and ge[k - 1] >= hi:
                        continue
                    kept.append((actor, nd))
                    owner.append(f)
        out = [[] for _ in frames]
        for f, b in zip(owner, serve.handle_needs_frames(agent, kept)):
            out[f].append(b)
        return [b"".join(p) for p in out]

    def timed(fn):
        for _ in range(args.warmup):
            out = fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps, out

    first_s = None
    if nbuf:                                                   # the first call on pool rows, apart from the steady state
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        device_path()
        torch.cuda.synchronize()
        first_s = time.perf_counter() - t0
    dev_s, got = timed(device_path)
    host_s, want = timed(host_path)
    if got != want:
        raise SystemExit("the device path and the host path answered differently")
    split = {}
    device_path(split)
    line = {"metric": "serving sync requests: request bytes to response bytes, ms", "value": dev_s * 1e3, "unit": "ms",
            "higher_is_better": False, "steps": args.steps, "warmup": args.warmup, "data": "synthetic",
            "config": {"actors": args.actors, "versions": args.versions, "changes_per_version": args.changes,
                       "peers": args.peers, "chunk": args.chunk, "assembled": path == "assembled", "path": path,
                       "buffered_versions_per_actor": nbuf,
                       "request_frames": len(frames), "request_bytes": len(buf),
                       "response_bytes": sum(len(b) for b in got)},
            "device_path_ms": dev_s * 1e3, "host_path_ms": host_s * 1e3, "host_over_device": host_s / dev_s,
            "device_stage_ms": {k: v * 1e3 for k, v in split.items()}}
    if first_s is not None:
        line["first_call_ms"] = first_s * 1e3
        on_dev = serve.buffered_index(agent)["on_device"]
        line["pool_versions_left"] = int(on_dev.sum())         # buffered versions still in the device row pool
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
