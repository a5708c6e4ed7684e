"""Sync request planning benchmark: corro_plan_requests over the need diff's own output, in HBM.

A config-4-shaped run (BASELINE.json configs[3]: node-pair sync states, 64 sparse actors per pair,
generated in HBM by synth.sync_entries_torch; by default 20,000 pairs with heads up to 1000, the slice
of sessions that one call plans comfortably, see --pairs and --max-head): corro_compute_needs_onepass diffs every (pair, actor)
entry, and its device-resident result goes straight into corro_plan_requests. A pair is one server
(a group of 64 entries); four consecutive pairs are one session, and actor slot k of every pair is the
same actor, so the servers of a session compete for the same versions as peers of one node do.
One step = pass 0 + pass 1 (plan + encode, output buffers allocated in between). The need diff is
timed on the same input in the same run. Algorithmic bytes: 16 B per need range in (Full ranges and
Partial seq ranges) + the frame bytes out. Prints one JSON line; no threshold is asserted.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=20_000,
                    help="node pairs (servers). One call holds every level of the plan in HBM (about 100 B per "
                         "chunk, 110 B per range, 16 B per segment) beside the frames, so config 4's 1M pairs do "
                         "not fit one call on one card: the caller slices sessions over calls. 20,000 pairs "
                         "(1.28 M entries, ~21 M frames) is the recorded size")
    ap.add_argument("--actors-per-pair", type=int, default=64)
    ap.add_argument("--servers", type=int, default=4)
    ap.add_argument("--max-head", type=int, default=1000,
                    help="heads are uniform in [1, max_head]; config 4's own 1M gives ~10^4 chunks per entry, "
                         "past the 2^32 - 1 items of one call at any useful number of pairs")
    ap.add_argument("--chunk", type=int, default=10)
    ap.add_argument("--drain", type=int, default=10)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()

    import numpy as np
    import torch
    import synth
    import corrosion_amd as ca
    from corrosion_amd.sync import _needs_device_1pass, plan_requests_device

    dev = torch.device("cuda", 0)
    eng = ca.MergeEngine({"t": ["a"]}, capacity_hint=1024)
    A = args.actors_per_pair
    ords = eng.register_sites(np.array([[k & 255, k >> 8] + [7] * 14 for k in range(A)], np.uint8))
    ent = synth.sync_entries_torch(args.pairs, A, synth.config_seed(4), device=dev, max_head=args.max_head)
    E = int(ent["their_head"].shape[0])
    pairs = E // A
    site = torch.from_numpy(ords.astype(np.int32)).to(dev).repeat(pairs)
    geo = torch.arange(pairs + 1, dtype=torch.int64, device=dev) * A
    ses = torch.arange(pairs, dtype=torch.int64, device=dev) // args.servers
    torch.cuda.synchronize()

    def timed(fn):
        for _ in range(args.warmup):
            out = fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps, out

    diff_s, needs = timed(lambda: _needs_device_1pass(eng, ent))
    plan_s, res = timed(lambda: plan_requests_device(eng, needs, site, geo, ses, args.chunk, args.drain))
    n_needs, n_seqs = int(needs["start"].shape[0]), int(needs["s_start"].shape[0])
    n_full = n_needs - int(needs["kind"].to(torch.int64).sum())
    alg = 16 * (n_full + n_seqs) + res["nbytes"]
    line = {"metric": "sync request planning: plan + encode ms (config-4 shape)", "value": plan_s * 1e3, "unit": "ms",
            "higher_is_better": False, "steps": args.steps, "warmup": args.warmup, "data": "synthetic (HBM)",
            "config": {"pairs": pairs, "entries": E, "servers_per_session": args.servers, "chunk": args.chunk,
                       "drain": args.drain, "max_head": args.max_head, "needs_in": n_needs, "full_ranges_in": n_full, "seq_ranges_in": n_seqs},
            "plan_encode_ms": plan_s * 1e3, "need_diff_onepass_ms": diff_s * 1e3,
            "frames": res["nframes"], "bytes_out": res["nbytes"], "alg_bytes": alg,
            "alg_gbs": alg / plan_s / 1e9}
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
