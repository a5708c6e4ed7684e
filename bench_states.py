"""Peer state bytes -> need-diff entries: the host path against corro_decode_states on MI355X.

Config 4's shape (BASELINE.json configs[3], synth.sync_entries_torch), scaled by --pairs: every pair is
two SyncStateV1 of --actors-per-pair sparse actors from a 100k-actor universe, heads uniform in
[1, 1e6] (ours lacks 10 % of the actors), Poisson(2) disjoint need ranges per actor and side, 5 % of the
actors with a partial version of 1-3 seq ranges. Each state is one SyncMessageV1::State frame.

Two paths over the same frames, in one process, alternating, each timed with a host clock around work
that ends in a device synchronise:
  host    wire.decode_sync_state per frame -> sync.entries_from_states -> the eighteen arrays copied to
          the device (what a caller without corro_decode_states does); the time of wire.encode_sync_state,
          which only a caller that holds dataclasses pays, is reported beside it
  device  sync.entries_from_state_frames(device=True) on the frames already in HBM: both passes of
          corro_decode_states and the output allocations
The device result is checked against the host path's arrays before anything is timed. Prints one JSON
line per size; --log appends them to a file.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def make_states(npairs, actors, seed, universe=100_000, max_head=1_000_000, need_rate=2.0, need_len=20, partial_frac=0.05):
    import numpy as np
    from corrosion_amd.sync import SyncStateV1
    rng = np.random.default_rng(seed)
    ids = lambda k: int(k).to_bytes(8, "little") + (int(k) * 0x9E3779B97F4A7C15 & 0xFFFFFFFFFFFFFFFF).to_bytes(8, "little")

    def ranges(k):
        pos, out = 0, []
        for g, ln in zip(rng.geometric(1.0 / (max_head // 80 + 2), k), rng.geometric(1.0 / need_len, k)):
            out.append((pos + int(g) + 1, pos + int(g) + int(ln)))
            pos = out[-1][1]
        return out

    def side(me, acts, drop):
        st = SyncStateV1(actor_id=ids(me))
        for a in acts:
            if rng.random() < drop:
                continue
            st.heads[ids(a)] = int(rng.integers(1, max_head + 1))
            k = int(rng.poisson(need_rate))
            if k:
                st.need[ids(a)] = ranges(k)
            if rng.random() < partial_frac:
                lo = [int(x) for x in sorted(rng.integers(0, 1000, 2 * int(rng.integers(1, 4))))]
                st.partial_need[ids(a)] = {int(rng.integers(1, max_head)): [(lo[2 * i], lo[2 * i + 1]) for i in range(len(lo) // 2)]}
        st.last_cleared_ts = int(rng.integers(1, 1 << 62))
        return st

    out = []
    for p in range(npairs):
        acts = rng.choice(universe, actors, replace=False)
        out.append((side(universe + 2 * p, rng.permutation(acts), 0.1), side(universe + 2 * p + 1, rng.permutation(acts), 0.0)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, nargs="+", default=[20, 200, 2000, 10000])
    ap.add_argument("--actors-per-pair", type=int, default=64)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=4)
    ap.add_argument("--log", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import corrosion_amd as ca
    from corrosion_amd import sync as S
    from corrosion_amd import wire as W
    if not torch.cuda.is_available():
        sys.exit("bench_states.py needs a GPU: there is no CPU path to measure")
    dev = torch.device("cuda", 0)
    eng = ca.MergeEngine({"t": ["a"]}, capacity_hint=1024, device=0)

    for npairs in args.pairs:
        states = make_states(npairs, args.actors_per_pair, args.seed + npairs)
        t0 = time.perf_counter()
        frames = [W.frame(W.encode_sync_state(st)) for pr in states for st in pr]
        encode_ms = (time.perf_counter() - t0) * 1e3
        off = np.zeros(len(frames) + 1, np.int64)
        off[1:] = np.cumsum([len(f) for f in frames])
        buf = b"".join(frames)
        pairs = np.arange(2 * npairs, dtype=np.int64).reshape(-1, 2)
        dbuf = torch.from_numpy(np.frombuffer(buf, np.uint8).copy()).to(dev)
        doff, dpairs = torch.from_numpy(off).to(dev), torch.from_numpy(pairs).to(dev)

        def host_path():
            dec = [(W.decode_sync_state(frames[2 * p][4:]), W.decode_sync_state(frames[2 * p + 1][4:])) for p in range(npairs)]
            ent, _index = S.entries_from_states(dec)
            up = {k: torch.from_numpy(v.view(np.int64) if v.dtype == np.uint64 else v).to(dev) for k, v in ent.items()}
            torch.cuda.synchronize()
            return up

        def device_path():
            res = S.entries_from_state_frames(eng, dbuf, doff, dpairs, device=True)
            torch.cuda.synchronize()
            return res

        want, got = host_path(), device_path()
        for k, v in want.items():                     # same entries, array for array, before any timing
            assert torch.equal(got[k], v), k
        assert int(got["frame_status"].abs().sum()) == 0
        hs, ds = [], []
        for i in range(args.warmup + args.steps):     # alternating, in one process
            t0 = time.perf_counter()
            host_path()
            t1 = time.perf_counter()
            device_path()
            t2 = time.perf_counter()
            if i >= args.warmup:
                hs.append((t1 - t0) * 1e3)
                ds.append((t2 - t1) * 1e3)
        med = lambda x: float(np.median(x))
        line = {"metric": "SyncStateV1 frames -> need-diff entries (config 4 shape)", "pairs": npairs,
                "actors_per_pair": args.actors_per_pair, "frames": len(frames), "frame_bytes": len(buf),
                "entries": int(got["their_head"].shape[0]), "steps": args.steps, "warmup": args.warmup,
                "host_ms": med(hs), "host_ms_min_max": [min(hs), max(hs)],
                "host_path": "wire.decode_sync_state + sync.entries_from_states + H2D, one Python thread",
                "encode_ms_once": encode_ms, "host_with_encode_ms": med(hs) + encode_ms,
                "device_ms": med(ds), "device_ms_min_max": [min(ds), max(ds)],
                "device_path": "corro_decode_states pass 0 + pass 1 on frames in HBM, outputs allocated per call",
                "speedup": med(hs) / med(ds), "pairs_per_s_device": npairs / (med(ds) * 1e-3),
                "data": "synthetic, seeded"}
        print(json.dumps(line), flush=True)
        if args.log:
            os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
            with open(args.log, "a") as f:
                f.write(json.dumps(line) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
