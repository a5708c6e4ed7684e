"""Wire-encode benchmark: the send half of sync on MI355X. A synthetic state (config-2
distribution: one table of 4 INTEGER columns, 1000 actors) is answered with one Full need per actor:
device extraction (corro_extract_changes, CORRO_MEM_DEVICE) -> spans gathered on the device ->
corro_encode_changesets (CORRO_MEM_DEVICE). Nothing but sizes leaves the GPU.

Reported: (a) extract + encode ms for the whole state, and the encode alone with its output GB/s;
(b) the same needs through the host object path (wire.frames over serve.handle_needs) on a subsample
of actors, scaled per row; (c) corro_decode_frames' device kernels over the same bytes (bench_wire.py's
measure), for encode vs decode throughput. Times are wall clock around synchronous calls, median of
--steps after --warmup. Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 22)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--max-buf-size", type=int, default=8192)
    ap.add_argument("--host-actors", type=int, default=2, help="actors answered through the host object path")
    ap.add_argument("--no-decode", action="store_true", help="skip the decode of the encoded bytes")
    args = ap.parse_args()
    import numpy as np
    import torch
    import corrosion_amd as ca
    import synth
    from corrosion_amd import serve, wire
    from corrosion_amd.sync import Full as NFull

    nsites = 1000
    sites = synth.site_ids(nsites, 1)
    b = synth.uniform_batch(args.rows, nsites, 1 << 22, 4, synth.config_seed(2))
    agent = ca.agent.Agent({"t": ["a", "b", "c", "d"]}, capacity_hint=args.rows)
    eng = agent.engine
    eng.register_sites(sites)
    eng.apply(b)
    state_rows = eng.count()
    dev = torch.device("cuda", 0)

    def up(a, dt):
        a = np.asarray(a, dt)
        return torch.from_numpy(a.view(np.int64 if a.itemsize == 8 else np.int32)).to(dev)

    nd = {"site": up(np.arange(nsites), np.uint32), "start": up(np.zeros(nsites), np.uint64),
          "end": up(np.full(nsites, 1 << 62), np.uint64)}

    def extract():
        res = eng.extract_changes(nd)
        per = (res["grp_off"][1:] - res["grp_off"][:-1])
        spans = {"site": torch.repeat_interleave(nd["site"], per), "version": res["version"], "last_seq": res["last_seq"],
                 "ts": res["ts"], "seq_start": torch.zeros_like(res["last_seq"]), "seq_end": res["last_seq"],
                 "row_off": res["grp_row_off"], "row_count": res["grp_rows"]}
        return spans, res["rows"]

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    both, enc_only, ext_only = [], [], []
    for i in range(args.warmup + args.steps):
        t_ext, (spans, rows) = timed(extract)
        t_enc, enc = timed(lambda: eng.encode_changesets(spans, rows, args.max_buf_size))
        if i >= args.warmup:
            ext_only.append(t_ext)
            enc_only.append(t_enc)
            both.append(t_ext + t_enc)
    nrows, nbytes, nframes = int(rows["pk"].shape[0]), enc["nbytes"], enc["nframes"]
    enc_ms = statistics.median(enc_only)

    # (b) the host object path on a few actors, scaled per row
    needs = [(bytes(sites[i]), NFull(0, 1 << 62)) for i in range(args.host_actors)]
    t0 = time.perf_counter()
    msgs = serve.handle_needs(agent, needs, args.max_buf_size)
    host_bytes = [wire.frames(m) for m in msgs]
    host_s = time.perf_counter() - t0
    host_rows = sum(len(m.changeset.changes) for out in msgs for m in out if hasattr(m.changeset, "changes"))
    # the device frames of those actors are the same bytes (spans are in need order: actor 0 first)
    fo, sfo = enc["frame_off"].cpu().numpy(), enc["span_frame_off"].cpu().numpy()
    go = eng.extract_changes({k: v[:args.host_actors] for k, v in nd.items()})["grp_off"].cpu().numpy()
    dev_head = enc["buf"][:int(fo[int(sfo[int(go[-1])])])].cpu().numpy().tobytes()
    full_only = b"".join(wire.frames([m for m in out if hasattr(m.changeset, "changes")]) for out in msgs)
    same = dev_head == full_only

    # (c) decode of the same bytes (device kernels, as bench_wire.py times them)
    dec_ms = None
    if not args.no_decode and nbytes < (1 << 32):
        buf = enc["buf"].cpu().numpy().tobytes()
        eng.set_profiling(True)
        ts = []
        for i in range(2 + 3):
            dec = eng.decode_frames(buf)
            if i >= 2:
                ts.append(eng.last_timings(apply_only=False)["k_needs_fill"])
        assert (dec["status"] == 0).all() and len(dec["changes"]["pk"]) == nrows
        dec_ms = statistics.median(ts)

    host_ms_scaled = host_s * 1e3 / max(host_rows, 1) * nrows
    line = {"metric": "wire encode: extract + encode of a state answered with Full needs", "unit": "ms",
            "value": statistics.median(both), "higher_is_better": False, "n_gpus": 1, "steps": args.steps,
            "warmup": args.warmup, "rows": nrows, "state_rows": state_rows, "spans": int(spans["site"].shape[0]),
            "frames": nframes, "bytes_out": nbytes, "max_buf_size": args.max_buf_size,
            "extract_ms": statistics.median(ext_only), "encode_ms": enc_ms,
            "encode_ms_min_max": [min(enc_only), max(enc_only)],
            "encode_GBps_out": nbytes / (enc_ms * 1e-3) / 1e9,
            "host_path": {"rows": host_rows, "seconds": host_s, "bytes": sum(map(len, host_bytes)),
                          "ms_scaled_to_all_rows": host_ms_scaled, "bytes_equal_device_frames": same,
                          "speedup_vs_extract_plus_encode": host_ms_scaled / statistics.median(both)},
            "decode_kernels_ms": dec_ms, "decode_GBps_in": (nbytes / (dec_ms * 1e-3) / 1e9) if dec_ms else None}
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
