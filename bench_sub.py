"""Benchmark of Subscription.update: a device-resident result set advanced by a batch of candidates; prints one
JSON line.

python bench_sub.py [--rows N] [--rounds R] [--warmup W] [--cands K] [--no-baseline]

State: bench_query.py's (two tables of N rows x 4 INTEGER columns, a = pk, b = pk % 1000; default N = 2^22). The
subscription selects a <= N / 16 of t0 and projects pk, a, b. Every round first merges one batch that rewrites
column a of 3/4 of K random rows below N / 8 (default K = 2^16) to a random value below N / 8, so the candidates
split into Inserts, Updates, Deletes and rows that make no event, then times
  update    Subscription.update over the K keys, both passes, keys and events in device memory
  baseline  what the engine offered before: the keyed query_rows over the K keys on the device, its answer
            copied to the host, and tests/sub_model.py's diff against a host copy of the set
on the same state (the baseline first: it does not touch the device set). Both must name the same events. Wall
clock around the synchronous calls; pass 0 and pass 1 of the update are timed apart, and each pass is split into
its stages by the library's own HIP events on the context's stream (corro_ctx_set_profiling;
corro_sub_last_timings): a stage holds its kernels, the waits between them and the host's read of its totals.
--no-baseline leaves the baseline and the comparison out, so that a kernel trace of the run (rocprofv3
--kernel-trace --stats) holds the update's kernels and the per-round apply alone.
"""
import argparse
import json
import time

import numpy as np

from bench_query import state_batch, stats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 22)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cands", type=int, default=1 << 16)
    ap.add_argument("--no-baseline", action="store_true")
    args = ap.parse_args()
    import corrosion_amd as ca
    if ca.device_count() == 0:
        raise SystemExit("bench_sub.py needs a GPU: there is no CPU path to time")
    import torch
    import synth
    from corrosion_amd import updates as U
    from tests import sub_model as S
    n, k, dev = args.rows, args.cands, "cuda:0"
    eng = ca.MergeEngine({"t0": ["a", "b", "c", "d"], "t1": ["a", "b", "c", "d"]}, capacity_hint=8 * n, device=0)
    eng.register_sites(synth.site_ids(1, 1))
    eng.apply(state_batch(n, dev))
    where, cols = [[("a", "<=", n // 16)]], ["pk", "a", "b"]
    sub = U.Subscription(eng, "t0", where, cols, row_cap=n // 8)
    first = sub.rows()
    model = S.SubModel([(int(p), [int(x) for x in c]) for p, c in zip(first["pk"], first["val0"].view(np.int64))])
    gen = torch.Generator(device=dev).manual_seed(7)
    out = {"bench": "sub_update", "rows_per_table": n, "set_rows": first["nrows"], "candidates": k,
           "protocol": f"{args.warmup} warm-up + {args.rounds} timed rounds; wall clock around the synchronous calls"}
    eng.set_profiling(True)
    runs, base, events, stages = [], [], [], []
    for rnd in range(args.warmup + args.rounds):
        keys = torch.randint(1, n // 8, (k,), generator=gen, device=dev, dtype=torch.int64)
        ch = torch.unique(keys[: 3 * k // 4])
        m = int(ch.numel())
        i32 = lambda v: torch.full((m,), v, device=dev, dtype=torch.int32)
        eng.apply({"pk": ch, "table_cid": i32(1), "col_version": torch.full((m,), rnd + 2, device=dev, dtype=torch.int64),
                   "db_version": torch.full((m,), 1 << 20, device=dev, dtype=torch.int64) + rnd, "cl": i32(1), "seq": i32(0),
                   "site": i32(0), "val0": torch.randint(1, n // 8, (m,), generator=gen, device=dev, dtype=torch.int64)})
        torch.cuda.synchronize()
        t0 = t1 = time.perf_counter()
        if not args.no_baseline:
            q = eng.query_rows("t0", where, cols, keys=keys, values=True)
            pk, v0 = q["pk"].cpu().numpy().view(np.uint64), q["val0"].cpu().numpy().view(np.int64)
            want = model.update(keys.cpu().numpy().view(np.uint64).tolist(),
                                {int(p): [int(x) for x in c] for p, c in zip(pk, v0)})
            t1 = time.perf_counter()
        tp, keep = sub.two_pass(keys)
        tp.bind(())
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        tp.call(0)
        t3 = time.perf_counter()
        tot = tp.totals(U._SUB_TOTALS)
        tot["ncells"] = tot["nevents"] * sub.nproj
        tp.bind(U._SUB_EVENTS + U._SUB_CELLS + U._SUB_DATA, tot)
        torch.cuda.synchronize()
        t4 = time.perf_counter()
        tp.call(1)
        t5 = time.perf_counter()
        got = tp.result()
        if args.no_baseline:
            want = None
        else:
            assert got["rowid"].cpu().numpy().view(np.uint64).tolist() == [e[1] for e in want], "the routes disagree"
            assert got["type"].cpu().numpy().tolist() == [S.TYPES.index(e[0]) for e in want], "the routes disagree"
        if rnd >= args.warmup:
            runs.append({"pass0": (t3 - t2) * 1e3, "pass1": (t5 - t4) * 1e3, "update": (t3 - t2 + t5 - t4) * 1e3})
            base.append((t1 - t0) * 1e3)
            events.append({x: tot[x] for x in ("ninsert", "nupdate", "ndelete")})
            stages.append(sub.last_timings())
    out["update_ms"] = stats([r["update"] for r in runs])
    out["pass0_ms"] = stats([r["pass0"] for r in runs])
    out["pass1_ms"] = stats([r["pass1"] for r in runs])
    # the medians of the stage times, and what of each pass's wall time they leave (the call's host work in
    # front of the first mark and behind the last)
    for which in (0, 1):
        med = {k: round(float(np.median([st[which][k] for st in stages])), 3) for k in stages[0][which]}
        out[f"pass{which}_stages_ms"] = med
        out[f"pass{which}_outside_stages_ms"] = round(out[f"pass{which}_ms"]["median_ms"] - sum(med.values()), 3)
    if not args.no_baseline:
        out["baseline_query_d2h_host_diff_ms"] = stats(base)
        out["ratio_baseline_over_update"] = round(out["baseline_query_d2h_host_diff_ms"]["median_ms"] / out["update_ms"]["median_ms"], 1)
    out["events_last_round"] = events[-1]
    print(json.dumps(out))
    sub.close()
    eng.close()


if __name__ == "__main__":
    main()
