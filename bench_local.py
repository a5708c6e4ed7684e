"""A local write on the device: corro_local_write (MergeEngine.local_write) of one transaction of N upserts x 4
columns, half the rows new and half live, with device arrays, next to the floor under it.

For each N (2^10, 2^14, 2^18 by default; --ops overrides) and each round: the state is reset and seeded with the
live half (one local write of N/2 inserts, not timed), then

  local_write  one corro_local_write of the N upserts (every listed value differs from the stored one, so the
               transaction leaves 4 N changes), device tensors in, device tensors out
  floor        on a state reset and seeded the same way, one plain corro_apply_batch of the rows that call
               returned (rows_as_batch): what the write costs when nothing is planned, compared or booked

Every entry point synchronises its stream before it returns, so the figures are wall-clock times around the
calls. After --warmup rounds, --steps rounds alternate the two routes in one process. Prints one JSON line: min /
max ms per route and N, and the ratio of the minima. No threshold is asserted.

The stage split comes from one more call per N after the timed rounds, with CORRO_AGENT_PROFILE set: the library
then drains the stream at every stage mark and prints the host time between marks on stderr, which is read back
here ("stages", ms: stage = scratch and uploads, validate, convert = affinity, sort, plan_scan = the plan kernel
and the two scans, fill = rows and long bytes, book, apply = corro_apply_batch, finish = handles and downloads).
The drains make that call slower than a timed one; its sum is reported beside it."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ops", default="1024,16384,262144")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()

    import numpy as np
    import torch
    import corrosion_amd as ca
    from corrosion_amd import _lib as L
    from corrosion_amd.engine import rows_as_batch

    actor = b"\xA0" * 16

    def ops_of(kind, pks, ncol, base):
        n = len(pks)
        o = {"kind": np.full(n, kind, np.uint8), "table": np.zeros(n, np.uint32), "pk": pks.astype(np.uint64),
             "cell_off": (np.arange(n + 1) * ncol).astype(np.uint64), "cid": np.tile(np.arange(1, ncol + 1), n).astype(np.uint32),
             "val0": (np.arange(n * ncol) + base).astype(np.uint64), "val1": np.zeros(n * ncol, np.uint64),
             "val_type": np.ones(n * ncol, np.uint8), "val_len": np.zeros(n * ncol, np.uint8)}
        sgn = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}
        return {k: torch.from_numpy(a.view(sgn.get(a.dtype, a.dtype))).cuda() for k, a in o.items()}

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def profiled(fn):
        """fn() with the library's stage marks on: the marks of its corro_local_write line, ms by name."""
        sys.stderr.flush()
        with tempfile.TemporaryFile() as f:
            keep = os.dup(2)
            os.dup2(f.fileno(), 2)
            os.environ["CORRO_AGENT_PROFILE"] = "1"
            try:
                fn()
            finally:
                del os.environ["CORRO_AGENT_PROFILE"]
                os.dup2(keep, 2)
                os.close(keep)
            f.seek(0)
            lines = [ln for ln in f.read().decode().splitlines() if ln.startswith("corro_local_write:")]
        return {k: float(v) for k, v in (kv.split("=") for kv in lines[-1].split()[1:]) if "." in v}

    runs = []
    for n in [int(x) for x in args.ops.split(",") if x]:
        agent = ca.agent.Agent({"t": ["a", "b", "c", "d"]}, capacity_hint=max(1 << 16, 8 * n), actor_id=actor)
        site = agent.site(actor)
        eng = agent.engine
        seed = ops_of(L.CORRO_OP_INSERT, np.arange(n // 2), 4, 0)
        tx = ops_of(L.CORRO_OP_UPSERT, np.arange(n), 4, 1 << 32)

        def fresh():
            eng.reset()
            res = eng.local_write(seed, 1, site)
            assert res["nrows"] == 4 * (n // 2)

        t = {"local_write": [], "floor": []}
        for step in range(args.warmup + args.steps):
            rec = step >= args.warmup
            fresh()
            ms, res = wall(lambda: eng.local_write(tx, 2, site))
            assert res["nrows"] == 4 * n and res["last_seq"] == 4 * n - 1
            count = eng.count()
            rec and t["local_write"].append(ms)
            batch = rows_as_batch(res)
            fresh()
            prep = eng.prepare(batch)
            ms, _ = wall(lambda: eng.apply_prepared(prep))
            assert eng.count() == count
            rec and t["floor"].append(ms)
        ms = {k: {"min": min(v), "max": max(v)} for k, v in t.items()}
        fresh()
        stages = profiled(lambda: eng.local_write(tx, 2, site))
        runs.append({"ops": n, "changes": 4 * n, "ms": ms, "local_over_floor": ms["local_write"]["min"] / ms["floor"]["min"],
                     "stages": stages, "stages_sum": sum(stages.values())})
        print(f"ops {n}: {ms}", file=sys.stderr, flush=True)
        eng.close()
    big = runs[-1]
    print(json.dumps({"metric": "local write of %d upserts x 4 columns, ms (min)" % big["ops"],
                      "value": big["ms"]["local_write"]["min"], "unit": "ms", "higher_is_better": False,
                      "steps": args.steps, "warmup": args.warmup, "data": "synthetic", "runs": runs,
                      "note": "stages: one extra call per N with a stream drain at every mark"}), flush=True)


if __name__ == "__main__":
    main()
