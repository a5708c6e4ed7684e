"""Benchmark of corro_read_rows: K rows read by primary key from a populated state; prints one JSON line.

python bench_read.py [--changes N ...] [--rounds R] [--warmup W]

State: bench.py's config 2 (N column changes, 1 table x 4 INTEGER columns, 1000 actors, uniform pks over
N / 16), generated in HBM and merged by one apply. The default runs two state sizes, config 2 itself
(2^26 changes, ~16.5 M cells) and an eighth of it, to tell a cost that follows K from one that follows
the state. Per state K = 2^10, 2^16 and 2^20 random keys are read, 90 % of them present, by three routes:
  device   read_rows with the keys and the result in HBM (CORRO_MEM_DEVICE)
  host     read_rows with numpy keys and a numpy result (CORRO_MEM_HOST: one copy per array)
  export   what the engine offered before: corro_state_export of the whole state, then a numpy filter of
           its rows on (table, pk)
All routes run in one process and alternate inside every round; after --warmup rounds, --rounds timed
ones, reported as min / median / max of the wall time of the whole call (each returns with its stream
idle). Before anything is timed the three routes' rows for the smallest K are compared.
"""
import argparse
import json
import time

import numpy as np

N_ACTORS, N_COLS = 1000, 4
KS = (1 << 10, 1 << 16, 1 << 20)


def keys_for(k, npk, seed):
    """k random keys, 90 % of them inside the pk space [1, npk]"""
    rng = np.random.default_rng(seed)
    pk = rng.integers(1, npk + 1, size=k).astype(np.uint64)
    miss = rng.random(k) < 0.1
    pk[miss] += np.uint64(1 << 40)
    return np.zeros(k, np.uint32), pk


def export_filter(eng, tables, pks):
    """the full export, then its rows whose (table, pk) was asked for"""
    rows = eng.export()
    key = (rows["table_cid"].astype(np.uint64) >> np.uint64(16)) << np.uint64(48) | rows["pk"]   # (pks here lie below 2^48)
    want = tables.astype(np.uint64) << np.uint64(48) | pks
    keep = np.isin(key, want)
    return {k: a[keep] for k, a in rows.items() if k != "long_values"}


def canon(rows):
    cols = ("table_cid", "pk", "col_version", "db_version", "cl", "seq", "site", "val0")
    return sorted(zip(*[np.asarray(rows[c]).tolist() for c in cols]))


def stats(ms):
    return {"min_ms": round(min(ms), 3), "median_ms": round(float(np.median(ms)), 3), "max_ms": round(max(ms), 3)}


def run_state(n, rounds, warmup):
    import torch
    import corrosion_amd as ca
    import synth
    npk = max(n // 16, 1024)
    dev = "cuda:0"
    eng = ca.MergeEngine({"t": ["a", "b", "c", "d"]}, capacity_hint=n, device=0)
    eng.register_sites(synth.site_ids(N_ACTORS, 1))
    eng.apply(synth.uniform_batch_torch(n, N_ACTORS, npk, N_COLS, seed=synth.config_seed(2), device=dev))
    torch.cuda.empty_cache()
    out = {"changes": n, "pk_space": npk, "state_rows": eng.metrics()["state_rows"], "state_cells": eng.count(), "reads": []}
    keys = {k: keys_for(k, npk, 100 + i) for i, k in enumerate(KS)}
    dkeys = {k: (torch.from_numpy(t.view(np.int32)).to(dev), torch.from_numpy(p.view(np.int64)).to(dev))
             for k, (t, p) in keys.items()}
    # the routes agree before they are timed (dedup: the export route answers a repeated key once)
    t0, p0 = keys[KS[0]]
    uniq = np.unique(p0)
    a = canon(eng.read_rows(np.zeros(len(uniq), np.uint32), uniq))
    d = eng.read_rows(torch.zeros(len(uniq), dtype=torch.int32, device=dev), torch.from_numpy(uniq.view(np.int64)).to(dev))
    b = canon({k: v.cpu().numpy().view(ca.engine.ROW_FIELDS[k]) for k, v in d.items() if k in ca.engine.ROW_FIELDS})
    c = canon(export_filter(eng, np.zeros(len(uniq), np.uint32), uniq))
    assert a == b == c and len(a) > 0, "the routes disagree"
    t = {(k, r): [] for k in KS for r in ("device", "host", "export")}
    nrows = {}
    for rnd in range(warmup + rounds):
        for k in KS:
            for route in ("device", "host", "export"):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if route == "device":
                    res = eng.read_rows(*dkeys[k])
                    nrows[k] = res["nrows"]
                elif route == "host":
                    res = eng.read_rows(*keys[k])
                else:
                    res = export_filter(eng, *keys[k])
                dt = (time.perf_counter() - t0) * 1e3
                del res
                if rnd >= warmup:
                    t[(k, route)].append(dt)
    for k in KS:
        out["reads"].append({"keys": k, "rows": nrows[k], **{r: stats(t[(k, r)]) for r in ("device", "host", "export")}})
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--changes", type=int, nargs="+", default=[1 << 26, 1 << 23])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    import corrosion_amd as ca
    if ca.device_count() == 0:
        raise SystemExit("bench_read.py needs a GPU: there is no CPU path to time")
    states = []
    for n in args.changes:
        st = run_state(n, args.rounds, args.warmup)
        states.append(st)
        for r in st["reads"]:
            print(f"state {st['state_cells']:>9} cells  K = {r['keys']:>7} ({r['rows']:>8} rows)  " + "  ".join(
                f"{name} {r[name]['min_ms']:.3f} - {r[name]['max_ms']:.3f} ms (median {r[name]['median_ms']:.3f})"
                for name in ("device", "host", "export")), flush=True)
    print(json.dumps({"bench": "read_rows", "protocol": f"{args.warmup} warm-up + {args.rounds} timed rounds, routes "
                      "alternating in one process, wall ms of the whole call", "states": states}))


if __name__ == "__main__":
    main()
