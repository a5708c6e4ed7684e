"""Value-arena compaction against the re-seed it replaces.

Two engines get the same state: `cells` cells, each overwritten `rounds` times with a fresh long
value of `size` bytes at rising col_version, so the arena holds rounds x the live bytes. On one,
compact_values() is timed; on the other the re-seed: export (rows and long values to the host),
reset, re-apply of the exported rows. Both calls end in a device synchronise, so the host clock
around them measures the work. The pair is repeated on freshly built states (the two sides
alternate), after a warm-up pair on a small state. Prints one JSON line.

python tools/bench_values_compact.py [--cells 100000] [--rounds 8] [--size 512] [--reps 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import corrosion_amd as ca  # noqa: E402
import synth  # noqa: E402

SCHEMA = {"t": ["a", "b", "c", "d"]}


def overwrite_batch(cells, size, cv, rng):
    """every cell (pk, cid 1) <- a fresh long BLOB of `size` bytes at col_version cv"""
    n = cells
    data = rng.integers(0, 256, n * size, dtype=np.uint8)
    off = np.arange(n, dtype=np.uint64) * np.uint64(size)
    head = data.reshape(n, size)[:, :8].astype(np.uint64)
    val0 = np.zeros(n, np.uint64)
    for k in range(8):
        val0 = (val0 << np.uint64(8)) | head[:, k]
    return {"pk": np.arange(1, n + 1, dtype=np.uint64), "table_cid": np.ones(n, np.uint32),
            "col_version": np.full(n, cv, np.int64), "db_version": np.full(n, cv, np.int64),
            "cl": np.ones(n, np.uint32), "seq": np.arange(n, dtype=np.uint32), "site": np.zeros(n, np.uint32),
            "val0": val0, "val1": np.zeros(n, np.uint64), "val_type": np.full(n, 4, np.uint8),
            "val_len": np.full(n, 255, np.uint8), "ts": np.full(n, cv, np.uint64), "val_off": off,
            "val_size": np.full(n, size, np.uint32), "val_data": data}


def build_pair(cells, rounds, size, seed):
    sites = synth.site_ids(2, 1)
    pair = []
    for _ in range(2):
        e = ca.MergeEngine(SCHEMA, capacity_hint=max(1 << 16, cells))
        e.register_sites(sites)
        pair.append(e)
    rng = np.random.default_rng(seed)
    for k in range(rounds):
        b = overwrite_batch(cells, size, k + 1, rng)
        for e in pair:
            e.apply(b)
    return pair


def reseed(e):
    """export + reset + re-apply of the exported rows; returns the three times and the bytes re-applied"""
    t0 = time.perf_counter()
    rows = e.export()
    t1 = time.perf_counter()
    n = len(rows["pk"])
    longs = rows["long_values"]
    size = np.zeros(n, np.uint32)
    for i, v in longs.items():
        size[i] = len(v)
    off = np.zeros(n, np.uint64)
    off[1:] = np.cumsum(size, dtype=np.uint64)[:-1]
    batch = {k: rows[k] for k in ("pk", "table_cid", "col_version", "db_version", "seq", "site", "val0", "val1",
                                  "val_type", "val_len", "ts")}
    batch["cl"] = rows["cl"].astype(np.uint32)
    batch["val_off"], batch["val_size"] = off, size
    batch["val_data"] = np.frombuffer(b"".join(longs[i] for i in sorted(longs)) or b"\0", np.uint8)
    t2 = time.perf_counter()
    e.reset()
    e.apply(batch)
    t3 = time.perf_counter()
    return {"export_s": t1 - t0, "host_rebuild_s": t2 - t1, "reset_apply_s": t3 - t2, "total_s": t3 - t0,
            "value_bytes": int(size.sum())}


def one_pair(cells, rounds, size, seed, compact_first):
    a, b = build_pair(cells, rounds, size, seed)
    out = {}
    for side in (("compact", "reseed") if compact_first else ("reseed", "compact")):
        if side == "compact":
            t0 = time.perf_counter()
            r = a.compact_values()
            out["compact"] = dict(r, seconds=time.perf_counter() - t0, state_records=a.count())
            t0 = time.perf_counter()
            a.compact_values()                      # (an already compact arena: the same passes and copy)
            out["compact"]["again_seconds"] = time.perf_counter() - t0
        else:
            out["reseed"] = reseed(b)
    # both sides end with the same live bytes in an arena of the same size
    assert a.metrics()["arena_bytes"] == b.metrics()["arena_bytes"], (a.metrics(), b.metrics())
    assert a.count() == b.count()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=100000)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    if ca.device_count() == 0:
        raise SystemExit("no GPU visible: nothing to measure")
    one_pair(2000, 2, 64, 1, True)                  # warm-up: code objects, the sort's and scans' first use
    reps = [one_pair(args.cells, args.rounds, args.size, 10 + k, k % 2 == 0) for k in range(args.reps)]
    cs = sorted(r["compact"]["seconds"] for r in reps)
    rs = sorted(r["reseed"]["total_s"] for r in reps)
    print(json.dumps({"bench": "values_compact", "cells": args.cells, "rounds": args.rounds, "size": args.size,
                      "compact_median_s": cs[len(cs) // 2], "reseed_median_s": rs[len(rs) // 2],
                      "bytes_moved": reps[0]["compact"]["live_bytes"], "arena_before": reps[0]["compact"]["arena_before"],
                      "reps": reps}))


if __name__ == "__main__":
    main()
