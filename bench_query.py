"""Benchmark of corro_query_rows: a table's live rows selected by a two-term predicate; prints one JSON line.

python bench_query.py [--rows N] [--rounds R] [--warmup W] [--baseline-rounds B]

State: two tables of N rows x 4 INTEGER columns in one store (default N = 2^22; the second table makes the
queried one half of the store's rows), generated in HBM and merged by one apply: a = pk, b = pk % 1000.
Queries, all with device memory (CORRO_MEM_DEVICE), projecting pk, a and b:
  table    WHERE a <= sel * N AND b >= 0 at selectivities 0.1 %, 10 % and 100 %
  keyed    the same predicate at 50 % over 2^18 random keys (an eighth of them absent)
Baselines, what the engine offered before the call existed, --baseline-rounds rounds each after one untimed:
  export   corro_state_export of the whole state, then the numpy filter and sort on the host (table form)
  read     read_rows of the keys on the device, then the filter on the host (keyed form)
Each pass is timed twice over: by the library's own HIP events on the context's stream, recorded around the
pass's device work from its first launch to its last copy (corro_ctx_set_profiling; corro_last_timings [6] /
[7]), and by the wall clock around the whole synchronous call, which adds the ctypes call, the scratch layout
and the final wait. After --warmup rounds, --rounds timed ones, min / median / max. Before anything is timed
the routes' answers for the 0.1 % query are compared. The sweep's algorithmic bytes -- slots x 32 B +
candidate Recs read x 64 B + 12 B per selected row -- over the pass-0 event time (one sweep and the readback
of its count) are reported against the measured HBM copy rate.
"""
import argparse
import ctypes as C
import json
import time

import numpy as np

HBM_MEASURED = 6.29e12   # B/s, a float4 copy on this part
NKEYS = 1 << 18
SELS = (0.001, 0.1, 1.0)


def state_batch(n, device):
    """two tables x n rows x 4 columns: a = pk, b = pk % 1000, c = -pk, d = 7"""
    import torch
    i = torch.arange(8 * n, device=device, dtype=torch.int64)
    t, r = i // (4 * n), i % (4 * n)
    pk, cid = r // 4 + 1, r % 4 + 1
    val = torch.where(cid == 1, pk, torch.where(cid == 2, pk % 1000, torch.where(cid == 3, -pk, torch.full_like(pk, 7))))
    return {"pk": pk.contiguous(), "table_cid": ((t << 16) | cid).to(torch.int32).contiguous(),
            "col_version": torch.ones_like(i), "db_version": (i // 64 + 1).contiguous(),
            "cl": torch.ones(8 * n, device=device, dtype=torch.int32), "seq": (i % 64).to(torch.int32).contiguous(),
            "site": torch.zeros(8 * n, device=device, dtype=torch.int32), "val0": val.contiguous()}


def store_slots(capacity_hint, rows):
    """B << log2S of a store created with capacity_hint after one apply left `rows` rows spread evenly over
    its regions, by the sizing rules of engine.hip: B = the least power of two >= hint / 1280 (at most 2^15);
    the regions start at the least S >= 16 with B * S >= 2 * max(1024, hint / 16); a region doubles while the
    fill asked of it passes 7/8 of S; after the apply, a store more than 5/8 full grows until at most half
    full. (A skewed region would double once more; with hundreds of rows per region, as here, none does.)"""
    lg_b = 0
    while (1 << lg_b) < max(1, capacity_hint // 1280) and lg_b < 15:
        lg_b += 1
    b, lg = 1 << lg_b, 4
    while (b << lg) < 2 * max(1024, capacity_hint // 16) and lg < 20:
        lg += 1
    while rows / b > (7 << lg) / 8:
        lg += 1
    if rows * 8 > (b << lg) * 5:
        while (b << lg) / 2 < rows:
            lg += 1
    return b << lg


def stats(ms):
    return {"min_ms": round(min(ms), 3), "median_ms": round(float(np.median(ms)), 3), "max_ms": round(max(ms), 3)}


def timed_query(eng, where, keys=None):
    """both passes of the device query, timed apart: ({"wall0", "wall1", "event0", "event1"} in ms, nrows, result)"""
    import torch
    from corrosion_amd import _lib as L, engine as E
    from corrosion_amd._twopass import TwoPass
    s, keep, mem, nkeys, nproj = eng.query_prepare("t0", where, ["pk", "a", "b"], keys=keys, values=False, device=True)
    tp = TwoPass(L.lib().corro_query_rows, (eng._h, C.byref(s), mem.const), mem, L.QueryOut())
    tp.bind((("key_status", np.uint8, nkeys),) if keys is not None else ())
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tp.call(0)
    t1 = time.perf_counter()
    tot = tp.totals(("nrows", "val_data_len"))
    tot["ncells"] = tot["nrows"] * nproj
    tp.bind(E._QUERY_ROWS + E._QUERY_CELLS + ((("key_index", np.uint32, "nrows"),) if keys is not None else ()), tot)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    tp.call(1)
    t3 = time.perf_counter()
    del keep
    ev = eng.last_timings(apply_only=False)
    ms = {"wall0": (t1 - t0) * 1e3, "wall1": (t3 - t2) * 1e3, "event0": ev["k_needs_count"], "event1": ev["k_needs_fill"]}
    return ms, tot["nrows"], tp.result()


def export_filter(eng, limit):
    rows = eng.export()
    tc = rows["table_cid"]
    a = rows["pk"][(tc == 1) & (rows["val0"].view(np.int64) <= limit)]          # table 0, cid 1: a <= limit
    b = rows["pk"][(tc == 2) & (rows["val0"].view(np.int64) >= 0)]
    return np.sort(np.intersect1d(a, b))


def read_filter(eng, tables, keys, limit):
    res = eng.read_rows(tables, keys, values=False)
    tc, pk, v = res["table_cid"].cpu().numpy(), res["pk"].cpu().numpy(), res["val0"].cpu().numpy()
    ok_a = set(pk[(tc == 1) & (v <= limit)].tolist())
    ok_b = set(pk[(tc == 2) & (v >= 0)].tolist())
    return [k for k in keys.cpu().numpy().tolist() if k in ok_a and k in ok_b]


def summary(runs):
    return {k: stats([r[k] for r in runs]) for k in ("event0", "event1", "wall0", "wall1")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 22)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--baseline-rounds", type=int, default=3)
    args = ap.parse_args()
    import corrosion_amd as ca
    if ca.device_count() == 0:
        raise SystemExit("bench_query.py needs a GPU: there is no CPU path to time")
    import torch
    import synth
    n, dev = args.rows, "cuda:0"
    eng = ca.MergeEngine({"t0": ["a", "b", "c", "d"], "t1": ["a", "b", "c", "d"]}, capacity_hint=8 * n, device=0)
    eng.register_sites(synth.site_ids(1, 1))
    eng.apply(state_batch(n, dev))
    torch.cuda.empty_cache()
    eng.set_profiling(True)
    m = eng.metrics()
    assert m["state_rows"] == 2 * n and eng.count() == 8 * n
    slots = store_slots(8 * n, 2 * n)
    where = {sel: [[("a", "<=", int(sel * n)), ("b", ">=", 0)]] for sel in SELS}
    rng = np.random.default_rng(5)
    hkeys = rng.integers(1, n + n // 7, size=NKEYS).astype(np.int64)
    dkeys = torch.from_numpy(hkeys).to(dev)
    dtables = torch.zeros(NKEYS, dtype=torch.int32, device=dev)
    kwhere = [[("a", "<=", n // 2), ("b", ">=", 0)]]
    # the routes agree before they are timed
    got = timed_query(eng, where[SELS[0]])[2]["pk"].cpu().numpy().tolist()
    assert got == export_filter(eng, int(SELS[0] * n)).tolist() == list(range(1, int(SELS[0] * n) + 1)), "the table routes disagree"
    kres = timed_query(eng, kwhere, dkeys)[2]
    assert kres["pk"].cpu().numpy().tolist() == read_filter(eng, dtables, dkeys, n // 2), "the keyed routes disagree"
    out = {"bench": "query_rows", "rows_per_table": n, "state_rows": m["state_rows"], "state_records": m["state_records"],
           "region_growths": m["region_growths"], "store_slots_by_the_sizing_rules": slots,
           "protocol": f"{args.warmup} warm-up + {args.rounds} timed rounds, device memory; event = HIP events on the "
                       "context's stream around the pass, wall = the whole synchronous call",
           "table": [], "keyed": None}
    runs, rows = {sel: [] for sel in SELS}, {}
    kruns, krows = [], 0
    for rnd in range(args.warmup + args.rounds):
        for sel in SELS:
            ms, rows[sel], _r = timed_query(eng, where[sel])
            if rnd >= args.warmup:
                runs[sel].append(ms)
        ms, krows, _r = timed_query(eng, kwhere, dkeys)
        if rnd >= args.warmup:
            kruns.append(ms)
    for sel in SELS:
        r = {"selectivity": sel, "rows": rows[sel], **summary(runs[sel])}
        # a candidate (every row of the table) reads a's Rec, and b's only when a passed (early exit)
        r["sweep_bytes"] = slots * 32 + (n + rows[sel]) * 64 + rows[sel] * 12
        sec = r["event0"]["median_ms"] / 1e3
        r["sweep_GBps"] = round(r["sweep_bytes"] / sec / 1e9, 1)
        r["share_of_measured_hbm"] = round(r["sweep_bytes"] / sec / HBM_MEASURED, 3)
        out["table"].append(r)
    out["keyed"] = {"keys": NKEYS, "rows": krows, **summary(kruns)}
    base_e, base_r = [], []
    for rnd in range(1 + args.baseline_rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        export_filter(eng, int(0.1 * n))
        t1 = time.perf_counter()
        read_filter(eng, dtables, dkeys, n // 2)
        t2 = time.perf_counter()
        if rnd:
            base_e.append((t1 - t0) * 1e3), base_r.append((t2 - t1) * 1e3)
    out["baseline_export_filter_10pct"] = stats(base_e)
    out["baseline_read_filter_keyed"] = stats(base_r)
    for r in out["table"]:
        print(f"table sel {r['selectivity']:<6} rows {r['rows']:>8}  pass0 event {r['event0']['median_ms']:.3f} wall "
              f"{r['wall0']['median_ms']:.3f} ms  pass1 event {r['event1']['median_ms']:.3f} wall {r['wall1']['median_ms']:.3f} ms"
              f"  sweep {r['sweep_GBps']} GB/s", flush=True)
    k = out["keyed"]
    print(f"keyed {NKEYS} keys rows {krows}  pass0 event {k['event0']['median_ms']:.3f} wall {k['wall0']['median_ms']:.3f} ms"
          f"  pass1 event {k['event1']['median_ms']:.3f} wall {k['wall1']['median_ms']:.3f} ms", flush=True)
    for name in ("baseline_export_filter_10pct", "baseline_read_filter_keyed"):
        b = out[name]
        print(f"{name}: {b['min_ms']:.1f} - {b['max_ms']:.1f} ms (median {b['median_ms']:.1f})", flush=True)
    print(json.dumps(out))
    eng.close()


if __name__ == "__main__":
    main()
