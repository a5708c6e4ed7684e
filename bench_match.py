"""Benchmark of corro_match_changes behind the agent call; prints one JSON line.

python bench_match.py [--changes N] [--steps K] [--warmup W] [--host-changes H]

The batch has bench.py's agent shape (config 2 as ChangeV1s: 1000 actors, versions of 64 changes arriving
interleaved across actors, the batch in arrival order, uniform pks, cl = 1) over a schema of 8 tables x 8
INTEGER columns, so that filters have something to tell apart. It is generated in HBM, merged once by
corro_process_multiple_changes (CORRO_MEM_DEVICE_HEADERS) into an empty state, and the impact flags of that
call feed the matching, where they lie. Two filter loads:
  8 classes    one update handle per table
  256 classes  320 subscriptions over overlapping column sets of one or two tables, 64 of them exact
               duplicates of others, which fold
Per load: device ms per pass (median of --steps after --warmup calls), matches and candidates per second,
and the algorithmic bytes -- the four input columns read once, the bit words of the impactful changes, the
output written once -- against the HBM peak. Next to it the only alternative without this entry point: the
D2H copy of impactful / pk / table_cid / cl and the headers, and the host model vectorised with numpy (on
the first --host-changes changes: the device runs that prefix too and its arrays are compared with the
host's before anything is timed).
"""
import argparse
import ctypes as C
import json
import time

import numpy as np

N_ACTORS, PER_VERSION, N_TABLES, N_COLS, N_PK = 1000, 64, 8, 8, 1 << 24
HBM_PEAK_GBS = 8000.0
SCHEMA = {f"t{t}": [f"c{k}" for k in range(N_COLS)] for t in range(N_TABLES)}


def agent_batch(n, dev, seed=2):
    """Changes in arrival order: changeset j holds changes [64 j, 64 j + 64), actor j % 1000, version
    j // 1000 + 1."""
    import torch
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    i = torch.arange(n, device=dev, dtype=torch.int64)
    j = i // PER_VERSION
    rnd = lambda lo, hi: torch.randint(lo, hi, (n,), device=dev, generator=g, dtype=torch.int64)  # noqa: E731
    batch = {"pk": rnd(1, N_PK + 1), "table_cid": (rnd(0, N_TABLES) << 16 | rnd(1, N_COLS + 1)).to(torch.int32),
             "col_version": rnd(1, 9), "db_version": j // N_ACTORS + 1, "cl": torch.ones(n, device=dev, dtype=torch.int32),
             "seq": (i % PER_VERSION).to(torch.int32), "site": (j % N_ACTORS).to(torch.int32), "val0": rnd(0, 1 << 40)}
    batch = {k: v.contiguous() for k, v in batch.items()}
    ncs = -(-n // PER_VERSION)
    jj = np.arange(ncs, dtype=np.int64)
    return batch, jj


def merge_flags(eng, batch, jj, n):
    """One corro_process_multiple_changes call with everything in HBM; returns (impact flags, headers)."""
    import torch
    import synth
    import corrosion_amd as ca
    from corrosion_amd import _lib as L
    dev = batch["pk"].device
    ids = np.ascontiguousarray(synth.site_ids(N_ACTORS, 1), dtype=np.uint8)
    eng.register_sites(ids)
    cs = np.zeros((len(jj), C.sizeof(L.Changeset) // 8), np.uint64)
    f = {name: getattr(L.Changeset, name).offset // 8 for name, _t in L.Changeset._fields_ if name not in ("site", "kind")}
    cs[:, f["actor_id"]] = ids.ctypes.data + 16 * (jj % N_ACTORS)
    cs[:, L.Changeset.site.offset // 8] = (jj % N_ACTORS) | (L.CORRO_CS_FULL << 32)     # site, kind: two u32
    cnt = np.minimum(PER_VERSION, n - jj * PER_VERSION)
    cs[:, f["version_start"]] = cs[:, f["version_end"]] = jj // N_ACTORS + 1
    cs[:, f["seq_end"]] = cs[:, f["last_seq"]] = cnt - 1
    cs[:, f["ts"]] = ((jj // N_ACTORS + 1) << 32) | (jj % N_ACTORS)
    cs[:, f["change_off"]], cs[:, f["change_count"]] = jj * PER_VERSION, cnt
    dcs = torch.from_numpy(cs.view(np.uint8).reshape(-1).copy()).to(dev)
    known = torch.full((len(jj),), -1, dtype=torch.int32, device=dev)
    imp = torch.zeros(n, dtype=torch.uint8, device=dev)
    s = L.Changes()
    s.n = n
    for k in ("pk", "table_cid", "col_version", "db_version", "cl", "seq", "site", "val0"):
        setattr(s, k, batch[k].data_ptr())
    out = L.ProcessOut()
    out.known, out.impactful = known.data_ptr(), imp.data_ptr()
    bk = ca.agent.Bookie()
    torch.cuda.synchronize()
    L.check(L.lib().corro_process_multiple_changes(eng._h, bk._h, C.c_void_p(dcs.data_ptr()), len(jj), C.byref(s),
                                                   L.CORRO_MEM_DEVICE_HEADERS, C.byref(out)))
    assert bool((known == 1).all().item()), "every version of the call is Current"
    return imp, dcs


def filter_loads(eng):
    from corrosion_amd.updates import MatchFilters
    rng = np.random.default_rng(7)
    tables = list(SCHEMA)
    small = MatchFilters(eng, updates=tables)
    subs, seen = [], set()
    while len(subs) < 256:
        sub = {}
        for t in rng.permutation(N_TABLES)[:int(rng.integers(1, 3))]:
            sub[tables[t]] = sorted(SCHEMA[tables[t]][c] for c in rng.permutation(N_COLS)[:int(rng.integers(1, 5))])
        key = tuple(sorted((t, tuple(c)) for t, c in sub.items()))
        if key not in seen:
            seen.add(key)
            subs.append(sub)
    subs += [subs[int(k)] for k in rng.integers(0, 256, 64)]          # 64 exact duplicates
    big = MatchFilters(eng, subs=subs)
    assert small.nclasses == 8 and big.nclasses == 256 and len(big.handles) == 320
    return {"8_classes": small, "256_classes": big}


def host_model(imp, pk, tcid, cl, cs_off, cs_cnt, filters):
    """match_changes over host arrays, vectorised with numpy: (class_off, cand_change)."""
    base = np.array([filters.base[t] for t in filters.tables], np.int64)
    take = np.zeros((filters.nslots, filters.nclasses), bool)
    for c in range(filters.nclasses):
        take[:, c] = (filters.bits[:, c // 32] >> np.uint32(c % 32)) & 1
    idx = np.flatnonzero(imp)
    slot = base[tcid[idx] >> 16] + (tcid[idx] & 0xFFFF)
    row, cls = np.nonzero(take[slot])                        # (change, class) order
    ch = idx[row]
    live = cs_cnt > 0
    cs = np.flatnonzero(live)[np.searchsorted((cs_off + cs_cnt)[live], ch, side="right")]
    order = np.lexsort((ch, pk[ch], tcid[ch] >> 16, cs, cls))
    k = np.stack([cls[order], cs[order], (tcid[ch] >> 16)[order].astype(np.int64), pk[ch][order].view(np.int64)])
    head = np.ones(len(order), bool)
    head[1:] = (k[:, 1:] != k[:, :-1]).any(axis=0)
    win_ch, win_cls = ch[order][head], cls[order][head]
    o2 = np.lexsort((win_ch, win_cls))
    class_off = np.searchsorted(win_cls[o2], np.arange(filters.nclasses + 1), side="left")
    return class_off.astype(np.uint64), win_ch[o2].astype(np.uint32), len(ch)


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--changes", type=int, default=1 << 24)
    ap.add_argument("--host-changes", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    import torch
    import corrosion_amd as ca
    from corrosion_amd import _lib as L
    from corrosion_amd import updates as U
    n = args.changes
    nh = min(n, args.host_changes) // PER_VERSION * PER_VERSION
    dev = torch.device("cuda:0")
    eng = ca.MergeEngine(SCHEMA, capacity_hint=n, device=0)
    batch, jj = agent_batch(n, dev)
    imp, dcs = merge_flags(eng, batch, jj, n)
    ncs = len(jj)
    result = {"bench": "match_changes", "changes": n, "changesets": ncs, "impactful": int(imp.sum().item()),
              "steps": args.steps, "warmup": args.warmup, "hbm_peak_gb_s": HBM_PEAK_GBS, "loads": {}}

    # the alternative: everything matching reads, copied to the host (pageable numpy arrays, as an
    # integrator following INTEGRATION section 3 would hold them)
    d2h = []
    for _ in range(args.warmup + args.steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h = {"imp": imp.cpu().numpy(), "pk": batch["pk"].cpu().numpy().view(np.uint64),
             "tcid": batch["table_cid"].cpu().numpy().view(np.uint32), "cl": batch["cl"].cpu().numpy().view(np.uint32),
             "cs": dcs.cpu().numpy()}
        d2h.append((time.perf_counter() - t0) * 1e3)
    d2h_bytes = n * (1 + 8 + 4 + 4) + ncs * C.sizeof(L.Changeset)
    result["d2h"] = {"ms": median(d2h[args.warmup:]), "bytes": d2h_bytes}
    rec = h["cs"].view(np.uint64).reshape(ncs, -1)
    cs_off = rec[:, L.Changeset.change_off.offset // 8].astype(np.int64)
    cs_cnt = rec[:, L.Changeset.change_count.offset // 8].astype(np.int64)

    for name, filters in filter_loads(eng).items():
        # 1. the prefix on both sides, compared before anything is timed
        pre = {k: batch[k][:nh] for k in ("pk", "table_cid", "cl")}
        got = U.match_changes(eng, pre, imp[:nh], dcs, filters, device=True, ncs=nh // PER_VERSION)
        hs = nh // PER_VERSION
        off, chg, _m = host_model(h["imp"][:nh], h["pk"][:nh], h["tcid"][:nh], h["cl"][:nh], cs_off[:hs], cs_cnt[:hs], filters)
        same = (got["class_off"].cpu().numpy().view(np.uint64).tolist() == off.tolist()
                and got["cand_change"].cpu().numpy().view(np.uint32).tolist() == chg.tolist())
        if not same:
            raise SystemExit(f"{name}: the device candidates differ from the host model's")
        host_ms = []
        for _ in range(3):
            t0 = time.perf_counter()
            _off, _chg, host_matches = host_model(h["imp"][:nh], h["pk"][:nh], h["tcid"][:nh], h["cl"][:nh], cs_off[:hs],
                                                  cs_cnt[:hs], filters)
            host_ms.append((time.perf_counter() - t0) * 1e3)
        # 2. the whole batch on the device
        p0, p1 = [], []
        for _ in range(args.warmup + args.steps):
            t = {}
            res = U.match_changes(eng, batch, imp, dcs, filters, device=True, ncs=ncs, timings=t)
            p0.append(t["pass0_ms"])
            p1.append(t["pass1_ms"])
        p0, p1 = median(p0[args.warmup:]), median(p1[args.warmup:])
        ncand = res["ncand"]
        t = {}
        U.match_changes(eng, pre, imp[:nh], dcs, filters, device=True, ncs=hs, timings=t)
        cnt = torch.from_numpy(np.array([bin(int(w)).count("1") for w in range(1 << 16)], np.int64)).to(dev)
        bits = filters.device_bits(dev).view(filters.nslots, filters.words).to(torch.int64) & 0xFFFFFFFF
        per_slot = (cnt[bits & 0xFFFF] + cnt[bits >> 16]).sum(dim=1)
        tc = batch["table_cid"].to(torch.int64)
        slot = (tc >> 16) * (N_COLS + 1) + (tc & 0xFFFF)
        matches = int((per_slot[slot] * (imp != 0)).sum().item())
        alg = n * (1 + 8 + 4 + 4) + result["impactful"] * filters.words * 4 + (filters.nclasses + 1) * 8 + ncand * 24
        result["loads"][name] = {
            "classes": filters.nclasses, "handles": len(filters.handles), "matches": matches, "candidates": ncand,
            "pass0_ms": p0, "pass1_ms": p1, "matches_per_s": matches / ((p0 + p1) * 1e-3),
            "candidates_per_s": ncand / ((p0 + p1) * 1e-3), "algorithmic_bytes": alg,
            "algorithmic_gb_s": alg / ((p0 + p1) * 1e-3) / 1e9,
            "fraction_of_hbm_peak": alg / ((p0 + p1) * 1e-3) / 1e9 / HBM_PEAK_GBS,
            "host_model": {"changes": nh, "matches": host_matches, "ms": median(host_ms),
                           "device_ms_same_prefix": t["pass0_ms"] + t["pass1_ms"], "arrays_equal": same,
                           "note": "numpy model and the device on the first `changes` changes of the batch"}}
    eng.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
