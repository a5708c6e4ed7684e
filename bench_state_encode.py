"""Sync books -> SyncStateV1 frames: corro_encode_states on MI355X, against the host path it replaces.

Two shapes, each with about 1/3 of its actors holding gaps and 1/8 a partial version:
  one    1 state x --actors actors (100k): one node's own State at the start of a sync session. The book is
         a real bookie's (Agent.sync_book() after process_multiple_changes), so the same bookie also gives
         the baseline: Agent.generate_sync() (corro_generate_sync + the dict rebuild) + wire.encode_sync_state
         + wire.frame, the only way to these bytes without corro_encode_states. The device frame is checked
         against the baseline's bytes before anything is timed. Filling the bookie goes through Python
         objects and takes minutes at 100k actors ("bookie_fill_s"; progress on stderr); it is set-up, part
         of neither timed path.
  many   --states states x --actors-per-state actors (4096 x 64, config 4's per-node shape): synthetic books
         of the same mix, resident in HBM; checked against the plain-Python model on its first states.

The device path is sync.state_frames_from_books(device=True) on book arrays already in HBM: both passes,
the output allocations and the read-back of the totals, timed with a host clock around work that ends in a
device synchronise; pass 0 and pass 1 are also timed apart. Algorithmic bytes = the book arrays read once
+ the frame bytes written once; their rate over the whole call is set against the 8 TB/s HBM peak. Prints
one JSON line; --log appends it to a file.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
HBM_PEAK_GBS = 8000.0


def ids(k):
    return int(k).to_bytes(8, "little") + (int(k) * 0x9E3779B97F4A7C15 & 0xFFFFFFFFFFFFFFFF).to_bytes(8, "little")


def fill_bookie(agent, actors, seed):
    """Every actor: version 1 whole. A third: versions 3 and 6 too (gaps 2 and 4-5). An eighth: seqs 1-2 of the
    six of the next version (an incomplete partial)."""
    import numpy as np
    from corrosion_amd.agent import Change, ChangeV1, Full
    rng = np.random.default_rng(seed)
    gaps, part = rng.random(actors) < 1 / 3, rng.random(actors) < 1 / 8
    batch, pk = [], 0

    def version(actor, v, seqs, last):
        nonlocal pk
        ch = []
        for k in range(seqs[0], seqs[1] + 1):
            pk += 1
            ch.append(Change("t", pk, "a", k, 1, v, k, actor, 1))
        return ChangeV1(actor, Full(v, ch, seqs, last, ts=v))

    for i in range(actors):
        actor = ids(i + 1)
        batch.append(version(actor, 1, (0, 0), 0))
        top = 1
        if gaps[i]:
            batch += [version(actor, 3, (0, 0), 0), version(actor, 6, (0, 0), 0)]
            top = 6
        if part[i]:
            batch.append(version(actor, top + 1, (1, 2), 5))
        if len(batch) >= 20000 or i == actors - 1:
            agent.process_multiple_changes(batch)
            batch = []
            print(f"bookie: {i + 1} / {actors} actors", file=sys.stderr, flush=True)


def synthetic_book(states, actors, seed):
    """`states` books of `actors` rows in one set of arrays (sync.concat_books' layout), the same mix."""
    import numpy as np
    rng = np.random.default_rng(seed)
    R = states * actors
    k = np.arange(1, R + 1, dtype=np.uint64)
    actor = np.stack([k, k * np.uint64(0x9E3779B97F4A7C15)], axis=1).view(np.uint8).reshape(R, 16)
    ngap = np.where(rng.random(R) < 1 / 3, rng.integers(1, 4, R), 0).astype(np.uint64)
    npart = (rng.random(R) < 1 / 8).astype(np.uint64)
    off = lambda c: np.concatenate([[0], np.cumsum(c)]).astype(np.uint64)
    gap_off, part_off = off(ngap), off(npart)
    NG, NP = int(gap_off[-1]), int(part_off[-1])
    within = np.arange(NG, dtype=np.uint64) - np.repeat(gap_off[:-1], ngap.astype(np.int64))
    gap_start = 10 * within + 2
    book = {"actor": actor, "max": rng.integers(100, 1_000_000, R).astype(np.int64), "gap_off": gap_off,
            "gap_start": gap_start, "gap_end": gap_start + rng.integers(0, 7, NG).astype(np.uint64),
            "part_off": part_off, "part_version": rng.integers(1, 100, NP).astype(np.uint64),
            "part_last_seq": np.full(NP, 9, np.uint64), "psr_off": 2 * np.arange(NP + 1, dtype=np.uint64),
            "psr_start": np.tile(np.array([1, 5], np.uint64), NP), "psr_end": np.tile(np.array([2, 6], np.uint64), NP),
            "state_row_off": actors * np.arange(states + 1, dtype=np.uint64)}
    return book


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--actors", type=int, default=100_000)
    ap.add_argument("--states", type=int, default=4096)
    ap.add_argument("--actors-per-state", type=int, default=64)
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
        sys.exit("bench_state_encode.py needs a GPU: there is no CPU path to measure")
    med = lambda x: float(np.median(x))

    def to_dev(book):
        return {k: torch.from_numpy(np.ascontiguousarray(v).reshape(-1).view(np.int64) if v.dtype == np.uint64 else
                                    np.ascontiguousarray(v).reshape(-1)).cuda() for k, v in book.items()}

    def measure(eng, dbook, me, ts, book_bytes):
        def whole():
            res = S.state_frames_from_books(eng, dbook, me, ts=ts, device=True)
            torch.cuda.synchronize()
            return res

        res = whole()
        assert int(res["state_status"].abs().sum()) == 0
        tot, p0, p1 = [], [], []
        for i in range(args.warmup + args.steps):
            t0 = time.perf_counter()
            whole()
            t1 = time.perf_counter()
            enc = S._StateEnc(eng, dbook, me, ts, 0, True)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            enc.write()
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            if i >= args.warmup:
                tot.append((t1 - t0) * 1e3)
                p0.append((t2 - t1) * 1e3)
                p1.append((t3 - t2) * 1e3)
        nb = int(res["total_bytes"])
        alg = book_bytes + nb
        return res, {"frame_bytes": nb, "book_bytes": book_bytes, "device_ms": med(tot), "device_ms_min_max": [min(tot), max(tot)],
                     "pass0_ms": med(p0), "pass1_ms": med(p1), "frame_bytes_per_s": nb / (med(tot) * 1e-3),
                     "algorithmic_bytes": alg, "roofline_frac": alg / (med(tot) * 1e-3) / 1e9 / HBM_PEAK_GBS}

    nbytes = lambda book: int(sum(np.asarray(v).nbytes for v in book.values()))

    # ---- one state of --actors actors, from a real bookie
    me = ids(0)
    ag = ca.agent.Agent({"t": ["a"]}, capacity_hint=1 << 20, actor_id=me)
    t0 = time.perf_counter()
    fill_bookie(ag, args.actors, args.seed)
    fill_s = time.perf_counter() - t0
    ts = 1 << 40
    t0 = time.perf_counter()
    book = S.concat_books([ag.sync_book()])
    book_ms = (time.perf_counter() - t0) * 1e3

    def host_path():
        st = ag.generate_sync()
        st.last_cleared_ts = ts
        return W.frame(W.encode_sync_state(st))

    want = host_path()
    res, one = measure(ag.engine, to_dev(book), [me], [ts], nbytes(book))
    assert res["buf"].cpu().numpy().tobytes() == want                 # the same bytes, before any timing
    hs = []
    for i in range(args.warmup + args.steps):
        t0 = time.perf_counter()
        host_path()
        if i >= args.warmup:
            hs.append((time.perf_counter() - t0) * 1e3)
    one.update({"states": 1, "actors": args.actors, "n_need": int(res["n_need"][0]), "n_partial": int(res["n_partial"][0]),
                "host_ms": med(hs), "host_ms_min_max": [min(hs), max(hs)],
                "host_path": "Agent.generate_sync (corro_generate_sync + dict rebuild) + wire.encode_sync_state + wire.frame",
                "sync_book_ms_once": book_ms, "speedup": med(hs) / one["device_ms"],
                "speedup_with_sync_book": med(hs) / (one["device_ms"] + book_ms), "bookie_fill_s": fill_s})

    # ---- many states of --actors-per-state actors, synthetic books in HBM
    from tests import state_encode_model as EM
    book = synthetic_book(args.states, args.actors_per_state, args.seed)
    mes = np.frombuffer(b"".join(ids(10_000_000 + b) for b in range(args.states)), np.uint8)
    tss = [b for b in range(args.states)]
    res, many = measure(ag.engine, to_dev(book), mes, tss, nbytes(book))
    off, buf = res["frame_off"].cpu().numpy(), res["buf"].cpu().numpy().tobytes()
    for b in range(min(args.states, 8)):                              # the first states against the model
        rows = EM.rows_of_book(book, b * args.actors_per_state, (b + 1) * args.actors_per_state)
        assert buf[off[b]:off[b + 1]] == W.frame(W.encode_sync_state(EM.generate_sync(rows, ids(10_000_000 + b), b))), b
    many.update({"states": args.states, "actors_per_state": args.actors_per_state,
                 "states_per_s": args.states / (many["device_ms"] * 1e-3)})

    line = {"metric": "sync books -> SyncStateV1 frames (corro_encode_states)", "steps": args.steps, "warmup": args.warmup,
            "device_path": "corro_encode_states pass 0 + pass 1 on books in HBM, outputs allocated per call",
            "hbm_peak_gbs": HBM_PEAK_GBS, "one_state": one, "many_states": many, "data": "synthetic, seeded"}
    print(json.dumps(line), flush=True)
    if args.log:
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        with open(args.log, "a") as f:
            f.write(json.dumps(line) + "\n")
    ag.engine.close()


if __name__ == "__main__":
    main()
