"""Shared by the extraction tests: the one checker every parity test of corro_extract_changes goes
through, hand-built batches whose clock rows carry chosen (site, db_version, seq, ts), and the
host -> device form of a need set."""
import numpy as np

from tests.extract_model import I_DBV, I_SEQ, I_SITE, ROWF, row_tuples, seq_classes

SCHEMA = {"t": ["a", "b", "c", "d"]}


def host_result(res):
    """An extract_changes result as numpy arrays in the ABI's dtypes (device results come back as
    signed torch tensors: viewed, not converted)."""
    from corrosion_amd.engine import ROW_FIELDS

    def np_of(v, dt=None):
        a = v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)
        return a.view(dt) if dt is not None and a.dtype != dt else a
    out = {k: np_of(v, np.int64 if k == "version" else np.uint64) for k, v in res.items() if k != "rows"}
    out["rows"] = {k: np_of(v, ROW_FIELDS[k]) for k, v in res["rows"].items()}
    return out


def check_extract(res, exp, needs):
    """res: engine.extract_changes' result (either memory); exp: the expected groups per need in the
    model's shape (extract_model.extract, or from_oracle); needs: the need set. Asserts, per need:
    counts, groups (versions DESC, last_seq, ts), the tiling of [row_off[e], row_off[e+1]) by the
    groups, the rows' EMITTED order (seq non-decreasing as written; its seq classes and each class's
    rows as a multiset equal the model's: only rows of equal (version, seq) may permute), and every
    row's site / db_version against its group. Nothing else is canonicalised."""
    R = host_result(res)
    n = len(needs["site"])
    assert len(exp) == n
    go, ro = [int(x) for x in R["grp_off"]], [int(x) for x in R["row_off"]]
    assert len(go) == n + 1 and len(ro) == n + 1 and go[0] == 0 and ro[0] == 0
    for k in ("version", "last_seq", "ts", "grp_row_off", "grp_rows"):
        assert len(R[k]) == go[n], k
    for k in ROWF:
        assert len(R["rows"][k]) == ro[n], k
    got_rows = row_tuples(R["rows"])
    for e in range(n):
        site = int(needs["site"][e])
        # counts (pass 0, as the offsets imply them)
        want_g, want_r = len(exp[e]), sum(len(g[3]) for g in exp[e])
        assert go[e + 1] - go[e] == want_g, f"need {e}: grp_count {go[e + 1] - go[e]}, the model has {want_g}"
        assert ro[e + 1] - ro[e] == want_r, f"need {e}: row_count {ro[e + 1] - ro[e]}, the model has {want_r}"
        cur = ro[e]
        for j, (v, last, ts, erows) in enumerate(exp[e]):
            g = go[e] + j
            assert (int(R["version"][g]), int(R["last_seq"][g]), int(R["ts"][g])) == (v, last, ts), (e, j)
            assert int(R["grp_row_off"][g]) == cur, ("tiling", e, j)
            cnt = int(R["grp_rows"][g])
            rows = got_rows[cur:cur + cnt]
            cur += cnt
            assert cur <= ro[e + 1], ("tiling", e, j)
            seqs = [r[I_SEQ] for r in rows]
            assert all(a <= b for a, b in zip(seqs, seqs[1:])), ("seq order as emitted", e, j, seqs[:8])
            # the emitted rows cut into runs of equal seq, in emitted order, against the model's classes
            runs = []
            for r in rows:
                if runs and runs[-1][0] == r[I_SEQ]:
                    runs[-1][1].append(r)
                else:
                    runs.append((r[I_SEQ], [r]))
            assert [(s, sorted(c)) for s, c in runs] == seq_classes(erows), (e, j)
            assert all(r[I_SITE] == site and r[I_DBV] == v for r in rows), (e, j)
        assert cur == ro[e + 1], ("tiling", e)
        vs = [g[0] for g in exp[e]]
        assert all(a > b for a, b in zip(vs, vs[1:])), ("expected versions not descending", e)


def batch(changes, ts=True, pk_base=1, cid=1):
    """A batch of plain column inserts (cl 1, col_version 1, INTEGER values) whose clock rows are
    exactly `changes`: tuples (site, db_version, seq, ts) in application order, each on a fresh row
    (pk = pk_base + its position), so no change displaces another. ts=False: a batch without ts."""
    n = len(changes)
    b = {"pk": np.arange(pk_base, pk_base + n, dtype=np.uint64),
         "table_cid": np.full(n, cid, np.uint32),
         "col_version": np.ones(n, np.int64),
         "db_version": np.array([x[1] for x in changes], np.int64),
         "cl": np.ones(n, np.uint32),
         "seq": np.array([x[2] for x in changes], np.uint32),
         "site": np.array([x[0] for x in changes], np.uint32),
         "val0": np.arange(n, dtype=np.uint64) * np.uint64(7919) + np.uint64(3)}
    if ts:
        b["ts"] = np.array([x[3] for x in changes], np.uint64)
    return b


def needs_arrays(needs, seq=None):
    """[(site, start, end)] (+ [(seq_start, seq_end)]) as the need dict of numpy arrays."""
    nd = {"site": np.array([x[0] for x in needs], np.uint32), "start": np.array([x[1] for x in needs], np.uint64),
          "end": np.array([x[2] for x in needs], np.uint64)}
    if seq is not None:
        assert len(seq) == len(needs)
        nd["seq_start"] = np.array([x[0] for x in seq], np.uint32)
        nd["seq_end"] = np.array([x[1] for x in seq], np.uint32)
    return nd


def device_needs(nd):
    """The same needs as CUDA tensors (the bits of the unsigned fields in torch's signed dtypes)."""
    import torch
    return {k: torch.from_numpy(np.ascontiguousarray(v).view(np.int64 if v.dtype == np.uint64 else np.int32)).cuda()
            for k, v in nd.items()}


def triples(rows):
    return [(int(s), int(d), int(q)) for s, d, q in zip(rows["site"], rows["db_version"], rows["seq"])]
