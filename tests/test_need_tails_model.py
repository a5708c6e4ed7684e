"""The model the GPU tests of corro_need_tails compare against (tests/need_tails_util.model, a loop
over the versions) pinned against the range arithmetic of the host path (serve._subtract, as
serve._bookie_messages uses it), on the 200 seeded books of the GPU test. No GPU."""
import numpy as np

from corrosion_amd import serve
from tests import need_tails_util as U

SEEDS = range(1000, 1200)


def by_subtraction(a, table_sites):
    nbook = len(a["gap_off"]) - 1
    off, host, ranges = [0], [], []
    for t in range(len(a["kind"])):
        site, s, e = int(a["need_site"][t]), int(a["start"][t]), int(a["end"][t])
        h, rs = 0, []
        if a["need_keep"][t] and site < nbook and site < table_sites:
            gaps = [(int(a["gap_start"][g]), int(a["gap_end"][g]))
                    for g in range(int(a["gap_off"][site]), int(a["gap_off"][site + 1]))]
            buffered = [int(v) for v in a["buf_version"][int(a["buf_off"][site]):int(a["buf_off"][site + 1])]]
            if a["kind"][t] == 0:
                k = int(a["need_ent_off"][t])
                found = sorted(int(v) for v in a["version"][int(a["grp_off"][k]):int(a["grp_off"][k + 1])])
                unprocessed = serve._subtract([(s, e)], [(v, v) for v in found])
                if any(x <= v <= y for x, y in unprocessed for v in buffered):
                    h = 1
                else:
                    empties = []
                    for x, y in unprocessed:
                        empties += serve._subtract([(x, y)], gaps + [(v, v) for v in buffered])
                    rs = serve._subtract(empties, [])
            elif not a["in_state"][t]:
                if s in buffered:
                    h = 1
                elif not serve._in_ranges(gaps, s):
                    rs = [(s, s)]
        ranges += [(site, x, y) for x, y in rs]
        off.append(len(ranges))
        host.append(h)
    return off, host, ranges


def test_model_equals_the_host_range_arithmetic():
    kept = flagged = emitting = 0
    for seed in SEEDS:
        a = U.random_case(np.random.default_rng(seed))
        assert len(a["kind"]) <= 40 and int(a["end"].max()) < 200
        got, want = U.model(a, 4), by_subtraction(a, 4)
        assert got == want, seed
        off, host, ranges = got
        # a version is in a range iff it is in none of F, G and P, and the ranges are maximal runs
        for t in range(len(a["kind"])):
            rs = ranges[off[t]:off[t + 1]]
            assert all(x <= y for _, x, y in rs) and all(rs[i][2] + 1 < rs[i + 1][1] for i in range(len(rs) - 1)), seed
            assert not (host[t] and rs)
            kept += int(a["need_keep"][t])
            flagged += host[t]
            emitting += 1 if rs else 0
    # the shares the GPU test asserts too: most kept needs are served on the device, many emit a range
    assert flagged * 2 < kept and emitting * 4 >= kept, (kept, flagged, emitting)


def test_runs_and_frames():
    assert U.runs([]) == [] and U.runs([3]) == [(3, 3)] and U.runs([1, 2, 4, 6, 7, 8]) == [(1, 2), (4, 4), (6, 8)]
    ids = [bytes([7]) * 16, bytes([9]) * 16]
    f = U.frames([(1, 5, 6)], ids)
    assert len(f) == U.FRAME[0] and f[:4] == b"\0\0\0\x2d" and f[12:28] == ids[1]
    assert len(U.frames([(0, 1, 1), (1, 2, 9)], ids, 1, 77)) == 2 * U.FRAME[1]
