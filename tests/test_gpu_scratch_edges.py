"""The two-pass sync entry points at the edges of their scratch layout (csrc/scratch.h): leading counts
(needs, frames, pairs, spans) of 0, 1, 31, 32 and 33, so that the 8-byte arrays of count + 1 elements end
one under, exactly on and one over a 256-byte region boundary, and the 4-byte and 1-byte ones lie well
inside one. Every entry point that stages host arrays runs both passes from host and from device memory;
the two must agree array for array, and with the host model where the helper modules have one. The inputs
and the comparisons are the existing GPU tests' own."""
import numpy as np
import pytest

from corrosion_amd import sync as S
from tests import assemble_util as AU
from tests import need_tails_util as TU
from tests import req_decode_util as RU
from tests import state_model as SM
from tests import test_gpu_assemble as TA
from tests import test_gpu_need_tails as TT
from tests import test_gpu_request_decode as RD
from tests import test_gpu_state_decode as SD
from tests import test_gpu_sync_requests as SR

pytestmark = pytest.mark.gpu
COUNTS = (0, 1, 31, 32, 33)
BOOKS = {0: ([(4, 5)], 12), 3: ([], 2), 4: ([(1, 1)], None)}


def host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def same_arrays(a, b, what):
    """Two results of one wrapper, one from host and one from device memory: equal key for key."""
    assert a.keys() == b.keys(), what
    for k in a:
        if isinstance(a[k], dict):
            same_arrays(a[k], b[k], (what, k))
        elif hasattr(a[k], "shape"):
            x, y = host(a[k]), host(b[k])                          # (a device tensor is the signed twin of the host dtype)
            assert x.shape == y.shape and x.dtype.itemsize == y.dtype.itemsize, (what, k)
            assert np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes(), (what, k)
        else:
            assert a[k] == b[k], (what, k)


def request_cases(n):
    """n frames of one pair and one Full need each: frames = pairs = needs = entries = n."""
    return [(RU.request_frame([(RD.ACT[i % 6], [S.Full(1 + i, 5 + i)])]), 0) for i in range(n)]


@pytest.mark.parametrize("n", COUNTS)
def test_decode_requests(n):
    cases = request_cases(n)
    exp = RD.check(cases, BOOKS, f"{n} frames, screened")        # host and device against the model
    assert exp["nframes"] == exp["npairs"] == exp["nneeds"] == n
    RD.check(cases, None, f"{n} frames")
    frames = [f for f, _ in cases]
    same_arrays(RD.decode(frames, BOOKS, "host"), RD.decode(frames, BOOKS, "device"), n)


def extraction_of(dec, put):
    """A made-up extraction of dec's entries: two groups per entry, two rows per group."""
    E = int(dec["nents"])
    G = 2 * E
    return {"grp_off": put(np.arange(0, G + 1, 2, dtype=np.uint64)),
            "version": put(np.repeat(host(dec["ent_end"]).astype(np.int64), 2) - np.tile([0, 1], E).astype(np.int64)),
            "last_seq": put(np.full(G, 3, np.uint64)), "ts": put(np.arange(G, dtype=np.uint64) + np.uint64(100)),
            "grp_row_off": put(np.arange(G, dtype=np.uint64) * np.uint64(2)), "grp_rows": put(np.full(G, 2, np.uint64))}


@pytest.mark.parametrize("n", COUNTS)
def test_need_spans(n):
    frames = [f for f, _ in request_cases(n)]
    res = {}
    for mem in ("host", "device"):
        dec = RD.decode(frames, None, mem)
        res[mem] = RD.engine().need_spans(dec, extraction_of(dec, RD.to_dev if mem == "device" else (lambda a: a)))
    same_arrays(res["host"], res["device"], n)
    h = res["host"]
    assert h["nspans"] == 2 * n and host(h["need_span_off"]).astype(np.int64).tolist() == list(range(0, 2 * n + 1, 2))
    assert host(h["row_off"]).astype(np.int64).tolist() == list(range(0, 4 * n, 2))
    assert host(h["version"]).astype(np.int64).tolist() == [v for i in range(n) for v in (5 + i, 4 + i)]


@pytest.mark.parametrize("n", COUNTS)
def test_need_tails(n):
    book = {0: ([(10, 12)], [30]), 1: ([], []), 2: ([(3 * k, 3 * k) for k in range(1, 8)], []), 3: ([], [])}
    c = TU.Case(book, 4)
    for i in range(n):
        c.full(i % 4, 1 + i, 6 + i, found=[2 + i, 4 + i])
    off, need_host, ranges = TT.check(c.arrays(), f"{n} needs")     # host and device, both payloads, against the model
    assert len(off) == n + 1 and len(need_host) == n


@pytest.mark.parametrize("n", COUNTS)
def test_assemble_answers(n):
    rng = np.random.default_rng(40 + n)
    needs = [(int(rng.integers(0, 70)), i % 3, 1, 0) for i in range(n)]
    a = AU.build(needs, rng, n % 2, pairs=[1] * n, frames=[1] * n)
    for mem in ("host", "device"):                               # each against the model, byte for byte
        _buf, nao, fao, _fh = TA.check(a, f"{n} needs {mem}", mem)
        assert len(nao) == n + 1 and len(fao) == n + 1


def encode_case(n):
    """n spans of one INTEGER row each, and the messages the host object path makes of them."""
    from corrosion_amd.agent import Change, ChangeV1, Full
    eng = RD.engine()
    site = np.arange(n, dtype=np.uint32) % np.uint32(6)
    rows = {"pk": np.arange(n, dtype=np.uint64) + np.uint64(7), "table_cid": np.full(n, eng.lookup("t", "a"), np.uint32),
            "col_version": np.ones(n, np.int64), "db_version": np.arange(n, dtype=np.int64) + 1, "cl": np.ones(n, np.int64),
            "seq": np.zeros(n, np.uint32), "site": site, "val0": np.arange(n, dtype=np.uint64) * np.uint64(1000003),
            "val1": np.zeros(n, np.uint64), "val_type": np.ones(n, np.uint8), "val_len": np.zeros(n, np.uint8)}
    spans = {"site": site, "version": np.arange(n, dtype=np.int64) + 1, "last_seq": np.zeros(n, np.uint64),
             "ts": np.arange(n, dtype=np.uint64) + np.uint64(9), "seq_start": np.zeros(n, np.uint64),
             "seq_end": np.zeros(n, np.uint64), "row_off": np.arange(n, dtype=np.uint64), "row_count": np.ones(n, np.uint64)}
    msgs = [ChangeV1(RD.ACT[i % 6], Full(i + 1, [Change("t", 7 + i, "a", 1000003 * i, 1, i + 1, 0, RD.ACT[i % 6], 1)],
                                         (0, 0), 0, ts=9 + i)) for i in range(n)]
    return spans, rows, msgs


@pytest.mark.parametrize("n", COUNTS)
def test_encode_changesets(n):
    from corrosion_amd import wire
    from tests.test_gpu_wire_encode import to_dev
    spans, rows, msgs = encode_case(n)
    hst = RD.engine().encode_changesets(spans, rows)
    dev = RD.engine().encode_changesets(to_dev(spans), to_dev(rows))
    assert n == 0 or dev["buf"].is_cuda
    same_arrays(hst, dev, n)
    assert hst["nframes"] == n and host(hst["buf"]).tobytes() == wire.frames(msgs, wire.PAYLOAD_SYNC)
    assert host(hst["span_frame_off"]).astype(np.int64).tolist() == list(range(n + 1))


@pytest.mark.parametrize("n", COUNTS)
def test_plan_requests(n):
    """n Full needs of one entry of one group: the planner's per-need arrays hold n and n + 1 elements."""
    ents = [(SR.A0, [("F", 20 * i + 1, 20 * i + 3) for i in range(n)])] if n else []
    res = [SR.run_sessions([[ents]], 10, 10, mem) for mem in SR.MEMS]   # each against the sequential oracle
    same_arrays(res[0], res[1], n)
    assert (res[0]["nframes"] > 0) == (n > 0)


@pytest.mark.parametrize("n", COUNTS)
def test_decode_states(n):
    """n frames and n pairs, frame i against frame i + 1."""
    pairs = SM.random_pairs(60 + n, (n + 1) // 2)
    frames = [SM.state_frame(st) for p in pairs for st in p][:n]
    idx = [(i, (i + 1) % n) for i in range(n)]
    got = {mem: SD.check(frames, idx, mem, f"{n} frames {mem}")[0] for mem in SD.MEMS}   # each against the model
    want = SM.decode_model(frames, idx, SD.site_of)
    SM.assert_same(got["host"], want)
    SM.assert_same(got["device"], want)
    assert len(want["pair_ent_off"]) == n + 1 and len(want["frame_status"]) == n
