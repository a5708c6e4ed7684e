"""The last refusal of corro_plan_requests' contract: a frame payload of 2^32 bytes or more returns
CORRO_E_RANGE, leaves sentinel-filled outputs unchanged, and the context plans a valid call after it.

A Full frame's payload is 32 + 20 * pieces, so the refusal needs 214,748,364 pieces in one item.
Server 0 asks for N = 214,748,363 one-version Full needs on the even versions 2, 4, .., 2N; server 1
asks for Full 1..=2N+1 with a chunk larger than that span (one item) and a drain that lets server 0
go first entirely. Server 1 is left with the N + 1 odd versions as N + 1 runs: payload 2^32 + 16.
With its end at 2N - 1 it is left with N runs, payload 2^32 - 4, the largest frame that is accepted.
The input is about 7 GB and is built on the card, so the case runs from device memory only. It is the
one planner test sized in gigabytes: three plans of 2^27.7 items, about four seconds each on an
MI355X, which is what the case costs at the only size where it exists. It owns its engine and closes
it, which returns the scratch."""
import ctypes as C

import numpy as np
import pytest

from corrosion_amd import _lib as L
from corrosion_amd import sync as S
from tests import sync_req_util as U

pytestmark = pytest.mark.gpu
SENTINEL = 0x5A
N = 214_748_363
assert 32 + 20 * (N + 1) >= 1 << 32 > 32 + 20 * N


def _call(eng, arr, o, pass_):
    import torch
    r = L.RequestIn()
    r.n, r.nneeds, r.nseqs, r.ngroups = (int(arr[k].numel()) for k in ("site", "kind", "s_start", "grp_session"))
    r.chunk_size, r.drain = 1 << 40, (1 << 32) - 1
    for k in S._REQ_IN:
        setattr(r, k, arr[k].data_ptr() if arr[k].numel() else None)
    torch.cuda.synchronize()
    return L.lib().corro_plan_requests(eng._h, C.byref(r), L.CORRO_MEM_DEVICE, C.byref(o), pass_)


def test_frame_payload_of_2_32_bytes_is_refused():
    import torch
    import corrosion_amd as ca
    eng = ca.MergeEngine({"t": ["a"]}, capacity_hint=1024)
    try:
        assert list(eng.register_sites(np.frombuffer(U.ACTORS[0], np.uint8))) == [0]
        dev = torch.device("cuda")
        i64 = lambda *v: torch.tensor(v, dtype=torch.int64, device=dev)
        start = torch.empty(N + 1, dtype=torch.int64, device=dev)
        torch.arange(2, 2 * N + 1, 2, out=start[:N])
        end = start.clone()
        start[N], end[N] = 1, 2 * N + 1
        zeros = torch.zeros(N + 1, dtype=torch.int64, device=dev)
        empty = torch.zeros(0, dtype=torch.int64, device=dev)
        arr = {"site": torch.zeros(2, dtype=torch.int32, device=dev), "need_off": i64(0, N, N + 1),
               "kind": torch.zeros(N + 1, dtype=torch.uint8, device=dev), "start": start, "end": end,
               "sr_off": zeros, "sr_n": zeros, "s_start": empty, "s_end": empty,
               "grp_ent_off": i64(0, 1, 2), "grp_session": i64(0, 0)}
        outs = {"grp_frame_off": (3, torch.int64), "buf": (64, torch.uint8), "frame_off": (2, torch.int64),
                "frame_entry": (1, torch.int64), "frame_round": (1, torch.int32), "frame_needs": (1, torch.int32)}
        held = {k: torch.full((m,), SENTINEL, dtype=dt, device=dev) for k, (m, dt) in outs.items()}
        o = L.Requests()
        for k, v in held.items():
            setattr(o, k, v.data_ptr())
        for pass_ in (0, 1):
            o.nframes, o.nbytes = (1, 64) if pass_ else (0, 0)
            assert _call(eng, arr, o, pass_) == -6                              # CORRO_E_RANGE
            assert b"frame payload" in L.lib().corro_last_error()
        for k, v in held.items():
            assert bool((v == SENTINEL).all()), k
        # one run fewer is the largest frame there is: the same context sizes it
        end[N] = 2 * N - 1
        o.nframes = o.nbytes = 0
        assert _call(eng, arr, o, 0) == 0
        assert (o.nframes, o.nbytes) == (N + 1, 56 * N + 4 + 32 + 20 * N)
        gfo = held["grp_frame_off"].cpu().tolist()
        assert gfo == [0, N, N + 1]
        del arr, start, end, zeros
        # and a small valid call on the same context is byte-exact
        got = S.plan_sync_requests(eng, [[{U.ACTORS[0]: [S.Full(12, 20)]}]])
        assert got == [[[(0, U.frame_bytes(U.ACTORS[0], [("F", 12, 20)]))]]]
    finally:
        eng.close()
