"""The three request-serving paths of corrosion_amd.serve over their shared pipeline, on the small fixture of
tests/test_gpu_serve_requests.py: the stages each path times, the early return when the screen leaves no
need, and the case in which all three must return the same bytes."""
import pytest

from tests import req_decode_util as U
from tests.test_gpu_serve_requests import A0, A1, _agent, _changes, _msg, expected_answers, st  # noqa: F401

pytestmark = pytest.mark.gpu

PLAIN = {"book", "decode", "extract", "spans", "encode", "tails", "readback", "bookie"}
KEYS = {"handle_request_frames": PLAIN, "handle_request_frames_assembled": PLAIN | {"assemble"},
        "handle_request_frames_buffered": PLAIN | {"assemble", "buffered"}}


@pytest.mark.parametrize("path", sorted(KEYS))
def test_each_path_times_its_own_stages(st, path):  # noqa: F811
    from corrosion_amd import serve
    buf, off = U.cat([f for f, _ in st.frames])
    timings = {}
    status, got = getattr(serve, path)(st.a, buf.tobytes(), off, timings=timings)
    assert status.tolist() == [s for _, s in st.frames]
    assert got == expected_answers(st.a, st.frames)[0] and any(got)     # the host path, need by need
    assert set(timings) == KEYS[path]
    assert all(isinstance(v, float) and v >= 0 for v in timings.values())


@pytest.mark.parametrize("path", sorted(KEYS))
def test_nothing_left_after_the_screen(st, path):  # noqa: F811
    """A stranger's need and a malformed frame: no extraction entry is left, and only the book and the
    decode have run."""
    from corrosion_amd import serve
    frames = [st.frames[2], st.frames[3], st.frames[2]]
    buf, off = U.cat([f for f, _ in frames])
    timings = {}
    status, got = getattr(serve, path)(st.a, buf.tobytes(), off, timings=timings)
    assert status.tolist() == [s for _, s in frames]
    assert got == [b""] * 3
    assert set(timings) == {"book", "decode"}


def test_three_paths_coincide_without_buffered_versions(st):  # noqa: F811
    """On an agent that buffers nothing no need goes to the pool, so the plain, the assembled and the
    buffered path answer alike, here with the uni payload and small chunks; and as the host path does."""
    from corrosion_amd import serve
    from corrosion_amd.agent import ChangeV1, Full
    ag = _agent(bytes([0xC0]) * 16)
    msgs = [_msg(A0, 0, v) for v in list(range(1, 7)) + list(range(8, 15))] + [_msg(A1, 1, v) for v in range(1, 13)]
    msgs.append(ChangeV1(A1, Full(13, _changes(A1, 1, 2, dbv=13, cv=2), (0, 2), 2, ts=2013)))
    res = ag.process_multiple_changes(msgs)
    assert res.known.count("current") == len(msgs)
    assert serve.buffered_index(ag)["version"].size == 0
    kw = dict(max_buf_size=150, payload=1, cluster_id=513)
    buf, off = U.cat([f for f, _ in st.frames])
    got = [getattr(serve, path)(ag, buf.tobytes(), off, **kw) for path in sorted(KEYS)]
    assert got[0][0].tolist() == [s for _, s in st.frames]
    for status, answers in got[1:]:
        assert status.tolist() == got[0][0].tolist() and answers == got[0][1]
    assert got[0][1] == expected_answers(ag, st.frames, **kw)[0]
    assert sum(map(bool, got[0][1])) >= 3
