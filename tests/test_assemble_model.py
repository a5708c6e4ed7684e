"""The model the GPU tests of corro_assemble_answers compare against (tests/assemble_util.model, the
two-pieces-per-need concatenation) against the join as serve.handle_request_frames writes it
(assemble_util.join, its per-need loop over numpy arrays), on seeded synthetic cases. No GPU."""
import numpy as np

from tests import assemble_util as U


def test_model_equals_the_host_join_on_seeded_cases():
    nonempty = frames = unkept = 0
    for seed in range(3000, 3300):
        a = U.random_case(np.random.default_rng(seed), hosts=False)
        buf, nao, fao, fh = U.model(a)
        want = U.join(a)
        assert [buf[fao[f]:fao[f + 1]] for f in range(len(want))] == want, seed
        assert fao[0] == 0 and fao[-1] == nao[-1] == len(buf) == sum(map(len, want)), seed
        assert fh == [0] * len(want), seed
        assert all(x <= y for x, y in zip(nao, nao[1:])) and len(nao) == len(a["need_keep"]) + 1
        nonempty += sum(1 for w in want if w)
        frames += len(want)
        unkept += int((a["need_keep"] == 0).sum())
    assert nonempty * 3 > frames and frames - nonempty > 300 and unkept > 1000, (nonempty, frames, unkept)


def test_model_on_a_case_by_hand():
    rng = np.random.default_rng(1)
    #        bytes tails keep host
    needs = [(5, 1, 1, 0), (0, 0, 0, 1), (3, 0, 1, 1), (0, 2, 1, 0), (0, 0, 1, 0), (7, 0, 1, 0)]
    a = U.build(needs, rng, payload=1, pairs=[2, 0, 3, 1], frames=[1, 0, 2, 1, 0], junk=2)
    buf, nao, fao, fh = U.model(a)
    assert nao == [0, 60, 60, 63, 173, 173, 180] and len(buf) == 180
    assert fao == [0, 60, 60, 173, 180, 180]
    assert fh == [0, 0, 1, 0, 0]                                  # the unkept host need of frame 0 does not count
    enc, tail = U.pieces(a)
    eb, tb = a["enc_buf"].tobytes(), a["tail_buf"].tobytes()
    assert buf[:5] == eb[enc[0][0]:enc[0][1]] and buf[5:60] == tb[110:165] and tail[0] == (110, 165)
    assert buf[60:63] == eb[enc[2][0]:enc[2][1]] and buf[63:173] == tb[165:275] and buf[173:] == eb[enc[5][0]:enc[5][1]]
    assert U.counts(a)["nranges"] == 7 and int(a["need_span_off"][0]) == 2 and int(a["enc_frame_off"][0]) == 2
    # without a span the encoder's arrays are not read
    b = U.build([(0, 1, 1, 0), (0, 0, 1, 0)], rng, split=False)
    b["span_frame_off"], b["need_span_off"] = np.zeros(1, np.uint64), np.zeros(3, np.uint64)
    assert U.counts(b)["nspans"] == 0 and U.model(b)[1] == [0, 49, 49]
