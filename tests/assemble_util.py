"""What corro_assemble_answers must give, restated in numpy, and the builders of its input arrays that
the tests share. Nothing here calls the code under test.

A case is the dict of input arrays the entry point takes (corro_assemble_in's names, numpy) plus
"payload". The call parses no frame byte, so the buffers hold random bytes and the offsets are made up."""
import numpy as np

FRAME = {0: 49, 1: 55}
DTYPES = {"frame_pair_off": np.uint64, "pair_need_off": np.uint64, "need_keep": np.uint8, "need_span_off": np.uint64,
          "span_frame_off": np.uint64, "enc_frame_off": np.uint64, "enc_buf": np.uint8, "need_tail_off": np.uint64,
          "need_host": np.uint8, "tail_buf": np.uint8}
OFFSETS = ("frame_pair_off", "pair_need_off", "need_span_off", "span_frame_off", "enc_frame_off", "need_tail_off")
TILE = 8192          # the bytes of output one workgroup of k_as_copy owns (AS_TILE blocks of 16)
WINDOW = 512         # the longest window of piece offsets k_as_copy keeps in LDS (AS_WIN)


def pieces(a):
    """Per need, the (start, end) of its encoded piece in enc_buf and of its tail piece in tail_buf."""
    tfs = FRAME[a["payload"]]
    nso, nto = a["need_span_off"].astype(np.int64), a["need_tail_off"].astype(np.int64)
    T = len(a["need_keep"])
    if len(a["span_frame_off"]) > 1:                           # nspans > 0
        fo, sfo = a["enc_frame_off"].astype(np.int64), a["span_frame_off"].astype(np.int64)
        enc = [(int(fo[sfo[nso[t]]]), int(fo[sfo[nso[t + 1]]])) for t in range(T)]
    else:
        enc = [(0, 0)] * T
    return enc, [(tfs * int(nto[t]), tfs * int(nto[t + 1])) for t in range(T)]


def model(a):
    """(buf bytes, need_ans_off, frame_ans_off, frame_host): the two-pieces-per-need concatenation."""
    enc, tail = pieces(a)
    eb, tb = a["enc_buf"].tobytes(), a["tail_buf"].tobytes()
    parts, nao = [], [0]
    for (e0, e1), (r0, r1) in zip(enc, tail):
        parts += [eb[e0:e1], tb[r0:r1]]
        nao.append(nao[-1] + (e1 - e0) + (r1 - r0))
    fpo, pno = a["frame_pair_off"].astype(np.int64), a["pair_need_off"].astype(np.int64)
    first = [int(pno[fpo[f]]) for f in range(len(fpo))]
    fao = [nao[t] for t in first]
    fh = [int(any(a["need_keep"][t] and a["need_host"][t] for t in range(first[f], first[f + 1])))
          for f in range(len(fpo) - 1)]
    return b"".join(parts), nao, fao, fh


def join(a):
    """Per frame, the answer as serve.handle_request_frames joins it on the host (its loop after the
    read-back, over numpy arrays; no need here is the host bookie's)."""
    tfs = FRAME[a["payload"]]
    out, tail = a["enc_buf"].tobytes(), a["tail_buf"].tobytes()
    fo, sfo, nso, nto = a["enc_frame_off"], a["span_frame_off"], a["need_span_off"], a["need_tail_off"]
    answers = []
    for f in range(len(a["frame_pair_off"]) - 1):
        parts = []
        for p in range(int(a["frame_pair_off"][f]), int(a["frame_pair_off"][f + 1])):
            for t in range(int(a["pair_need_off"][p]), int(a["pair_need_off"][p + 1])):
                if not a["need_keep"][t]:
                    continue
                parts.append(out[int(fo[int(sfo[int(nso[t])])]):int(fo[int(sfo[int(nso[t + 1])])])])
                if not a["need_host"][t]:
                    parts.append(tail[tfs * int(nto[t]):tfs * int(nto[t + 1])])
        answers.append(b"".join(parts))
    return answers


def csr(sizes):
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, np.int64))]).astype(np.uint64)


def build(needs, rng, payload=0, pairs=None, frames=None, junk=0, split=True):
    """needs: [(encoded bytes, tail frames, need_keep, need_host)] in wire order; pairs: needs per pair
    (default: one pair); frames: pairs per frame (default: one frame). A need's encoded bytes are cut
    into 0..2 spans of 0..3 frames each (split = False: one span of one frame; no bytes: sometimes no
    span at all). junk > 0: that many unused spans, frames, ranges and bytes before the first need and
    after the last, so no offset array starts at 0 or ends at its bound."""
    T = len(needs)
    pairs = [T] if pairs is None else list(pairs)
    frames = [len(pairs)] if frames is None else list(frames)
    assert sum(pairs) == T and sum(frames) == len(pairs)
    spans_of, frames_of, flen, ntail = [], [], [], []
    for nbytes, nt, _keep, _host in needs:
        ns = int(rng.integers(1, 3)) if split else 1
        if nbytes == 0 and split and rng.integers(0, 2):
            ns = 0
        cuts = []
        for _ in range(ns):
            cuts.append(int(rng.integers(0, 4)) if split else 1)
        if nbytes and sum(cuts) == 0:
            cuts[0] = 1
        k = sum(cuts)
        edges = np.sort(rng.integers(0, nbytes + 1, max(k - 1, 0))) if k else np.zeros(0, np.int64)
        edges = np.concatenate([[0], edges, [nbytes]]) if k else np.zeros(1, np.int64)
        flen += np.diff(edges).astype(np.int64).tolist()
        spans_of.append(ns)
        frames_of += cuts
        ntail.append(nt)
    j = int(junk)
    tfs = FRAME[payload]
    a = {"payload": payload,
         "frame_pair_off": csr(frames), "pair_need_off": csr(pairs),
         "need_keep": np.array([n[2] for n in needs], np.uint8), "need_host": np.array([n[3] for n in needs], np.uint8),
         "need_span_off": csr(spans_of) + np.uint64(j), "need_tail_off": csr(ntail) + np.uint64(j)}
    nspans = sum(spans_of) + 2 * j
    a["span_frame_off"] = csr([1] * j + frames_of + [1] * j) + np.uint64(j) if nspans else np.zeros(1, np.uint64)
    a["enc_frame_off"] = csr([3] * (2 * j) + flen + [3] * (2 * j)) + np.uint64(j) if nspans else np.zeros(1, np.uint64)
    a["enc_buf"] = rng.integers(0, 256, int(a["enc_frame_off"][-1]) + j, dtype=np.uint8) if nspans else np.zeros(0, np.uint8)
    a["tail_buf"] = rng.integers(0, 256, tfs * (sum(ntail) + 2 * j), dtype=np.uint8)
    return a


def counts(a):
    """The scalar fields of corro_assemble_in for the case."""
    nspans = len(a["span_frame_off"]) - 1
    return {"nframes": len(a["frame_pair_off"]) - 1, "npairs": len(a["pair_need_off"]) - 1, "nneeds": len(a["need_keep"]),
            "nspans": nspans, "enc_nframes": len(a["enc_frame_off"]) - 1 if nspans else 0,
            "enc_nbytes": len(a["enc_buf"]) if nspans else 0, "nranges": len(a["tail_buf"]) // FRAME[a["payload"]],
            "tail_nbytes": len(a["tail_buf"]), "payload": a["payload"]}


def random_case(rng, max_frames=64, max_needs=300, hosts=True):
    """A seeded case: some frames without a pair, some pairs without a need, unkept needs (no bytes, by
    the construction of the real inputs), host needs (no tail), short and long pieces."""
    F = int(rng.integers(1, max_frames + 1))
    frames = rng.integers(0, 4, F).tolist()
    NP = sum(frames)
    pairs = rng.integers(0, 8, NP)
    while pairs.sum() > max_needs:
        pairs = pairs // 2
    T = int(pairs.sum())
    style = int(rng.integers(0, 3))                            # mostly tiny, mixed, or a few large pieces
    needs = []
    for _ in range(T):
        keep = int(rng.integers(0, 4) > 0)
        host = int(hosts and keep and rng.integers(0, 8) == 0)
        if not keep:
            needs.append((0, 0, 0, int(hosts and rng.integers(0, 2))))    # (a host flag on an unkept need counts for nothing)
            continue
        nb = int(rng.integers(0, (4, 70, 700)[style])) if rng.integers(0, 5) else 0
        if style == 2 and rng.integers(0, 30) == 0:
            nb = int(rng.integers(5000, 20000))
        nt = 0 if host or rng.integers(0, 2) else int(rng.integers(1, 4))
        needs.append((nb, nt, 1, host))
    return build(needs, rng, int(rng.integers(0, 2)), pairs.tolist(), frames, junk=int(rng.integers(0, 3)))
