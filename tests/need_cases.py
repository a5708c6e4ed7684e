"""Case builders for the need diff's edge tests, shared by the host model's CPU test
(tests/test_need_model.py) and the GPU test (tests/test_gpu_need_edges.py), so both see the same
entries. A case is an (our, their) pair of tests.sync_util.entries_from_pairs.

Domain: their-need ranges and their seq ranges with start > end are left out everywhere: the
reference removes them from a RangeInclusiveSet, and RangeInclusiveSet::remove asserts start <= end
(the peer's message panics the reference before any need is computed). Ranges of OURS may be
inverted: they only go through overlapping(), which compares bounds as given.

Every entry built here has at most one need range of ours and at most one seq range per partial of
ours unless its ranges are disjoint, so its needs never exceed corro_needs_bound and the packed form
takes all of them (overlapping ranges of THEIRS only ever lower the count).
"""
import itertools

import numpy as np

from tests.sync_util import entries_from_pairs

H = 30          # their head of the directed families
I63 = 2 ** 63 - 1
U64 = 2 ** 64 - 1

# LDS caps of the need kernels: NEEDS_CAP_R / _O / _P / _S in corrosion_amd/csrc/sync_needs.hip
CAP_R, CAP_O, CAP_P, CAP_S = 576, 800, 64, 160
NEEDS_T = 256   # entries per workgroup


def side(head, need=(), partials=None):
    return {"head": head, "need": [list(r) for r in need],
            "partials": {str(v): [list(r) for r in rs] for v, rs in (partials or {}).items()}}


def _edge_ranges(edges, top, lo=1):
    """Ranges of ours around `edges`: starting or ending at an edge, at edge +- 1, at lo, at top and
    at top + 1, and inverted [t + k, t] for k = 1, 2 around each edge (under a have range too)."""
    pts = {lo, top, top + 1}
    for e in edges:
        pts.update(p for p in (e - 1, e, e + 1) if p >= 0)
    out = [(lo - 1 if lo else 0, top + 1)]
    for p in sorted(pts):
        out.append((p, p))
        if p >= lo:
            out.append((lo, p))
        if p <= top + 1:
            out.append((p, top + 1))
    for e in sorted(edges):
        # t and t + k on either side of the edge, astride it, and both inside what lies next to it
        for t in (e - 3, e - 2, e - 1, e, e + 1):
            if t >= 0:
                out.extend([(t + 1, t), (t + 2, t)])
    return list(dict.fromkeys(out))


def hole_configs():
    """(name, their need ranges, their partials) of the Holes family."""
    two = {"touching": [(3, 5), (6, 8)], "overlapping": [(3, 7), (5, 9)], "nested": [(2, 20), (5, 6)],
           "duplicate": [(4, 9), (4, 9)]}
    geo = []
    for name, rs in two.items():
        geo += [(name, rs), (name + "-rev", rs[::-1])]
    chain3, chain4 = [(3, 4), (5, 6), (7, 8)], [(3, 4), (5, 6), (7, 8), (9, 10)]
    geo += [("chain3", chain3), ("chain3-rev", chain3[::-1]), ("chain4", chain4), ("chain4-rev", chain4[::-1])]
    for i, p in enumerate(itertools.permutations([(2, 20), (5, 6), (18, 25)])):
        geo.append(("mixed3-%d" % i, list(p)))
    cfg = [(n, rs, {}) for n, rs in geo]
    # the same geometry with one partial of theirs, which takes the holes out of registers
    cfg += [(n + "+partial", rs, {28: []}) for n, rs in geo if len(rs) <= 3]
    k = 4
    for n, r in (("from0", (0, k)), ("to-head", (k, H)), ("across-head", (k, H + 5)),
                 ("above-head", (H + 1, H + 9)), ("no-haves", (1, H)), ("head-only", (H, H))):
        cfg.append((n, [r], {}))
    for n, v in (("partial@1", 1), ("partial@head", H), ("partial-above-head", H + 3)):
        cfg.append((n, [], {v: []}))
    cfg += [("partial-in-need", [(5, 9)], {7: []}), ("partial-after-need", [(5, 9)], {10: []}),
            ("partial-before-need", [(5, 9)], {4: []})]
    return cfg


def holes_family():
    pairs = []
    for _, rs, parts in hole_configs():
        their = side(H, rs, parts)
        edges = {x for r in rs for x in r} | set(parts)
        for r in _edge_ranges(edges, H):
            pairs.append((side(H, [r]), their))
    return pairs


def heads_family(top=H):
    """Heads and tails at `top`: their head, a hole and a range of ours ending there. top = H is the
    plain family, 2^63 - 1 the State decoder's limit, 2^64 - 1 what the direct ABI accepts."""
    pairs = []
    our_heads = lambda head: [None] + [h for h in (0, head - 1, head, head + 1, I63) if 0 <= h <= I63]
    their1 = [side(1), side(1, [(1, 1)]), side(1, [(0, 1)]), side(1, [(0, 0)]), side(1, [], {1: []}),
              side(1, [(1, 5)]), side(1, [(2, 9)])]
    for their in their1:
        for oh in our_heads(1):
            for r in [None, (1, 1), (0, 1), (1, 2), (0, 0), (2, 2), (2, 1), (1, 0)]:
                pairs.append((side(oh, [r] if r else []), their))
    holes = [[], [(top - 5, top)], [(top, top)], [(top - 8, top - 3)], [(top - 1, top - 1)],
             [(top - 5, top), (top - 9, top - 4)], [(top, top), (top - 2, top - 2), (top - 4, top - 4), (top - 6, top - 6)]]
    if top < U64:
        holes += [[(top - 2, top + 5)], [(top + 1, top + 1)]]
    tparts = [{}, {top: []}, {top - 1: []}]
    ours = [None, (top - 10, top), (top, top), (top - 1, top), (top - 6, top - 4), (1, top), (0, top),
            (top, top - 1), (top, top - 2), (top - 1, top - 2), (top - 2, top - 3)]
    if top < U64:
        ours += [(top - 3, top + 1), (top + 1, top + 1), (top + 1, top)]
    for hs in holes:
        for tp in tparts:
            their = side(top, hs, tp)
            for oh in (our_heads(top) if not hs or not tp else [None, min(top - 1, I63)]):
                for r in ours:
                    pairs.append((side(oh, [r] if r else []), their))
    return pairs


def our_partials_family():
    pairs = []
    tneed = [(10, 15)]
    vs = [0, 1, 5, 12, 20, H, H + 1]
    tseq_opts = [None, [], [(5, 9)]]
    oseq_opts = [[], [(3, 12)], [(0, 4), (20, 25)]]
    for v in vs:
        for ts in tseq_opts:
            their = side(H, tneed, {} if ts is None else {v: ts})
            for os_ in oseq_opts:
                for oh in (H, None):
                    pairs.append((side(oh, [], {v: os_}), their))
    # every version at once, so that the order and the seq offsets of several partials show
    for ts in tseq_opts[1:]:
        their = side(H, tneed, {v: ts for v in vs})
        for os_ in oseq_opts:
            pairs.append((side(7, [(2, 11)], {v: os_ for v in vs}), their))
    return pairs


def seq_configs():
    two = {"touching": [(3, 5), (6, 8)], "overlapping": [(3, 7), (5, 9)], "nested": [(2, 20), (5, 6)],
           "duplicate": [(4, 9), (4, 9)], "unsorted-apart": [(12, 14), (3, 5)]}
    cfg = []
    for rs in two.values():
        cfg += [rs, rs[::-1]]
    cfg += [[(3, 4), (5, 6), (7, 8), (9, 10)], [(9, 10), (7, 8), (5, 6), (3, 4)], [(0, 4)], [(0, 0)],
            [(0, 4), (5, 9)], [(0, 40)], []]
    return cfg


def seq_diff_family():
    """Version 5 partial on both sides: our seq ranges against their seq holes over {0..=end}."""
    pairs = []
    for ts in seq_configs():
        their = side(H, [], {5: ts})
        edges = {x for r in ts for x in r}
        top = max([e for _, e in ts], default=6)
        seqs = _edge_ranges(edges, top, lo=0) + [(top + 3, top + 9), (top + 9, top + 3), (top + 2, top + 1)]
        for r in seqs:
            pairs.append((side(H, [], {5: [r]}), their))
        # several ranges of ours, disjoint and ascending, around their holes and above their max end
        pairs.append((side(H, [], {5: [(0, 2), (4, 6), (8, top + 4)]}), their))
        pairs.append((side(H, [], {5: [(1, 1), (top + 2, top + 2), (top + 7, top + 5)]}), their))
        pairs.append((side(H, [], {5: []}), their))
    return pairs


FAMILIES = {"holes": holes_family, "heads": heads_family, "heads@2^63-1": lambda: heads_family(I63),
            "heads@2^64-1": lambda: heads_family(U64), "our_partials": our_partials_family,
            "seq_diff": seq_diff_family}


def exhaustive_pairs():
    """Every entry over versions 0..5: 0, 1 or 2 ranges of theirs (start <= end, both orders), one
    range of ours (inverted included), their head 1..5, our head None / 2 / 9, with and without a
    partial of theirs at 3. Sides are shared between pairs; do not modify them."""
    V = range(6)
    tr = [(s, e) for s in V for e in V if s <= e]
    tneeds = [[]] + [[a] for a in tr] + [[a, b] for a in tr for b in tr]
    theirs = [side(h, rs, p) for rs in tneeds for h in range(1, 6) for p in ({}, {3: []})]
    ours = [side(oh, [(s, e)]) for s in V for e in V for oh in (None, 2, 9)]
    return [(o, t) for t in theirs for o in ours]


# ---- CSR plumbing: gather entries of one CSR dict by index (numpy, no per-entry Python) -------------

def _csr_take(off, idx):
    off = off.astype(np.int64)
    cnt = off[idx + 1] - off[idx]
    new = np.zeros(len(idx) + 1, np.int64)
    new[1:] = np.cumsum(cnt)
    src = np.repeat(off[idx] - new[:-1], cnt) + np.arange(int(new[-1]))
    return new.astype(np.uint64), src


def take_entries(ent, idx):
    """The CSR entries ent[idx[0]], ent[idx[1]], ... as a new CSR dict."""
    idx = np.asarray(idx, dtype=np.int64)
    out = {"their_head": ent["their_head"][idx], "our_head": ent["our_head"][idx]}
    for p in ("tn", "on"):
        out[p + "_off"], g = _csr_take(ent[p + "_off"], idx)
        out[p + "_start"], out[p + "_end"] = ent[p + "_start"][g], ent[p + "_end"][g]
    for p in ("tp", "op"):
        out[p + "_off"], g = _csr_take(ent[p + "_off"], idx)
        out[p + "_ver"] = ent[p + "_ver"][g]
        out[p + "s_off"], gs = _csr_take(ent[p + "s_off"], g)
        out[p + "s_start"], out[p + "s_end"] = ent[p + "s_start"][gs], ent[p + "s_end"][gs]
    return out


def plain_pairs(n=NEEDS_T, seed=3):
    """Ordinary entries: up to 2 sorted, disjoint need ranges per side and no partials, so that a
    workgroup of them stays below every LDS cap."""
    rng = np.random.default_rng(seed)
    def one(head):
        need, x = [], 1
        for _ in range(int(rng.integers(0, 3))):
            s = x + int(rng.integers(1, 30))
            e = s + int(rng.integers(0, 12))
            need.append((s, e))
            x = e + 2
        return side(head, need)
    return [(one(None if rng.random() < 0.1 else int(rng.integers(0, 120))), one(int(rng.integers(1, 120))))
            for _ in range(n)]


def ballast_pair(kind):
    """One entry that alone exceeds an LDS cap of its workgroup: `kind` is tn / on (need ranges of
    theirs / ours above CAP_R) or tp / op (partial versions above CAP_P)."""
    ranges = [(3 * k + 2, 3 * k + 3) for k in range(CAP_R + 24)]
    parts = {5 * k + 1: [(k, k + 2)] for k in range(CAP_P + 1)}
    head = 3 * (CAP_R + 30)
    if kind == "tn":
        return side(40, [(1, head)]), side(head, ranges)
    if kind == "on":
        return side(40, ranges), side(head, [(7, 9)])
    if kind == "tp":
        return side(40, [(1, head)], {6: [(0, 9)], 7: [(1, 2)]}), side(head, [], parts)
    if kind == "op":
        return side(40, [], parts), side(head, [(4, 8)], {6: [(1, 1)], 11: [(2, 2)]})
    raise ValueError(kind)


PLACEMENTS = ("alone", "lane0", "lane255", "ballast-tn", "ballast-on", "ballast-tp", "ballast-op", "final")


def place(pairs, placement):
    """The launches (CSR dicts) that run `pairs` under a placement, each with the positions of the
    directed entries in it:
      alone      the family by itself, one launch
      lane0 / lane255   every case as the first / last lane of a full workgroup of plain entries
      ballast-K  every case in a workgroup of plain entries plus one ballast entry over cap K
      final      the cases, 255 at a time, as the final, partial workgroup after a plain one
    """
    n = len(pairs)
    if placement == "alone":
        return [(entries_from_pairs(pairs), np.arange(n))]
    plain = plain_pairs()
    if placement == "final":
        out = []
        for a in range(0, n, NEEDS_T - 1):
            chunk = pairs[a:a + NEEDS_T - 1]
            out.append((entries_from_pairs(plain + chunk), NEEDS_T + np.arange(len(chunk))))
        return out
    extra = [ballast_pair(placement[8:])] if placement.startswith("ballast-") else []
    base = entries_from_pairs(pairs + plain + extra)
    fill = n + np.arange(NEEDS_T - 1)          # 255 plain entries
    if extra:
        fill[100] = n + NEEDS_T                # the ballast, in the middle of the workgroup
    lane = 0 if placement == "lane0" else NEEDS_T - 1 if placement == "lane255" else 17
    idx = np.empty((n, NEEDS_T), np.int64)
    idx[:, :lane] = fill[:lane]
    idx[:, lane] = np.arange(n)
    idx[:, lane + 1:] = fill[lane:]
    return [(take_entries(base, idx.reshape(-1)), lane + NEEDS_T * np.arange(n))]


# ---- LDS cap boundaries -----------------------------------------------------------------------------

CAP_KINDS = ("R-theirs", "R-ours", "P-theirs", "P-ours", "S-theirs", "S-ours", "O", "middle")


def _spread(total, n):
    return [total // n + (1 if i < total % n else 0) for i in range(n)]


def _ranges(rng, cnt, x=1):
    out = []
    for _ in range(cnt):
        s = x + int(rng.integers(1, 4))
        e = s + int(rng.integers(0, 3))
        out.append((s, e))
        x = e + 2
    return out


def _middle(kind, total, rng):
    """256 entries whose workgroup total of `kind` is exactly `total`, every other total below its cap."""
    pairs = []
    if kind in ("R-theirs", "R-ours"):
        for c in _spread(total, NEEDS_T):
            dense, few = _ranges(rng, c), _ranges(rng, int(rng.integers(0, 3)), int(rng.integers(1, 9)))
            t, o = (dense, few) if kind == "R-theirs" else (few, dense)
            pairs.append((side(int(rng.integers(0, 12)), o), side(5 * c + 9, t)))
    elif kind == "O":
        # no hole of theirs: every range of ours is one Full, and no head of ours adds the tail
        for c in _spread(total - NEEDS_T, NEEDS_T):
            pairs.append((side(None, _ranges(rng, c)), side(400)))
    else:
        theirs = kind in ("P-theirs", "S-theirs", "middle")
        if kind.startswith("P-"):
            np_, seqs = total, _spread(2 * total - 5, total)
        elif kind == "middle":
            np_, seqs = CAP_P, _spread(total, CAP_P)
        else:
            np_, seqs = 40, _spread(total, 40)
        for i in range(NEEDS_T):
            if i % 3 or i // 3 >= np_:     # every third entry carries one partial
                pairs.append((side(int(rng.integers(0, 30)), _ranges(rng, 1)), side(25, _ranges(rng, 2))))
                continue
            v = 2 + i % 20
            a = i % 2
            heavy = {v: [(2 * a + 4 * k, 2 * a + 4 * k + 1) for k in range(seqs[i // 3])]}
            # most partials meet one of the other side at their version (the seq diff), the
            # workgroup's last one among them: its seq ranges end at the last staged seq offset
            light = {} if i % 4 == 2 else {v: [(1, 6)] if a else [(0, 2), (5, 4 * seqs[i // 3] + 3)]}
            op, tp = (light, heavy) if theirs else (heavy, light)
            pairs.append((side(9, [(1, 40)], op), side(25, [(3, 4)], tp)))
    assert len(pairs) == NEEDS_T
    return pairs


_COUNT = {"R-theirs": lambda e, a, b: int(e["tn_off"][b]) - int(e["tn_off"][a]),
          "R-ours": lambda e, a, b: int(e["on_off"][b]) - int(e["on_off"][a]),
          "P-theirs": lambda e, a, b: int(e["tp_off"][b]) - int(e["tp_off"][a]),
          "P-ours": lambda e, a, b: int(e["op_off"][b]) - int(e["op_off"][a]),
          "S-theirs": lambda e, a, b: int(e["tps_off"][int(e["tp_off"][b])]) - int(e["tps_off"][int(e["tp_off"][a])]),
          "S-ours": lambda e, a, b: int(e["ops_off"][int(e["op_off"][b])]) - int(e["ops_off"][int(e["op_off"][a])])}
_COUNT["middle"] = _COUNT["S-theirs"]
_THEIRS = ("R-theirs", "P-theirs", "S-theirs", "middle")
_CAP = {"R-theirs": CAP_R, "R-ours": CAP_R, "P-theirs": CAP_P, "P-ours": CAP_P, "S-theirs": CAP_S,
        "S-ours": CAP_S, "O": CAP_O, "middle": CAP_S}


def _bump(pair, kind):
    """One more element of `kind` in a plain pair (flips the parity of the first workgroup's total)."""
    our, their = pair
    tgt = their if kind in _THEIRS else our
    tgt = dict(tgt, need=list(tgt["need"]), partials=dict(tgt["partials"]))
    if kind.startswith("R-"):
        tgt["need"].append([900 + 10 * len(tgt["need"]), 905 + 10 * len(tgt["need"])])
    else:
        tgt["partials"][str(77 + len(tgt["partials"]))] = [[1, 2]]
    return (our, tgt) if kind in _THEIRS else (tgt, their)


def cap_launches(kind):
    """Launches of three workgroups around a cap: (label, CSR dict, middle total, over) with the middle
    workgroup exactly at the cap and one past it; the first workgroup's total of the same kind odd
    and even (the middle segment starts at an odd and at an even CSR index), and the last workgroup
    with and without elements of that kind (the middle segment ends the array)."""
    cap = _CAP[kind]
    out = []
    for over in (0, 1):
        for odd in (0, 1):
            for tail in (1, 0):
                rng = np.random.default_rng(100 + 2 * over + odd)
                first = plain_pairs(seed=21)
                if kind[0] in "PSm":     # a few partials in the ordinary workgroups too
                    for i in (5, 90, 200):
                        first[i] = _bump(first[i], kind)
                last = plain_pairs(seed=22)
                if not tail:
                    strip = {"need": []} if kind.startswith("R-") else {"partials": {}}
                    last = [(o, dict(t, **strip)) if kind in _THEIRS else (dict(o, **strip), t) for o, t in last]
                mid = _middle(kind, cap + over, rng)
                if kind != "O":
                    cnt0 = _COUNT[kind](entries_from_pairs(first), 0, NEEDS_T)
                    if cnt0 % 2 != odd:
                        first[0] = _bump(first[0], kind)
                ent = entries_from_pairs(first + mid + last)
                if kind != "O":
                    assert _COUNT[kind](ent, 0, NEEDS_T) % 2 == odd
                    assert _COUNT[kind](ent, NEEDS_T, 2 * NEEDS_T) == cap + over, kind
                    if not tail:
                        assert _COUNT[kind](ent, 2 * NEEDS_T, 3 * NEEDS_T) == 0
                    if kind == "middle":
                        assert _COUNT["P-theirs"](ent, NEEDS_T, 2 * NEEDS_T) == CAP_P
                same = {kind, "S-theirs", "middle"} if kind in ("S-theirs", "middle") else {kind}
                for other, f in _COUNT.items():     # nothing else pushes a workgroup off the LDS path
                    for w in range(3):
                        if other not in same or w != 1:
                            assert f(ent, w * NEEDS_T, (w + 1) * NEEDS_T) <= _CAP[other], (kind, other, w)
                out.append(("%s=%d first-%s %s" % (kind, cap + over, "odd" if odd else "even",
                                                   "tail" if tail else "ends-array"), ent, cap + over, over))
    return out
