"""What corro_need_tails must give, restated as a plain loop over the versions, and the builders of its
input arrays that the tests share. Nothing here calls the code under test.

A case is the dict of input arrays the entry point takes (corro_tails_in's names, numpy): the decoded
needs, in_state, the extraction's groups and the book as a CSR over site ordinals."""
import numpy as np

FRAME = {0: 49, 1: 55}
DTYPES = {"kind": np.uint8, "start": np.uint64, "end": np.uint64, "need_keep": np.uint8, "need_site": np.uint32,
          "need_ent_off": np.uint64, "in_state": np.uint8, "grp_off": np.uint64, "version": np.int64,
          "gap_off": np.uint64, "gap_start": np.uint64, "gap_end": np.uint64, "buf_off": np.uint64,
          "buf_version": np.uint64}
DEC_KEYS = ("kind", "start", "end", "need_keep", "need_site", "need_ent_off")
BOOK_KEYS = ("gap_off", "gap_start", "gap_end", "buf_off", "buf_version")


class Case:
    """Needs one by one, then arrays(). book: {site: (gaps [(s, e)], buffered [v])} over nsites ordinals."""

    def __init__(self, book, nsites):
        self.book, self.nsites = book, nsites
        self.kind, self.start, self.end, self.keep, self.site, self.ins = [], [], [], [], [], []
        self.ent_off, self.grp_off, self.version = [0], [0], []

    def _need(self, kind, site, s, e, keep, ins):
        self.kind.append(kind); self.start.append(s); self.end.append(e)
        self.keep.append(keep); self.site.append(site); self.ins.append(ins)

    def _entry(self, versions):
        self.version += list(versions)
        self.grp_off.append(len(self.version))

    def full(self, site, s, e, found=(), keep=1):
        """A Full need; found: the versions the state returned (listed db_version DESC, as the extraction does)."""
        self._need(0, site, s, e, keep, 0)
        if keep:
            self._entry(sorted(found, reverse=True))
        self.ent_off.append(len(self.grp_off) - 1)
        return self

    def partial(self, site, v, in_state=0, nseq=1, keep=1):
        """A Partial need: its every-seq entry (one group when the version is in the state) and one entry
        per seq range."""
        self._need(1, site, v, v, keep, in_state if keep else 0)
        if keep:
            self._entry([v] if in_state else [])
            for _ in range(nseq):
                self._entry([v] if in_state else [])
        self.ent_off.append(len(self.grp_off) - 1)
        return self

    def arrays(self):
        gap_off, gs, ge, buf_off, bv = [0], [], [], [0], []
        for site in range(self.nsites):
            gaps, buffered = self.book.get(site, ([], []))
            gs += [s for s, _ in gaps]
            ge += [e for _, e in gaps]
            gap_off.append(len(gs))
            bv += list(buffered)
            buf_off.append(len(bv))
        a = {"kind": self.kind, "start": self.start, "end": self.end, "need_keep": self.keep, "need_site": self.site,
             "need_ent_off": self.ent_off, "in_state": self.ins, "grp_off": self.grp_off, "version": self.version,
             "gap_off": gap_off, "gap_start": gs, "gap_end": ge, "buf_off": buf_off, "buf_version": bv}
        return {k: np.asarray(v, DTYPES[k]) for k, v in a.items()}


def runs(versions):
    """Ascending versions -> their maximal runs [(s, e)]."""
    out = []
    for v in versions:
        if out and out[-1][1] + 1 == v:
            out[-1] = (out[-1][0], v)
        else:
            out.append((v, v))
    return out


def model(a, table_sites):
    """The rules of serve._bookie_messages for the needs that touch nothing buffered, one version at a
    time. a: a case's arrays; table_sites: ids in the engine's site table. Returns (need_tail_off,
    need_host, [(site, start, end)] in need order then ascending)."""
    nbook = len(a["gap_off"]) - 1
    off, host, ranges = [0], [], []
    for t in range(len(a["kind"])):
        site, s, e = int(a["need_site"][t]), int(a["start"][t]), int(a["end"][t])
        h, rs = 0, []
        if a["need_keep"][t] and site < nbook and site < table_sites:
            g0, g1 = int(a["gap_off"][site]), int(a["gap_off"][site + 1])
            gaps = [(int(a["gap_start"][g]), int(a["gap_end"][g])) for g in range(g0, g1)]
            P = {int(v) for v in a["buf_version"][int(a["buf_off"][site]):int(a["buf_off"][site + 1])]}

            def in_gap(v):
                return any(x <= v <= y for x, y in gaps)
            if a["kind"][t] == 0:
                k = int(a["need_ent_off"][t])
                F = {int(v) for v in a["version"][int(a["grp_off"][k]):int(a["grp_off"][k + 1])]}
                if any(v in P and v not in F for v in range(s, e + 1)):
                    h = 1
                else:
                    rs = runs([v for v in range(s, e + 1) if v not in F and v not in P and not in_gap(v)])
            elif not a["in_state"][t]:
                if s in P:
                    h = 1
                elif not in_gap(s):
                    rs = [(s, s)]
        ranges += [(site, x, y) for x, y in rs]
        off.append(len(ranges))
        host.append(h)
    return off, host, ranges


def frames(ranges, site_ids, payload=0, cluster_id=0):
    """The wire bytes of the ranges: wire.frames over ChangeV1(actor, Empty(versions, ts=None))."""
    from corrosion_amd import wire
    from corrosion_amd.agent import ChangeV1, Empty
    msgs = [ChangeV1(site_ids[site], Empty(versions=(s, e), ts=None)) for site, s, e in ranges]
    if payload == wire.PAYLOAD_SYNC:
        return wire.frames(msgs, wire.PAYLOAD_SYNC)
    return b"".join(wire.frame(wire.encode_uni_change(cv, cluster_id)) for cv in msgs)


def random_case(rng, nsites=4, table_sites=4):
    """A seeded book and up to 40 needs over versions below 200. A site's buffered versions lie outside
    its gaps; a Full need finds a random part of its versions, a buffered one among them more often than
    not (a version whose first seqs are applied and whose rest is buffered)."""
    book = {}
    for site in range(nsites):
        if rng.random() < 0.15:
            continue
        gaps, v = [], int(rng.integers(1, 40))
        while v < 190 and rng.random() < 0.7:
            e = v + int(rng.integers(0, 6))
            gaps.append((v, e))
            v = e + 2 + int(rng.integers(0, 50))
        free = [x for x in range(1, 200) if not any(s <= x <= e for s, e in gaps)]
        buffered = sorted(int(x) for x in rng.choice(free, size=int(rng.integers(0, 3)), replace=False))
        book[site] = (gaps, buffered)
    c = Case(book, nsites)
    for _ in range(int(rng.integers(1, 41))):
        site = int(rng.integers(0, nsites + 1))             # nsites: past the book
        keep = 0 if rng.random() < 0.1 else 1
        gaps, buffered = book.get(site, ([], []))
        if rng.random() < 0.7:
            s = int(rng.integers(1, 190))
            e = min(199, s + int(rng.integers(0, 30)))
            dense = rng.random()
            found = [v for v in range(s, e + 1) if rng.random() < dense and not any(x <= v <= y for x, y in gaps)
                     and v not in buffered]
            found += [v for v in buffered if s <= v <= e and rng.random() < 0.6]
            c.full(site, s, e, found, keep)
        else:
            v = int(rng.choice(buffered)) if buffered and rng.random() < 0.2 else int(rng.integers(1, 200))
            c.partial(site, v, int(rng.random() < 0.4 and v not in buffered), int(rng.integers(0, 3)), keep)
    return c.arrays()
