"""What corro_bookie_buffered_index derives and what corro_buffered_spans must give, restated as plain
loops, for the tests of the buffered serve path. Nothing here calls the code under test."""


def derive_tail_gaps(gaps, on_device):
    """needed() united with the on_device buffered versions, canonical again: sorted, disjoint, touching
    runs merged. gaps: [(s, e)]; on_device: [v]."""
    out = []
    for s, e in sorted(list(gaps) + [(v, v) for v in on_device]):
        if out and s <= out[-1][1] + 1:
            out[-1] = (out[-1][0], max(out[-1][1], e))
        else:
            out.append((s, e))
    return out


def is_canonical(ranges):
    return all(s <= e for s, e in ranges) and all(a[1] + 1 < b[0] for a, b in zip(ranges, ranges[1:]))


def hit(qs, qe, rs, re_):
    """The predicate of handle_need's partial branch, as serve._bookie_messages writes it."""
    return (qs <= rs <= qe) or (rs <= qs and re_ >= qe) or (rs <= qe and re_ >= qe) or (qs <= re_ <= qe)


def span_model(needs, index):
    """The spans corro_buffered_spans must give. needs: [(kind, site, start, end, seqs, keep, host, in_state,
    found)]; index: {site: {version: (on_device, last_seq, ts, [(rs, re)], [(pool_off, seq0, n)])}}. Returns
    (need_bspan_off, [(site, version, last_seq, ts, seq_start, seq_end, [pool rows])])."""
    off, spans = [0], []

    def add(site, v, ent, s, e):
        _dev, last, ts, _sr, segs = ent
        rows = []
        for po, q0, n in segs:
            rows += [po + (q - q0) for q in range(q0, q0 + n) if s <= q <= e]
        spans.append((site, v, last, ts, s, e, rows))

    for kind, site, start, end, seqs, keep, host, in_state, found in needs:
        book = index.get(site, {})
        if keep and not host:
            if kind == 0:
                for v in sorted(book):
                    if start <= v <= end and v not in found and book[v][0]:
                        for rs, re_ in book[v][3]:
                            add(site, v, book[v], rs, re_)
            elif not in_state and start in book and book[start][0]:
                for qs, qe in seqs:
                    for rs, re_ in book[start][3]:
                        if hit(qs, qe, rs, re_):
                            add(site, start, book[start], max(rs, qs), min(re_, qe))
        off.append(len(spans))
    return off, spans
