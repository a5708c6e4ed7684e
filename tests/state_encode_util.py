"""A bookie in a mixed state for the sync book and state encode tests, built through
Agent.process_multiple_changes (the only entry point that fills a bookie)."""
from tests.state_model import aid

ME = aid(900)
A, B, C_, D = aid(1), aid(2), aid(3), aid(4)


def _version(actor, v, nseq, seqs=None):
    """Version v of `actor`: nseq one-column changes (seq 0 .. nseq - 1), whole or the seqs [lo, hi] of it."""
    from corrosion_amd.agent import Change, ChangeV1, Full
    lo, hi = seqs or (0, nseq - 1)
    ch = [Change("t", 1000 * v + k, "a", k, 1, v, k, actor, 1) for k in range(lo, hi + 1)]
    return ChangeV1(actor, Full(v, ch, (lo, hi), nseq - 1, ts=10 + v))


def mixed_agent():
    """A: versions 1-2, 5 and 9 whole and 12 in two pieces of its ten seqs -> gaps (3,4), (6,8), (10,11) and an
    incomplete partial missing seq 0-1, 4-5 and 8-9 (the start, the middle, last_seq). B: version 1 whole,
    version 2 buffered in two pieces that cover it -> no gap, its only partial complete. C: version 1 without
    its seq 0 -> complete as is_complete() sees it (1..=last_seq). D: versions 1-3 whole -> a head alone."""
    import corrosion_amd as ca
    ag = ca.agent.Agent({"t": ["a"]}, capacity_hint=1 << 12, actor_id=ME)
    batch = [_version(A, v, 2) for v in (1, 2, 5, 9)] + [_version(A, 12, 10, (2, 3)), _version(A, 12, 10, (6, 7))]
    batch += [_version(B, 1, 2), _version(B, 2, 4, (0, 1)), _version(B, 2, 4, (2, 3))]
    batch += [_version(C_, 1, 4, (1, 3))]
    batch += [_version(D, v, 1) for v in (1, 2, 3)]
    ag.process_multiple_changes(batch)
    return ag
