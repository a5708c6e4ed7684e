"""The generator behind the row query's random parity test, checked where no GPU is: its seeded predicates
must select something and not everything in at least half the cases, or the parity test would compare empty
answers. CPU only."""
from tests import query_gen as G

TABLE_SEED, KEYED_SEED = 11, 12


def test_history_has_every_kind_of_row():
    batches, rows = G.history()
    assert sum(len(t) for t in rows.values()) == 2000
    states = [s for t in rows.values() for s, _v in t.values()]
    assert states.count("dead") > 100 and states.count("live") > 1500
    assert len(batches[2]) > 0 and any(c[2] == 0 and c[3] == 1 for c in batches[0])      # resurrections, bare sentinels
    assert any(isinstance(c[8], (str, bytes)) and len(c[8]) > 16 for c in batches[0])    # long values
    assert any(pk >> 63 for pk in rows["ta"])                                            # negative pks


def test_the_seeded_predicates_are_selective_in_at_least_half_the_cases():
    _batches, rows = G.history()
    assert G.interesting_share(rows, G.predicates(rows, 200, TABLE_SEED)) >= 0.5
    assert G.interesting_share(rows, G.predicates(rows, 100, KEYED_SEED, keyed=True)) >= 0.5
