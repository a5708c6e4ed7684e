"""The need diff (corrosion_amd/csrc/sync_needs.hip) at its hole, head, seq-range and LDS-cap edges:
all four forms -- two-pass on host arrays, two-pass on device arrays, one-pass, packed -- array for
array against the oracle, and for the directed families against the host model too
(tests/need_model.py; tests/test_need_model.py holds model == oracle on the same entries).

The caps below are NEEDS_CAP_R / _O / _P / _S of sync_needs.hip, named once in tests/need_cases.py.
"""
from functools import lru_cache

import numpy as np
import pytest

from oracle import oracle as O
from tests import need_cases as NC
from tests import need_model as M
from tests.need_cases import CAP_O, CAP_P, CAP_R, CAP_S  # noqa: F401  (sync_needs.hip: NEEDS_CAP_*)
from tests.sync_util import decode_needs, entries_from_pairs

pytestmark = pytest.mark.gpu
KEYS = ("need_off", "seq_off", "kind", "start", "end", "sr_off", "sr_n", "s_start", "s_end")


@lru_cache(maxsize=1)
def _engine():
    import corrosion_amd as ca
    return ca.MergeEngine({"t": ["a"]}, capacity_hint=1024)


def _to_dev(ent):
    import torch
    return {k: torch.from_numpy(np.ascontiguousarray(v).view(np.int64)).cuda() for k, v in ent.items()}


def _host(res):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)) for k, v in res.items()}


def run_forms(ent):
    """The CSR result of every form of the need diff."""
    from corrosion_amd.sync import _needs_device, _needs_device_1pass, _needs_device_packed, packed_to_csr
    e, dev = _engine(), _to_dev(ent)
    return {"two-pass host": e.compute_needs(ent),
            "two-pass device": _host(_needs_device(e, dev)),
            "one-pass": _host(_needs_device_1pass(e, dev)),
            "packed": packed_to_csr(_needs_device_packed(e, dev))}


def check_forms(ent, exp, label):
    for form, got in run_forms(ent).items():
        for k in KEYS:
            a, b = np.asarray(got[k]).astype(np.uint64), exp[k].astype(np.uint64)
            if a.shape != b.shape or not np.array_equal(a, b):
                n = len(ent["their_head"])
                dg, de = decode_needs(got, n), decode_needs(exp, n)
                bad = [i for i in range(n) if dg[i] != de[i]]
                raise AssertionError("%s, %s: %s differs; first entries %s: got %s, oracle %s" % (
                    label, form, k, bad[:5], [dg[i] for i in bad[:3]], [de[i] for i in bad[:3]]))


@lru_cache(maxsize=None)
def _family(name):
    pairs = NC.FAMILIES[name]()
    return pairs, M.needs(pairs)


@pytest.mark.parametrize("placement", NC.PLACEMENTS)
@pytest.mark.parametrize("family", list(NC.FAMILIES))
def test_directed_family(family, placement):
    pairs, model = _family(family)
    seen = 0
    for ent, pos in NC.place(pairs, placement):
        exp = O.needs(ent)
        n = len(ent["their_head"])
        # the oracle's needs of the directed entries are the model's (whole launch when alone)
        if placement in ("alone", "final"):
            dec = decode_needs(exp, n)
            assert [dec[int(p)] for p in pos] == model[seen:seen + len(pos)]
        else:
            sub = NC.take_entries(ent, pos)
            assert decode_needs(O.needs(sub), len(pos)) == model[seen:seen + len(pos)]
        seen += len(pos)
        check_forms(ent, exp, "%s, %s" % (family, placement))
    assert seen == len(pairs)


def test_inverted_seq_range_of_ours():
    """Our partial 5 [(10, 3)] against their partial 5 [(20, 30)]: the seq have range 0..=19 spans
    [3, 10], so the reference's overlapping() keeps the range as is; (10, 3) under a hole does not."""
    pairs = [(NC.side(None, [], {5: [(10, 3)]}), NC.side(7, [], {5: [(20, 30)]})),
             (NC.side(None, [], {5: [(10, 3)]}), NC.side(7, [], {5: [(5, 6)]}))]
    assert M.needs(pairs) == [[("partial", 5, [(10, 3)]), ("full", 1, 7)], [("full", 1, 7)]]
    ent = entries_from_pairs(pairs)
    exp = O.needs(ent)
    assert decode_needs(exp, 2) == M.needs(pairs)
    check_forms(ent, exp, "inverted seq range")


@lru_cache(maxsize=1)
def _exhaustive():
    ent = entries_from_pairs(NC.exhaustive_pairs())
    return ent, O.needs(ent)


def test_exhaustive_small_universe():
    """Every entry over versions 0..5 (tests/need_cases.py: exhaustive_pairs), one launch per form."""
    ent, exp = _exhaustive()
    check_forms(ent, exp, "exhaustive")


@pytest.mark.parametrize("kind", NC.CAP_KINDS)
def test_cap_boundaries(kind):
    """Three workgroups, the middle one exactly at an LDS cap and one past it (the global-memory
    path; for `middle`, P = 64 with S = 161: staged need ranges, seq ranges read from global memory)."""
    for label, ent, total, over in NC.cap_launches(kind):
        exp = O.needs(ent)
        if kind == "O":
            assert int(exp["need_off"][2 * NC.NEEDS_T]) - int(exp["need_off"][NC.NEEDS_T]) == total
        check_forms(ent, exp, label)
