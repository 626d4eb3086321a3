"""The massive sub-peak clean-up on the device: the three piece drop-ins of consenrich_amd.cleanup over the whole case table
against the fixtures the reference's own functions made -- integers exact, floats by bit pattern, strings, key order and Python
types -- with the coordinates as a uniform step and as an edge array, node lengths on both sides of the LDS sort tile, and
several children in one call."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import cleanup_cases as CC  # noqa: E402
import cleanup_compare as CMP  # noqa: E402

from consenrich_amd import _lib as L  # noqa: E402
from consenrich_amd import cleanup as K  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("coords", ["auto", "edges"])
@pytest.mark.parametrize("name", CMP.force_ids())
def test_force_drop_in_matches_the_reference(monkeypatch, name, coords):
    monkeypatch.setattr(K, "COORDS", coords)
    before = dict(K.STATS)
    CMP.check_force(K.force_massive_subpeak_segments, name)
    calls = len(next(c for c in CC.FORCE if c["name"] == name)["children"])
    assert K.STATS["calls"] - before["calls"] == calls and K.STATS["children"] - before["children"] == calls


@pytest.mark.parametrize("coords", ["auto", "edges"])
def test_piece_drop_ins_match_the_reference(monkeypatch, coords):
    monkeypatch.setattr(K, "COORDS", coords)
    CMP.check_splits(K.best_massive_subpeak_split)
    CMP.check_contracts(K.contract_massive_subpeak_segment)


def test_nonfinite_candidate_is_refused_with_the_references_text():
    with pytest.raises(ValueError) as e:
        K.force_massive_subpeak_segments(**CC.nonfinite_inputs())
    assert str(e.value) == "`scores` contains non-finite values"


def test_several_children_in_one_call():
    """One call, three children (the first in bin 0, the last ending in bin n - 1, the middle one no candidate) and a second call
    with a child beyond the sort tile next to short ones: the packed records are those of one call per child, in order."""
    for name, kids in (("ends", None), ("beyond_tile", [(0, 99), (100, 100 + 3 * K.SORT_TILE), (100 + 3 * K.SORT_TILE + 1, 3 * K.SORT_TILE + 299)])):
        case = next(c for c in CC.FORCE if c["name"] == name)
        kids = kids or case["children"]
        iv, en = CC.coords(case["widths"])
        edges = np.concatenate((iv, en[-1:]))
        row = (1500.0, 1000.0, 0.25, 2.0, case["cost"], 1, 8)
        seg, cnt = K.plan(L.CLEANUP_OP_FORCE, case["scores"], edges, 0, 0, kids, row)
        assert cnt["n_segments"].sum() == seg.size and seg["child"].tolist() == np.repeat(np.arange(len(kids)), cnt["n_segments"]).tolist()
        at = 0
        for k, (a, b) in enumerate(kids):
            one, c1 = K.plan(L.CLEANUP_OP_FORCE, case["scores"], edges, 0, 0, [(a, b)], row)
            mine = seg[at:at + one.size].copy()
            mine["child"] = 0
            assert mine.tobytes() == one.tobytes() and cnt[k].tobytes() == c1[0].tobytes(), (name, k)
            at += one.size
        # and with the coordinates as a step
        seg2, cnt2 = K.plan(L.CLEANUP_OP_FORCE, case["scores"], None, int(edges[0]), int(edges[1] - edges[0]), kids, row)
        assert seg2.tobytes() == seg.tobytes() and cnt2.tobytes() == cnt.tobytes()


@pytest.mark.parametrize("name", CMP.row_ids())
def test_rows_drop_in_under_a_policy_matches_the_reference(name):
    """`cleanup.solution_to_chrom_narrowpeak_rows`: rows, meta and export details of the reference under a width policy -- active,
    inactive, switched off, without a null, without a threshold, with a coordinate gap in front of a candidate."""
    from consenrich_amd import narrowpeak as P

    before = dict(P.STATS)
    CMP.check_rows(K.solution_to_chrom_narrowpeak_rows, name)
    assert P.STATS["decided_on_host"] == before["decided_on_host"]
