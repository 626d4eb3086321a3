"""CPU: the pure-Python twin of the multiscale candidate-segment native (tests/twin_segments.py) equals the compiled reference's
recorded outputs on every case of the table, bit for bit; its bin-by-bin form agrees on the short cases; the facts about the cap
case that the GPU test relies on hold; and the drop-in raises the reference's error before any GPU call."""
import os

import numpy as np
import pytest

import segments_cases as SC
import twin_segments as T

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(SC.__file__)), "segments")


class _Loop:
    cMultiscaleCandidateSegmentStats = staticmethod(T.loop_native)


@pytest.fixture(scope="module")
def golden():
    out = {}
    for g in SC.GROUPS:
        out.update(SC.load_group(os.path.join(GOLDEN, f"segments_{g}.npz")))
    return out


def test_every_case_has_a_fixture_and_no_fixture_is_large(golden):
    assert sorted(golden) == sorted(c["name"] for c in SC.cases())
    here = os.path.dirname(GOLDEN)
    largest_other = max(os.path.getsize(os.path.join(here, f)) for f in os.listdir(here) if os.path.isfile(os.path.join(here, f)))
    for g in SC.GROUPS:
        assert os.path.getsize(os.path.join(GOLDEN, f"segments_{g}.npz")) <= largest_other


@pytest.mark.parametrize("group", SC.GROUPS)
def test_twin_equals_the_reference(golden, group):
    bad = {c["name"]: d for c in SC.cases() if c["group"] == group
           for d in [SC.differences(SC.run_case(T, c), golden[c["name"]])] if d}
    assert bad == {}


def test_bin_by_bin_twin_equals_the_reference_on_the_short_cases(golden):
    short = [c for c in SC.cases() if c["n"] <= SC.FETCH + 1 or c["group"] == "special"]
    assert len(short) >= 20
    bad = {c["name"]: d for c in short for d in [SC.differences(SC.run_case(_Loop, c), golden[c["name"]])] if d}
    assert bad == {}


def test_the_degenerate_cases_are_what_the_table_says(golden):
    for name in ("empty_track", "no_views", "no_scales", "all_below"):
        assert int(golden[name]["rows"][0]) == 0 and list(golden[name]["counters"]) == [0, 0, 0], name
    tail = golden["last_bin_ends_a_run"]
    n = SC.TILE + 1
    assert int(tail["end"].max()) == n - 1
    # two low bins separate the last three bins from the two high bins before them: a gap of 1 does not bridge them
    assert np.any((tail["start"] == n - 3) & (tail["end"] == n - 1))
    dup = golden["scales_zero_dup_beyond"]
    assert sorted(set(int(s) for s in dup["scale"])) == [1, 5, SC.TILE + 1]
    # the fourth view's null scale clamps to DBL_MIN: excesses near 1e307 whose prefix overflows, and NaN from inf - inf
    case = next(c for c in SC.cases() if c["name"] == "table_n8193_run1_gap0")
    big = SC.run_case(T, case)
    assert SC.differences(big, golden[case["name"]]) == []
    v3 = big[3] == 3
    assert np.any(np.isinf(big[5][v3])) and np.any(np.isnan(big[4][v3])) and np.all(np.isfinite(big[4][~v3]))


def test_the_cap_case_has_a_tie_a_non_finite_view_and_views_the_select_decides(golden):
    case = next(c for c in SC.cases() if c["name"] == "cap16_n8193")
    x, sc, thr, ns = SC.inputs(case)
    over = SC.cap_probe(x, sc, thr, ns, case["min_run"], case["gap"], case["cap"])
    assert len(over) == 9 and int(golden["cap16_n8193"]["counters"][1]) == 9
    assert over[(1, 2)] == (24, True, True)
    assert over[(0, 3)][0] == 52 and not over[(0, 3)][1]
    assert sum(1 for v in over.values() if v[1] and not v[2]) >= 1
    assert int(golden["cap16_n8193"]["counters"][2]) == sum(v[0] - SC.CAP for v in over.values())


def test_the_twin_composition_caps_orders_and_counts():
    x = SC.scores(2000)
    views = {f"z{z:g}": dict(threshold_z=z, threshold=t, null_scale=s) for z, t, s in zip(SC.Z, SC.THRESHOLDS, (1.3, 1.3, 0.05, 0.7, 2.0))}
    cands, diag = T.multiscale_candidates(x, views, scale_bins=(1, 2, 5, 5, 3000), max_segments=40, max_segments_per_view=16)
    assert diag["total_cap_hit"] and diag["candidate_count"] == 40 == len(cands) and diag["per_view_cap_hit_count"] > 0
    assert diag["discarded_by_total_cap"] == diag["candidate_count_before_total_cap"] - 40
    keys = [(c["start_idx"], c["end_idx"], c["scale_bins"], c["threshold_key"]) for c in cands]
    assert keys == sorted(keys) and len(set(keys)) == 40
    assert T.resolve_scales(100, (0, 5, 5, 300)) == [1, 5, 100] and T.resolve_scales(50, None, 9) == [1, 4, 9]
    assert T.resolve_scales(0, (3,)) == [1]


def test_the_drop_in_raises_before_any_gpu_call():
    from consenrich_amd import segments

    with pytest.raises(ValueError, match="thresholds and nullScales must have the same length"):
        segments.cMultiscaleCandidateSegmentStats(np.zeros(4), [1], [0.0, 1.0], [1.0])
    with pytest.raises(OverflowError):
        segments.cMultiscaleCandidateSegmentStats(np.zeros(4), [1], [0.0], [1.0], 1 << 40)
    out = segments.cMultiscaleCandidateSegmentStats(np.zeros(0), [1], [0.0], [1.0])
    assert len(out) == 11 and out[0].dtype == np.int64 and out[4].dtype == np.float64 and out[8:] == (0, 0, 0)
    assert segments.resolve_scales(100, (0, 5, 5, 300)) == [1, 5, 100] and segments.resolve_scales(50, None, 9) == [1, 4, 9]
    from consenrich_amd import cconsenrich

    assert cconsenrich.cMultiscaleCandidateSegmentStats is segments.cMultiscaleCandidateSegmentStats
