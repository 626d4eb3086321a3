"""Nested ROCCO refinement on the device against the fixtures made from the reference's own functions
(tests/golden/make_nested_golden.py), bit for bit: masks with array_equal, floats by bit pattern, integers and strings exactly.

  1. the two drop-ins (host arrays) on every case of tests/nested_cases.py;
  2. DeviceBatch.rocco_nested from uploaded resident scores and masks: several chains of different lengths in one call, one of
     them masked out, one with an empty mask; equal to the fixtures; rocco_runs / rocco_solution / best_segment_scores afterwards
     see the refined mask;
  3. a fitted batch: driver.nested_peaks_batch between first_pass_peaks_batch and score_peaks_batch, equal to the twin fed with
     the downloaded tracks; the fit's arrays, the score tracks and the templates are bit-equal afterwards."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import cases  # noqa: E402
import nested_cases as NC  # noqa: E402
import twin_nested as T  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(HERE, "golden", "nested")


def golden(kind, name):
    with np.load(os.path.join(GOLD, f"nested_{kind}.npz")) as z:
        return {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(name + "/")}


@pytest.fixture(scope="module")
def product():
    from consenrich_amd import _lib, nested

    _lib.require_gpu()
    return nested


@pytest.mark.parametrize("case", NC.SOLVE, ids=lambda c: c["name"])
def test_solver_drop_in_equals_the_reference(product, case):
    kw = NC.solve_inputs(case)
    mask, objective, details = product.solve_parent_conditioned_subpeaks(**kw)
    assert mask.dtype == np.bool_ and isinstance(objective, float)
    assert T.same_flat(T.flatten_solve(mask, objective, details), golden("solve", case["name"])) == []
    # every key of the reference's details, with its type (the twin's steps form is equal to the reference on this case)
    assert T.differences(details, T.solve(form="steps", **kw)[2]) == []


@pytest.mark.parametrize("case", NC.REFINE, ids=lambda c: c["name"])
def test_refinement_drop_in_equals_the_reference(product, case):
    kw = NC.refine_inputs(case)
    mask, details = product.refine_nested_rocco_solution(**kw)
    assert mask.dtype == np.uint8
    assert T.same_flat(T.flatten_refine(mask, details), golden("refine", case["name"])) == []
    want_mask, want = T.refine(form="steps", **kw)
    assert np.array_equal(mask, want_mask) and T.differences(details, want) == []


def test_solver_beyond_the_state_limit_is_a_value_error(product):
    x = np.linspace(-1.0, 1.0, 600)
    with pytest.raises(ValueError, match="`minRunBins` 256 exceeds the supported maximum 255"):
        product.solve_parent_conditioned_subpeaks(x, 0.1, 0.0, 256, requiredIndex=3)


BATCH = ["planted40", "dyadic", "empty_mask", "min_run_wide", "ragged", "selected_over_8192"]     # chain 4 (ragged) is masked out


def test_rocco_nested_of_resident_tracks_equals_the_reference(product):
    from consenrich_amd.batch import DeviceBatch, ModelParams

    table = [next(c for c in NC.REFINE if c["name"] == name) for name in BATCH]
    kws = [NC.refine_inputs(c) for c in table]
    # one call serves every chain with the same iteration settings: the cases differ in gamma, penalty and min_region_bins only,
    # so min_run_wide (min_region_bins 9) goes through a call of its own, the other chains masked out
    lens = [kw["scores"].size for kw in kws]
    with DeviceBatch(0) as b:
        b.configure(ModelParams(state_dim=2), 2, lens)
        for c, kw in enumerate(kws):
            b.upload_scores(c, kw["scores"])
        b.rocco(budget=0.1, gamma=0.5)
        for c, kw in enumerate(kws):
            b.upload_solution(c, kw["solution"])
        scores = [b.download_scores(c) for c in range(len(kws))]
        take = [True, True, True, False, False, True]
        got = b.rocco_nested([kw["gamma"] for kw in kws], [kw["selectionPenalty"] for kw in kws], chains=take)
        wide = b.rocco_nested([kw["gamma"] for kw in kws], [kw["selectionPenalty"] for kw in kws], min_region_bins=NC.WIDE_MIN_RUN,
                              chains=[False, False, False, True, False, False])
        got[3] = wide[3]
        assert got[4] is None and np.array_equal(b.rocco_solution(4), kws[4]["solution"])      # masked out: untouched
        for c in (0, 1, 2, 3, 5):
            mask = b.rocco_solution(c)
            assert T.same_flat(T.flatten_refine(mask, got[c]), golden("refine", BATCH[c])) == [], BATCH[c]
            st, en = b.rocco_runs(c)
            assert list(zip(st.tolist(), en.tolist())) == T.run_bounds(mask)
            leaves = sorted((n["start_idx"], n["end_idx"]) for n in got[c]["hierarchy"] if n["id"] in set(got[c]["leaf_node_ids"]))
            assert leaves == T.run_bounds(mask)
        assert got[2]["hierarchy"] == [] and got[2]["stop_reason"] == "mask_equal" and not b.rocco_solution(2).any()
        # the exported peaks of a scorer that takes the chain's runs are the refined ones
        views = {"z2": dict(threshold_z=2.0, threshold=0.5, null_scale=0.5, null_center=0.0)}
        rows = b.best_segment_scores(0, views)
        assert len(rows) == len(T.run_bounds(b.rocco_solution(0))) > len(T.run_bounds(kws[0]["solution"]))
        for c in range(len(kws)):
            assert np.array_equal(T.bits(b.download_scores(c)), T.bits(scores[c])), c
        # a second refinement starts from the refined mask
        again = b.rocco_nested(kws[0]["gamma"], kws[0]["selectionPenalty"], chains=[True] + [False] * 5)
        want_mask, want = T.refine(form="steps", **{**kws[0], "solution": T.refine(form="steps", **kws[0])[0]})
        assert np.array_equal(b.rocco_solution(0), want_mask) and T.differences(again[0], want) == []


def test_rocco_nested_with_coordinates_and_its_errors(product):
    from consenrich_amd import _lib as L
    from consenrich_amd.batch import DeviceBatch, ModelParams

    names = ["planted40_bp25", "mixed_widths"]
    kws = [NC.refine_inputs(next(c for c in NC.REFINE if c["name"] == name)) for name in names]
    with DeviceBatch(0) as b:
        b.configure(ModelParams(state_dim=2), 2, [kw["scores"].size for kw in kws])
        with pytest.raises(L.ConsenrichAMDError, match="chain 0 has no ROCCO solution"):
            b.rocco_nested(1.0, 0.3)
        for c, kw in enumerate(kws):
            b.upload_scores(c, kw["scores"])
        b.rocco(budget=0.1, gamma=0.5)
        for c, kw in enumerate(kws):
            b.upload_solution(c, kw["solution"])
        with pytest.raises(ValueError, match="`gamma` must be finite and non-negative"):
            b.rocco_nested(-1.0, 0.3)
        with pytest.raises(ValueError, match="`intervals` and `ends` must be supplied together"):
            b.rocco_nested(1.0, 0.3, intervals=[kw["intervals"] for kw in kws])
        for c, kw in enumerate(kws):
            assert np.array_equal(b.rocco_solution(c), kw["solution"])
        got = b.rocco_nested(1.0, 0.3, intervals=[kw["intervals"] for kw in kws], ends=[kw["ends"] for kw in kws], min_region_bp=125)
        for c, name in enumerate(names):
            assert T.same_flat(T.flatten_refine(b.rocco_solution(c), got[c]), golden("refine", name)) == [], name
            assert T.differences(got[c], T.refine(form="steps", **kws[c])[1]) == []


def test_nested_peaks_batch_on_a_fitted_batch_feeds_the_scorer(product):
    from consenrich_amd import _lib as L
    from consenrich_amd import driver, ess
    from consenrich_amd.batch import DeviceBatch, ModelParams

    lens, m, spans, seed, replays, step = [3001, 2049, 900], 3, [6, 3, 4], 5, 4, 25
    names = ("D", "xf", "Pf", "pnoise", "xs", "Ps", "lag")
    grid = (1.5, 2.0, 2.5, 3.0)
    with DeviceBatch(0) as b:
        b.configure(ModelParams(state_dim=2), m, lens)
        for c, n in enumerate(lens):
            b.upload(c, *cases.synth(n, m, 990 + c))
        b.stats()
        b.forward_backward(L.RETURN_NLL)
        b.export(L.EXPORT_FORWARD | L.EXPORT_SMOOTH)
        first = driver.first_pass_peaks_batch(b, dependence_spans=spans, threshold_z=2.0, threshold_z_grid=grid, num_bootstrap=9,
                                              random_seed=seed, gamma=-1.0, gamma_scale=0.5, score_mode="state", z=1.0, max_gap_bins=0)
        views = b.dwb_panel(threshold_z_grid=ess.resolve_z_grid(2.0, grid), bandwidths=spans, num_bootstrap=9, random_seed=seed,
                            calibration_quantile=0.9)
        scores = [b.download_scores(c) for c in range(3)]
        # chain 0's first pass selects nothing: plant the upper fifth of its scores instead, so that there is something to refine
        b.upload_solution(0, (scores[0] > np.quantile(scores[0], 0.8)).astype(np.uint8))
        first[0]["starts"], first[0]["ends"] = b.rocco_runs(0)
        fit = {(c, a): b.download(c, a) for c in range(3) for a in names}
        tmpls = [b.download_template(c) for c in range(3)]
        masks = [b.rocco_solution(c) for c in range(3)]
        cands = b.segment_candidates(views, dependence_spans=spans)
        nested = driver.nested_peaks_batch(b, first, interval_bp=step)
        changed = 0
        for c in range(3):
            iv = np.arange(lens[c], dtype=np.int64) * step
            want_mask, want = T.refine(scores[c], masks[c], first[c]["gamma"], first[c]["selection_penalty"], intervals=iv, ends=iv + step,
                                       minRegionBP=5 * step, minRegionBins=5, form="steps")
            assert np.array_equal(b.rocco_solution(c), want_mask), c
            assert T.differences(nested[c]["nested_rocco"], want) == [], c
            assert nested[c]["nested_rocco_stop_reason"] == want["stop_reason"]
            assert nested[c]["first_pass_selected_count"] == int(masks[c].sum())
            assert nested[c]["final_selected_count"] == int(want_mask.sum())
            assert list(zip(nested[c]["starts"].tolist(), nested[c]["ends"].tolist())) == T.run_bounds(want_mask)
            assert T.bits(nested[c]["objective"])[()] == T.bits(T.rocco_objective(scores[c], want_mask > 0, first[c]["gamma"], "steps"))[()]
            changed += int(not np.array_equal(want_mask, masks[c]))
        print("refined chains", changed, [r["nested_rocco_stop_reason"] for r in nested])
        assert changed >= 1
        got = driver.score_peaks_batch(b, nested, views, dependence_spans=spans, random_seed=seed, num_replay=replays)
        from_runs = b.dwb_peak_scoring(views, bandwidths=spans, num_replay=replays, random_seed=seed)
        for c in range(3):
            assert T.differences(got[c], from_runs[c]) == [], c
        # segment_candidates reads the score tracks only: the refinement leaves it as it was
        after = b.segment_candidates(views, dependence_spans=spans)
        for c in range(3):
            assert len(after[c][0]) == len(cands[c][0])
        for (c, a), v in fit.items():
            assert np.array_equal(b.download(c, a).view(np.uint32), v.view(np.uint32)), (c, a)
        for c in range(3):
            assert np.array_equal(T.bits(b.download_scores(c)), T.bits(scores[c])), c
            assert np.array_equal(T.bits(b.download_template(c)), T.bits(tmpls[c])), c


def test_nested_peaks_batch_without_layers_and_the_state_limit(product):
    """iters = 0 leaves the masks alone and still reports `_roccoObjectiveForSolution` of them; a minimum child run above the device's
    255 states is refused before anything is launched, so no mask is left partly refined."""
    from consenrich_amd import driver
    from consenrich_amd.batch import DeviceBatch, ModelParams

    kws = [NC.refine_inputs(next(c for c in NC.REFINE if c["name"] == name)) for name in ("planted40", "empty_mask", "min_run_255")]
    with DeviceBatch(0) as b:
        b.configure(ModelParams(state_dim=2), 2, [kw["scores"].size for kw in kws])
        for c, kw in enumerate(kws):
            b.upload_scores(c, kw["scores"])
        b.rocco(budget=0.1, gamma=0.5)
        for c, kw in enumerate(kws):
            b.upload_solution(c, kw["solution"])
        first = [dict(gamma=kw["gamma"], selection_penalty=kw["selectionPenalty"], objective=123.0, selected_count=-1) for kw in kws]
        got = driver.nested_peaks_batch(b, first, interval_bp=25, iters=0)
        for c, kw in enumerate(kws):
            want = T.rocco_objective(kw["scores"], kw["solution"] > 0, kw["gamma"], "steps")
            assert T.bits(got[c]["objective"])[()] == T.bits(want)[()] and got[c]["nested_rocco_stop_reason"] == "disabled"
            assert got[c]["final_selected_count"] == int(kw["solution"].sum())
            assert list(zip(got[c]["starts"].tolist(), got[c]["ends"].tolist())) == T.run_bounds(kw["solution"])
        assert b.rocco_objective(1.0, chains=[False, True, False]) == [None, 0.0, None]
        # chain 2 holds runs of 255, 256 and 300 bins: 256 states are one too many
        with pytest.raises(ValueError, match="`minRunBins` 256 exceeds the supported maximum 255"):
            b.rocco_nested(1.0, 0.3, min_region_bins=256)
        # mixed widths: at the median width (50 bp) 10 000 bp are 200 bins, at the smallest (1 bp) more than a run holds: the bound
        # refuses what a later layer could ask for
        width = np.where(np.arange(kws[2]["scores"].size) % 7 == 0, 1, 50).astype(np.int64)
        ends = np.cumsum(width)
        with pytest.raises(ValueError, match="`minRunBins` 256 exceeds the supported maximum 255"):
            b.rocco_nested(1.0, 0.3, intervals=[None, None, ends - width], ends=[None, None, ends], min_region_bp=10000,
                           chains=[False, False, True])
        for c, kw in enumerate(kws):
            assert np.array_equal(b.rocco_solution(c), kw["solution"])
