"""narrowPeak export on the device against the fixtures made from the reference's own functions
(tests/golden/make_narrowpeak_golden.py), bit for bit: integers exactly, floats by bit pattern, strings, key order and Python
types exactly.

  1. the drop-ins (host arrays) on every case of tests/narrowpeak_cases.py, against the fixtures;
  2. DeviceBatch.narrowpeak_rows from uploaded resident scores and masks of a fitted batch: six chains of different lengths in
     one call, one masked out, one with an empty mask, a second call with another min_subpeak_bins.  The signal and the
     uncertainty of the batch form are the fit's own (xs[:,0], sqrt(Ps00)), which no fixture made without a GPU can hold: the
     scores, masks and coordinates are the fixtures' cases, the expected rows the reference-steps twin (which
     tests/test_narrowpeak_twin.py holds equal to the fixtures) fed with the downloaded tracks.  Nothing resident changes;
  3. a fitted batch through first_pass_peaks_batch -> nested_peaks_batch -> export_peaks_batch -> score_peaks_batch, both state
     models and both score modes, equal to the twin fed with the downloaded tracks; the scorer is handed the exported peaks."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import cases  # noqa: E402
import narrowpeak_cases as NC  # noqa: E402
import twin_narrowpeak as T  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(HERE, "golden", "narrowpeak", "narrowpeak_rows.npz")


def golden(name):
    with np.load(GOLD) as z:
        return {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(name + "/")}


@pytest.fixture(scope="module")
def product():
    from consenrich_amd import _lib, narrowpeak

    _lib.require_gpu()
    return narrowpeak


@pytest.mark.parametrize("case", NC.CASES, ids=lambda c: c["name"])
def test_drop_in_equals_the_reference(product, case):
    kw = NC.inputs(case)
    before = dict(product.STATS)
    got = product.solution_to_chrom_narrowpeak_rows(**kw)
    assert type(got) is tuple and len(got) == (3 if kw["returnExportDetails"] else 2)
    with np.errstate(invalid="ignore"):
        want = T.rows(form="steps", **kw)
    if len(got) == 3:
        assert T.same_flat(T.flatten(got), golden(case["name"])) == []
    # every key, its order and its type (the twin's steps form is equal to the reference on this case)
    assert T.differences(got, want) == []
    for row in got[0]:
        assert [type(v) for v in row] == [str, int, int, str, int, str, float, int, int, int]
    # the cap on host decisions: the NaN chain and no other
    assert product.STATS["decided_on_host"] - before["decided_on_host"] == int(case["name"] in NC.HOST_DECIDED)


def test_pieces_equal_the_twin(product):
    for name in ("splits", "ties", "lengths_min5", "min_run_wide"):
        kw = NC.inputs(NC.case(name))
        for a, b in T.TN.run_bounds(kw["solution"] > 0):
            args = (kw["scores"][a:b + 1], kw["state"][a:b + 1], a, b, kw["subpeakSelectionPenalty"], kw["subpeakBoundaryCost"],
                    kw["minSubpeakBins"])
            got, want = product.solve_parent_conditioned_subpeak_segments(*args), T.segments(*args)
            assert T.TN.differences(got, want) == [] and [list(g) for g in got] == [list(w) for w in want], (name, a)
    kw = NC.inputs(NC.case("trims"))
    for a, b in T.TN.run_bounds(kw["solution"] > 0)[:3]:
        for k in (a, a + 4, b):
            for floor in (0.0, 0.5, None):
                assert product.trim_child_segment_around_summit(a, b, k, kw["scores"], floor) == T.trim(a, b, k, kw["scores"], floor)
    with pytest.raises(ValueError, match="`minRunBins` 256 exceeds the supported maximum 255"):
        product.solve_parent_conditioned_subpeak_segments(np.linspace(0, 1, 600), np.zeros(600), 0, 599, 0.1, 0.1, 256)


BATCH = ["word_edges", "splits", "trims", "medians", "empty_mask", "gaps"]      # chain 3 (medians) is masked out in the first call
FIT = ("D", "xf", "Pf", "pnoise", "xs", "Ps", "lag")


def _tracks(b, c):
    """signal and uncertainty as the reference's caller forms them from the downloaded fit"""
    return b.download(c, "xs")[:, 0].astype(np.float64), np.sqrt(b.download(c, "Ps")[:, 0, 0]).astype(np.float64)


def test_narrowpeak_rows_of_resident_tracks(product):
    from consenrich_amd import _lib as L
    from consenrich_amd.batch import DeviceBatch, ModelParams

    kws = [NC.inputs(NC.case(name)) for name in BATCH]
    lens = [kw["scores"].size for kw in kws]
    nc = len(kws)
    with DeviceBatch(0) as b:
        b.configure(ModelParams(state_dim=2), 2, lens)
        for c, n in enumerate(lens):
            b.upload(c, *cases.synth(n, 2, 770 + c))
        b.stats()
        b.forward_backward(L.RETURN_NLL)
        b.export(L.EXPORT_FORWARD | L.EXPORT_SMOOTH)
        for c, kw in enumerate(kws):
            b.upload_scores(c, kw["scores"])
        b.rocco(budget=0.1, gamma=0.5)
        for c, kw in enumerate(kws):
            b.upload_solution(c, kw["solution"])
            b.upload_template(c, NC.wave(lens[c], 40 + c))
        fit = {(c, a): b.download(c, a) for c in range(nc) for a in FIT}
        scores = [b.download_scores(c) for c in range(nc)]
        tmpls = [b.download_template(c) for c in range(nc)]
        pens = [kw["subpeakSelectionPenalty"] for kw in kws]
        gammas = [4.0 * kw["subpeakBoundaryCost"] for kw in kws]
        names = [f"chr{c + 1}" for c in range(nc)]
        common = dict(intervals=[kw["intervals"] for kw in kws], ends=[kw["ends"] for kw in kws], chroms=names, prefix="np")

        def expect(c, min_bins, unc=True):
            x, u = _tracks(b, c)
            return T.rows(names[c], kws[c]["intervals"], kws[c]["ends"], x, kws[c]["scores"], kws[c]["solution"], "np", 0.5,
                          uncertainty=u if unc else None, trimScoreFloor=0.0, subpeakSelectionPenalty=pens[c],
                          subpeakBoundaryCost=0.25 * gammas[c], minSubpeakBins=min_bins, returnExportDetails=True, form="steps")

        got = b.narrowpeak_rows(pens, gammas, chains=[True, True, True, False, True, True], **common)
        assert got[3] is None
        total = 0
        for c in (0, 1, 2, 4, 5):
            want = expect(c, 5)
            assert T.differences((got[c]["rows"], got[c]["peak_meta"], got[c]["export_details"]), want) == [], BATCH[c]
            assert got[c]["decided_on_host"] is False
            total += len(want[0])
        assert got[4]["rows"] == [] and got[4]["export_details"]["num_segments_kept"] == 0
        assert got[5]["export_details"]["num_coordinate_gap_splits"] == 1
        assert total > 10 and b.narrowpeak_stats["decided_on_host"] == 0 and b.narrowpeak_stats["chains"] == 5
        # another minimum run (the states-as-lanes kernel), the chain that was left out, no uncertainty
        wide = b.narrowpeak_rows(pens, gammas, min_subpeak_bins=NC.WIDE_MIN_RUN, chains=[True, False, False, True, False, False], **common)
        for c in (0, 3):
            want = expect(c, NC.WIDE_MIN_RUN)
            assert T.differences((wide[c]["rows"], wide[c]["peak_meta"], wide[c]["export_details"]), want) == [], BATCH[c]
        assert T.differences(wide[0]["peak_meta"], got[0]["peak_meta"]) != []
        plain = b.narrowpeak_rows(pens, gammas, use_uncertainty=False, chains=[False, False, False, True, False, False], **common)
        want = expect(3, 5, unc=False)
        assert T.differences((plain[3]["rows"], plain[3]["peak_meta"], plain[3]["export_details"]), want) == []
        assert want[2]["median_signal_local_p_filter_active"] is False
        # a minimum run beyond every parent is clamped to each parent's length, as the reference clamps it
        long = b.narrowpeak_rows(pens, gammas, min_subpeak_bins=300, chains=[True] + [False] * 5, **common)
        want = expect(0, 300)
        assert T.differences((long[0]["rows"], long[0]["peak_meta"], long[0]["export_details"]), want) == []
        with pytest.raises(ValueError, match="`exportFilterUncertaintyMultiplier` must be finite and non-negative"):
            b.narrowpeak_rows(pens, gammas, multiplier=-1.0, **common)
        # nothing resident has changed
        for c, kw in enumerate(kws):
            assert np.array_equal(b.rocco_solution(c), kw["solution"]), c
            assert np.array_equal(T.bits(b.download_scores(c)), T.bits(scores[c])), c
            assert np.array_equal(T.bits(b.download_template(c)), T.bits(tmpls[c])), c
        for (c, a), v in fit.items():
            assert np.array_equal(b.download(c, a).view(np.uint32), v.view(np.uint32)), (c, a)


@pytest.mark.parametrize("state_dim,mode", [(2, "state"), (2, "lower_confidence"), (1, "state"), (1, "lower_confidence")])
def test_export_peaks_batch_between_the_refinement_and_the_scorer(product, state_dim, mode):
    from consenrich_amd import _lib as L
    from consenrich_amd import driver, ess
    from consenrich_amd.batch import DeviceBatch, ModelParams

    lens, m, spans, seed, replays, step = [3001, 2049], 3, [6, 3], 5, 4, 25
    grid = (1.5, 2.0, 2.5, 3.0)
    mp = ModelParams(state_dim=2) if state_dim == 2 else ModelParams(state_dim=1, Q0=((1e-3, 0), (0, 0)))
    with DeviceBatch(0) as b:
        b.configure(mp, m, lens)
        for c, n in enumerate(lens):
            b.upload(c, *cases.synth(n, m, 990 + c))
        b.stats()
        b.forward_backward(L.RETURN_NLL)
        b.export(L.EXPORT_FORWARD | L.EXPORT_SMOOTH)
        first = driver.first_pass_peaks_batch(b, dependence_spans=spans, threshold_z=2.0, threshold_z_grid=grid, num_bootstrap=9,
                                              random_seed=seed, gamma=-1.0, gamma_scale=0.5, score_mode=mode, z=1.0, max_gap_bins=0)
        views = b.dwb_panel(threshold_z_grid=ess.resolve_z_grid(2.0, grid), bandwidths=spans, num_bootstrap=9, random_seed=seed,
                            calibration_quantile=0.9)
        scores = [b.download_scores(c) for c in range(2)]
        # chain 0's first pass may select nothing: plant the upper fifth of its scores instead, so that there is something to export
        b.upload_solution(0, (scores[0] > np.quantile(scores[0], 0.8)).astype(np.uint8))
        first[0]["starts"], first[0]["ends"] = b.rocco_runs(0)
        nested = driver.nested_peaks_batch(b, first, interval_bp=step)
        fit = {(c, a): b.download(c, a) for c in range(2) for a in ("xs", "Ps", "xf", "Pf")}
        masks = [b.rocco_solution(c) for c in range(2)]
        tmpls = [b.download_template(c) for c in range(2)]
        exported = driver.export_peaks_batch(b, nested, interval_bp=step, chroms=["chrA", "chrB"], prefix="cs")
        kept = 0
        for c in range(2):
            iv = np.arange(lens[c], dtype=np.int64) * step
            x, u = _tracks(b, c)
            want = T.rows(["chrA", "chrB"][c], iv, iv + step, x, scores[c], masks[c], "cs", 0.5, uncertainty=u, trimScoreFloor=0.0,
                          subpeakSelectionPenalty=nested[c]["selection_penalty"], subpeakBoundaryCost=0.25 * nested[c]["gamma"],
                          minSubpeakBins=5, returnExportDetails=True, form="steps")
            r = exported[c]
            assert T.differences((r["rows"], r["peak_meta"], r["export_details"]), want) == [], c
            assert r["decided_on_host"] is False
            assert r["starts"].tolist() == [q["start_idx"] for q in want[1]] and r["ends"].tolist() == [q["end_idx"] for q in want[1]]
            assert r["gamma"] == nested[c]["gamma"] and r["nested_rocco_stop_reason"] == nested[c]["nested_rocco_stop_reason"]
            kept += len(want[0])
            print("chain", c, want[2])
        assert kept >= 1
        # the scorer takes the exported peaks, not the mask's runs
        got = driver.score_peaks_batch(b, exported, views, dependence_spans=spans, random_seed=seed, num_replay=replays)
        direct = b.dwb_peak_scoring(views, bandwidths=spans, peaks=[(r["starts"], r["ends"]) for r in exported], num_replay=replays,
                                    random_seed=seed)
        for c in range(2):
            assert T.TN.differences(got[c], direct[c]) == [], c
        for (c, a), v in fit.items():
            assert np.array_equal(b.download(c, a).view(np.uint32), v.view(np.uint32)), (c, a)
        for c in range(2):
            assert np.array_equal(b.rocco_solution(c), masks[c])
            assert np.array_equal(T.bits(b.download_scores(c)), T.bits(scores[c])), c
            assert np.array_equal(T.bits(b.download_template(c)), T.bits(tmpls[c])), c
