"""GPU tests of the numeric side of the DWB peak scoring on the device (run with -m gpu).  Every float is compared by its 64-bit
pattern, every integer with ==.  References: the reference's recorded outputs (tests/golden/peakscore/peakscore_*.npz) and the
pure-Python twin (tests/twin_peakscore.py, pinned to those recordings by tests/test_peakscore_twin.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import cases
import peakscore_cases as PC
import twin_peakscore as T
from conftest import gpu_available

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "peakscore")


@pytest.fixture(scope="module")
def product():
    if not gpu_available():
        pytest.fail("GPU tests selected but no HIP device / library: the product has no CPU fallback")
    from consenrich_amd import peakscore

    return peakscore


@pytest.fixture(scope="module")
def golden():
    out = {}
    for name in ("segments", "pq"):
        with np.load(os.path.join(GOLDEN, f"peakscore_{name}.npz")) as z:
            out.update({k: z[k] for k in z.files})
    return out


def _differences(details, golden, name, views):
    keys = [k for k, v in views.items() if isinstance(v, dict)]
    bad = [f for f in T.NUMERIC if not np.array_equal(T.bits([d[f] for d in details]), T.bits(golden[f"{name}/{f}"]))]
    if [keys.index(d["threshold_key"]) for d in details] != list(golden[f"{name}/view"]):
        bad.append("view")
    return bad


# ---------------------------------------------------------------------------------------------------------------
# 1. segment scores
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", PC.segment_cases(), ids=lambda c: c["name"])
def test_segment_scores_of_a_host_array_equal_the_reference(product, golden, case):
    """n = 20 001: lengths 1, 7, 8, 9, 127, 128, 129, 8191, 8192, 8193 and 20 001 at two offsets each, a segment clamped at each
    end, four empty ones; four views (an exact tie, an all-NaN view behind a finite one, a null scale that clamps to DBL_MIN and
    gives inf), a NaN view in front, one view, a skipped entry.  n = 1, 9, 300: the short ends of the same."""
    x, (st, en), views = PC.track(case["n"]), PC.segments(case["n"]), PC.view_sets()[case["views"]]
    got = product.best_segment_scores(x, st, en, views)
    assert _differences(got, golden, case["name"], views) == []
    with np.errstate(all="ignore"):
        assert T.same_details(got, [T.best_score_steps(x, a, b, views) for a, b in zip(st, en)])


def test_segment_scores_of_a_resident_track_equal_the_reference(product, golden):
    """The same segments from the resident score tracks of a fitted batch: chain 1 holds the case table's track, chain 0 another
    one; the fit, the scores and the masks are bit-equal afterwards and starts=None takes the chain's ROCCO runs."""
    from consenrich_amd import _lib as L
    from consenrich_amd.batch import DeviceBatch, ModelParams

    n_list, m = [1031, PC.N_TRACK], 2
    names = ("D", "xf", "Pf", "pnoise", "xs", "Ps", "lag")
    views = PC.view_sets()["views4"]
    x, (st, en) = PC.track(), PC.segments()
    with DeviceBatch(0) as b:
        b.configure(ModelParams(state_dim=2), m, n_list)
        for c, n in enumerate(n_list):
            b.upload(c, *cases.synth(n, m, 900 + c))
        b.stats()
        b.forward_backward(L.RETURN_NLL)
        b.export(L.EXPORT_FORWARD | L.EXPORT_SMOOTH)
        b.rocco_scores("state")
        own = b.download_scores(0)
        b.upload_scores(1, x)
        b.rocco(budget=0.1, gamma=0.5)
        before = {(c, a): b.download(c, a) for c in range(2) for a in names}
        masks = [b.rocco_solution(c) for c in range(2)]
        got = b.best_segment_scores(1, views, st, en)
        assert _differences(got, golden, f"seg_n{PC.N_TRACK}_views4", views) == []
        plain = PC.view_sets()["skipped"]
        runs = b.rocco_runs(0)
        assert runs[0].shape[0] > 0
        got = b.best_segment_scores(0, plain)
        assert T.same_details(got, [T.best_score_steps(own, a, e, plain) for a, e in zip(*runs)])
        for (c, a), v in before.items():
            assert np.array_equal(b.download(c, a).view(np.uint32), v.view(np.uint32)), (c, a)
        assert np.array_equal(T.bits(b.download_scores(0)), T.bits(own)) and np.array_equal(T.bits(b.download_scores(1)), T.bits(x))
        for c in range(2):
            assert np.array_equal(b.rocco_solution(c), masks[c])
    with DeviceBatch(0) as b:
        b.configure(ModelParams(state_dim=2), 2, [10])
        with pytest.raises(L.ConsenrichAMDError, match="no scores"):
            b.best_segment_scores(0, views, [0], [1])


# ---------------------------------------------------------------------------------------------------------------
# 2. the p / q drop-ins on host arrays
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", PC.pq_cases(), ids=lambda c: c["name"])
def test_p_and_q_values_equal_the_reference(product, golden, case):
    """K in {0, 1, 33, 4097} x draws: none; one of one value; one empty; five (one empty) whose pool is one past a sort tile.
    Observed values copied from the pool, repeated, +0.0 and -0.0 on both sides, one above and one below the whole pool."""
    obs, draws = PC.pq_inputs(case)
    p = product.empirical_replay_segment_pvalues(obs, draws)
    q = product.replay_fdr_qvalues(obs, draws)
    assert p.dtype == q.dtype == np.float64 and p.shape == q.shape == obs.shape
    assert np.array_equal(T.bits(p), T.bits(golden[f"{case['name']}/p"]))
    assert np.array_equal(T.bits(q), T.bits(golden[f"{case['name']}/q"]))


def test_three_metrics_in_one_run_with_max_q_p_and_exceedances(product, golden):
    """What the scorer keeps: p, max(q, p) and the exceedance counts of three metrics from one device run."""
    case = dict(name="pq_k4097_r5", k=4097, draws="r5")
    obs, draws = PC.pq_inputs(case)
    pool = np.concatenate(draws)
    obs3 = np.stack([obs, obs * 2.0 + 1.0, -obs])
    pool3 = np.stack([pool, (pool * 2.0 + 1.0)[::-1], -pool])
    got = product.replay_pq(obs3, pool3, len(draws))
    for m in range(3):
        p, q, c = T.pq_device(obs3[m], pool3[m], len(draws))
        assert np.array_equal(T.bits(got["p"][m]), T.bits(p)), m
        assert np.array_equal(T.bits(got["q"][m]), T.bits(np.maximum(q, p))), m
        assert np.array_equal(got["exceedances"][m], c), m
    assert np.array_equal(T.bits(got["p"][0]), T.bits(golden["pq_k4097_r5/p"]))
    assert np.array_equal(T.bits(got["q"][0]), T.bits(np.maximum(golden["pq_k4097_r5/q"], golden["pq_k4097_r5/p"])))


def test_non_finite_statistics_raise_the_references_errors(product):
    from consenrich_amd import _lib as L

    obs, draws = PC.pq_inputs(dict(k=33, draws="r5"))
    bad_obs = obs.copy()
    bad_obs[17] = np.nan
    bad_draws = [d.copy() for d in draws]
    bad_draws[3][5] = np.inf
    with pytest.raises(ValueError, match=f"^{T.P_TEXT}$"):
        product.empirical_replay_segment_pvalues(bad_obs, draws)
    with pytest.raises(ValueError, match=f"^{T.P_TEXT}$"):
        product.empirical_replay_segment_pvalues(obs, bad_draws)
    with pytest.raises(ValueError, match=f"^{T.Q_TEXT}$"):
        product.replay_fdr_qvalues(bad_obs, draws)
    with pytest.raises(ValueError, match=f"^{T.Q_TEXT}$"):
        product.replay_fdr_qvalues(obs, bad_draws)
    with pytest.raises(ValueError, match=f"^{T.Q_TEXT}$"):
        product.replay_fdr_qvalues(bad_obs, [])
    with pytest.raises(ValueError, match=f"^{T.P_TEXT}$"):      # the scorer takes every p value first
        product.replay_pq(bad_obs, np.concatenate(draws), len(draws))
    # the C ABI names where, and writes no result
    lib, flags = L.lib(), C.c_uint32(9)
    pool = np.concatenate(bad_draws)
    p, q = np.full(33, 7.0), np.full(33, 7.0)
    rc = lib.csr_peakscore_pq(L.dp(bad_obs), 33, L.dp(pool), pool.shape[0], 5, 1, L.PEAK_P | L.PEAK_Q, L.dp(p), L.dp(q), None, C.byref(flags))
    assert rc == L.ERR_VALUE and flags.value == L.PEAK_BAD_OBSERVED | L.PEAK_BAD_POOL and np.all(p == 7.0) and np.all(q == 7.0)
    assert lib.csr_peakscore_pq(L.dp(obs), 33, L.dp(pool), pool.shape[0], 0, 1, L.PEAK_P, L.dp(p), None, None, None) == -1
    assert lib.csr_peakscore_pq(L.dp(obs), 33, None, 0, 0, 4, L.PEAK_P, L.dp(p), None, None, None) == -1
    assert lib.csr_peakscore_pq(L.dp(obs), 33, None, 0, 0, 1, L.PEAK_Q_MAX_P, None, L.dp(q), None, None) == -1


# ---------------------------------------------------------------------------------------------------------------
# 3. the scorer of a batch against the twin
# ---------------------------------------------------------------------------------------------------------------
def test_dwb_peak_scoring_of_a_batch_equals_the_twin(product):
    """Two chains (n = 4097 and 1031) with planted bumps, 3 views, scales (1, 2, 5), 4 replays in groups of 3 (a group boundary
    inside the replays), caps 16 per view and 40 in total: every draw of chain 0 exceeds the total cap, every draw of chain 1
    stays under it, an exported peak coincides with an observed candidate (asserted on the twin by tests/test_peakscore_twin.py).
    Every field of candidate_details, peaks and summary against the step-by-step twin on tests/twin_dwb.py's draws.  Draw 2 of chain 0 has equal
    scores at ranks 40 and 41, so the cut is decided by the stable order (`PC.scorer_case_facts`, asserted on the twin by the CPU test
    and the generator).  Then the early exits, the driver's
    composition, and that nothing resident changed."""
    from consenrich_amd import driver
    from consenrich_amd.batch import DeviceBatch, ModelParams

    scores, tmpls, views = PC.scorer_inputs()
    twin = PC.scorer_twin(scores, tmpls, views)
    peaks = PC.scorer_peaks(twin)
    want = [T.score_steps(scores[c], twin[c]["views"], twin[c]["observed"], twin[c]["replays"], peaks[c], scale_bins=twin[c]["scale_bins"],
                          dependence_span=PC.SCORER_BWS[c], random_seed=PC.SCORER_SEED) for c in range(2)]
    as_arrays = [([a for a, _ in p], [b for _, b in p]) for p in peaks]
    kw = dict(bandwidths=PC.SCORER_BWS, templates=tmpls, num_replay=PC.SCORER_REPLAYS, random_seed=PC.SCORER_SEED,
              scale_bins=PC.SCORER_SCALES, max_segments=PC.SCORER_TOTAL_CAP, max_segments_per_view=PC.SCORER_VIEW_CAP)
    with DeviceBatch(0) as b:
        b.configure(ModelParams(state_dim=2), 2, list(PC.SCORER_LENS))
        for c in range(2):
            b.upload_scores(c, scores[c])
            b.upload_template(c, tmpls[c])
        got = b.dwb_peak_scoring(views, peaks=as_arrays, draws_per_group=PC.SCORER_GROUP, **kw)
        for c in range(2):
            assert T.differences(got[c], want[c]) == [], c
        assert product.last_pool_stats()["fetched_replay_tracks"] == 0 == product.last_pool_stats()["host_decided_draws"]
        # all draws at once, and the resident templates: the same
        again = b.dwb_peak_scoring(views, peaks=as_arrays, **dict(kw, templates=None))
        for c in range(2):
            assert T.differences(again[c], want[c]) == [], c
        # the early exits
        some = b.dwb_peak_scoring(views, peaks=[as_arrays[0], ([], [])], **kw)
        assert T.differences(some[0], want[0]) == [] and some[1] == dict(enabled=False, reason="no_peaks", num_peaks=0)
        none = b.dwb_peak_scoring(views, peaks=as_arrays, **dict(kw, num_replay=0))
        assert none == [dict(enabled=False, reason="no_bootstrap_draws", num_peaks=len(p)) for p in peaks]
        # the driver's composition: the first pass's runs as peaks, the scales from the dependence span
        first_pass = [dict(starts=np.asarray(a, np.int64), ends=np.asarray(e, np.int64)) for a, e in as_arrays]
        composed = driver.score_peaks_batch(b, first_pass, views, dependence_spans=PC.SCORER_BWS, random_seed=PC.SCORER_SEED,
                                            num_replay=PC.SCORER_REPLAYS)
        direct = b.dwb_peak_scoring(views, bandwidths=PC.SCORER_BWS, peaks=as_arrays, num_replay=PC.SCORER_REPLAYS,
                                    random_seed=PC.SCORER_SEED)
        for c in range(2):
            assert composed[c]["enabled"] and T.differences(composed[c], direct[c]) == [], c
        for c in range(2):
            assert np.array_equal(T.bits(b.download_scores(c)), T.bits(scores[c]))
            assert np.array_equal(T.bits(b.download_template(c)), T.bits(tmpls[c]))


def _rows(cols):
    a = np.stack([T.bits(cols[k]) for k in ("score", "integrated_excess", "max_excess")])
    return a[:, np.lexsort(a[::-1])]


def _pool_differences(pool, twin):
    """The pool of every chain against the twin's replays, draw by draw: the counts, np.max of the scores, and the three columns --
    in the twin's order for a draw under the cap or decided on the host, as a set of rows for a draw the device capped (there
    the pool holds the rows in descending order of score)."""
    bad = []
    for c in range(len(twin)):
        cols, at = pool.download(c), 0
        for b, (cands, diag) in enumerate(twin[c]["replays"]):
            n = len(cands)
            if int(pool.stats["count"][c, b]) != n or int(pool.stats["before"][c, b]) != diag["candidate_count_before_total_cap"]:
                bad.append((c, b, "counts"))
                break
            want = {k: np.asarray([x[k] for x in cands], np.float64) for k in cols}
            got = {k: v[at:at + n] for k, v in cols.items()}
            with np.errstate(all="ignore"):
                mx = float(np.max(want["score"])) if n else 0.0
            got_mx = float(pool.stats["max_score"][c, b])
            # (which of several different NaN patterns np.max returns follows its SIMD order, not the values; the reference
            # raises on a non-finite statistic before it reads this maximum: a NaN is compared as a NaN)
            if not (np.isnan(got_mx) if np.isnan(mx) else T.bits(got_mx) == T.bits(mx)):
                bad.append((c, b, "max"))
            capped_here = diag["total_cap_hit"] and not np.isnan(twin[c]["scores_before_total_cap"][b]).any()
            same = np.array_equal(_rows(got), _rows(want)) if capped_here else all(np.array_equal(T.bits(got[k]), T.bits(want[k])) for k in cols)
            if capped_here and n > 1 and not np.all(np.diff(got["score"]) <= 0.0):
                bad.append((c, b, "order"))
            if not same:
                bad.append((c, b, "columns"))
            at += n
        if at != cols["score"].shape[0]:
            bad.append((c, "size"))
    return bad


def test_the_replay_pool_on_the_device_equals_the_twins_replays_draw_by_draw(product):
    """The scorer case: chain 0's draws are capped on the device by rank count (draw 2 with equal scores across the cut), chain 1's
    stay under the cap; groups of 3 and of 1.  No replay row leaves the device."""
    scores, tmpls, views = PC.scorer_inputs()
    twin = PC.scorer_twin(scores, tmpls, views)
    for group in (PC.SCORER_GROUP, 1):
        with product.ReplayPool(None, list(PC.SCORER_LENS), tmpls, views, bandwidths=PC.SCORER_BWS, num_replay=PC.SCORER_REPLAYS,
                                random_seed=PC.SCORER_SEED, scale_bins=PC.SCORER_SCALES, max_segments=PC.SCORER_TOTAL_CAP,
                                max_segments_per_view=PC.SCORER_VIEW_CAP, draws_per_group=group) as pool:
            assert _pool_differences(pool, twin) == [], group
            for c in range(2):
                for b, (_, diag) in enumerate(twin[c]["replays"]):
                    assert pool.chain(c)["diagnostics"][b] == diag, (c, b)
        stats = product.last_pool_stats()
        assert stats["fetched_replay_tracks"] == 0 == stats["host_decided_draws"]


def test_a_draw_over_the_cap_with_a_nan_score_is_decided_on_the_host_and_equals_the_twin(product):
    """Test 3's case with a fourth view whose null scale clamps to DBL_MIN: every draw of chain 0 is over the total cap AND holds
    NaN scores, so its order is Python's, not the values': reported as host-decided, composed from its fetched rows, uploaded --
    and the pool still equals the twin.  Those are the only replay rows fetched."""
    from consenrich_amd import _lib as L

    scores, tmpls, views = PC.scorer_inputs()
    bad = [list(v) + [dict(threshold_z=3.0, threshold=v[0]["threshold"], null_scale=0.0, null_center=v[0]["null_center"])] for v in views]
    with np.errstate(all="ignore"):
        twin = PC.scorer_twin(scores, tmpls, bad)
    undecided = [[len(s) > PC.SCORER_TOTAL_CAP and bool(np.isnan(s).any()) for s in ch["scores_before_total_cap"]] for ch in twin]
    assert all(undecided[0]) and not any(undecided[1])
    with product.ReplayPool(None, list(PC.SCORER_LENS), tmpls, bad, bandwidths=PC.SCORER_BWS, num_replay=PC.SCORER_REPLAYS,
                            random_seed=PC.SCORER_SEED, scale_bins=PC.SCORER_SCALES, max_segments=PC.SCORER_TOTAL_CAP,
                            max_segments_per_view=PC.SCORER_VIEW_CAP, draws_per_group=PC.SCORER_GROUP) as pool:
        assert _pool_differences(pool, twin) == []
        obs = {k: np.asarray([1.0, 2.0]) for k in product.POOL_COLUMNS}
        with pytest.raises(ValueError, match=f"^{T.P_TEXT}$"):
            pool.pq(0, obs)
        assert np.all(pool.pq(1, obs)["p"]["score"] <= 1.0)
        # a run's rows are not on the host while a pool is open
        assert L.lib().csr_segments_fetch(None, None, None, None, None, None, None, None, None) == -1 and "replay pool" in L.last_error()
    stats = product.last_pool_stats()
    assert stats["host_decided_draws"] == stats["fetched_replay_tracks"] == PC.SCORER_REPLAYS
    assert L.lib().csr_dwb_panel_pool_append(None, 0, None) == -1 and "csr_dwb_panel_begin" in L.last_error()


def test_a_non_finite_candidate_statistic_raises_the_references_error_from_the_scorer(product):
    """A view whose null scale clamps to DBL_MIN makes candidate statistics infinite: the scorer raises what the reference's p
    values raise, before any result is returned."""
    from consenrich_amd.batch import DeviceBatch, ModelParams

    scores, tmpls, views = PC.scorer_inputs()
    bad = [list(v) + [dict(threshold_z=3.0, threshold=v[0]["threshold"], null_scale=0.0, null_center=v[0]["null_center"])] for v in views]
    with DeviceBatch(0) as b:
        b.configure(ModelParams(state_dim=2), 2, list(PC.SCORER_LENS))
        for c in range(2):
            b.upload_scores(c, scores[c])
        with pytest.raises(ValueError, match=f"^{T.P_TEXT}$"):
            b.dwb_peak_scoring(bad, bandwidths=PC.SCORER_BWS, templates=tmpls, peaks=[([5], [9]), ([5], [9])], num_replay=2,
                               random_seed=PC.SCORER_SEED, scale_bins=PC.SCORER_SCALES, max_segments=PC.SCORER_TOTAL_CAP,
                               max_segments_per_view=PC.SCORER_VIEW_CAP)


# ---------------------------------------------------------------------------------------------------------------
# 5. a fitted batch: the driver's composition against the twin fed with downloaded tracks; residency
# ---------------------------------------------------------------------------------------------------------------
def test_score_peaks_batch_on_a_fitted_batch_equals_the_twin_and_leaves_everything_resident(product):
    """A small fitted batch through first_pass_peaks_batch, then score_peaks_batch: per chain equal to the step-by-step twin fed
    with the downloaded score track and template and the first pass's peaks.  Chain 2's mask is planted empty: its record is the
    reference's "no_peaks", taken from the chain's resident ROCCO runs (peaks=None gives the same for every chain).  Every array
    of the fit, the score tracks, the templates and the masks are bit-equal afterwards."""
    from consenrich_amd import _lib as L
    from consenrich_amd import driver, ess
    from consenrich_amd.batch import DeviceBatch, ModelParams

    lens, m, spans, seed, replays = [3001, 2049, 900], 3, [6, 3, 4], 5, 4
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
        b.upload_solution(2, np.zeros(lens[2], np.uint8))
        first[2]["starts"], first[2]["ends"] = b.rocco_runs(2)
        print("first-pass peaks per chain", [int(r["starts"].shape[0]) for r in first])
        assert [int(r["starts"].shape[0]) for r in first] == [0, 3, 0]     # chain 0: the first pass itself selects nothing
        fit = {(c, a): b.download(c, a) for c in range(3) for a in names}
        scores = [b.download_scores(c) for c in range(3)]
        tmpls = [b.download_template(c) for c in range(3)]
        masks = [b.rocco_solution(c) for c in range(3)]
        got = driver.score_peaks_batch(b, first, views, dependence_spans=spans, random_seed=seed, num_replay=replays)
        from_runs = b.dwb_peak_scoring(views, bandwidths=spans, num_replay=replays, random_seed=seed)
        twin = PC.scorer_twin(scores, tmpls, views, bws=spans, scales=None, replays=replays, seed=seed, total_cap=20000, view_cap=1000)
        for c in range(3):
            peaks = list(zip(first[c]["starts"].tolist(), first[c]["ends"].tolist()))
            want = T.score_steps(scores[c], twin[c]["views"], twin[c]["observed"], twin[c]["replays"], peaks,
                                 scale_bins=twin[c]["scale_bins"], dependence_span=spans[c], random_seed=seed)
            assert T.differences(got[c], want) == [], c
            assert T.differences(from_runs[c], want) == [], c
        assert got[0] == got[2] == dict(enabled=False, reason="no_peaks", num_peaks=0) and got[1]["enabled"]
        assert product.last_pool_stats()["fetched_replay_tracks"] == 0
        for (c, a), v in fit.items():
            assert np.array_equal(b.download(c, a).view(np.uint32), v.view(np.uint32)), (c, a)
        for c in range(3):
            assert np.array_equal(T.bits(b.download_scores(c)), T.bits(scores[c])), c
            assert np.array_equal(T.bits(b.download_template(c)), T.bits(tmpls[c])), c
            assert np.array_equal(b.rocco_solution(c), masks[c]), c
