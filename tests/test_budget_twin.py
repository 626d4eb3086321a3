"""CPU: the pure-Python twin of the ROCCO budget path (tests/twin_budget.py) equals the compiled reference's recorded outputs on
every case of the table, bit for bit; the budget policy, the gamma rule, the "integrated" series and the fallback wrapper of the
product equal the twin's restatement of the reference and hand-computed values; the drop-in raises the reference's errors
before any GPU call."""
import os

import numpy as np
import pytest

import ess_cases
import twin_budget as T

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(ess_cases.__file__)), "ess")


def _bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def golden():
    out = {}
    for g in ess_cases.GROUPS:
        out.update(ess_cases.load_group(os.path.join(GOLDEN, f"ess_{g}.npz")))
    return out


@pytest.fixture(scope="module")
def twin_results():
    return {c["name"]: ess_cases.run_case(T, c) for c in ess_cases.cases()}


@pytest.fixture(scope="module")
def product():
    from consenrich_amd import build

    build.build()
    from consenrich_amd import cconsenrich, ess, rocco

    return cconsenrich, ess, rocco


# ---------------------------------------------------------------------------------------------------------------
# the native
# ---------------------------------------------------------------------------------------------------------------
def test_every_case_has_a_fixture(golden):
    assert sorted(golden) == sorted(c["name"] for c in ess_cases.cases())
    assert len({c["name"] for c in ess_cases.cases()}) == len(ess_cases.cases())


@pytest.mark.parametrize("group", ess_cases.GROUPS)
def test_twin_equals_the_reference(golden, twin_results, group):
    bad = [c["name"] for c in ess_cases.cases() if c["group"] == group and not ess_cases.same(twin_results[c["name"]], golden[c["name"]])]
    assert bad == []


def test_twin_raises_the_recorded_error_texts():
    with np.load(os.path.join(GOLDEN, "ess_errors.npz")) as z:
        recorded = {k: str(z[k]) for k in z.files}
    assert sorted(recorded) == sorted(c["name"] for c, _ in ess_cases.error_cases())
    for case, text in ess_cases.error_cases():
        assert recorded[case["name"]] == text
        with pytest.raises(ValueError) as e:
            ess_cases.call(T, case)
        assert str(e.value) == text


def test_the_cases_are_what_the_table_says(golden):
    def lags(name):
        return int(golden[name]["lags"][0])

    def out(name):
        return [float(v) for v in golden[name]["out"]]

    # the planted breaks: the last lag of the first round of 256 (lags 0..255) and the first lag of the next
    assert lags("fast_break_round_end") == ess_cases.ROUND - 2 and lags("fast_break_round_start") == ess_cases.ROUND - 1
    for n in (2, 3, 64, 65, 2049):
        assert lags(f"fast_alternating_n{n}") == 0
    for n, lag in ((2049, 255), (2049, 256), (2049, 257), (131073, 700), (65, 7)):       # the ramp never breaks
        assert lags(f"fast_ramp_n{n}_lag{lag}") == lag
    for series in ("const", "nan", "inf", "huge"):                                       # the variance branch
        for n in (2, 65, 2049):
            assert out(f"fast_{series}_n{n}") == [float(n), 1.0] and lags(f"fast_{series}_n{n}") == 0
    assert lags("fast_const_tenth_n2049") >= 0 and out("fast_const_tenth_n2049")[1] >= 1.0
    assert out("fast_n0") == [0.0, 1.0] and out("fast_ar_occ_n1_lag0") == [1.0, 1.0]
    assert out("gen_none_active_n65") == [0.0, 1.0] and out("gen_one_active_n65") == [1.0, 1.0]
    # pairs exist at the multiples of 4 only; without a window the scan runs on past the lags without a pair
    assert lags("gen_every4_n2049") % 4 == 0 and lags("gen_every4_n2049") >= 4
    assert lags("gen_every4_window_n2049") % 4 == 0
    # window 1: no lag at all; the clamp at the window; a window beyond maxLag leaves maxLag alone
    assert out("gen_window1_ramp")[1] == 1.0 and lags("gen_window1_ramp") == 0
    assert out("gen_tau_clamped")[1] == 2.0 and out("gen_tau_unclamped")[1] > 2.0
    assert lags("gen_window5000_ramp") == 300 and lags("gen_window_is_lag_plus_one") == 63
    assert lags("gen_window64_ramp") == 63 and lags("gen_window65_ramp") == 64 and lags("gen_window257_ramp") == 256


def test_walk_adds_in_index_order():
    rng = np.random.default_rng(1)
    x = rng.standard_normal(1000) * 10.0 ** rng.integers(-8, 8, 1000)
    acc = 0.0
    for v in x:
        acc += float(v)
    assert _bits(T.walk(x)) == _bits(acc) and T.walk([]) == 0.0


def test_the_drop_in_checks_its_arguments_without_a_gpu(product):
    cc, E, _ = product
    assert "cEstimateEffectiveSampleSize" in cc.__all__ and cc.cEstimateEffectiveSampleSize is E.cEstimateEffectiveSampleSize
    for mod in (E, T):
        for case, text in ess_cases.error_cases():
            if case["name"] == "err_variance":      # (depends on the sums)
                continue
            with pytest.raises(ValueError) as e:
                ess_cases.call(mod, case)
            assert str(e.value) == text
        with pytest.raises(OverflowError, match="value too large to convert to int"):
            mod.cEstimateEffectiveSampleSize(np.zeros(4), 2 ** 31)
        with pytest.raises(OverflowError, match="value too large to convert to int"):
            mod.cEstimateEffectiveSampleSize(np.zeros(4), 1, None, False, -2 ** 31 - 1)
        # what the reference answers without a sum
        assert mod.cEstimateEffectiveSampleSize([], 3) == (0.0, 1.0, 0)
        assert mod.cEstimateEffectiveSampleSize([4.0], 3) == (1.0, 1.0, 0)
        assert mod.cEstimateEffectiveSampleSize([4.0, 2.0, 1.0], 3, [0, 1, 0]) == (1.0, 1.0, 0)
        assert mod.cEstimateEffectiveSampleSize([4.0, -2.0, 1.0], 3, [0, 0, 0], True) == (0.0, 1.0, 0)


# ---------------------------------------------------------------------------------------------------------------
# the series
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nz", [1, 2, 3, 8])
def test_integrated_series_added_in_grid_order_is_numpys_mean_of_the_stack(nz):
    rng = np.random.default_rng(40 + nz)
    score = rng.normal(0.5, 1.5, 4099) * np.exp(rng.normal(0.0, 1.0, 4099))
    thr = [0.1 + 0.37 * k for k in range(nz)]
    sc = [0.9 + 0.13 * k for k in range(nz)]
    want = np.mean(np.vstack([np.clip((score - t) / max(s, T.TINY), 0.0, None) for t, s in zip(thr, sc)]), axis=0)
    assert np.array_equal(_bits(T.integrated_in_order(score, thr, sc)), _bits(want))
    assert np.array_equal(_bits(T.series("integrated", score, thr, sc)), _bits(want))


# ---------------------------------------------------------------------------------------------------------------
# the budget policy
# ---------------------------------------------------------------------------------------------------------------
def _view(z, occ_raw, soft_raw, thr):
    return dict(threshold_z=float(z), threshold=float(thr), null_center=0.125, null_scale=0.75 + 0.0625 * z, num_bootstrap=16,
                null_quantile=0.9, observed_tail_occupancy=0.2, null_tail_occupancy=0.05, null_tail_occupancy_calibrated=0.07,
                null_tail_occupancy_sd=0.01, observed_soft_tail=0.3, null_soft_tail=0.1, null_soft_tail_calibrated=0.12,
                null_soft_tail_sd=0.02, budget_occupancy_raw=occ_raw, budget_soft_raw=soft_raw)


PANEL = [_view(1.5, 0.375, 0.5, 1.0), _view(2.0, 0.125, 0.0625, 1.5), _view(2.5, 0.0, 0.03125, 2.0), _view(3.0, 0.0625, 0.0, 2.5)]
GRID = (1.5, 2.0, 2.5, 3.0)


def _score():
    return ess_cases.values(dict(n=3001, series="ar_soft", seed=12)) * 2.0


def _product_budget(E, score, views, *, statistic, threshold_z, threshold_z_grid, dependence_span, **bounds):
    lo, hi = bounds.get("budget_min", E.BUDGET_MIN), bounds.get("budget_max", E.BUDGET_MAX)
    pol = E.budget_policy(views, statistic=statistic, threshold_z=threshold_z, threshold_z_grid=threshold_z_grid, budget_min=lo,
                          budget_max=hi)
    series = T.series(E.SERIES_OF[pol["statistic"]], score, [v["threshold"] for v in pol["series_views"]],
                      [v["null_scale"] for v in pol["series_views"]])
    span = max(int(dependence_span), 2)
    return E.budget_details(pol, threshold_z, span, T.cEstimateEffectiveSampleSize(series, max(4 * span, span)))


def test_budgets_of_the_three_statistics_by_hand(product):
    _, E, _ = product
    assert (E.BUDGET_MIN, E.BUDGET_MAX, E.TINY) == (0.001, 0.25, 2.2250738585072014e-308)
    score = _score()
    kw = dict(threshold_z=2.0, threshold_z_grid=GRID, dependence_span=5)
    # occupancy: the primary view's raw budget 0.125, inside [0.001, 0.25]
    d = _product_budget(E, score, PANEL, statistic="occupancy", **kw)
    assert (d["statistic"], d["budget"], d["budget_raw"], d["budget_clipped"]) == ("tail_occupancy", 0.125, 0.125, False)
    assert d["threshold"] == 1.5 and d["threshold_z_grid"] == [1.5, 2.0, 2.5, 3.0] and d["dependence_span"] == 5
    # soft: 0.0625; integrated: the mean of the four soft budgets (0.5 + 0.0625 + 0.03125 + 0) / 4 = 0.1484375
    assert _product_budget(E, score, PANEL, statistic="soft", **kw)["budget"] == 0.0625
    d = _product_budget(E, score, PANEL, statistic="integrated", **kw)
    assert (d["budget"], d["budget_integrated_raw"], d["budget_occupancy"], d["budget_soft"]) == (0.1484375, 0.1484375, 0.125, 0.0625)
    # the clips: primary z = 1.5 has raw 0.375 (occupancy) and 0.5 (soft), above 0.25; z = 2.5 has raw 0 below 0.001
    d = _product_budget(E, score, PANEL, statistic="occupancy", threshold_z=1.5, threshold_z_grid=GRID, dependence_span=5)
    assert (d["budget"], d["budget_raw"], d["budget_clipped"], d["budget_soft"]) == (0.25, 0.375, True, 0.25)
    d = _product_budget(E, score, PANEL, statistic="occupancy", threshold_z=2.5, threshold_z_grid=GRID, dependence_span=5)
    assert (d["budget"], d["budget_raw"], d["budget_clipped"]) == (0.001, 0.0, True)
    d = _product_budget(E, score, PANEL, statistic="soft", threshold_z=1.5, threshold_z_grid=GRID, dependence_span=5, budget_min=-1.0,
                        budget_max=0.4)
    assert (d["budget"], d["budget_min"], d["budget_max"]) == (0.4, 0.0, 0.4)
    assert d["effective_count"] == d["budget"] * d["effective_total_count"]


@pytest.mark.parametrize("statistic", ["occupancy", "soft", "integrated"])
def test_product_policy_equals_the_twin(product, statistic):
    _, E, _ = product
    score = _score()
    for tz, grid, span in ((2.0, GRID, 5), (1.5, GRID, 1), (3.0, GRID, 64), (-1.0, (0.0, 2.0), 7)):
        views = PANEL if tz > 0 else [_view(0.0, 0.2, 0.1, 0.4), _view(2.0, 0.05, 0.02, 1.5)]
        a = _product_budget(E, score, views, statistic=statistic, threshold_z=tz, threshold_z_grid=grid, dependence_span=span)
        b = T.budget(score, views, statistic=statistic, threshold_z=tz, threshold_z_grid=grid, dependence_span=max(span, 2))
        assert T.same_details(a, b) == [], (tz, span)


def test_statistic_aliases_and_the_missing_primary_key(product):
    _, E, _ = product
    table = {"tail_occupancy": ["occupancy", "calibrated_occupancy", "calibrated_tail_occupancy", "tail_fraction", "fraction", "tail",
                                "tail_occupancy", " Tail-Occupancy "],
             "soft": ["soft", "soft_occupancy", "soft-tail", "SOFT"],
             "integrated_excess_tail": ["integrated", "integrated_excess", "integrated-excess-tail", "excess"]}
    for want, names in table.items():
        for name in names:
            assert E.resolve_statistic(name) == want
    for mod_call in (lambda: E.resolve_statistic("hard"), lambda: T.budget(_score(), PANEL, statistic="hard", threshold_z=2.0,
                                                                            threshold_z_grid=GRID, dependence_span=3)):
        with pytest.raises(ValueError, match="Unknown budget statistic: hard"):
            mod_call()
    # threshold_z = 2.25 has no view in the panel: the view of the first z of the resolved grid (1.5) is the primary one
    score = _score()
    for statistic in ("occupancy", "soft"):
        a = _product_budget(E, score, PANEL, statistic=statistic, threshold_z=2.25, threshold_z_grid=GRID, dependence_span=4)
        b = T.budget(score, PANEL, statistic=statistic, threshold_z=2.25, threshold_z_grid=GRID, dependence_span=4)
        assert T.same_details(a, b) == [] and a["threshold"] == 1.0 and a["threshold_z"] == 2.25
        assert a["threshold_z_grid"] == [1.5, 2.0, 2.25, 2.5, 3.0]
    assert E.resolve_z_grid(2.0, (3.0, 2.0, -1.0, 1.5)) == [0.0, 1.5, 2.0, 3.0] == T.resolve_z_grid(2.0, (3.0, 2.0, -1.0, 1.5))
    assert [E.z_key(z) for z in (2.0, 1.5, 0.0, 2.123456789)] == ["2", "1.5", "0", "2.123457"]


# ---------------------------------------------------------------------------------------------------------------
# gamma
# ---------------------------------------------------------------------------------------------------------------
def _gamma_from_ranks(E, score, *, span, gamma_span, gamma_scale, clip_min, clip_max, null_center, threshold):
    """The product's composition from what the device returns: the count above the level and the two middle sorted scores."""
    level, method = E.gamma_reference_level(threshold, null_center)
    s = np.sort(score)
    below = int(np.count_nonzero((s - level) <= 0.0))
    count = s.size - below
    if count <= 0:
        scale = 1.0
    else:
        hi = count // 2
        lo = hi if count % 2 else hi - 1
        a, b = float(s[below + lo]) - level, float(s[below + hi]) - level
        scale = b if count % 2 else (a + b) / 2.0
    return E.gamma_from_scale(scale, span=span, gamma_span=gamma_span, gamma_scale=gamma_scale, clip_min=clip_min,
                              clip_max=clip_max, level=level, method=method)


def test_gamma_from_ranks_equals_the_reference_rule(product):
    _, E, _ = product
    rng = np.random.default_rng(8)
    base = np.round(rng.normal(0.2, 1.0, 1001), 2) + 0.0          # rounded: ties, also at the level
    tracks = {"odd": base, "even": base[:-1], "none": -np.abs(base) - 1.0, "one": np.r_[-np.abs(base), 3.5],
              "two": np.r_[-np.abs(base), 3.5, 1.25], "ties": np.r_[base, np.full(40, 0.5)]}
    seen = set()
    for name, score in tracks.items():
        for thr, cen in ((0.5, 0.1), (None, 0.1), (np.nan, 0.1), (None, None), (np.inf, np.nan)):
            for span, gspan, scale, cmin, cmax in ((5, None, 0.5, 0.5, 50.0), (1, 9, 2.0, 0.0, None), (40, 1, 0.5, 3.0, 2.0), (7, 7, -1.0, 0.5, 50.0)):
                got = _gamma_from_ranks(E, score, span=span, gamma_span=gspan, gamma_scale=scale, clip_min=cmin, clip_max=cmax,
                                        null_center=cen, threshold=thr)
                want = T.estimate_gamma(score, dependence_span=span, gamma_span=gspan, gamma=-1.0, gamma_scale=scale, clip_min=cmin,
                                        clip_max=cmax, null_center=cen, threshold=thr)
                assert _bits(got[0]) == _bits(want[0]) and T.same_details(got[1], want[1]) == [], (name, thr, cen, span)
                seen.add(want[1]["reference_method"])
    assert seen == {"threshold", "null_center", "zero"}
    assert T.estimate_gamma(tracks["none"], dependence_span=5, gamma=-1.0)[1]["positive_score_median"] == 1.0
    # by hand: positives of [1, 2, 4, -3] above 0.5 are 0.5, 1.5, 3.5 -> median 1.5; gamma = 0.5 * 6 * 1.5
    assert T.estimate_gamma([1.0, 2.0, 4.0, -3.0], dependence_span=6, gamma=-1.0, threshold=0.5)[0] == 4.5
    assert T.estimate_gamma([1.0, 2.0, 4.0, -3.0], dependence_span=6, gamma=None)[0] == 0.5
    assert T.estimate_gamma([1.0], dependence_span=6, gamma=0.25)[0] == 0.25
    with pytest.raises(ValueError, match="`gamma` must be finite"):
        T.estimate_gamma([1.0], dependence_span=6, gamma=np.nan)


# ---------------------------------------------------------------------------------------------------------------
# the fallback window of the solve's wrapper
# ---------------------------------------------------------------------------------------------------------------
def flat_track(n=400):
    """Nearly constant: the penalised solve selects all bins or none, whatever the penalty; every window passes the range test."""
    return 1.0 + 1.0e-3 * np.sin(np.arange(n) * 0.7)


def wavy_track(n=400):
    """A wave of 18 % around 1 under a boundary cost that no single crest repays: all or none again, but a window of 5 % of the
    bins spans a whole period and fails the 5 % range test."""
    return 1.0 + 0.1 * np.sin(np.arange(n) * (2.0 * np.pi / 20.0))


def test_the_wrapper_takes_the_window_only_when_it_passes_the_range_test(product):
    import twin_rocco

    _, _, R = product
    for track, gamma, used in ((flat_track(), 0.5, True), (wavy_track(), 5.0, False)):
        native = twin_rocco.csolveChromROCCOExact(track, budget=0.05, gamma=gamma)
        assert native[3] == 0                       # the calibrated solve selects nothing ...
        solution, d = T.solve_chrom(track, 0.05, gamma)
        assert d["budget_target_count"] == 20 and d["budget_fallback_window"] == used       # ... although 20 bins were asked for
        mask, ok = R.best_contiguous_budget_fallback_mask(track, 20, 0.0, gamma, maxRelativeRange=0.05)
        assert ok == used and np.array_equal(mask.astype(np.uint8), solution)
        assert R.budget_target_count(track.size, 0.05) == 20 and R.budget_target_count(track.size, np.inf) is None
        if used:
            assert d["selected_count"] == 20 and int(solution.sum()) == 20 and np.all(np.diff(np.flatnonzero(solution)) == 1)
            assert _bits(R.objective_for_solution(track, solution, gamma)) == _bits(d["objective"])
            assert _bits(d["penalized_objective"]) == _bits(d["objective"] - native[4] * 20.0)
        else:
            assert d["selected_count"] == 0 and not solution.any()
        # without the range test both windows stand (their objective is positive)
        assert R.best_contiguous_budget_fallback_mask(track, 20, 0.0, gamma)[1]
    # the vectorised window search keeps the reference loop's first best start, ties included
    rng = np.random.default_rng(2)
    for n, target in ((1, 1), (7, 7), (50, 5), (333, 40)):
        for track in (np.round(rng.normal(1.0, 0.5, n), 1), np.ones(n), -np.ones(n)):
            for pen, gamma in ((0.0, 0.0), (0.3, 0.4), (0.0, 7.0)):
                for rel in (None, 0.05, 0.9):
                    a = R.best_contiguous_budget_fallback_mask(track, target, pen, gamma, maxRelativeRange=rel)
                    b = T.best_window(track, target, pen, gamma, rel)
                    assert a[1] == b[1] and np.array_equal(a[0], b[0]), (n, target, pen, gamma, rel)
