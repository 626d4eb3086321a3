"""GPU tests of the ROCCO budget path on the device (run with -m gpu): the effective sample size scan, the series it scans, the
budget policy, gamma, and the first-pass composition with its fallback window.  Every float is compared by its 64-bit pattern,
every integer, boolean and string with ==.  References: the compiled reference's recorded outputs (tests/golden/ess) and the
NumPy / Python twins (tests/twin_budget.py, twin_null.py, twin_dwb.py, twin_rocco.py), held equal to the reference on the CPU by
tests/test_budget_twin.py and their own twin tests."""
import os

import numpy as np
import pytest

import cases
import ess_cases
import twin_budget as T
from conftest import gpu_available

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(ess_cases.__file__)), "ess")


@pytest.fixture(scope="module")
def E():
    if not gpu_available():
        pytest.fail("GPU tests selected but no HIP device / library: the product has no CPU fallback")
    from consenrich_amd import ess

    return ess


def _bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


def _same_triple(a, b):
    return _bits(a[0]) == _bits(b[0]) and _bits(a[1]) == _bits(b[1]) and int(a[2]) == int(b[2])


# ---------------------------------------------------------------------------------------------------------------
# 1. the drop-in on host arrays: the whole table against the reference's recorded outputs
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", ess_cases.GROUPS)
def test_drop_in_equals_the_reference_on_the_whole_table(E, group):
    golden = ess_cases.load_group(os.path.join(GOLDEN, f"ess_{group}.npz"))
    mine = [c for c in ess_cases.cases() if c["group"] == group]
    assert sorted(golden) == sorted(c["name"] for c in mine)
    bad = {}
    for c in mine:
        got = ess_cases.run_case(E, c)
        if not ess_cases.same(got, golden[c["name"]]):
            bad[c["name"]] = (got, golden[c["name"]])
    assert bad == {}


def test_the_drop_in_is_exported_and_leaves_its_input_alone(E):
    from consenrich_amd import cconsenrich

    assert cconsenrich.cEstimateEffectiveSampleSize is E.cEstimateEffectiveSampleSize
    x = ess_cases.values(dict(n=2049, series="ar_pos", seed=5))
    keep = x.copy()
    E.cEstimateEffectiveSampleSize(x, 70)
    E.cEstimateEffectiveSampleSize(x, 70, None, True, 9)
    assert np.array_equal(_bits(x), _bits(keep))
    # any array-like, any shape: flattened like the reference's reshape(-1)
    want = T.cEstimateEffectiveSampleSize(keep, 70)
    assert _same_triple(E.cEstimateEffectiveSampleSize(keep.reshape(3, 683).tolist(), 70), want)
    assert _same_triple(E.cEstimateEffectiveSampleSize(keep.astype(np.float32), 70), T.cEstimateEffectiveSampleSize(keep.astype(np.float32), 70))


def test_value_errors_carry_the_reference_texts(E):
    import ctypes as C

    from consenrich_amd import _lib as L

    with np.load(os.path.join(GOLDEN, "ess_errors.npz")) as z:
        recorded = {k: str(z[k]) for k in z.files}
    for case, text in ess_cases.error_cases():
        assert recorded[case["name"]] == text
        with pytest.raises(ValueError) as e:
            ess_cases.call(E, case)
        assert str(e.value) == text, case["name"]
    with pytest.raises(OverflowError, match="value too large to convert to int"):
        E.cEstimateEffectiveSampleSize(np.zeros(4), 2 ** 31)
    # the C ABI itself: the reference's text and the value-error code before anything is launched
    lib, out, x = L.lib(), L.EssOut(), np.array([1.0, np.nan, 2.0, 0.5])
    assert lib.csr_ess_scan(L.dp(x), 4, 3, None, 0, -1, C.byref(out)) == L.ESS_ERR_VALUE
    assert L.last_error() == "windowIntervals must be nonnegative"
    assert lib.csr_ess_scan(L.dp(x), 4, 3, None, 1, 0, C.byref(out)) == L.ESS_ERR_VALUE
    assert L.last_error() == "active values must be finite"
    # ... and the fast path takes the same vector: a NaN is data there
    assert lib.csr_ess_scan(L.dp(x), 4, 3, None, 0, 0, C.byref(out)) == 0
    assert (out.n_eff, out.tau, out.lags_used) == (4.0, 1.0, 0)


# ---------------------------------------------------------------------------------------------------------------
# 2. a batch: the series built on the device from resident scores
# ---------------------------------------------------------------------------------------------------------------
CHAINS = (1, 2, 65, 2049, 131073)
ARRAYS = ("D", "xf", "Pf", "pnoise", "xs", "Ps", "lag")
Z_GRID = (1.5, 2.0, 2.5, 3.0)
MAX_LAGS = (4, 1, 64, 257, 256)


def _score(c, n):
    return ess_cases.values(dict(n=n, series="ar_soft", seed=700 + c)) * 1.7 - 0.4 + 0.0


def _views(c, nz):
    """(thresholds, scales) of chain c: ascending thresholds, one scale below DBL_MIN (raised to it)."""
    thr = [0.3 + 0.45 * k + 0.01 * c for k in range(nz)]
    sc = [0.8 + 0.1 * k for k in range(nz)]
    if c == 2:
        sc[0] = 0.0
    return thr, sc


@pytest.fixture(scope="module")
def series_reference():
    """(kind, nz, chain) -> the twin's scan of the series NumPy builds; computed once."""
    ref = {}
    for c, n in enumerate(CHAINS):
        s = _score(c, n)
        for kind, nz in (("occupancy", 1), ("soft", 1), ("integrated", 1), ("integrated", 2), ("integrated", 4), ("integrated", 16)):
            thr, sc = _views(c, nz)
            ref[kind, nz, c] = T.cEstimateEffectiveSampleSize(T.series(kind, s, thr, sc), MAX_LAGS[c])
    return ref


def test_batch_ess_equals_the_drop_in_per_chain_and_changes_nothing_resident(E, series_reference):
    from consenrich_amd import _lib as L
    from consenrich_amd.batch import DeviceBatch, ModelParams

    m, nc = 2, len(CHAINS)
    with DeviceBatch(0) as b:
        b.configure(ModelParams(state_dim=2), m, list(CHAINS))
        for c, n in enumerate(CHAINS):
            b.upload(c, *cases.synth(n, m, 950 + c))
        b.stats()
        b.forward_backward(L.RETURN_NLL)
        b.export(L.EXPORT_FORWARD | L.EXPORT_SMOOTH)
        with pytest.raises(L.ConsenrichAMDError, match="no scores"):
            b.ess("occupancy", [0.0] * nc, [1.0] * nc, 4)
        for c, n in enumerate(CHAINS):
            b.upload_scores(c, _score(c, n))
        b.rocco_null()
        before = {(c, a): b.download(c, a) for c in range(nc) for a in ARRAYS}
        templates = [b.download_template(c) for c in range(nc)]
        for kind, nz in (("occupancy", 1), ("soft", 1), ("integrated", 1), ("integrated", 2), ("integrated", 4), ("integrated", 16)):
            views = [_views(c, nz) for c in range(nc)]
            thr = [v[0] if kind == "integrated" else v[0][0] for v in views]
            sc = [v[1] if kind == "integrated" else v[1][0] for v in views]
            got = b.ess(kind, thr, sc, list(MAX_LAGS))
            for c, n in enumerate(CHAINS):
                assert _same_triple(got[c], series_reference[kind, nz, c]), (kind, nz, n, got[c], series_reference[kind, nz, c])
                drop = E.cEstimateEffectiveSampleSize(T.series(kind, _score(c, n), *views[c]), MAX_LAGS[c])
                assert _same_triple(got[c], drop), (kind, nz, n)
        # a chain mask: the others are not scanned
        take = [False, True, False, True, False]
        got = b.ess("soft", [_views(c, 1)[0][0] for c in range(nc)], [_views(c, 1)[1][0] for c in range(nc)], list(MAX_LAGS), chains=take)
        for c in range(nc):
            assert (got[c] is None) == (not take[c])
            assert got[c] is None or _same_triple(got[c], series_reference["soft", 1, c])
        with pytest.raises(ValueError, match="Unknown series kind"):
            b.ess("hard", [0.0] * nc, [1.0] * nc, 4)
        # neither the scores, the templates nor any array of the fit moved
        for c, n in enumerate(CHAINS):
            assert np.array_equal(_bits(b.download_scores(c)), _bits(_score(c, n))), n
            assert np.array_equal(_bits(b.download_template(c)), _bits(templates[c])), n
        for (c, a), v in before.items():
            assert np.array_equal(b.download(c, a).view(np.uint32), v.view(np.uint32)), (c, a)


# ---------------------------------------------------------------------------------------------------------------
# 3. budget and gamma of a batch from a real panel
# ---------------------------------------------------------------------------------------------------------------
P_CHAINS = (2049, 65, 3001, 131073)
P_SPANS = (5, 1, 12, 64)
P_KW = dict(num_bootstrap=9, random_seed=11)


def _p_score(c, n):
    x = ess_cases.values(dict(n=n, series="ar_soft", seed=800 + c)) * 1.3 - 0.2 + 0.0
    return np.round(x, 3) + 0.0 if c == 2 else x        # ties, also at a level


def test_budget_and_gamma_equal_the_twin_on_a_real_panel(E):
    from consenrich_amd.batch import DeviceBatch, ModelParams

    nc = len(P_CHAINS)
    scores = [_p_score(c, n) for c, n in enumerate(P_CHAINS)]
    spans = [max(s, 2) for s in P_SPANS]
    with DeviceBatch(0) as b:
        b.configure(ModelParams(state_dim=2), 2, list(P_CHAINS))
        for c in range(nc):
            b.upload_scores(c, scores[c])
        b.rocco_null()
        panel = b.dwb_panel(threshold_z_grid=Z_GRID, bandwidths=spans, **P_KW)
        budgets = {}
        for statistic, tz in (("occupancy", 2.0), ("soft", 1.5), ("integrated", 3.0), ("fraction", 2.25)):
            got = b.rocco_budget(panel, statistic=statistic, threshold_z=tz, threshold_z_grid=Z_GRID, dependence_spans=list(P_SPANS))
            for c in range(nc):         # ("fraction" at 2.25: no view of the panel has that z, the first of the grid is primary)
                want = T.budget(scores[c], panel[c], statistic=statistic, threshold_z=tz, threshold_z_grid=Z_GRID,
                                dependence_span=P_SPANS[c])
                assert T.same_details(got[c], want) == [], (statistic, c, got[c], want)
            budgets[statistic] = got
        with pytest.raises(ValueError, match="Unknown budget statistic: hard"):
            b.rocco_budget(panel, statistic="hard", threshold_z=2.0, threshold_z_grid=Z_GRID, dependence_spans=5)
        # gamma: fixed values pass through; a negative one takes the median of the positive excess from the device's ranks
        assert b.rocco_gamma(None, dependence_spans=5) == [(0.5, {"method": "fixed", "gamma": 0.5})] * nc
        assert b.rocco_gamma(0.75, dependence_spans=5) == [(0.75, {"method": "fixed", "gamma": 0.75})] * nc
        with pytest.raises(ValueError, match="`gamma` must be finite"):
            b.rocco_gamma(np.inf, dependence_spans=5)
        occ = budgets["occupancy"]
        for thr, cen in (([d["threshold"] for d in occ], [d["null_center"] for d in occ]), (None, [d["null_center"] for d in occ]),
                         (None, None), ([0.25, 1.0e9, 0.0, -1.0e9], None)):
            got = b.rocco_gamma(-1.0, dependence_spans=list(P_SPANS), gamma_spans=[None, 9, 1, None], gamma_scale=0.5,
                                null_centers=cen, thresholds=thr)
            for c in range(nc):
                want = T.estimate_gamma(scores[c], dependence_span=P_SPANS[c], gamma_span=[None, 9, 1, None][c], gamma=-1.0,
                                        gamma_scale=0.5, null_center=None if cen is None else cen[c],
                                        threshold=None if thr is None else thr[c])
                assert _bits(got[c][0]) == _bits(want[0]) and T.same_details(got[c][1], want[1]) == [], (c, got[c], want)
        assert got[1][1]["positive_score_median"] == 1.0            # no score above 1e9
        for c in range(nc):
            assert np.array_equal(_bits(b.download_scores(c)), _bits(scores[c]))


# ---------------------------------------------------------------------------------------------------------------
# 4. the first-pass composition, one chain forced into the fallback window
# ---------------------------------------------------------------------------------------------------------------
F_CHAINS = (3001, 2049, 1200)
F_KW = dict(dependence_spans=[6, 3, 4], threshold_z=2.0, threshold_z_grid=Z_GRID, num_bootstrap=9, random_seed=5, gamma=-1.0,
            gamma_scale=0.5, score_mode="state", z=1.0, max_gap_bins=2)


def _f_data(c, n, m):
    """Chain 2: the same constant in every track -- its smoothed state is flat up to the filter's start-up, so the calibrated solve
    selects all bins or none and the wrapper's window applies."""
    data, munc = cases.synth(n, m, 990 + c)
    if c == 2:
        data = np.full_like(data, 3.0)
        munc = np.full_like(munc, 1.0)
    return data, munc


def test_first_pass_equals_the_twin_composition(E):
    from consenrich_amd import _lib as L
    from consenrich_amd import driver
    from consenrich_amd.batch import DeviceBatch, ModelParams

    m, nc = 3, len(F_CHAINS)
    with DeviceBatch(0) as b:
        b.configure(ModelParams(state_dim=2), m, list(F_CHAINS))
        for c, n in enumerate(F_CHAINS):
            b.upload(c, *_f_data(c, n, m))
        b.stats()
        b.forward_backward(L.RETURN_NLL)
        b.export(L.EXPORT_SMOOTH)
        got = driver.first_pass_peaks_batch(b, **F_KW)
        scores = [b.download_scores(c) for c in range(nc)]
        masks = [b.rocco_solution(c) for c in range(nc)]
        for c in range(nc):
            kw = {k: v for k, v in F_KW.items() if k not in ("dependence_spans", "score_mode", "z")}
            want = T.first_pass(scores[c], dependence_span=F_KW["dependence_spans"][c], **kw)
            r = got[c]
            assert T.same_details(r["budget_details"], want["budget_details"]) == [], c
            assert _bits(r["gamma"]) == _bits(want["gamma"]) and T.same_details(r["gamma_details"], want["gamma_details"]) == [], c
            for k in ("objective", "penalized_objective", "selection_penalty", "budget"):
                assert _bits(r[k]) == _bits(want[k]), (c, k, r[k], want[k])
            for k in ("selected_count", "budget_target_count", "budget_fallback_window"):
                assert r[k] == want[k], (c, k, r[k], want[k])
            assert np.array_equal(masks[c], want["solution"]), c
            assert np.array_equal(r["starts"], want["starts"]) and np.array_equal(r["ends"], want["ends"]), c
        assert [r["budget_fallback_window"] for r in got] == [False, False, True]
        assert got[2]["selected_count"] == got[2]["budget_target_count"] > 0 and len(got[2]["starts"]) == 1
        # call_peaks_batch with the derived numbers gives the native's answer: the same for the chains without a fallback
        plain = driver.call_peaks_batch(b, budget=[r["budget"] for r in got], gamma=[r["gamma"] for r in got], max_gap_bins=2)
        for c in (0, 1):
            assert plain[c]["selected_count"] == got[c]["selected_count"] and np.array_equal(plain[c]["starts"], got[c]["starts"])
        assert plain[2]["selected_count"] == 0
