"""GPU tests of the budgeted chain peak selection (ROCCO) on the device (run with -m gpu).  Every comparison is exact: the
uint8 mask with array_equal, counts with ==, floats by their 64-bit patterns.  References: the compiled reference's recorded
outputs (tests/golden/rocco/rocco_*.npz) for the case table, the pure-Python twin (tests/twin_rocco.py, itself pinned to those
recordings by tests/test_rocco_twin.py) for everything else."""
import os

import numpy as np
import pytest

import cases
import rocco_cases
import twin_rocco
from conftest import gpu_available

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(rocco_cases.__file__)), "rocco")


@pytest.fixture(scope="module")
def product():
    if not gpu_available():
        pytest.fail("GPU tests selected but no HIP device / library: the product has no CPU fallback")
    from consenrich_amd import cconsenrich

    return cconsenrich


@pytest.fixture(scope="module")
def golden():
    out = {}
    for g in ("fixed", "ties", "costs", "calib"):
        out.update(rocco_cases.load_group(os.path.join(GOLDEN, f"rocco_{g}.npz")))
    return out


def _bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


def _same_tuple(got, ref):
    """the 5-tuple of csolveChromROCCOExact, exactly"""
    assert np.array_equal(got[0], ref[0]) and got[0].dtype == np.uint8
    assert got[3] == ref[3]
    assert np.array_equal(_bits([got[1], got[2], got[4]]), _bits([ref[1], ref[2], ref[4]])), (got[1:], ref[1:])


def _record(sol, r):
    return (sol, r["objective"], r["penalized_objective"], r["selected_count"], r["selection_penalty"])


@pytest.mark.parametrize("group", ["fixed", "ties", "costs", "calib"])
def test_case_table_equals_the_reference(product, golden, group):
    """fixed: n = 1, 2, around the 32 steps of a backtrace word, the 64 lanes and the 1024-step LDS tile (n - 1 = T-1, T, T+1,
    2T, 2T+1), penalties below / inside / above the scores, n = 1 with s >, <, == p.  ties: integer scores, all-equal scores,
    alternating +-1.  costs: non-constant switch costs through csolvePenalizedChainROCCO / ccalibrateSelectionPenaltyROCCO.
    calib: targets 0 and n, budgets 0.01 / 0.3 / 0.99 / < 0 / > 1, maxIter 0 / 1 / 7 / 60 / 100, the expansion loop."""
    bad = []
    for c in rocco_cases.cases():
        if c["group"] == group and not rocco_cases.same(rocco_cases.run_case(product, c), golden[c["name"]]):
            bad.append(c["name"])
    assert bad == []


def test_the_expansion_loop_case_returns_the_reference_penalty(product, golden):
    got = product.ccalibrateSelectionPenaltyROCCO([1e17, 2e17], [0.0], 1, 60)
    ref = twin_rocco.ccalibrateSelectionPenaltyROCCO([1e17, 2e17], [0.0], 1, 60)
    assert _bits(got[0]) == _bits(ref[0]) == _bits(golden["calib_expand"]["floats"][2])
    assert np.array_equal(got[1], ref[1]) and _bits(got[2]) == _bits(ref[2]) and got[3] == ref[3] == 1


def test_the_result_does_not_depend_on_the_speculation_depth(product):
    from consenrich_amd import rocco

    s = np.random.default_rng(77).normal(0.0, 1.0, 3001)
    ref = twin_rocco.csolveChromROCCOExact(s, budget=0.07, gamma=0.5, maxIter=61)
    try:
        for depth in (1, 0, 8, 5):
            rocco.set_depth(depth)
            _same_tuple(product.csolveChromROCCOExact(s, budget=0.07, gamma=0.5, maxIter=61), ref)
    finally:
        rocco.set_depth(0)
    with pytest.raises(Exception, match="depth"):
        rocco.set_depth(9)


BATCH_LENS = [1, 33, 1025, 4097, 70001]


@pytest.fixture(scope="module")
def batch_scores():
    rng = np.random.default_rng(11)
    return [rng.normal(0.0, 1.0, n) for n in BATCH_LENS]


def test_a_batch_with_a_mode_per_chain_equals_single_chain_calls(product, batch_scores):
    from consenrich_amd.batch import DeviceBatch, ModelParams

    budget = [None, 0.2, 0.05, None, None]
    penalty = [0.3, None, None, None, 1.1]
    gamma = [0.5, 0.0, 2.0, 0.25, 0.5]
    iters = [60, 7, 60, 60, 60]
    with DeviceBatch(0) as b:
        b.configure(ModelParams(state_dim=2), 2, BATCH_LENS)
        for c, s in enumerate(batch_scores):
            b.upload_scores(c, s)
        res = b.rocco(budget=budget, gamma=gamma, selection_penalty=penalty, max_iter=iters)
        first = [_record(b.rocco_solution(c), res[c]) for c in range(len(BATCH_LENS))]
        for c, s in enumerate(batch_scores):
            single = product.csolveChromROCCOExact(s, budget=budget[c], gamma=gamma[c], selectionPenalty=penalty[c],
                                                   maxIter=iters[c])
            _same_tuple(first[c], single)
            if BATCH_LENS[c] <= 4097:
                _same_tuple(first[c], twin_rocco.csolveChromROCCOExact(s, budget=budget[c], gamma=gamma[c],
                                                                       selectionPenalty=penalty[c], maxIter=iters[c]))
        # the 70 001-bin chain against the twin: one sequential pass (fixed penalty)
        _same_tuple(first[4], twin_rocco.csolveChromROCCOExact(batch_scores[4], gamma=0.5, selectionPenalty=1.1))
        # a chain mask: only chains 1 and 3 are solved again (other parameters); the others keep their masks
        res2 = b.rocco(budget=0.5, gamma=1.0, chains=[False, True, False, True, False])
        assert [r is None for r in res2] == [True, False, True, False, True]
        for c in (0, 2, 4):
            assert np.array_equal(b.rocco_solution(c), first[c][0])
        for c in (1, 3):
            _same_tuple(_record(b.rocco_solution(c), res2[c]),
                        twin_rocco.csolveChromROCCOExact(batch_scores[c], budget=0.5, gamma=1.0))


@pytest.mark.parametrize("kind", ["random", "zeros", "ones"])
def test_run_bounds_equal_the_twin(product, kind):
    from consenrich_amd.batch import DeviceBatch, ModelParams

    n = 5003
    rng = np.random.default_rng(5)
    # penalties that leave a mixed mask / nothing / everything selected
    s = rng.normal(0.0, 1.0, n)
    pen = {"random": 0.2, "zeros": 100.0, "ones": -100.0}[kind]
    with DeviceBatch(0) as b:
        b.configure(ModelParams(state_dim=2), 2, [n, 40])
        b.upload_scores(0, s)
        b.upload_scores(1, np.ones(40))
        b.rocco(gamma=0.1, selection_penalty=pen)
        sol = b.rocco_solution(0)
        assert {"random": 0 < sol.sum() < n, "zeros": sol.sum() == 0, "ones": sol.sum() == n}[kind]
        for gap in (0, 1, 3):
            got, ref = b.rocco_runs(0, gap), twin_rocco.cBooleanRunBounds(sol, gap)
            assert got[0].dtype == np.int64 and np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])


@pytest.fixture(scope="module")
def fitted():
    """a small fitted batch: (batch, chain lengths); closed when the module's tests are done"""
    from consenrich_amd import _lib as L
    from consenrich_amd.batch import DeviceBatch, ModelParams

    n_list, m = [3000, 65, 1500], 3
    b = DeviceBatch(0)
    b.configure(ModelParams(state_dim=2), m, n_list)
    for c, n in enumerate(n_list):
        d_, v_ = cases.synth(n, m, 4100 + c)
        if c == 2:
            d_ = d_ - 50.0      # a chain whose smoothed level is negative everywhere: no floor in lower_confidence
        b.upload(c, d_, v_)
    b.stats()
    b.forward_backward(L.RETURN_NLL)
    b.export(L.EXPORT_FORWARD | L.EXPORT_SMOOTH)
    yield b, n_list
    b.close()


def test_scores_from_the_resident_fit(product, fitted):
    b, n_list = fitted
    xs = [b.download(c, "xs") for c in range(len(n_list))]
    Ps = [b.download(c, "Ps") for c in range(len(n_list))]
    b.rocco_scores("state")
    res = b.rocco(budget=0.1, gamma=0.5)
    for c in range(len(n_list)):
        sc = xs[c][:, 0].astype(np.float64)
        assert np.array_equal(_bits(b.download_scores(c)), _bits(sc))
        _same_tuple(_record(b.rocco_solution(c), res[c]), twin_rocco.csolveChromROCCOExact(sc, budget=0.1, gamma=0.5))
    z = 1.7
    b.rocco_scores("lower_confidence", z=z)
    res = b.rocco(budget=0.1, gamma=0.5)
    for c in range(len(n_list)):
        unc = np.sqrt(Ps[c][:, 0, 0])
        assert unc.dtype == np.float32
        sc = twin_rocco.score_track(xs[c][:, 0], unc, "lower_confidence", z)
        assert np.array_equal(_bits(b.download_scores(c)), _bits(sc))
        _same_tuple(_record(b.rocco_solution(c), res[c]), twin_rocco.csolveChromROCCOExact(sc, budget=0.1, gamma=0.5))
    assert float(np.max(xs[2][:, 0])) <= 0.0        # chain 2 takes the branch without a floor


def test_the_floor_branch_of_lower_confidence(product, fitted):
    """z large enough that raw = xs0 - z sqrt(Ps00) falls below -2 max(xs0) somewhere: those bins are floored"""
    b, n_list = fitted
    xs, Ps = b.download(0, "xs"), b.download(0, "Ps")
    assert float(np.max(xs[:, 0])) > 0.0
    unc = np.sqrt(Ps[:, 0, 0])
    z = float(4.0 * np.max(xs[:, 0]) / np.min(unc[unc > 0]))
    b.rocco_scores("lower_confidence", z=z)
    sc = twin_rocco.score_track(xs[:, 0], unc, "lower_confidence", z)
    assert np.any(sc == -2.0 * float(np.max(xs[:, 0])))
    assert np.array_equal(_bits(b.download_scores(0)), _bits(sc))


def test_peak_selection_leaves_the_fit_resident(product, fitted):
    from consenrich_amd import _lib as L
    from consenrich_amd import driver

    b, n_list = fitted
    names = ("D", "xf", "Pf", "pnoise", "xs", "Ps", "lag")
    before = {(c, a): b.download(c, a) for c in range(len(n_list)) for a in names}
    inputs = [b.download_inputs(c) for c in range(len(n_list))]
    peaks = driver.call_peaks_batch(b, budget=0.05, gamma=0.5, score_mode="lower_confidence", z=1.0, max_gap_bins=1)
    for c, r in enumerate(peaks):
        sol = b.rocco_solution(c)
        ref = twin_rocco.cBooleanRunBounds(sol, 1)
        assert np.array_equal(r["starts"], ref[0]) and np.array_equal(r["ends"], ref[1]) and r["selected_count"] == int(sol.sum())
    for (c, a), v in before.items():
        assert np.array_equal(b.download(c, a).view(np.uint32), v.view(np.uint32)), (c, a)
    for c, (d_, v_) in enumerate(inputs):
        got = b.download_inputs(c)
        assert np.array_equal(got[0], d_) and np.array_equal(got[1], v_)
    # a step afterwards returns what a step returned before the selection existed
    what = L.EXPORT_FORWARD | L.EXPORT_SMOOTH
    sums1 = b.step(L.RETURN_NLL, what)
    after1 = {(c, a): b.download(c, a) for c in range(len(n_list)) for a in names}
    driver.call_peaks_batch(b, budget=0.05, gamma=0.5)
    sums2 = b.step(L.RETURN_NLL, what)
    for k in range(2):
        assert np.array_equal(_bits(sums1[k]), _bits(sums2[k]))
    for (c, a), v in after1.items():
        assert np.array_equal(b.download(c, a).view(np.uint32), v.view(np.uint32)), (c, a)


def test_scores_without_a_prior_export_of_the_smoothed_fit(product):
    """rocco_scores makes the reference-layout copies of xs / Ps itself when no export has; the fit's values are what a later
    export returns"""
    from consenrich_amd import _lib as L
    from consenrich_amd.batch import DeviceBatch, ModelParams

    n_list, m = [700, 130], 2
    with DeviceBatch(0) as b:
        b.configure(ModelParams(state_dim=2), m, n_list)
        for c, n in enumerate(n_list):
            b.upload(c, *cases.synth(n, m, 4300 + c))
        b.stats()
        b.forward_backward(L.RETURN_NLL)
        b.rocco_scores("lower_confidence", z=0.5)
        got = [b.download_scores(c) for c in range(2)]
        b.export(L.EXPORT_SMOOTH)
        for c in range(2):
            xs, Ps = b.download(c, "xs"), b.download(c, "Ps")
            sc = twin_rocco.score_track(xs[:, 0], np.sqrt(Ps[:, 0, 0]), "lower_confidence", 0.5)
            assert np.array_equal(_bits(got[c]), _bits(sc))
        with pytest.raises(ValueError, match="uncertaintyScoreZ"):
            b.rocco_scores("lower_confidence", z=-1.0)


def test_errors_of_the_batch_calls(product):
    from consenrich_amd import _lib as L
    from consenrich_amd.batch import DeviceBatch, ModelParams

    with DeviceBatch(0) as b:
        b.configure(ModelParams(state_dim=2), 2, [10, 20])
        with pytest.raises(L.ConsenrichAMDError, match="no scores"):
            b.rocco(budget=0.5)
        with pytest.raises(L.ConsenrichAMDError, match="no smoothed results"):
            b.rocco_scores("state")
        b.upload_scores(0, np.arange(10.0))
        with pytest.raises(L.ConsenrichAMDError, match="chain 1 has no scores"):
            b.rocco(budget=0.5)
        b.rocco(budget=0.5, chains=[True, False])
        with pytest.raises(L.ConsenrichAMDError, match="no ROCCO solution"):
            b.rocco_solution(1)
        with pytest.raises(ValueError, match="`gamma` must be finite and non-negative"):
            b.rocco(budget=0.5, gamma=-1.0, chains=[True, False])
