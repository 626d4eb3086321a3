"""The dependence span without a GPU: the NumPy twins (tests/twin_depspan.py) and the host steps of consenrich_amd/depspan.py
against the goldens of the compiled reference (tests/golden/depspan, made by tests/golden/make_depspan_golden.py), and the
validations and error texts of the drop-in, which come before the device is asked for."""
import json
import os

import numpy as np
import pytest

import depspan_cases as DC
import twin_depspan as T
from consenrich_amd import depspan as D

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "depspan")
CASES = {c["name"]: c for c in DC.cases()}


def golden(name):
    with np.load(os.path.join(GOLDEN, f"depspan_{name}.npz")) as z:
        return {"result": json.loads(str(z["result"])), "sha": str(z["sha"]), "e_ref": float(z["e_ref"]),
                "e_strength": float(z["e_strength"]), "e_revival": float(z["e_revival"]), "min_margin": float(z["min_margin"])}


def plain(result):
    return json.loads(json.dumps(T.strip(result)))


@pytest.fixture(scope="module")
def inputs():
    return {name: DC.build_any(case) for name, case in CASES.items()}


@pytest.mark.parametrize("name", list(CASES))
def test_inputs_are_the_goldens_inputs(name, inputs):
    assert DC.input_sha(inputs[name][1]) == golden(name)["sha"]


@pytest.mark.parametrize("route", ["fft", "truth"])
@pytest.mark.parametrize("name", list(CASES))
def test_twin_equals_reference(name, route, inputs):
    g = golden(name)
    names, mats = inputs[name]
    assert DC.input_sha(mats) == g["sha"]
    got = plain(T.run(names, mats, CASES[name]["interval"], route=route, **CASES[name]["kw"])[0])
    assert T.discrete_differences(g["result"], got) == []
    # the FFT twin repeats the reference's arithmetic; the truth twin is as far from it as the reference is from the truth
    bound = {"fft": (1.0e-12, 1.0e-12), "truth": (max(g["e_strength"], 1e-15), max(g["e_revival"], 1e-15))}[route]
    assert T.continuous_error(g["result"], got, "oscillationStrength") <= bound[0]
    assert T.continuous_error(g["result"], got, "postCrossingRevival") <= bound[1]


def test_goldens_cover_the_outcomes():
    d = golden("outcomes")["result"][3]
    assert d["supportCensoredWindowCount"] >= 1 and d["capCensoredWindowCount"] >= 1
    assert d["selectedWindowCount"] == d["evaluatedCandidateWindowCount"] - 1      # the constant window answers None
    assert golden("base")["result"][3]["duplicateRowCount"] == 1
    assert golden("base")["result"][3]["chromosomesExcluded"] == ["chr3", "chrX"]
    ranks = [w["positiveSignalRank"] for w in golden("ties")["result"][3]["selectedWindows"]]
    assert any(r != int(r) for r in ranks)                                          # a tied pair shares a half rank
    assert golden("row_rules")["result"][3]["candidateWindowCount"] == 19          # the window no row covers is no candidate
    assert any(w["dominantACFPeriodBP"] is not None for w in golden("tile_edges")["result"][3]["selectedWindows"])
    s = golden("contract_shortened")["result"][3]
    assert (s["candidateWindowCount"], s["evaluatedCandidateWindowCount"], s["selectedWindowCount"]) == (12, 12, 11)
    for name in CASES:
        assert golden(name)["min_margin"] >= 1.0e-9
        assert D.MARGIN >= 100.0 * golden(name)["e_ref"]


def test_long_window_sum_is_a_fold_of_pairwise_chunks():
    """np.sum of one contiguous float64 array longer than 8192 is the ascending fold of the pairwise sums of chunks of 8192 (one
    pairwise tree over the whole array gives another last bit at 8193 values): the rule the device's np_sum_f states,
    written out here and compared with np.sum itself."""
    def leaf(x):
        n = x.size
        if n < 8:
            res = 0.0
            for v in x:
                res = res + float(v)
            return res
        r = [float(v) for v in x[:8]]
        i = 8
        while i < n - (n % 8):
            for k in range(8):
                r[k] = r[k] + float(x[i + k])
            i += 8
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
        for v in x[i:]:
            res = res + float(v)
        return res

    def tree(x):
        if x.size <= 128:
            return leaf(x)
        n2 = x.size // 2
        n2 -= n2 % 8
        return tree(x[:n2]) + tree(x[n2:])

    rng = np.random.default_rng(3)
    for n in (5, 127, 129, 4000, 8192, 8193, 8448, 20011):
        x = (rng.random(n) - 0.25) * 1000.0
        total = tree(x[:8192])
        for c0 in range(8192, n, 8192):
            total = total + tree(x[c0:c0 + 8192])
        assert total == float(np.sum(x)), n


@pytest.mark.parametrize("entry", DC.value_error_cases(), ids=lambda e: e[0])
def test_value_errors_before_the_device(entry):
    name, names, mats, interval, kw, text = entry
    with np.load(os.path.join(GOLDEN, "depspan_errors.npz")) as z:
        assert str(z[name]) == text
    with pytest.raises(ValueError) as err:
        D.cchooseDependenceSpan(names if names is not None else 5, mats, interval, **kw)
    assert str(err.value) == text


def test_type_error_for_values_float32_cannot_hold():
    m = np.zeros((2, 600), dtype=np.float64)
    m[0, 3] = 0.1
    with pytest.raises(TypeError, match="float32"):
        D.cchooseDependenceSpan(["chr1"], [m], 1, windowBP=100, maxLagBP=50, acfSmoothingBP=5, crossingPersistenceBP=5,
                                minFinitePairs=10, windowCount=4, minWindowCount=2, bootstrapDraws=5)
    assert D._as_float32(np.arange(12, dtype=np.int64).reshape(2, 6)).dtype == np.float32


def test_runtime_error_texts():
    with np.load(os.path.join(GOLDEN, "depspan_errors.npz")) as z:
        for case, text in DC.runtime_error_cases():
            with pytest.raises(RuntimeError) as err:
                DC.call(T.fft_twin, case)
            assert str(err.value) == str(z[case["name"]]) and text in str(err.value)


def test_host_pieces_given_the_goldens_radii():
    """Kaplan-Meier quantiles, the coordinate runs and the Politis-White block length from the golden's windows alone."""
    for name in CASES:
        d = golden(name)["result"][3]
        radii, censored, windows = d["radiusDistributionBP"], d["radiusCensored"], d["selectedWindows"]
        assert D.km_quantile(radii, censored, 0.5) == d["fullSampleMedianRadiusBP"]
        assert D.km_quantile(radii, censored, d["workingQuantile"]) == d["fullSampleWorkingSpanBP"]
        by_chrom = {}
        for i, w in enumerate(windows):
            by_chrom.setdefault(w["chromosome"], []).append(i)
        block, adjacent, longest = D.bootstrap_geometry(windows, by_chrom, radii, censored)
        assert (block, adjacent, longest) == (d["bootstrapBlockLengthWindows"], d["selectedAdjacencyCount"], d["selectedLongestRun"])
        grid = np.unique(np.asarray(radii))
        s = D.km_survival_at(radii, censored, grid)
        assert np.all(np.diff(s) <= 0.0) and s[0] <= 1.0


def test_reexport_and_signature():
    import inspect

    from consenrich_amd import cconsenrich

    assert cconsenrich.cchooseDependenceSpan is D.cchooseDependenceSpan
    p = inspect.signature(D.cchooseDependenceSpan).parameters
    assert list(p)[:15] == ["chromosomeNames", "chromosomeMatrices", "intervalSizeBP", "windowBP", "windowCount", "maxLagBP",
                            "workingQuantile", "bootstrapDraws", "randSeed", "minWindowCount", "acfThreshold", "acfSmoothingBP",
                            "crossingPersistenceBP", "minFinitePairs", "minFinitePairCoverage"]
    assert [p[k].default for k in list(p)[3:15]] == [100000, 256, 50000, 0.75, 500, 1729, 20, 0.1, 250, 250, 200, 0.5]
    assert p["period_diagnostics"].default is True and p["period_diagnostics"].kind is inspect.Parameter.KEYWORD_ONLY
