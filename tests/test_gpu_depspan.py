"""GPU tests of the dependence span on the device (run with -m gpu): the drop-in `cchooseDependenceSpan`, the same estimate from
the resident matrices of a batch, and the three device stages underneath.  References: the compiled reference's recorded results
(tests/golden/depspan) for every discrete field, score, rank, radius and bootstrap list, compared exactly; the truth twin
(tests/twin_depspan.py: the same steps with exact long-double lag sums) for the continuous quantities, which may be no further
from the truth than the reference's FFT route is (the golden's e_ref / e_strength / e_revival, with a floor of 1e-15: two
divisions and two near-exact sums on values of magnitude at most 1)."""
import json
import os

import numpy as np
import pytest

import depspan_cases as DC
import twin_depspan as T
from conftest import gpu_available

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "depspan")
CASES = {c["name"]: c for c in DC.cases()}
FLOOR = 1.0e-15


@pytest.fixture(scope="module")
def D():
    if not gpu_available():
        pytest.fail("GPU tests selected but no HIP device / library: the product has no CPU fallback")
    from consenrich_amd import depspan

    return depspan


def golden(name):
    with np.load(os.path.join(GOLDEN, f"depspan_{name}.npz")) as z:
        return {"result": json.loads(str(z["result"])), "sha": str(z["sha"]), "e_ref": float(z["e_ref"]),
                "e_strength": float(z["e_strength"]), "e_revival": float(z["e_revival"])}


def plain(result):
    return json.loads(json.dumps(T.strip(result)))


_CACHE = {}


def prepared(name):
    """(names, matrices, golden, truth twin's result and backend) of a case, computed once."""
    if name not in _CACHE:
        names, mats = DC.build_any(CASES[name])
        g = golden(name)
        assert DC.input_sha(mats) == g["sha"]
        truth, backend = T.run(names, mats, CASES[name]["interval"], route="truth", **CASES[name]["kw"])
        _CACHE[name] = (names, mats, g, plain(truth), backend)
    return _CACHE[name]


def check_against_golden(result, name, decided_on_host):
    names, mats, g, truth, _ = prepared(name)
    got = plain(result)
    assert T.discrete_differences(g["result"], got) == []
    e_s, e_r = T.continuous_error(truth, got, "oscillationStrength"), T.continuous_error(truth, got, "postCrossingRevival")
    print(name, "oscillationStrength error", e_s, "allowed", max(g["e_strength"], FLOOR), "postCrossingRevival error", e_r,
          "allowed", max(g["e_revival"], FLOOR))
    assert e_s <= max(g["e_strength"], FLOOR)
    assert e_r <= max(g["e_revival"], FLOOR)
    assert result[3]["decided_on_host"] == decided_on_host


@pytest.mark.parametrize("name", list(CASES))
def test_drop_in_equals_the_goldens(D, name):
    names, mats, g, _, _ = prepared(name)
    keep = [m.copy() for m in mats]
    result = D.cchooseDependenceSpan(names, mats, CASES[name]["interval"], **CASES[name]["kw"])
    check_against_golden(result, name, 0)
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(mats, keep))


@pytest.mark.parametrize("name", list(CASES))
def test_stages_rows_scores_and_pooled_acf(D, name):
    """The three stages on their own, through the host-array entry: the retained rows and every window score equal the twin's
    bit for bit; every evaluated window's record equals the truth twin's and its pooled ACF is within the reference's own error of it."""
    names, mats, g, _, tb = prepared(name)
    st = T.settings(len(names), len(mats), CASES[name]["interval"], CASES[name]["kw"])
    eligible, _ = D.eligible_autosomes(names, [m.shape[1] for m in mats], st.window_bins)
    dev = D.HostArrayBackend(mats, st)
    dev.open([p for _, _, p in eligible])
    rows = dev.unique_rows()
    assert rows == tb.unique_rows()
    score, count = dev.window_scores(rows)
    want_score, want_count = tb.window_scores(rows)
    assert np.array_equal(count, want_count)
    assert np.array_equal(score.view(np.uint64)[count > 0], want_score.view(np.uint64)[count > 0])
    keys = sorted(tb.windows)
    recs, pooled = dev.window_acf(rows, keys)
    worst = 0.0
    for k, key in enumerate(keys):
        want = tb.windows[key]
        for f in ("status", "valid_rows", "support_cap_lag"):
            assert int(recs[k][f]) == int(want[f]), (key, f)
        if not want["status"]:
            continue
        for f in ("crossing_lag", "last_crossing_start", "valid_rows_at_crossing"):
            assert int(recs[k][f]) == int(want[f]), (key, f)
        assert float(recs[k]["finite_pair_min"]) == want["finite_pair_min"]
        assert float(recs[k]["finite_pair_coverage_min"]) == want["finite_pair_coverage_min"]
        assert int(recs[k]["flags"]) == 0
        assert abs(float(recs[k]["margin"]) - want["margin"]) <= 1.0e-12
        assert np.array_equal(np.isnan(pooled[k]), np.isnan(want["pooled"])), key
        fin = np.isfinite(want["pooled"])
        worst = max(worst, float(np.max(np.abs(pooled[k][fin] - want["pooled"][fin]))))
    print(name, "pooled ACF: device against truth", worst, "reference against truth", g["e_ref"])
    assert worst <= max(g["e_ref"], FLOOR)


@pytest.mark.parametrize("name", ["base", "outcomes", "single_row"])
def test_forced_host_route_gives_the_goldens_again(D, name):
    names, mats, g, _, _ = prepared(name)
    result = D.cchooseDependenceSpan(names, mats, CASES[name]["interval"], _margin=float("inf"), **CASES[name]["kw"])
    check_against_golden(result, name, g["result"][3]["selectedWindowCount"])


def test_period_diagnostics_off(D):
    names, mats, g, _, _ = prepared("tile_edges")
    result = D.cchooseDependenceSpan(names, mats, CASES["tile_edges"]["interval"], period_diagnostics=False, **CASES["tile_edges"]["kw"])
    assert all(w["dominantACFPeriodBP"] is None and w["oscillationStrength"] is None for w in result[3]["selectedWindows"])
    assert result[3]["dominantACFPeriodBPMedian"] is None and result[3]["unresolvedPeriodFraction"] == 1.0
    assert T.discrete_differences(g["result"], plain(result), skip_period=True) == []


def test_runtime_errors(D):
    with np.load(os.path.join(GOLDEN, "depspan_errors.npz")) as z:
        for case, text in DC.runtime_error_cases():
            with pytest.raises(RuntimeError) as err:
                DC.call(D.cchooseDependenceSpan, case)
            assert str(err.value) == str(z[case["name"]])


def _batch_of(mats, m):
    from consenrich_amd.batch import DeviceBatch, ModelParams

    b = DeviceBatch(0)
    b.configure(ModelParams(state_dim=2), m, [x.shape[1] for x in mats])
    for c, x in enumerate(mats):
        b.upload(c, x, np.ones_like(x))
    return b


@pytest.mark.parametrize("name", ["base", "row_rules", "long_window"])
def test_batch_form_equals_the_goldens_and_leaves_the_data_resident(D, name):
    """`DeviceBatch.dependence_span` on the resident matrices: the host-array form's result, the resident data byte-identical
    afterwards.  In `base` the chains are listed without the last one, the way a fold chain is left out."""
    names, mats, g, _, _ = prepared(name)
    with _batch_of(mats, mats[0].shape[0]) as b:
        before = [b.download_inputs(c)[0] for c in range(len(mats))]
        assert all(np.array_equal(a.view(np.uint32), x.view(np.uint32)) for a, x in zip(before, mats))
        result = b.dependence_span(names, CASES[name]["interval"], **CASES[name]["kw"])
        check_against_golden(result, name, 0)
        after = [b.download_inputs(c)[0] for c in range(len(mats))]
        assert all(np.array_equal(a.view(np.uint32), x.view(np.uint32)) for a, x in zip(before, after))
        host = D.cchooseDependenceSpan(names, mats, CASES[name]["interval"], **CASES[name]["kw"])
        assert T.discrete_differences(plain(host), plain(result)) == []
        assert plain(host) == plain(result)
        if name == "base":      # chr3 (shorter than a window) left out by not listing it: it no longer shows as excluded
            part = b.dependence_span(names[:3], CASES[name]["interval"], chains=[0, 1, 2], **CASES[name]["kw"])
            assert part[3]["chromosomesExcluded"] == ["chrX"]
            assert part[3]["radiusDistributionBP"] == result[3]["radiusDistributionBP"] and part[:3] == result[:3]


def test_forced_host_route_through_the_batch(D):
    """`_margin=inf` on resident data: every selected window is re-decided from rows downloaded from the batch (the chain and row
    mapping of `BatchBackend.window_rows`; `base` has chains out of ordinal order, a chain that is not eligible in between and a
    dropped duplicate row), and the goldens come out again."""
    names, mats, g, _, _ = prepared("base")
    with _batch_of(mats, mats[0].shape[0]) as b:
        result = b.dependence_span(names, CASES["base"]["interval"], _margin=float("inf"), **CASES["base"]["kw"])
        check_against_golden(result, "base", g["result"][3]["selectedWindowCount"])


def test_dependence_span_batch_feeds_the_first_pass(D):
    """A small fitted batch: `driver.dependence_span_batch` yields the golden's span from the resident data of the fit, and
    `first_pass_peaks_batch` accepts its `span_intervals`."""
    import math

    from consenrich_amd import _lib as L
    from consenrich_amd import driver

    name = "ties"
    names, mats, g, _, _ = prepared(name)
    interval = CASES[name]["interval"]
    with _batch_of(mats, mats[0].shape[0]) as b:
        b.stats()
        b.forward_backward(L.RETURN_NLL)
        b.export(L.EXPORT_FORWARD | L.EXPORT_SMOOTH)
        out = driver.dependence_span_batch(b, names, interval, **CASES[name]["kw"])
        assert [out["point"], out["lower"], out["upper"]] == g["result"][:3]
        assert T.discrete_differences(g["result"], plain((out["point"], out["lower"], out["upper"], out["diagnostics"]))) == []
        assert out["span_intervals"] == int(math.ceil(g["result"][3]["workingSpanBP"] / interval))
        assert out["context_bp"] == 2 * out["span_intervals"] * interval + 1
        first = driver.first_pass_peaks_batch(b, dependence_spans=out["span_intervals"], threshold_z=2.0,
                                              threshold_z_grid=(1.5, 2.0, 2.5, 3.0), num_bootstrap=9, random_seed=5, gamma=-1.0,
                                              gamma_scale=0.5, score_mode="state", z=1.0, max_gap_bins=0)
        assert len(first) == len(mats)
        assert all(r["budget_details"]["dependence_span"] == max(out["span_intervals"], 2) for r in first)
