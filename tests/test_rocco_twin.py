"""CPU: the pure-Python twin of the ROCCO natives (tests/twin_rocco.py) equals the compiled reference's recorded outputs on
every case of the table, bit for bit, and the drop-in wrappers raise the reference's errors before any GPU call."""
import os

import numpy as np
import pytest

import rocco_cases
import twin_rocco

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(rocco_cases.__file__)), "rocco")
GROUPS = ("fixed", "ties", "costs", "calib")


@pytest.fixture(scope="module")
def golden():
    out = {}
    for g in GROUPS:
        out.update(rocco_cases.load_group(os.path.join(GOLDEN, f"rocco_{g}.npz")))
    return out


def test_every_case_has_a_fixture(golden):
    assert sorted(golden) == sorted(c["name"] for c in rocco_cases.cases())


@pytest.mark.parametrize("group", GROUPS)
def test_twin_equals_the_reference(golden, group):
    bad = [c["name"] for c in rocco_cases.cases() if c["group"] == group
           and not rocco_cases.same(rocco_cases.run_case(twin_rocco, c), golden[c["name"]])]
    assert bad == []


def test_the_expansion_case_leaves_the_initial_bracket(golden):
    """scores = [1e17, 2e17]: lower = scoreMin - 0 - 1 rounds onto scoreMin, one bin is selected there, and 1 <= target makes the
    reference's `while lowerCount <= targetCount_` loop run; the penalty it returns is recorded bit for bit."""
    case = next(c for c in rocco_cases.cases() if c["name"] == "calib_expand")
    s, _ = rocco_cases.inputs(case)
    assert s[0] - 0.0 - 1.0 == s[0]
    assert twin_rocco.csolvePenalizedChainROCCO(s, [0.0], s[0])[2] <= case["target"]
    assert int(golden["calib_expand"]["count"][0]) == 1


@pytest.fixture(scope="module")
def product():
    from consenrich_amd import build

    build.build()
    from consenrich_amd import cconsenrich

    return cconsenrich


@pytest.mark.parametrize("who", ["product", "twin"])
def test_wrappers_raise_the_reference_errors_without_a_gpu(product, who):
    mod = product if who == "product" else twin_rocco
    s = np.arange(5.0)
    cost = np.full(4, 0.5)
    for f, extra in ((mod.csolvePenalizedChainROCCO, (0.1,)), (mod.ccalibrateSelectionPenaltyROCCO, (2,))):
        with pytest.raises(ValueError, match="`scores` cannot be empty"):
            f([], [], *extra)
        with pytest.raises(ValueError, match="`scores` contains non-finite values"):
            f([1.0, np.nan, 2.0, 3.0, 4.0], cost, *extra)
        with pytest.raises(ValueError, match="`switchCosts` contains non-finite values"):
            f(s, [0.5, np.inf, 0.5, 0.5], *extra)
        with pytest.raises(ValueError, match=r"`switchCosts` must have length len\(scores\) - 1"):
            f(s, cost[:3], *extra)
    with pytest.raises(ValueError, match="`scores` cannot be empty"):
        mod.csolveChromROCCOExact([])
    with pytest.raises(ValueError, match="`scores` contains non-finite values"):
        mod.csolveChromROCCOExact([0.0, np.inf])
    for g in (-0.1, np.nan, np.inf):
        with pytest.raises(ValueError, match="`gamma` must be finite and non-negative"):
            mod.csolveChromROCCOExact(s, budget=0.5, gamma=g)
    with pytest.raises(ValueError, match="`budget` must be finite"):
        mod.csolveChromROCCOExact(s, budget=np.nan)
    # `int targetCount`, `int maxIter` are C ints in the reference
    for args in ((s, cost, 2 ** 31, 60), (s, cost, 2, 2 ** 31), (s, cost, -2 ** 31 - 1, 60)):
        with pytest.raises(OverflowError, match="value too large to convert to int"):
            mod.ccalibrateSelectionPenaltyROCCO(*args)
    with pytest.raises(OverflowError, match="value too large to convert to int"):
        mod.csolveChromROCCOExact(s, budget=0.5, maxIter=2 ** 40)


def test_the_callables_are_exported_by_the_drop_in_module(product):
    for name in ("csolvePenalizedChainROCCO", "ccalibrateSelectionPenaltyROCCO", "csolveChromROCCOExact"):
        assert name in product.__all__ and callable(getattr(product, name))


def test_run_bounds_twin():
    m = np.array([0, 1, 1, 0, 1, 0, 0, 1, 0, 0, 0, 1], np.uint8)
    assert [a.tolist() for a in twin_rocco.cBooleanRunBounds(m, 0)] == [[1, 4, 7, 11], [2, 4, 7, 11]]
    assert [a.tolist() for a in twin_rocco.cBooleanRunBounds(m, 1)] == [[1, 7, 11], [4, 7, 11]]
    assert [a.tolist() for a in twin_rocco.cBooleanRunBounds(m, 3)] == [[1], [11]]
    assert [a.tolist() for a in twin_rocco.cBooleanRunBounds(np.zeros(4, np.uint8), 2)] == [[], []]
