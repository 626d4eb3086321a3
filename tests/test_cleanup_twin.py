"""The massive sub-peak clean-up without a GPU: both forms of the pure-Python twin against the fixtures the reference's own
functions made (tests/golden/make_cleanup_golden.py), and the package's host drop-ins for the width policy against them bit for
bit, with the same keys, key order and Python types."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import cleanup_cases as CC  # noqa: E402
import cleanup_compare as CMP  # noqa: E402
import twin_cleanup as T  # noqa: E402

from consenrich_amd import cleanup as K  # noqa: E402

LONG = ("beyond_tile",)     # (the pure-Python merge network over 6444 values takes seconds: the steps form of that case is left to the fixture maker)


@pytest.mark.parametrize("name,form", [(n, f) for n in CMP.force_ids() for f in ("steps", "device") if (n, f) != (LONG[0], "steps")])
def test_force_twin_matches_the_reference(name, form):
    CMP.check_force(lambda **kw: T.force(form=form, **kw), name)


def test_uniform_step_path_gives_identical_records():
    for name in ("two_plateaus", "comb", "flat", "core"):
        CMP.check_force(lambda **kw: T.force(form="device", coords="step", **kw), name)


@pytest.mark.parametrize("form", ["steps", "device"])
def test_piece_twins_match_the_reference(form):
    CMP.check_splits(lambda **kw: T.best_split(form=form, **kw))
    CMP.check_contracts(lambda **kw: T.contract_segment(form=form, **kw))


def test_nonfinite_candidate_raises_in_both_forms():
    for form in ("steps", "device"):
        with pytest.raises(ValueError) as e:
            T.force(form=form, **CC.nonfinite_inputs())
        assert str(e.value) == "`scores` contains non-finite values"


def test_network_sort_sorts_any_length():
    rng = np.random.default_rng(5)
    for n in list(range(0, 40)) + [63, 64, 65, 127, 129, 500]:
        v = np.round(rng.standard_normal(n) * 4.0) / 4.0
        assert T.network_sort([float(x) for x in v]) == sorted(float(x) for x in v)


@pytest.mark.parametrize("case", CC.POLICIES, ids=[c["name"] for c in CC.POLICIES])
def test_host_policy_drop_ins_match_the_reference(case):
    kw = {k: v for k, v in case.items() if k != "name"}
    name = case["name"]
    d = K.learn_massive_subpeak_width_policy(**kw)
    want = CMP.golden("policy", name)
    flat = T.flatten_policy(d)
    assert T.same_flat({f"policy_{k}": v for k, v in flat.items()}, {k: v for k, v in want.items() if k.startswith("policy_")}) == []
    assert ("num_width_tail_gap_candidates" in d) == bool(d["active"])
    w = np.asarray(kw["widthsBP"], np.float64)
    w = w[np.isfinite(w) & (w > 0.0)]
    p, q, null = K.massive_subpeak_width_scores(w, **({"bulkQuantile": kw["bulkQuantile"]} if "bulkQuantile" in kw else {}))
    assert type(null["center"]) is float and type(null["scale"]) is float and list(null) == ["center", "scale"]
    got = {"p": np.asarray(p, np.float64), "q": np.asarray(q, np.float64), "null": np.asarray([null["center"], null["scale"]], np.float64)}
    pv = [K.massive_subpeak_width_pvalue(float(v), d) for v in (0.5, 1.0, 800.0, 7500.0, 1.0e5)]
    assert all(b is None and (a is None or type(a) is float) for a, b in pv)
    got["pvalue"] = np.asarray([float("nan") if a is None else a for a, _ in pv], np.float64)
    assert T.same_flat(got, {k: v for k, v in want.items() if not k.startswith("policy_")}) == []


def test_width_pvalue_without_a_null():
    assert K.massive_subpeak_width_pvalue(900.0, None) == (None, None)
    assert K.massive_subpeak_width_pvalue(900.0, {"null_center": 6.0, "null_scale": 0.0}) == (None, None)
    assert K.massive_subpeak_width_pvalue(900.0, {"null_center": 6.0}) == (None, None)
    with pytest.raises(RuntimeError, match="width-score p-values contain non-finite values"):
        K.massive_subpeak_width_scores([500.0, float("nan"), 700.0])


@pytest.mark.parametrize("form", ["steps", "device"])
@pytest.mark.parametrize("name", CMP.row_ids())
def test_rows_twin_under_a_policy_matches_the_reference(name, form):
    """parents, children, forced segments and the finishing step per segment, against the reference's own rows"""
    CMP.check_rows(lambda **kw: T.rows(form=form, **kw), name)
