"""Both forms of the narrowPeak twin (tests/twin_narrowpeak.py) against the fixtures made from the reference's own functions
(tests/golden/make_narrowpeak_golden.py): floats by bit pattern, integers, strings and key order exactly; and the case table still
takes the branches the device tests rely on."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import narrowpeak_cases as NC  # noqa: E402
import twin_narrowpeak as T  # noqa: E402

GOLD = os.path.join(HERE, "golden", "narrowpeak", "narrowpeak_rows.npz")


def golden(name):
    with np.load(GOLD) as z:
        return {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(name + "/")}


def test_fixture_holds_every_case_and_is_small():
    with np.load(GOLD) as z:
        assert {k.split("/", 1)[0] for k in z.files} == {c["name"] for c in NC.CASES}
    assert os.path.getsize(GOLD) < 256 * 1024


@pytest.mark.parametrize("form", ["steps", "device"])
@pytest.mark.parametrize("case", NC.CASES, ids=lambda c: c["name"])
def test_twin_equals_the_reference(case, form):
    kw = NC.inputs(case)
    with np.errstate(invalid="ignore"):
        got = T.rows(form=form, **kw)
        other = T.rows(form="steps", **kw)
    assert T.differences(got, other) == []
    if kw["returnExportDetails"]:
        assert T.same_flat(T.flatten(got), golden(case["name"])) == []
        assert list(got[2])[-1] == "num_segments_kept"
    else:
        assert len(got) == 2
        full = T.rows(form=form, **{**kw, "returnExportDetails": True})
        assert T.differences(got, full[:2]) == []
    for row in got[0]:
        assert [type(v) for v in row] == [str, int, int, str, int, str, float, int, int, int]


def test_case_table_takes_the_branches():
    seen = {}
    for case in NC.CASES:
        T.reset_branches()
        with np.errstate(invalid="ignore"):
            T.rows(form="device", **NC.inputs(case))
        for k, v in T.BRANCHES.items():
            seen.setdefault(k, []).append(case["name"])
        if case["name"] == "ties":
            assert T.TN.COUNTERS["count_tie"] > 0
        if case["name"] == "near_ties":
            assert T.TN.COUNTERS["tolerance"] > 0
    for k in ("parent_len_1", "parent_len_4", "parent_len_5", "parent_len_6", "parent_len_31", "parent_len_32", "parent_len_33",
              "parent_len_64", "parent_len_65", "gap_inside_run", "children_3plus", "single_child_shorter", "kept_whole", "argmax_tie",
              "trim_left", "trim_right", "trim_both", "trim_none", "trim_summit_below", "median_of_1", "median_of_2", "median_of_3",
              "median_of_4", "uncertainty_some_nonfinite", "uncertainty_none_finite", "dropped_median", "median_equal_threshold",
              "span_floor", "half_way", "dropped_min_bp"):
        assert seen.get(k), k
    assert seen["decided_on_host"] == list(NC.HOST_DECIDED)
