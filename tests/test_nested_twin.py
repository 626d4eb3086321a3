"""Both forms of the nested-refinement twin (tests/twin_nested.py) against the fixtures made from the reference's own functions
(tests/golden/make_nested_golden.py), bit for bit, on every case of tests/nested_cases.py; and the facts about the case table
that the GPU tests rely on."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import nested_cases as NC  # noqa: E402
import twin_nested as T  # noqa: E402

GOLD = os.path.join(HERE, "golden", "nested")


def golden(kind, name):
    with np.load(os.path.join(GOLD, f"nested_{kind}.npz")) as z:
        return {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(name + "/")}


@pytest.fixture(scope="module")
def refined():
    """(mask, details) of every refinement case in both forms: computed once, shared, left unchanged"""
    out = {}
    for case in NC.REFINE:
        kw = NC.refine_inputs(case)
        out[case["name"]] = {form: T.refine(form=form, **kw) for form in ("steps", "device")}
    return out


@pytest.mark.parametrize("form", ["steps", "device"])
@pytest.mark.parametrize("case", NC.SOLVE, ids=lambda c: c["name"])
def test_solver_twin_equals_the_reference(case, form):
    want = golden("solve", case["name"])
    assert want and not T.same_flat(T.flatten_solve(*T.solve(form=form, **NC.solve_inputs(case))), want)


@pytest.mark.parametrize("form", ["steps", "device"])
@pytest.mark.parametrize("case", NC.REFINE, ids=lambda c: c["name"])
def test_refinement_twin_equals_the_reference(refined, case, form):
    want = golden("refine", case["name"])
    assert want and not T.same_flat(T.flatten_refine(*refined[case["name"]][form]), want)


def test_both_forms_agree_on_every_key(refined):
    for name, forms in refined.items():
        assert np.array_equal(forms["steps"][0], forms["device"][0]), name
        assert T.differences(forms["device"][1], forms["steps"][1]) == [], name


def test_case_table_takes_every_branch(refined):
    details = {k: v["steps"][1] for k, v in refined.items()}
    decisions = {n["decision"] for d in details.values() for n in d["hierarchy"]}
    assert decisions == set(T.DECISIONS)
    assert {d["stop_reason"] for d in details.values()} >= {"disabled", "mask_equal", "jaccard", "max_iter"}
    assert details["iters0"]["stop_reason"] == "disabled" and details["mask_equal"]["stop_reason"] == "mask_equal"
    assert details["jaccard04"]["stop_reason"] == "jaccard" and details["iters1"]["completed_iters"] == 1
    deep = details["planted40"]
    assert len(deep["layers"]) == 4 and all(layer["node_count"] > 0 for layer in deep["layers"])
    assert details["selected_over_8192"]["initial_selected_count"] > NC.CHUNK
    tiny = sorted(n["length_bins"] for n in details["tiny_children"]["hierarchy"] if n["layer"] == 1 and n["decision"] != "leaf")
    assert tiny[:2] == [1, 1] and 2 in tiny          # children of one and of two bins are processed at layer 2
    assert max(n["min_child_bins"] for n in details["min_run_255"]["hierarchy"] if n["decision"] != "leaf") == 255
    assert details["empty_mask"]["hierarchy"] == [] and details["empty_mask"]["stop_reason"] == "mask_equal"
    # the all-negative regions keep exactly one run of minRun bins around the required bin
    for n in details["all_negative"]["hierarchy"]:
        if n["layer"] == 0:
            assert n["decision"] in ("shrink", "keep_parent") and n["child_widths_bins"] == [min(5, n["length_bins"])]
    req = details["required_ends"]["hierarchy"]
    assert [n["required_idx"] - n["start_idx"] for n in req[:3]] == [0, 11, 3]
    mixed = {n["min_child_bins"] for n in details["mixed_widths"]["hierarchy"] if n["decision"] not in ("leaf", "skipped_short")}
    assert len(mixed) > 1
    wide = [n["min_child_bins"] for n in details["min_run_wide"]["hierarchy"] if n["decision"] not in ("leaf", "skipped_short")]
    assert wide and max(wide) == NC.WIDE_MIN_RUN and max(
        n["min_child_bins"] for n in details["min_run_wide40"]["hierarchy"] if n["decision"] != "leaf") == 40


def test_tie_break_counters():
    def counters(case):
        T.reset_counters()
        T.solve(form="device", **NC.solve_inputs(case))
        return dict(T.COUNTERS)

    by = {c["name"]: c for c in NC.SOLVE}
    assert counters(by["dyadic"])["count_tie"] > 0
    assert counters(by["near_ties"])["tolerance"] > 0
