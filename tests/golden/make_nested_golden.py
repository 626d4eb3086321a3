"""Regenerate tests/golden/nested/nested_*.npz from the REFERENCE's own functions (build image only: it needs the reference's
source tree, whose path is the first argument or $CONSENRICH_REFERENCE).

`consenrich.peaks` cannot be imported there, so the file is parsed with `ast` and only the thirteen pure functions from
`_asFloatVector` to `_refineNestedROCCOSolution` are executed, in a namespace that holds `np`, `npt`, `math`, the typing names
and the module constants they read.  Nothing of the reference's text is written anywhere: the fixtures hold OUTPUTS only, the
inputs are re-synthesised from tests/nested_cases.py.  Each case also goes through both forms of the pure-Python twin
(tests/twin_nested.py); a fixture is written only if all three agree bit for bit, and only if the case table still takes every
branch the tests rely on."""
import ast
import math
import os
import sys
import typing
from pathlib import Path

import numpy as np
import numpy.typing as npt

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import nested_cases as NC  # noqa: E402
import twin_nested as T  # noqa: E402

WANTED = ("_asFloatVector", "_selectedRunBounds", "_maskJaccard", "_roccoObjectiveForSolution", "_selectedRunLengthBP",
          "_minimumChildBinsForRegion", "_nestedSoftBudgetTargetCount", "_positiveScoreScale", "_nestedSoftSelectionPenalty",
          "_asParentBoundaryCosts", "_parentConditionedSubpeakObjective", "_solveParentConditionedSubpeaks",
          "_refineNestedROCCOSolution")


def load_reference(root):
    path = os.path.join(root, "src", "consenrich", "peaks.py")
    with open(path) as fh:
        tree = ast.parse(fh.read(), path)
    body = [node for node in tree.body if isinstance(node, ast.FunctionDef) and node.name in WANTED]
    missing = set(WANTED) - {node.name for node in body}
    if missing:
        raise SystemExit(f"{path} lacks {sorted(missing)}")
    ns = {k: getattr(typing, k) for k in ("Any", "Dict", "Iterable", "List", "Mapping", "Tuple", "Optional")}
    ns.update(np=np, npt=npt, math=math, Path=Path, json=None, logger=None,
              _NESTED_ROCCO_ITERS_DEFAULT=3, _NESTED_ROCCO_JACCARD_DEFAULT=0.999, _NESTED_ROCCO_MIN_PARENT_STEPS=5,
              _NESTED_ROCCO_MIN_CHILD_STEPS=5, _NESTED_ROCCO_BUDGET_SCALE_DEFAULT=0.75, _NESTED_ROCCO_SUBTASK_MAX_ITER=5,
              _NESTED_ROCCO_BUDGET_POLICY="soft_selection_penalty", _NESTED_ROCCO_PARENT_EDGE_COST=1.0e-12)
    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), ns)
    return ns


def main():
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("CONSENRICH_REFERENCE", "")
    if not root:
        raise SystemExit("usage: make_nested_golden.py <reference source tree>")
    ref = load_reference(root)
    out = os.path.join(HERE, "nested")
    os.makedirs(out, exist_ok=True)

    # ---- the subproblem solver
    rec, facts = {}, dict(count_tie=0, tolerance=0, empty=0, multi_run=0)
    for case in NC.SOLVE:
        kw = NC.solve_inputs(case)
        want = T.flatten_solve(*ref["_solveParentConditionedSubpeaks"](**kw))
        steps = T.flatten_solve(*T.solve(form="steps", **kw))
        T.reset_counters()
        dev = T.flatten_solve(*T.solve(form="device", **kw))
        if T.same_flat(want, steps) or T.same_flat(want, dev):
            raise SystemExit(f"solve/{case['name']}: the twin disagrees with the reference: {T.same_flat(want, steps)} "
                             f"{T.same_flat(want, dev)}")
        if case["name"] == "near_ties" and not (T.COUNTERS["tolerance"] > 0):
            raise SystemExit(f"solve/{case['name']}: the tolerance branch was not taken")
        if case["name"] == "dyadic" and not (T.COUNTERS["count_tie"] > 0):
            raise SystemExit(f"solve/{case['name']}: the count tie-break was not taken")
        for k in ("count_tie", "tolerance"):
            facts[k] += T.COUNTERS[k]
        facts["empty"] += int(want["i"][0] == 0)
        facts["multi_run"] += int(want["i"][2] > 1)
        rec.update({f"{case['name']}/{k}": v for k, v in want.items()})
    for (good, errors), fn in ((NC.solve_errors(), "_solveParentConditionedSubpeaks"), (NC.refine_errors(), "_refineNestedROCCOSolution")):
        for override, message in errors:
            try:
                ref[fn](**{**good, **override})
            except ValueError as e:
                if str(e) != message:
                    raise SystemExit(f"{fn}{sorted(override)}: the reference says {e!s}")
            else:
                raise SystemExit(f"{fn}{sorted(override)}: the reference raises nothing")
    if not all(facts.values()):
        raise SystemExit(f"the solver cases lack {[k for k, v in facts.items() if not v]}")
    np.savez_compressed(os.path.join(out, "nested_solve.npz"), **rec)

    # ---- the refinement
    rec, seen = {}, dict(decisions=set(), stops=set(), layers=0, tie=0, selected_over_chunk=0, quantile_of_1=0, quantile_of_2=0,
                         positives_0=0, positives_1=0, positives_2=0, positives_more=0)
    for case in NC.REFINE:
        kw = NC.refine_inputs(case)
        mask, details = ref["_refineNestedROCCOSolution"](**kw)
        want = T.flatten_refine(mask, details)
        sm, sd = T.refine(form="steps", **kw)
        T.reset_counters()
        dm, dd = T.refine(form="device", **kw)
        for name, m, d in (("steps", sm, sd), ("device", dm, dd)):
            diff = T.differences(d, details)
            if diff or not np.array_equal(m, mask) or m.dtype != mask.dtype:
                raise SystemExit(f"refine/{case['name']}: the twin's {name} form disagrees with the reference: {diff[:5]}")
        if T.same_flat(want, T.flatten_refine(dm, dd)):
            raise SystemExit(f"refine/{case['name']}: flattening loses something")
        seen["decisions"] |= {n["decision"] for n in details["hierarchy"]}
        seen["stops"].add(details["stop_reason"])
        seen["layers"] = max(seen["layers"], len(details["layers"]))
        seen["tie"] += T.COUNTERS["count_tie"]
        if case["name"] == "selected_over_8192":
            seen["selected_over_chunk"] += int(details["initial_selected_count"] > NC.CHUNK > details["final_selected_count"])
        # (counted by the twin's device form: quantiles of one and of two values, and the strictly positive solver scores of
        # the regions that were PROCESSED, not skipped as short)
        for k in ("quantile_of_1", "quantile_of_2", "positives_0", "positives_1", "positives_2", "positives_more"):
            seen[k] += T.COUNTERS[k]
        if case["name"] == "tiny_children":
            lens2 = sorted(n["length_bins"] for n in details["hierarchy"] if n["layer"] == 1 and n["decision"] != "leaf")
            if lens2[:2] != [1, 1] or 2 not in lens2 or not (T.COUNTERS["quantile_of_1"] and T.COUNTERS["quantile_of_2"]):
                raise SystemExit(f"refine/tiny_children: no child of one and of two bins is processed at layer 2: {lens2}")
        if case["name"] == "mask_equal" and details["stop_reason"] != "mask_equal":
            raise SystemExit(f"refine/mask_equal stops with {details['stop_reason']}")
        if case["name"] == "jaccard04" and details["stop_reason"] != "jaccard":
            raise SystemExit(f"refine/jaccard04 stops with {details['stop_reason']}")
        rec.update({f"{case['name']}/{k}": v for k, v in want.items()})
    need = dict(decisions=set(T.DECISIONS), stops={"disabled", "mask_equal", "jaccard", "max_iter"})
    for k, v in need.items():
        if not v <= seen[k]:
            raise SystemExit(f"the refinement cases lack {k} {sorted(v - seen[k])}")
    if seen["layers"] < 4 or not all(seen[k] for k in ("tie", "selected_over_chunk", "quantile_of_1", "quantile_of_2", "positives_0",
                                                        "positives_1", "positives_2", "positives_more")):
        raise SystemExit(f"the refinement cases lack a branch: {seen}")
    np.savez_compressed(os.path.join(out, "nested_refine.npz"), **rec)
    print(f"wrote nested_solve.npz and nested_refine.npz to {out}; decisions {sorted(seen['decisions'])}, stops {sorted(seen['stops'])}, "
          f"deepest hierarchy {seen['layers']} layers")


if __name__ == "__main__":
    main()
