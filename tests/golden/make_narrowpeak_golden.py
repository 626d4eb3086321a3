"""Regenerate tests/golden/narrowpeak/narrowpeak_*.npz from the REFERENCE's own functions (build image only: it needs the
reference's source tree, whose path is the first argument or $CONSENRICH_REFERENCE).

`consenrich.peaks` cannot be imported there, so the file is parsed with `ast` and only the eleven functions of WANTED are
executed, in a namespace that holds `np`, `npt`, `math`, the typing names and the module constants they read (`scipy.stats` is
not reached without a width policy).  Nothing of the reference's text is written anywhere: the fixtures hold OUTPUTS only, the
inputs are re-synthesised from tests/narrowpeak_cases.py.  Each case also goes through both forms of the pure-Python twin
(tests/twin_narrowpeak.py); a fixture is written only if all three agree bit for bit, and only if the case table still takes
every branch the tests rely on."""
import ast
import math
import os
import sys
import typing

import numpy as np
import numpy.typing as npt

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import narrowpeak_cases as NC  # noqa: E402
import twin_narrowpeak as T  # noqa: E402
import twin_nested as TN  # noqa: E402

WANTED = ("_validateExportFilterUncertaintyMultiplier", "_selectedRunBounds", "_asParentBoundaryCosts",
          "_parentConditionedSubpeakObjective", "_solveParentConditionedSubpeaks", "_solveParentConditionedSubpeakSegments",
          "_trimChildSegmentAroundSummit", "_massiveSubpeakWidthPValue", "_resolveRoccoExportHierarchy",
          "_annotateRoccoPeakHierarchy", "_solutionToChromNarrowPeakRows")
# what the case table must still do (BRANCHES of the twin's device form, summed over the cases)
NEEDED = ("parent_len_1", "parent_len_4", "parent_len_5", "parent_len_6", "parent_len_31", "parent_len_32", "parent_len_33",
          "parent_len_64", "parent_len_65", "gap_inside_run", "children_3plus", "single_child_shorter", "kept_whole", "argmax_tie",
          "trim_left", "trim_right", "trim_both", "trim_none", "trim_summit_below", "median_of_1", "median_of_2", "median_of_3",
          "median_of_4", "uncertainty_some_nonfinite", "uncertainty_none_finite", "dropped_median", "median_equal_threshold",
          "span_floor", "half_way", "dropped_min_bp")


def load_reference(root):
    path = os.path.join(root, "src", "consenrich", "peaks.py")
    with open(path) as fh:
        tree = ast.parse(fh.read(), path)
    body = [node for node in tree.body if isinstance(node, ast.FunctionDef) and node.name in WANTED]
    missing = set(WANTED) - {node.name for node in body}
    if missing:
        raise SystemExit(f"{path} lacks {sorted(missing)}")
    ns = {k: getattr(typing, k) for k in ("Any", "Dict", "Iterable", "List", "Mapping", "Tuple", "Optional", "Sequence")}
    ns.update(np=np, npt=npt, math=math, stats=None, logger=None, _ROCCO_MIN_PEAK_BP=200,
              _EXPORT_MEDIAN_SIGNAL_LOCAL_UNCERTAINTY_MULTIPLIER=2.0, _MASSIVE_SUBPEAK_SPLIT_QUANTILE=0.25,
              _MASSIVE_SUBPEAK_SPLIT_Z=2.0)
    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), ns)
    return ns


def as_triple(result, kw, ref_details=None):
    """(rows, meta, details) of either return form (the pair form has no details: an empty stand-in keeps the arrays' shapes)"""
    if len(result) == 3:
        return result
    return result[0], result[1], {**{k: -1 for k in T.DETAIL_INTS}, "median_signal_local_p_multiplier": float("nan"),
                                  "median_signal_local_p_filter_active": False, "massive_subpeak_cleanup_active": False,
                                  "massive_subpeak_width_policy": None}


def main():
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("CONSENRICH_REFERENCE", "")
    if not root:
        raise SystemExit("usage: make_narrowpeak_golden.py <reference source tree>")
    ref = load_reference(root)
    out = os.path.join(HERE, "narrowpeak")
    os.makedirs(out, exist_ok=True)
    rec, seen, count_tie, tolerance, wide, nan_rows = {}, {}, 0, 0, 0, 0
    for case in NC.CASES:
        kw = NC.inputs(case)
        with np.errstate(invalid="ignore"):
            want = ref["_solutionToChromNarrowPeakRows"](**kw)
            steps = T.rows(form="steps", **kw)
            T.reset_branches()
            dev = T.rows(form="device", **kw)
        if type(want) is not tuple or len(want) != (3 if kw["returnExportDetails"] else 2):
            raise SystemExit(f"{case['name']}: the reference returns {type(want)} of {len(want)}")
        for name, got in (("steps", steps), ("device", dev)):
            diff = T.differences(got, want)
            if diff:
                raise SystemExit(f"{case['name']}: the twin's {name} form disagrees with the reference: {diff[:5]}")
        flat = T.flatten(as_triple(want, kw))
        if T.same_flat(flat, T.flatten(as_triple(dev, kw))):
            raise SystemExit(f"{case['name']}: flattening loses something")
        for k, v in T.BRANCHES.items():
            seen[k] = seen.get(k, 0) + v
        count_tie += TN.COUNTERS["count_tie"] if case["name"] == "ties" else 0
        tolerance += TN.COUNTERS["tolerance"] if case["name"] == "near_ties" else 0
        wide += int(case["name"] == "min_run_wide" and kw["minSubpeakBins"] >= NC.WIDE_MIN_RUN)
        if case["name"] in NC.HOST_DECIDED:
            nan_rows += sum(int(math.isnan(m["median_state"]) or math.isnan(m["max_state"])) for m in want[1])
        if case["name"].startswith("empty_mask") and (want[0] != [] or want[1] != []):
            raise SystemExit(f"{case['name']}: rows from an empty mask")
        if case["name"] == "one_score" and {r[4] for r in want[0]} != {250}:
            raise SystemExit("one_score: the scores are not all 250")
        if case["name"] == "half_way" and 812 not in {r[4] for r in want[0]}:
            raise SystemExit(f"half_way: no score of 812: {[r[4] for r in want[0]]}")
        rec.update({f"{case['name']}/{k}": v for k, v in flat.items()})
    good, errs = NC.errors()
    for override, message in errs:
        try:
            ref["_solutionToChromNarrowPeakRows"](**{**good, **override})
        except ValueError as e:
            if str(e) != message:
                raise SystemExit(f"{sorted(override)}: the reference says {e!s}")
        else:
            raise SystemExit(f"{sorted(override)}: the reference raises nothing")
    lacking = [k for k in NEEDED if not seen.get(k)]
    if lacking or not (count_tie and tolerance and wide and nan_rows):
        raise SystemExit(f"the case table lacks {lacking}; count tie {count_tie}, tolerance {tolerance}, wide {wide}, NaN rows {nan_rows}")
    np.savez_compressed(os.path.join(out, "narrowpeak_rows.npz"), **rec)
    print(f"wrote narrowpeak_rows.npz to {out}: {len(NC.CASES)} cases; branches {dict(sorted(seen.items()))}")


if __name__ == "__main__":
    main()
