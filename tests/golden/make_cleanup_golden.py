"""Regenerate tests/golden/cleanup/cleanup_*.npz from the REFERENCE's own functions (build image only: it needs the reference's
source tree, whose path is the first argument or $CONSENRICH_REFERENCE).

`consenrich.peaks` cannot be imported there, so the file is parsed with `ast` and only the functions of WANTED are executed -- the
eleven that make_narrowpeak_golden.py takes and the seven of the clean-up -- in a namespace that holds `np`, `npt`, `math`, the
typing names, `stats = scipy.stats` and the `_MASSIVE_SUBPEAK_*` constants.  Nothing of the reference's text is written anywhere:
the fixtures hold OUTPUTS only, the inputs are re-synthesised from tests/cleanup_cases.py.  Each force, split and contract case
also goes through both forms of the pure-Python twin (tests/twin_cleanup.py); a fixture is written only if all three agree bit for
bit, and only if the case table still takes every branch of NEEDED.

What the table cannot reach, by construction of the reference: a split with a side shorter than minBins (the scan starts its gaps
at minBins and ends them minBins before the end), and a contraction refused for its width inside the recursion (the contract
threshold never exceeds a candidate's width; the contract piece on its own reaches it).  The deepest accepted split is printed."""
import ast
import math
import os
import sys
import typing

import numpy as np
import numpy.typing as npt

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import cleanup_cases as CC  # noqa: E402
import twin_cleanup as T  # noqa: E402
from make_narrowpeak_golden import WANTED as ROWS_WANTED  # noqa: E402

WANTED = ROWS_WANTED + ("_bhQValues", "_massiveSubpeakWidthScores", "_learnMassiveSubpeakWidthPolicy", "_bestMassiveSubpeakSplit",
                        "_contractMassiveSubpeakSegment", "_makeSubpeakSegment", "_forceMassiveSubpeakSegments")
CONSTANTS = dict(_MASSIVE_SUBPEAK_CLEANUP_DEFAULT=True, _MASSIVE_SUBPEAK_MIN_BP=7500, _MASSIVE_SUBPEAK_WIDTH_ALPHA=0.1,
                 _MASSIVE_SUBPEAK_WIDTH_BULK_QUANTILE=0.95, _MASSIVE_SUBPEAK_MAX_FRACTION=0.005, _MASSIVE_SUBPEAK_MIN_LOG_GAP=0.10,
                 _MASSIVE_SUBPEAK_MIN_PEAKS=25, _MASSIVE_SUBPEAK_SPLIT_QUANTILE=0.25, _MASSIVE_SUBPEAK_SPLIT_Z=2.0,
                 _MASSIVE_SUBPEAK_MAX_DEPTH=8, _MASSIVE_SUBPEAK_MIN_CHILD_BP=250, _MASSIVE_SUBPEAK_MIN_CHILD_FRACTION=0.05,
                 _MASSIVE_SUBPEAK_TRIGGER_Z_CAP=3.0, _ROCCO_MIN_PEAK_BP=200, _EXPORT_MEDIAN_SIGNAL_LOCAL_UNCERTAINTY_MULTIPLIER=2.0)
# what the case table must still do (BRANCHES of the twin's device form, summed over the cases)
NEEDED = ("not_a_candidate", "split_too_short", "split_gain_nonpos", "split_z_below", "z_just_below", "z_at_threshold",
          "split_accepted_depth0", "split_accepted_depth1", "outer_overwrites_inner", "outer_over_core", "max_depth_stop",
          "child_contract_depth", "leaf_below_thresholds", "quantile_integral", "quantile_t_low", "quantile_t_high", "prefix_tie",
          "gap_tie", "scale_mad", "scale_iqr", "scale_one", "adaptive_accepted", "centre_not_kept", "flat_scores", "adaptive_too_wide",
          "capped_accepted", "capped_tie_score", "capped_tie_score_distance", "max_even_count", "max_several", "argmin_tie",
          "contract_refused_bins", "contract_refused_width", "unsplit_with_details", "uneven_widths", "contract_width_missing",
          "contract_min_applies", "min_bins_by_fraction", "min_bins_by_bp", "min_bins_by_run", "node_len_tile_minus_1", "node_len_tile",
          "node_len_tile_plus_1", "sort_lds", "sort_global")
# the row cases whose peak set the policy changes
ROWS_CLEANED = ("rows_active", "rows_gap_in_front", "rows_no_split", "rows_no_filter", "rows_no_null", "rows_own_quantile")
# what every policy case must show of the reference's answer
POLICY_EXPECT = {
    "few_widths": lambda d: not d["active"] and d["null_center"] is None and d["num_peaks"] == 24,
    "disabled": lambda d: not d["active"] and d["null_center"] is None and not d["enabled"],
    "no_tail": lambda d: not d["active"] and d["null_center"] is not None and d["num_width_tail_candidates"] == 0,
    "cluster_too_large": lambda d: not d["active"] and d["num_width_tail_candidates"] == 2,
    "log_gap_too_small": lambda d: not d["active"] and d["num_width_tail_candidates"] == 1,
    "cluster_q_above_alpha": lambda d: not d["active"] and d["num_width_tail_candidates"] == 1,
    "active_gap": lambda d: d["active"] and d["width_threshold_bp"] == d["gap_width_threshold_bp"] < d["width_cap_bp"],
    "active_cap": lambda d: d["active"] and d["width_threshold_bp"] == d["width_cap_bp"] < d["gap_width_threshold_bp"] and d["width_cap_bp"] > 7500,
    "active_min_bp": lambda d: d["active"] and d["width_threshold_bp"] == d["width_cap_bp"] == d["min_bp"] == 7500,
    "active_own_min_bp": lambda d: d["active"] and d["width_threshold_bp"] == d["min_bp"] == 2500,
    "mad_zero": lambda d: d["active"] and d["null_scale"] not in (None, 1.0),
    "mad_and_iqr_zero": lambda d: d["active"] and d["null_scale"] == 1.0,
    "small_bulk": lambda d: d["active"] and d["num_peaks"] == 4,
    "invalid_widths": lambda d: d["active"] and d["num_peaks"] == 31,
    "empty": lambda d: not d["active"] and d["num_peaks"] == 0,
    "alpha_out_of_range": lambda d: d["active"] and d["alpha"] == 1.5,
}


def load_reference(root):
    path = os.path.join(root, "src", "consenrich", "peaks.py")
    with open(path) as fh:
        tree = ast.parse(fh.read(), path)
    body = [node for node in tree.body if isinstance(node, ast.FunctionDef) and node.name in WANTED]
    missing = set(WANTED) - {node.name for node in body}
    if missing:
        raise SystemExit(f"{path} lacks {sorted(missing)}")
    from scipy import stats

    ns = {k: getattr(typing, k) for k in ("Any", "Dict", "Iterable", "List", "Mapping", "Tuple", "Optional", "Sequence")}
    ns.update(np=np, npt=npt, math=math, stats=stats, logger=None, **CONSTANTS)
    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), ns)
    return ns


def agree(name, ref, call, flatten):
    """the reference's answer, checked against both forms of the twin; BRANCHES holds the device form's afterwards"""
    want = ref()
    steps = call("steps")
    T.reset_branches()
    dev = call("device")
    for form, got in (("steps", steps), ("device", dev)):
        diff = T.differences(got, want)
        if diff:
            raise SystemExit(f"{name}: the twin's {form} form disagrees with the reference: {diff[:5]}")
    if T.same_flat(flatten(want), flatten(dev)):
        raise SystemExit(f"{name}: flattening loses something")
    return want


def main():
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("CONSENRICH_REFERENCE", "")
    if not root:
        raise SystemExit("usage: make_cleanup_golden.py <reference source tree>")
    ref = load_reference(root)
    out = os.path.join(HERE, "cleanup")
    os.makedirs(out, exist_ok=True)
    seen, per_case = {}, {}

    def tally(name):
        per_case[name] = dict(T.BRANCHES)
        for k, v in T.BRANCHES.items():
            seen[k] = seen.get(k, 0) + v

    rec = {}
    for case in CC.FORCE:
        for k, kw in enumerate(CC.force_inputs(case)):
            name = f"{case['name']}/{k}"
            want = agree(name, lambda: ref["_forceMassiveSubpeakSegments"](**kw), lambda form: T.force(form=form, **kw), T.flatten_force)
            tally(name)
            again = T.force(form="device", coords="step", **kw)     # the uniform-step path: identical records
            if T.differences(again, want):
                raise SystemExit(f"{name}: the uniform-step path differs")
            rec.update({f"{name}/{key}": v for key, v in T.flatten_force(want).items()})
    np.savez_compressed(os.path.join(out, "cleanup_force.npz"), **rec)
    rec = {}
    for case in CC.SPLITS:
        kw = {k: v for k, v in case.items() if k != "name"}
        want = agree(case["name"], lambda: ref["_bestMassiveSubpeakSplit"](**kw), lambda form: T.best_split(form=form, **kw), T.flatten_split)
        tally(case["name"])
        rec.update({f"{case['name']}/{key}": v for key, v in T.flatten_split(want).items()})
    np.savez_compressed(os.path.join(out, "cleanup_split.npz"), **rec)
    rec = {}
    for case in CC.CONTRACTS:
        kw = {k: v for k, v in case.items() if k != "name"}
        want = agree(case["name"], lambda: ref["_contractMassiveSubpeakSegment"](**kw), lambda form: T.contract_segment(form=form, **kw),
                     T.flatten_contract)
        tally(case["name"])
        rec.update({f"{case['name']}/{key}": v for key, v in T.flatten_contract(want).items()})
    np.savez_compressed(os.path.join(out, "cleanup_contract.npz"), **rec)
    # the one non-finite case: the reference raises from the contraction
    try:
        ref["_forceMassiveSubpeakSegments"](**CC.nonfinite_inputs())
    except ValueError as e:
        if str(e) != "`scores` contains non-finite values":
            raise SystemExit(f"non-finite case: the reference says {e!s}")
    else:
        raise SystemExit("non-finite case: the reference raises nothing")
    rec = {}
    for case in CC.POLICIES:
        kw = {k: v for k, v in case.items() if k != "name"}
        d = ref["_learnMassiveSubpeakWidthPolicy"](**kw)
        if not POLICY_EXPECT[case["name"]](d):
            raise SystemExit(f"{case['name']}: the policy is not what the case is for: {d}")
        if ("num_width_tail_gap_candidates" in d) != bool(d["active"]):
            raise SystemExit(f"{case['name']}: num_width_tail_gap_candidates and active disagree")
        rec.update({f"{case['name']}/policy_{key}": v for key, v in T.flatten_policy(d).items()})
        w = np.asarray(kw["widthsBP"], np.float64)
        w = w[np.isfinite(w) & (w > 0.0)]
        p, q, null = ref["_massiveSubpeakWidthScores"](w, **({"bulkQuantile": kw["bulkQuantile"]} if "bulkQuantile" in kw else {}))
        rec.update({f"{case['name']}/p": np.asarray(p, np.float64), f"{case['name']}/q": np.asarray(q, np.float64),
                    f"{case['name']}/null": np.asarray([null["center"], null["scale"]], np.float64)})
        pv = [ref["_massiveSubpeakWidthPValue"](float(v), d) for v in (0.5, 1.0, 800.0, 7500.0, 1.0e5)]
        rec[f"{case['name']}/pvalue"] = np.asarray([float("nan") if a is None else a for a, _ in pv], np.float64)
        if any(b is not None for _, b in pv):
            raise SystemExit("a width q value that is not None")
    np.savez_compressed(os.path.join(out, "cleanup_policy.npz"), **rec)
    # the rows under a policy: the reference, and both forms of the twin's rows (finishing per segment)
    rec, cleaned = {}, 0
    for case in CC.ROWS:
        kw = CC.row_inputs(case)
        want = ref["_solutionToChromNarrowPeakRows"](**kw)
        for form in ("steps", "device"):
            diff = T.differences(T.rows(form=form, **kw), want)
            if diff:
                raise SystemExit(f"{case['name']}: the twin's {form} rows disagree with the reference: {diff[:5]}")
        plain = ref["_solutionToChromNarrowPeakRows"](**{**kw, "massiveSubpeakWidthPolicy": None})
        changed = [m["start"] for m in want[1]] != [m["start"] for m in plain[1]] or [m["end"] for m in want[1]] != [m["end"] for m in plain[1]]
        if changed != (case["name"] in ROWS_CLEANED):
            raise SystemExit(f"{case['name']}: the policy {'changes' if changed else 'does not change'} the peak set")
        cleaned += int(changed)
        rec.update({f"{case['name']}/{key}": v for key, v in T.flatten_rows(want).items()})
    np.savez_compressed(os.path.join(out, "cleanup_rows.npz"), **rec)
    lacking = [k for k in NEEDED if not seen.get(k)]
    if lacking:
        for name, b in per_case.items():
            print(name, dict(sorted(b.items())))
        raise SystemExit(f"the case table lacks {lacking}")
    deepest = max(int(k[len("split_accepted_depth"):]) for k in seen if k.startswith("split_accepted_depth"))
    print(f"wrote cleanup_force / split / contract / policy.npz to {out}: {len(CC.FORCE)} + {len(CC.SPLITS)} + {len(CC.CONTRACTS)} + "
          f"{len(CC.POLICIES)} cases; the deepest accepted split is at depth {deepest}"
          + ("" if deepest >= 8 else " (no case reaches depth 8)") + f"; branches {dict(sorted(seen.items()))}")


if __name__ == "__main__":
    main()
