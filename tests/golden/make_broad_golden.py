"""Regenerate tests/golden/broad/broad_*.npz from the REFERENCE's own functions (build image only: it needs the reference's
source tree, whose path is the first argument or $CONSENRICH_REFERENCE).

`consenrich.peaks` cannot be imported there, so the file is parsed with `ast` and only the six functions of WANTED are executed,
in a namespace that holds `np`, the typing names and the two default constants they read.  Nothing of the reference's text is
written anywhere: the fixtures hold OUTPUTS only (tests/broad_cases.py: `pack`), the inputs are re-synthesised from the case table.
Each case also goes through both forms of the pure-Python twin (tests/twin_broad.py); a fixture is written only if all three agree
bit for bit, and only if the case table still takes every branch the tests rely on."""
import ast
import math
import os
import sys
import typing

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import broad_cases as BC  # noqa: E402
import twin_broad as T  # noqa: E402

WANTED = ("_validateExportFilterUncertaintyMultiplier", "_selectedCoordinateRunBounds", "_intervalOverlapsBlacklist",
          "_mergeBroadRunsByObjective", "_blocksForBroadParent", "_solutionToChromBroadPeakRows")


def load_reference(root):
    path = os.path.join(root, "src", "consenrich", "peaks.py")
    with open(path) as fh:
        tree = ast.parse(fh.read(), path)
    body = [node for node in tree.body if isinstance(node, ast.FunctionDef) and node.name in WANTED]
    missing = set(WANTED) - {node.name for node in body}
    if missing:
        raise SystemExit(f"{path} lacks {sorted(missing)}")
    ns = {k: getattr(typing, k) for k in ("Any", "Dict", "Iterable", "List", "Mapping", "Tuple", "Optional", "Sequence")}
    ns.update(np=np, math=math, _EXPORT_MEDIAN_SIGNAL_LOCAL_UNCERTAINTY_MULTIPLIER=2.0, _MATCHING_DEFAULT_BROAD_MIN_PEAK_BP=1000)
    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), ns)
    return ns


def reference_parents(ref, kw):
    """peaks.py:6884-6932 around the reference's own two functions: the envelope, the support runs that touch it (or the envelope's
    runs), the bridging.  The result in the form of twin_broad.parents, without the mask (it is the merged runs filled in)"""
    s = np.asarray(kw["scores"], np.float64)
    env = (np.asarray(kw["weak"], np.uint8) > 0) | (np.asarray(kw["strong"], np.uint8) > 0)
    support = ref["_selectedCoordinateRunBounds"](np.asarray(s >= float(kw["threshold"]), dtype=np.uint8), kw["intervals"], kw["ends"])
    touching = [(int(a), int(b)) for a, b in support if np.any(env[int(a):int(b) + 1])]
    fallback = not touching
    if fallback:
        touching = ref["_selectedCoordinateRunBounds"](env.astype(np.uint8), kw["intervals"], kw["ends"])
    merged, details = ref["_mergeBroadRunsByObjective"](
        touching, s, kw["intervals"], kw["ends"], str(kw["chromosome"]), selectionPenalty=float(kw["selection_penalty"]),
        boundaryCost=float(kw["boundary_cost"]), maxGapBP=int(kw["max_gap_bp"]), blacklistByChrom=kw["blacklist"] or {},
        runPenalty=float(kw["run_penalty"]), dipPenaltyFraction=float(kw["dip_penalty_fraction"]))
    return {"starts": [int(a) for a, _ in merged], "ends": [int(b) for _, b in merged], "merge_details": details,
            "weak_support_run_count": int(len(support)), "weak_support_touching_run_count": int(len(touching)),
            "envelope_fallback": bool(fallback)}


def need(ok, what):
    if not ok:
        raise SystemExit(f"the case table no longer shows: {what}")


def check_errors(fn, good, errors):
    for override, message in errors:
        try:
            fn(**{**good, **override})
        except ValueError as e:
            if str(e) != message:
                raise SystemExit(f"{sorted(override)}: the reference says {e!s}")
        else:
            raise SystemExit(f"{sorted(override)}: the reference raises nothing")


def main():
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("CONSENRICH_REFERENCE", "")
    if not root:
        raise SystemExit("usage: make_broad_golden.py <reference source tree>")
    ref = load_reference(root)
    out = os.path.join(HERE, "broad")
    os.makedirs(out, exist_ok=True)

    merged = {}
    for case in BC.merge_cases():
        merged[case["name"]] = ref["_mergeBroadRunsByObjective"](**case["kw"])
    d = {k: v[1] for k, v in merged.items()}
    for name in ("gap_lengths_soft", "gap_lengths_hard", "gap_lengths_above_one", "gap_lengths_below_zero"):
        need(0 < d[name]["num_gaps_merged"] < d[name]["num_gaps_evaluated"] == len(BC.GAP_LENGTHS) + 1, f"{name}: some gaps merge, some do not")
    need({d["gap_lengths_soft"]["policy"], d["gap_lengths_below_zero"]["policy"]} == {"soft_dip_objective_delta"} and
         {d["gap_lengths_hard"]["policy"], d["gap_lengths_above_one"]["policy"]} == {"objective_delta"}, "both policy strings")
    need(d["gain_zero"]["num_gaps_merged"] == 1 and merged["gain_zero"][0] == [(1, 4), (7, 16), (19, 22)], "a gain of exactly 0 does not merge")
    need(d["run_penalty"]["num_gaps_merged"] == 3, "the run penalty turns the zero gains")
    need((d["distance_blacklist"]["num_gaps_blocked_by_distance"], d["distance_blacklist"]["num_gaps_blocked_by_blacklist"],
          d["distance_blacklist"]["num_gaps_merged"]) == (2, 1, 3), "distance before blacklist, touching intervals, gapBP == maxGapBP")
    need(d["nonfinite_gap"]["num_gaps_merged"] == 1, "a NaN gain does not merge, an infinite one does")
    need(d["max_gap_zero"]["max_gap_bp"] == 0 and merged["max_gap_zero"][0] == [(0, 5), (8, 11)], "maxGapBP floored at 0")
    need(len(d["empty_soft"]) == 10 and len(d["gain_zero"]) == 12, "the two forms of the details")
    check_errors(ref["_mergeBroadRunsByObjective"], *BC.merge_errors())

    rows = {}
    for case in BC.rows_cases():
        with np.errstate(invalid="ignore"):
            rows[case["name"]] = ref["_solutionToChromBroadPeakRows"](**case["kw"])
        need(len(rows[case["name"]]) == (4 if case["kw"]["returnExportDetails"] else 3), f"{case['name']}: the return form")
    lengths = sorted(m["end_idx"] - m["start_idx"] + 1 for k in ("lengths", "lengths_chunk") for m in rows[k][2])
    need(set(BC.PARENT_LENGTHS) <= set(lengths), f"every parent length is kept: {lengths}")
    f = rows["filters"]
    need((f[3]["num_segments_dropped_median_signal_local_p"], f[3]["num_segments_dropped_min_peak_bp"], len(f[2])) == (1, 1, 5),
         f"one parent dropped by the median filter, one by width: {f[3]}")
    need(f[2][0]["median_state"] == f[2][0]["median_signal_threshold"] == -1.0, "a median equal to the threshold is kept")
    need(f[2][2]["local_median_p"] is None and f[2][1]["local_median_p"] == 0.5, "uncertainty with none and with some finite values")
    need(f[2][3]["summit_idx"] == f[2][3]["start_idx"] + 4, "the leftmost arg-max wins a tie")
    b = rows["blocks"]
    need(b[3]["num_candidate_segments"] == 8, f"coordinate breaks cut two parents: {b[3]}")
    counts = [m["block_count"] for m in b[2]]
    need(1 in counts and 2 in counts and 3 in counts, f"blocks with and without sentinels: {counts}")
    need(any(m["block_sizes"][0] == 1 and m["block_sizes"][-1] == 1 for m in b[2]), "a child in the middle takes both 1 bp sentinels")
    need({r[4] for r in rows["one_score"][0]} == {250}, "one raw score: all 250")
    need([r[4] for r in rows["half_way"][0]] == [250, 812, 1000, 438], f"half-way scores: {[r[4] for r in rows['half_way'][0]]}")
    need(any(math.isnan(m["median_state"]) for m in rows["nan_signal"][2]), "a NaN parent")
    need(rows["empty_masks"] == ([], [], [], {**rows["empty_masks"][3]}) and rows["empty_masks_pair"] == ([], [], []), "empty returns")
    need(rows["all_dropped"][:3] == ([], [], []) and rows["all_dropped"][3]["num_segments_dropped_min_peak_bp"] == 1, "all dropped")
    check_errors(ref["_solutionToChromBroadPeakRows"], *BC.rows_errors())

    # both forms of the twin agree with the reference, and the device form takes every branch
    T.reset_branches()
    for table, got, fn in ((BC.merge_cases(), merged, T.merge), (BC.rows_cases(), rows, T.rows)):
        for case in table:
            for form in ("steps", "device"):
                with np.errstate(invalid="ignore"):
                    diff = BC.differences(BC.canon(fn(form=form, **case["kw"])), BC.canon(got[case["name"]]))
                if diff:
                    raise SystemExit(f"{case['name']}: the twin's {form} form disagrees with the reference: {diff[:5]}")
    lacking = [k for k in BC.NEEDED if not T.BRANCHES.get(k)]
    need(not lacking, f"branches {lacking}")
    # the envelope and the support runs: the reference's functions composed as `solveRocco` composes them, both forms of the twin
    parents = {}
    T.reset_branches()
    for case in BC.parents_cases():
        want = parents[case["name"]] = reference_parents(ref, case["kw"])
        for form in ("steps", "device"):
            got = T.parents(form=form, **case["kw"])
            mask = got.pop("mask")
            diff = BC.differences(BC.canon(got), BC.canon(want))
            filled = np.zeros(mask.size, np.uint8)
            for a, b in zip(want["starts"], want["ends"]):
                filled[a:b + 1] = 1
            if diff or not np.array_equal(mask, filled):
                raise SystemExit(f"{case['name']}: the twin's {form} form of the parents disagrees with the reference: {diff[:5]}")
    lacking = [k for k in BC.NEEDED_PARENTS if not T.BRANCHES.get(k)]
    need(not lacking, f"branches {lacking}")

    # the two host functions on their own: every mask of the rows cases, and the blocks of every parent against ALL children
    runs, blocks = {}, {}
    for case in BC.rows_cases():
        kw = case["kw"]
        pr = ref["_selectedCoordinateRunBounds"](kw["parentSolution"], kw["intervals"], kw["ends"])
        cr = ref["_selectedCoordinateRunBounds"](kw["childSolution"], kw["intervals"], kw["ends"])
        runs[case["name"]] = (pr, cr)
        blocks[case["name"]] = [ref["_blocksForBroadParent"](a, b, cr, kw["intervals"], kw["ends"]) for a, b in pr]
    np.savez_compressed(os.path.join(out, "broad_merge.npz"), **{k: BC.pack(v) for k, v in merged.items()})
    np.savez_compressed(os.path.join(out, "broad_rows.npz"), **{k: BC.pack(v) for k, v in rows.items()})
    np.savez_compressed(os.path.join(out, "broad_parents.npz"), **{k: BC.pack(v) for k, v in parents.items()})
    np.savez_compressed(os.path.join(out, "broad_host.npz"), **{f"runs/{k}": BC.pack(v) for k, v in runs.items()},
                        **{f"blocks/{k}": BC.pack(v) for k, v in blocks.items()})
    print(f"wrote broad_merge.npz ({len(merged)} cases), broad_rows.npz ({len(rows)}), broad_parents.npz ({len(parents)}), "
          f"broad_host.npz to {out}")


if __name__ == "__main__":
    main()
