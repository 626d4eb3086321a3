"""Pure-Python twin of the narrowPeak export (`_solutionToChromNarrowPeakRows` without a width policy and without a hierarchy,
`_solveParentConditionedSubpeakSegments`, `_trimChildSegmentAroundSummit`), in two forms:

  form="steps"   the reference's steps in the reference's order, bin by bin over the mask, with NumPy's argmax / median / max;
  form="device"  the device's decomposition: the mask's runs cut at the coordinate gaps, per parent the dynamic programme in
                 its register form with a uniform cost (twin_nested), per child leftmost-tie scans for the summit and the maxima
                 and medians as two order statistics of a sort, then the host's assembly from compact records.

tests/golden/make_narrowpeak_golden.py writes a fixture only where the reference and both forms agree bit for bit.  BRANCHES
(device form) tells the fixture maker which branches a case took."""
import math

import numpy as np

import twin_nested as TN

MIN_PEAK_BP = 200
BRANCHES = {}
META_FLOATS = ("median_state", "local_median_p", "median_signal_threshold", "max_state", "max_score", "subpeak_objective",
               "subpeak_boundary_penalty", "trim_score_floor")
META_INTS = ("start", "end", "summit", "start_idx", "end_idx", "summit_idx", "untrimmed_start_idx", "untrimmed_end_idx",
             "segment_length_bins", "num_subpeaks", "split_from_parent", "trimmed_from_parent", "untrimmed_start", "untrimmed_end")
META_NONE = ("massive_subpeak_cleanup_mode", "massive_subpeak_width_p", "massive_subpeak_width_q",
             "massive_subpeak_width_threshold_bp", "massive_subpeak_split_gain", "massive_subpeak_split_z", "massive_subpeak_gap_bins",
             "massive_subpeak_core_width_bp", "massive_subpeak_core_score_floor")
DETAIL_INTS = ("num_candidate_segments", "num_segments_dropped_median_signal_local_p", "num_segments_dropped_min_peak_bp",
               "min_peak_bp", "num_coordinate_gap_splits", "num_segments_kept")


def reset_branches():
    BRANCHES.clear()
    TN.reset_counters()


def took(name, n=1):
    BRANCHES[name] = BRANCHES.get(name, 0) + n


def bits(x):
    return TN.bits(x)


# ---------------------------------------------------------------------------------------------------------------
# the pieces
# ---------------------------------------------------------------------------------------------------------------
def segments(segmentScores, segmentState, startIdx, endIdx, selectionPenalty, boundaryCost, minRunBins, form="steps", signal_form=None):
    """`_solveParentConditionedSubpeakSegments` (signal_form: how the summit is found, where that differs from `form`)"""
    signal_form = signal_form or form
    s = np.asarray(segmentScores, np.float64)
    x = np.asarray(segmentState, np.float64)
    if s.size != x.size:
        raise ValueError("`segmentScores` and `segmentState` must match")
    required = int(np.argmax(s)) if form == "steps" else leftmost_argmax(s)
    mask, _, d = TN.solve(s, float(max(float(boundaryCost), 0.0)), float(selectionPenalty), int(max(int(minRunBins), 1)),
                          requiredIndex=required, form=form)
    runs = TN.run_bounds(mask)
    common = dict(subpeak_objective=float(d["penalized_objective"]), subpeak_boundary_penalty=float(d["boundary_penalty"]),
                  massive_subpeak_cleanup_candidate=False, massive_subpeak_cleanup_applied=False, massive_subpeak_split_gain=None,
                  massive_subpeak_split_z=None, massive_subpeak_gap_bins=None, massive_subpeak_parent_start_idx=int(startIdx),
                  massive_subpeak_parent_end_idx=int(endIdx))
    if not runs:
        return [whole_parent(x, startIdx, endIdx, signal_form, common)]
    out = []
    for a, b in runs:
        k = a + (int(np.argmax(x[a:b + 1])) if signal_form == "steps" else leftmost_argmax(x[a:b + 1]))
        out.append(order_child(dict(start_idx=int(startIdx + a), end_idx=int(startIdx + b), summit_idx=int(startIdx + k),
                                    segment_length_bins=int(b - a + 1), num_subpeaks=len(runs),
                                    split_from_parent=bool(len(runs) > 1 or a > 0 or b < x.size - 1), **common)))
    return out


CHILD_KEYS = ("start_idx", "end_idx", "summit_idx", "segment_length_bins", "num_subpeaks", "split_from_parent", "subpeak_objective",
              "subpeak_boundary_penalty", "massive_subpeak_cleanup_candidate", "massive_subpeak_cleanup_applied",
              "massive_subpeak_split_gain", "massive_subpeak_split_z", "massive_subpeak_gap_bins", "massive_subpeak_parent_start_idx",
              "massive_subpeak_parent_end_idx")


def order_child(d):
    return {k: d[k] for k in CHILD_KEYS}


def whole_parent(x, startIdx, endIdx, form, common):
    k = int(np.argmax(x)) if form == "steps" else leftmost_argmax(x)
    return order_child(dict(start_idx=int(startIdx), end_idx=int(endIdx), summit_idx=int(startIdx + k),
                            segment_length_bins=int(max(endIdx - startIdx + 1, 0)), num_subpeaks=1, split_from_parent=False, **common))


def leftmost_argmax(v):
    k, best = 0, float(v[0])
    for i in range(1, len(v)):
        if float(v[i]) > best:
            k, best = i, float(v[i])
        elif float(v[i]) == best:
            took("argmax_tie")
    return k


def trim(childStartIdx, childEndIdx, summitIdx, scores, trimScoreFloor):
    """`_trimChildSegmentAroundSummit`"""
    a, b = int(childStartIdx), int(childEndIdx)
    if trimScoreFloor is None or not math.isfinite(float(trimScoreFloor)):
        return a, b, False
    floor = float(trimScoreFloor)
    k = min(max(int(summitIdx), a), b)
    if b < a:
        return a, b, False
    if not scores[k] > floor:
        took("trim_summit_below")
        return a, b, False
    lo = hi = k
    while lo > a and scores[lo - 1] > floor:
        lo -= 1
    while hi < b and scores[hi + 1] > floor:
        hi += 1
    took("trim_" + ("both" if lo != a and hi != b else "left" if lo != a else "right" if hi != b else "none"))
    return lo, hi, bool(lo != a or hi != b)


def median_sorted(values):
    """np.median as two order statistics"""
    w = sorted(float(v) for v in values)
    m = len(w)
    took(f"median_of_{min(m, 5)}")
    return w[m // 2] if m % 2 else (w[m // 2 - 1] + w[m // 2]) / 2.0


def loop_max(values):
    best = float(values[0])
    for v in values[1:]:
        if float(v) > best:
            best = float(v)
    return best


# ---------------------------------------------------------------------------------------------------------------
# `_solutionToChromNarrowPeakRows`
# ---------------------------------------------------------------------------------------------------------------
def rows(chromosome, intervals, ends, state, scores, solution, prefix, nullScale, uncertainty=None, splitSubpeaks=True,
         trimScoreFloor=0.0, subpeakSelectionPenalty=None, subpeakBoundaryCost=None, minSubpeakBins=1,
         dropMedianSignalBelowNegativeLocalP=True, exportFilterUncertaintyMultiplier=2.0, scoreFloor=250.0, scoreCeil=1000.0,
         returnExportDetails=False, form="steps"):
    iv = np.asarray(intervals, np.int64).ravel()
    en = np.asarray(ends, np.int64).ravel()
    x = np.asarray(state, np.float64).ravel()
    s = np.asarray(scores, np.float64).ravel()
    sol = np.asarray(solution, np.uint8).ravel()
    if not (iv.size == en.size == s.size == sol.size == x.size):
        raise ValueError("`intervals`, `ends`, `state`, `scores`, and `solution` must match length")
    u = None
    if uncertainty is not None:
        u = np.asarray(uncertainty, np.float64).ravel()
        if u.size != x.size:
            raise ValueError("`uncertainty` must match `state` length")
    mult = float(exportFilterUncertaintyMultiplier)
    if not math.isfinite(mult) or mult < 0.0:
        raise ValueError("`exportFilterUncertaintyMultiplier` must be finite and non-negative")
    filt = bool(dropMedianSignalBelowNegativeLocalP and u is not None)
    details = {
        "num_candidate_segments": 0, "num_segments_dropped_median_signal_local_p": 0, "num_segments_dropped_min_peak_bp": 0,
        "min_peak_bp": MIN_PEAK_BP, "median_signal_local_p_multiplier": mult, "median_signal_local_p_filter_active": filt,
        "massive_subpeak_cleanup_active": False, "massive_subpeak_width_policy": None, "num_massive_subpeak_candidates": 0,
        "num_massive_subpeak_splits": 0, "num_massive_subpeak_segments_added": 0, "num_massive_subpeak_evaluated": 0,
        "num_massive_subpeak_contracts": 0, "num_coordinate_gap_splits": 0,
    }
    fallback = float(max(float(nullScale), 0.0))
    penalty = fallback if subpeakSelectionPenalty is None else float(subpeakSelectionPenalty)
    cost = fallback if subpeakBoundaryCost is None else float(subpeakBoundaryCost)
    min_run = int(max(int(minSubpeakBins), 1))
    n = int(sol.size)
    # parents
    parents = []
    if form == "steps":
        i = 0
        while i < n:
            if sol[i] == 0:
                i += 1
                continue
            a = i
            while i + 1 < n and sol[i + 1] > 0 and en[i] == iv[i + 1]:
                i += 1
            if i + 1 < n and sol[i + 1] > 0 and en[i] != iv[i + 1]:
                details["num_coordinate_gap_splits"] += 1
            parents.append((a, i))
            i += 1
    else:
        gaps = np.flatnonzero(en[:-1] != iv[1:]).tolist() if n > 1 else []
        for a, b in TN.run_bounds(sol > 0):
            cur = a
            for g in gaps:
                if a <= g < b:
                    parents.append((cur, g))
                    cur = g + 1
                    details["num_coordinate_gap_splits"] += 1
                    took("gap_inside_run")
            parents.append((cur, b))
    took("parents", len(parents))
    # the device form of a chain with a non-finite signal value inside a parent: the children from the dynamic programme as ever,
    # the signal-dependent numbers with NumPy's steps (the host decision of consenrich_amd/narrowpeak.py)
    sig = form
    if form == "device" and any(not np.all(np.isfinite(x[a:b + 1])) for a, b in parents):
        sig = "steps"
        took("decided_on_host")
    kept, meta = [], []
    for a, b in parents:
        seg_x = x[a:b + 1]
        if splitSubpeaks:
            kids = segments(s[a:b + 1], seg_x, a, b, penalty, cost, min_run, form, sig)
            took(f"parent_len_{b - a + 1}")
            took("children_%s" % ("3plus" if len(kids) >= 3 else len(kids)))
            if len(kids) == 1 and kids[0]["split_from_parent"]:
                took("single_child_shorter")
            if len(kids) == 1 and not kids[0]["split_from_parent"]:
                took("kept_whole")
        else:
            kids = [whole_parent(seg_x, a, b, sig, dict(
                subpeak_objective=0.0, subpeak_boundary_penalty=0.0, massive_subpeak_cleanup_candidate=False,
                massive_subpeak_cleanup_applied=False, massive_subpeak_split_gain=None, massive_subpeak_split_z=None,
                massive_subpeak_gap_bins=None, massive_subpeak_parent_start_idx=int(a), massive_subpeak_parent_end_idx=int(b)))]
        for kid in kids:
            ua, ub, k = kid["start_idx"], kid["end_idx"], kid["summit_idx"]
            ca, cb, trimmed = trim(ua, ub, k, s, trimScoreFloor)
            cx, cs = x[ca:cb + 1], s[ca:cb + 1]
            details["num_candidate_segments"] += 1
            if sig == "steps":
                med, mx, ms = float(np.median(cx)), float(np.max(cx)), float(np.max(cs))
            else:
                med, mx, ms = float(median_sorted(cx)), loop_max(cx), loop_max(cs)
            local = thr = None
            if filt:
                p = u[ca:cb + 1]
                p = p[np.isfinite(p)]
                if p.size != cb - ca + 1:
                    took("uncertainty_some_nonfinite" if p.size else "uncertainty_none_finite")
                if p.size > 0:
                    local = float(np.median(p)) if form == "steps" else float(median_sorted(p))
                    thr = float(-mult * local)
                    if med == thr:
                        took("median_equal_threshold")
                    if med < thr:
                        details["num_segments_dropped_median_signal_local_p"] += 1
                        took("dropped_median")
                        continue
            summit = int(iv[k] + max(1, int((en[k] - iv[k]) // 2)))
            cstart, cend = int(iv[ca]), int(en[cb])
            if cend - cstart < MIN_PEAK_BP:
                details["num_segments_dropped_min_peak_bp"] += 1
                took("dropped_min_bp")
                continue
            name = f"{prefix}_{chromosome}_{len(kept) + 1}"
            kept.append(dict(start=cstart, end=cend, signal=mx, raw=ms, peak=int(max(0, summit - cstart)), name=name))
            meta.append({
                "name": name, "chromosome": str(chromosome), "start": cstart, "end": cend, "summit": summit, "start_idx": int(ca),
                "end_idx": int(cb), "summit_idx": int(k), "untrimmed_start_idx": int(ua), "untrimmed_end_idx": int(ub),
                "segment_length_bins": int(kid["segment_length_bins"]), "median_state": med, "local_median_p": local,
                "median_signal_threshold": thr, "max_state": mx, "max_score": ms, "num_subpeaks": int(kid["num_subpeaks"]),
                "split_from_parent": bool(kid["split_from_parent"]), "subpeak_objective": float(kid["subpeak_objective"]),
                "subpeak_boundary_penalty": float(kid["subpeak_boundary_penalty"]), "massive_subpeak_cleanup_candidate": False,
                "massive_subpeak_cleanup_applied": False, "massive_subpeak_cleanup_mode": None, "massive_subpeak_width_p": None,
                "massive_subpeak_width_q": None, "massive_subpeak_width_threshold_bp": None, "massive_subpeak_split_gain": None,
                "massive_subpeak_split_z": None, "massive_subpeak_gap_bins": None, "massive_subpeak_core_width_bp": None,
                "massive_subpeak_core_score_floor": None, "trimmed_from_parent": bool(trimmed),
                "trim_score_floor": None if trimScoreFloor is None else float(trimScoreFloor),
                "untrimmed_start": int(iv[ua]), "untrimmed_end": int(en[ub]),
            })
    if not kept:
        if returnExportDetails:
            details["num_segments_kept"] = 0
            return [], [], details
        return [], []
    raw = np.asarray([r["raw"] for r in kept], np.float64)
    lo, hi = float(np.min(raw)), float(np.max(raw))
    span = max(hi - lo, 1.0e-12)
    if hi - lo < 1.0e-12:
        took("span_floor")
    out = []
    for r in kept:
        scaled = scoreFloor + (scoreCeil - scoreFloor) * ((float(r["raw"]) - lo) / span)
        if scaled - math.floor(scaled) == 0.5:
            took("half_way")
        out.append([str(chromosome), r["start"], r["end"], r["name"], int(round(scaled)), ".", float(r["signal"]), -1, -1, r["peak"]])
    details["num_segments_kept"] = len(out)
    if returnExportDetails:
        return out, meta, details
    return out, meta


# ---------------------------------------------------------------------------------------------------------------
# comparison and flattening (fixtures hold arrays only)
# ---------------------------------------------------------------------------------------------------------------
def differences(got, want):
    """Paths at which two results (rows, meta[, details]) differ: floats by bit pattern, everything else with its type; dicts
    with their key order."""
    out = TN.differences(list(got), list(want))
    if not out:
        for a, b in zip(got, want):
            for p, q in zip(a if isinstance(a, list) else [a], b if isinstance(b, list) else [b]):
                if isinstance(q, dict) and list(p) != list(q):
                    out.append("key order")
    return out


def flatten(result):
    """What a fixture keeps of (rows, meta, details): every number, as arrays; names and key lists as strings."""
    rws, meta, details = result
    nan = float("nan")
    return {
        "row_i": np.asarray([[r[1], r[2], r[4], r[7], r[8], r[9]] for r in rws], np.int64).reshape(len(rws), 6),
        "row_f": np.asarray([r[6] for r in rws], np.float64),
        "row_s": np.asarray(["\t".join((r[0], r[3], r[5])) for r in rws], dtype="U"),
        "meta_f": np.asarray([[nan if m[k] is None else float(m[k]) for k in META_FLOATS] for m in meta], np.float64).reshape(
            len(meta), len(META_FLOATS)),
        "meta_none": np.asarray([[int(m[k] is None) for k in META_FLOATS + META_NONE] for m in meta], np.int64).reshape(
            len(meta), len(META_FLOATS + META_NONE)),
        "meta_i": np.asarray([[int(m[k]) for k in META_INTS] for m in meta], np.int64).reshape(len(meta), len(META_INTS)),
        "meta_s": np.asarray(["\t".join((m["name"], m["chromosome"])) for m in meta], dtype="U"),
        "meta_keys": np.asarray(["\t".join(meta[0]) if meta else ""], dtype="U"),
        "detail_i": np.asarray([details[k] for k in DETAIL_INTS], np.int64),
        "detail_f": np.asarray([details["median_signal_local_p_multiplier"]], np.float64),
        "detail_b": np.asarray([int(details["median_signal_local_p_filter_active"]), int(details["massive_subpeak_cleanup_active"]),
                                int(details["massive_subpeak_width_policy"] is None)], np.int64),
        "detail_keys": np.asarray(["\t".join(details)], dtype="U"),
    }


def same_flat(a, b):
    bad = TN.same_flat({k: v for k, v in a.items() if v.dtype.kind != "U"}, {k: v for k, v in b.items() if v.dtype.kind != "U"})
    for k in set(a) | set(b):
        if k in a and k in b and a[k].dtype.kind == "U" and (a[k].shape != b[k].shape or not np.array_equal(a[k], b[k])):
            bad.append(k)
    return sorted(bad)
