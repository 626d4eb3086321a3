"""The massive sub-peak clean-up (csrc/csr_cleanup.h), bit for bit the reference's `_forceMassiveSubpeakSegments` (peaks.py:4579-4786)
with `_bestMassiveSubpeakSplit` (3299-3352), `_contractMassiveSubpeakSegment` (3355-3460) and `_makeSubpeakSegment` (3463-3516),
and the width policy it runs under: `_massiveSubpeakWidthScores`, `_learnMassiveSubpeakWidthPolicy`, `_massiveSubpeakWidthPValue`
(3160-3296).

What runs where.  The POLICY is scalar work on a few thousand peak widths and stays on the host (NumPy, and `scipy.stats.norm.sf`,
the reference's own source, imported when first needed).  The recursion over a child's bins -- the order statistics of every node
from one cooperative sort, the gap scan, the contraction -- runs on the DEVICE, one wavefront per child (`csr_cleanup_plan`).  Only
the child's own bins travel: its scores and its n + 1 bin edges, or no coordinates at all where the bins are equally wide.

`solution_to_chrom_narrowpeak_rows` is the reference's row export under a width policy on host arrays, composed of three device
calls: the first pass's children (csr_export_peaks), their final segments (csr_cleanup_plan), and the finishing step per SEGMENT,
which is csr_export_peaks again with the segments as parents that do not split.

From the RESIDENT fit the same three steps are `DeviceBatch.narrowpeak_rows(width_policy=...)` (the segments come from
`csr_batch_cleanup_plan`, which reads the resident score tracks), and `driver.cleanup_peaks_batch` learns the policy from a
batch's kept widths and runs that second pass.  `consenrich_amd.narrowpeak`'s own drop-in still refuses a policy.  A child
that holds a coordinate gap is refused here (the export never forms one: it cuts parents at gaps)."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib as L
from ._lib import _vp

# the reference's constants (constants.py:541-552, peaks.py:120)
CLEANUP_DEFAULT = True
MIN_BP = 7500
WIDTH_ALPHA = 0.1
WIDTH_BULK_QUANTILE = 0.95
MAX_FRACTION = 0.005
MIN_LOG_GAP = 0.10
MIN_PEAKS = 25
SPLIT_QUANTILE = 0.25
SPLIT_Z = 2.0
MAX_DEPTH = 8
TRIGGER_Z_CAP = 3.0
# the device's limits (include/consenrich_amd.h)
SORT_TILE = L.CLEANUP_SORT_TILE             # node lengths up to it are sorted in LDS, longer ones in global memory
MAX_SEGMENTS = L.CLEANUP_MAX_SEGMENTS
MAX_DEPTH_SUPPORTED = L.CLEANUP_MAX_DEPTH
COORDS = "auto"     # "auto": equally wide bins travel as a step, others as edges; "edges": always the edge array (tests)
STATS = {"calls": 0, "children": 0, "segments": 0}

POLICY = np.dtype([("threshold", "<f8"), ("contract_threshold", "<f8"), ("split_quantile", "<f8"), ("min_split_z", "<f8"),
                   ("boundary_cost", "<f8"), ("min_run", "<i4"), ("max_depth", "<i4")])
CHILD = np.dtype([("start", "<i8"), ("end", "<i8")])
SEGMENT = np.dtype([("start", "<i8"), ("end", "<i8"), ("core_width_bp", "<i8"), ("gain", "<f8"), ("z", "<f8"),
                    ("core_score_floor", "<f8"), ("gap_bins", "<i4"), ("mode", "<i4"), ("flags", "<i4"), ("child", "<i4")])
COUNTS = np.dtype([(k, "<i4") for k in ("candidates", "splits", "segments_added", "evaluated", "contracts", "n_segments", "flags",
                                        "reserved")])
NODE = np.dtype([("a", "<i8"), ("b", "<i8"), ("width", "<i8"), ("baseline", "<f8"), ("scale", "<f8"), ("deficit", "<f8"),
                 ("gain", "<f8"), ("z", "<f8"), ("floor", "<f8"), ("found", "<i4"), ("mode", "<i4"), ("gap_bins", "<i4"),
                 ("reserved", "<i4")])
COUNTERS = ("candidates", "splits", "segments_added", "evaluated", "contracts")


def _i32(v):
    return int(min(max(int(v), -(1 << 31)), (1 << 31) - 1))


# ---------------------------------------------------------------------------------------------------------------
# the width policy, on the host
# ---------------------------------------------------------------------------------------------------------------
def _norm_sf(z):
    from scipy import stats      # the reference's own source of norm.sf

    return stats.norm.sf(z)


def bh_q_values(p_values):
    """Benjamini-Hochberg q values as the reference takes them: a stable sort, the running minimum from the largest p down."""
    p = np.asarray(p_values, dtype=np.float64).ravel()
    if p.size == 0:
        return np.asarray([], dtype=np.float64)
    if not np.all(np.isfinite(p)):
        raise ValueError("`pValues` contains non-finite values")
    p = np.clip(p, 0.0, 1.0)
    ranked = np.argsort(p, kind="mergesort")
    q = np.empty_like(p)
    m, running = int(p.size), 1.0
    for rank in range(m, 0, -1):
        k = int(ranked[rank - 1])
        running = min(running, float(p[k]) * float(m) / float(rank))
        q[k] = min(running, 1.0)
    return q


def _robust_log_null(logs):
    """centre and scale of the bulk's log widths: median and 1.4826 MAD, then IQR / 1.349, then 1"""
    centre = float(np.median(logs))
    scale = 1.4826 * float(np.median(np.abs(logs - centre)))
    if not math.isfinite(scale) or scale <= 1.0e-12:
        scale = float(np.quantile(logs, 0.75) - np.quantile(logs, 0.25)) / 1.349
    if not math.isfinite(scale) or scale <= 1.0e-12:
        scale = 1.0
    return centre, scale


def massive_subpeak_width_scores(widthsBP, bulkQuantile=WIDTH_BULK_QUANTILE):
    """Drop-in for `_massiveSubpeakWidthScores`: (p, q, {"center", "scale"}) of the widths under a robust log-normal null."""
    widths = np.asarray(widthsBP, dtype=np.float64).ravel()
    usable = widths[np.isfinite(widths) & (widths > 0.0)]
    if usable.size == 0:
        ones = np.ones_like(widths, dtype=np.float64)
        return ones, ones, {"center": 0.0, "scale": 1.0}
    all_logs, logs = np.log(np.maximum(widths, 1.0)), np.log(usable)
    cutoff = float(np.quantile(logs, float(np.clip(float(bulkQuantile), 0.5, 0.99))))
    bulk = logs[logs <= cutoff]
    if bulk.size < max(5, int(math.ceil(0.1 * logs.size))):
        bulk = logs
    centre, scale = _robust_log_null(bulk)
    p = _norm_sf((all_logs - centre) / scale)
    if not np.all(np.isfinite(p)):
        raise RuntimeError("width-score p-values contain non-finite values")
    p = np.clip(p, 0.0, 1.0)
    return p, bh_q_values(p), {"center": float(centre), "scale": float(scale)}


def learn_massive_subpeak_width_policy(widthsBP, enabled=CLEANUP_DEFAULT, minBP=MIN_BP, alpha=WIDTH_ALPHA,
                                       bulkQuantile=WIDTH_BULK_QUANTILE, maxFraction=MAX_FRACTION, minLogGap=MIN_LOG_GAP,
                                       minPeaks=MIN_PEAKS):
    """Drop-in for `_learnMassiveSubpeakWidthPolicy`: the policy dict, with the reference's keys, key order and Python types."""
    widths = np.asarray(widthsBP, dtype=np.float64).ravel()
    usable = widths[np.isfinite(widths) & (widths > 0.0)]
    floor_bp = int(max(int(minBP), 1))
    policy = {
        "enabled": bool(enabled), "method": "robust_log_width_tail_gap", "width_threshold_bp": None,
        "gap_width_threshold_bp": None, "width_cap_bp": None, "width_cap_z": float(TRIGGER_Z_CAP), "min_bp": floor_bp,
        "contract_width_bp": floor_bp, "alpha": float(alpha), "bulk_quantile": float(bulkQuantile),
        "max_fraction": float(maxFraction), "min_log_gap": float(minLogGap), "min_peaks": int(max(int(minPeaks), 1)),
        "num_peaks": int(usable.size), "num_width_tail_candidates": 0, "num_width_cluster_candidates": 0,
        "selected_log_gap": None, "null_center": None, "null_scale": None, "active": False,
    }
    if not enabled or usable.size < policy["min_peaks"]:
        return policy
    _, q, null = massive_subpeak_width_scores(usable, bulkQuantile=float(bulkQuantile))
    policy["null_center"], policy["null_scale"] = float(null["center"]), float(null["scale"])
    level = float(np.clip(float(alpha), 0.0, 1.0))
    least = float(floor_bp)
    in_tail = (usable >= least) & np.isfinite(q) & (q <= level)
    policy["num_width_tail_candidates"] = int(np.sum(in_tail))
    if not np.any(in_tail):
        return policy
    # the narrowest width that opens a clean upper cluster: a log gap of at least minLogGap below it, at most maxFraction of the
    # peaks from it upwards, every one of them significant
    distinct = np.unique(usable)
    most = int(max(1, math.floor(float(maxFraction) * float(usable.size))))
    chosen = None
    for below, width in zip(distinct[:-1].tolist(), distinct[1:].tolist()):
        if width < least:
            continue
        gap = float(np.log(width) - np.log(below))
        if gap < float(minLogGap):
            continue
        upper = usable >= float(width)
        members = int(np.sum(upper))
        if members < 1 or members > most or not np.all(q[upper] <= level):
            continue
        chosen = (float(width), members, gap)       # `distinct` ascends: the first admissible one is the minimum
        break
    if chosen is None:
        return policy
    gap_width, members, gap = chosen
    cap = math.exp(float(null["center"]) + float(TRIGGER_Z_CAP) * float(null["scale"]))
    if not math.isfinite(cap) or cap <= 0.0:
        cap = gap_width
    cap = float(max(least, cap))
    threshold = float(max(least, min(gap_width, cap)))
    policy["gap_width_threshold_bp"] = int(round(gap_width))
    policy["width_cap_bp"] = int(round(cap))
    policy["width_threshold_bp"] = int(round(threshold))
    policy["num_width_cluster_candidates"] = int(np.sum(usable >= threshold))
    policy["num_width_tail_gap_candidates"] = int(members)
    policy["selected_log_gap"] = float(gap)
    policy["active"] = True
    return policy


def massive_subpeak_width_pvalue(widthBP, policy):
    """Drop-in for `_massiveSubpeakWidthPValue`: (p, None) of one width under the policy's null, (None, None) without one."""
    if policy is None:
        return None, None
    centre, scale = policy.get("null_center"), policy.get("null_scale")
    if centre is None or scale is None:
        return None, None
    scale = float(scale)
    if not math.isfinite(scale) or scale <= 0.0:
        return None, None
    z = (math.log(max(float(widthBP), 1.0)) - float(centre)) / scale
    return float(np.clip(float(_norm_sf(z)), 0.0, 1.0)), None


# ---------------------------------------------------------------------------------------------------------------
# the recursion, on the device
# ---------------------------------------------------------------------------------------------------------------
def _coords(intervals, ends, start, end):
    """What the device reads of the coordinates of bins [start, end]: (edges or None, origin, step)."""
    iv = np.asarray(intervals, dtype=np.int64)[start:end + 1]
    en = np.asarray(ends, dtype=np.int64)[start:end + 1]
    if iv.size != end - start + 1 or en.size != iv.size:
        raise ValueError("`intervals` and `ends` do not cover the segment")
    if np.any(en[:-1] != iv[1:]):
        raise ValueError("a segment that holds a coordinate gap is not supported")
    edges = np.ascontiguousarray(np.concatenate((iv, en[-1:])))
    steps = np.diff(edges)
    if np.any(steps < 0):
        raise ValueError("bin edges must not decrease")
    if COORDS == "auto" and steps.size and np.all(steps == steps[0]):
        return None, int(edges[0]), int(steps[0])
    return edges, 0, 0


def plan(op, scores, edges, origin, step, children, policy_row):
    """csr_cleanup_plan on host arrays: (segments, counts) of a FORCE call, the node records of a piece operation."""
    s = np.ascontiguousarray(scores, dtype=np.float64)
    kids = np.ascontiguousarray(children, dtype=CHILD)
    pol = np.asarray([policy_row], POLICY)
    lib = L.lib()
    STATS["calls"] += 1
    STATS["children"] += int(kids.size)
    if op == L.CLEANUP_OP_FORCE:
        seg = np.zeros(MAX_SEGMENTS * max(int(kids.size), 1), SEGMENT)
        cnt = np.zeros(kids.size, COUNTS)
        total = C.c_int64(0)
        L.check_value(lib.csr_cleanup_plan(op, s.size, L.dp(s), None if edges is None else edges.ctypes.data_as(L.I64P), origin, step,
                                           kids.size, _vp(kids), _vp(pol), seg.size, _vp(seg), C.byref(total), _vp(cnt), None))
        STATS["segments"] += int(total.value)
        return seg[:int(total.value)], cnt
    nodes = np.zeros(kids.size, NODE)
    L.check_value(lib.csr_cleanup_plan(op, s.size, L.dp(s), None if edges is None else edges.ctypes.data_as(L.I64P), origin, step,
                                       kids.size, _vp(kids), _vp(pol), 0, None, None, None, _vp(nodes)))
    return nodes


def best_massive_subpeak_split(scores, boundaryCost, minRunBins, splitQuantile=SPLIT_QUANTILE):
    """Drop-in for `_bestMassiveSubpeakSplit`: the best low-score gap of the scores as a dict, or None.  (Non-finite scores, which
    the reference carries into a NaN baseline, are refused.)"""
    s = np.ascontiguousarray(np.asarray(scores, dtype=np.float64).ravel())
    n, min_bins = int(s.size), int(max(int(minRunBins), 1))
    if n < 3 * min_bins:
        return None
    nd = plan(L.CLEANUP_OP_SPLIT, s, None, 0, 1, [(0, n - 1)], (0.0, 0.0, float(splitQuantile), 0.0, float(boundaryCost), min_bins, 0))[0]
    if not nd["found"]:
        return None
    return {"gap_start_local": int(nd["a"]), "gap_end_local": int(nd["b"]), "gap_bins": int(nd["gap_bins"]),
            "baseline": float(nd["baseline"]), "scale": float(nd["scale"]), "deficit": float(nd["deficit"]), "gain": float(nd["gain"]),
            "z": float(nd["z"])}


def contract_massive_subpeak_segment(startIdx, endIdx, scores, intervals, ends, thresholdBP, minRunBins, splitQuantile=SPLIT_QUANTILE):
    """Drop-in for `_contractMassiveSubpeakSegment`: (start, end, details) of the adaptive or width-capped core, or None."""
    s = np.asarray(scores, dtype=np.float64)
    start, end = int(startIdx), int(endIdx)
    if start < 0 or end < start or end >= s.size:
        return None
    threshold = float(thresholdBP)
    if not math.isfinite(threshold) or threshold <= 0.0:
        return None
    local = np.ascontiguousarray(s[start:end + 1])
    if not np.all(np.isfinite(local)):
        raise ValueError("`scores` contains non-finite values")
    edges, origin, step = _coords(intervals, ends, start, end)
    row = (0.0, threshold, float(splitQuantile), 0.0, 0.0, _i32(max(int(minRunBins), 1)), 0)
    nd = plan(L.CLEANUP_OP_CONTRACT, local, edges, origin, step, [(0, local.size - 1)], row)[0]
    if not nd["found"]:
        return None
    mode = L.CLEANUP_MODES[int(nd["mode"])]
    return int(start + int(nd["a"])), int(start + int(nd["b"])), {
        "mode": mode, "core_score_floor": float(nd["floor"]) if mode == "adaptive_core" else None, "core_width_bp": int(nd["width"])}


def contract_threshold(policy, threshold):
    """min(contract_width_bp or min_bp or 7500, threshold), as `_forceMassiveSubpeakSegments` forms it"""
    value = float(policy.get("contract_width_bp", policy.get("min_bp", MIN_BP)))
    if not math.isfinite(value) or value <= 0.0:
        value = float(MIN_BP)
    return float(min(value, threshold))


def segment_dict(seg, offset, state, parent_start, parent_end, num_subpeaks, split_from_parent, objective, boundary_penalty):
    """One segment record as the dict `_makeSubpeakSegment` makes (the summit is the arg-max of the signal over the segment)."""
    a, b, flags = int(offset + int(seg["start"])), int(offset + int(seg["end"])), int(seg["flags"])
    has_split = bool(flags & L.CLEANUP_HAS_SPLIT)
    return {
        "start_idx": a,
        "end_idx": b,
        "summit_idx": int(a + int(np.argmax(state[a:b + 1]))),
        "segment_length_bins": int(max(b - a + 1, 0)),
        "num_subpeaks": int(num_subpeaks),
        "split_from_parent": bool(split_from_parent),
        "subpeak_objective": float(objective),
        "subpeak_boundary_penalty": float(boundary_penalty),
        "massive_subpeak_cleanup_candidate": bool(flags & L.CLEANUP_CANDIDATE),
        "massive_subpeak_cleanup_applied": bool(flags & L.CLEANUP_APPLIED),
        "massive_subpeak_cleanup_mode": L.CLEANUP_MODES[int(seg["mode"])],
        "massive_subpeak_split_gain": float(seg["gain"]) if has_split else None,
        "massive_subpeak_split_z": float(seg["z"]) if has_split else None,
        "massive_subpeak_gap_bins": int(seg["gap_bins"]) if has_split else None,
        "massive_subpeak_core_width_bp": int(seg["core_width_bp"]) if flags & L.CLEANUP_HAS_CORE_WIDTH else None,
        "massive_subpeak_core_score_floor": float(seg["core_score_floor"]) if flags & L.CLEANUP_HAS_CORE_FLOOR else None,
        "massive_subpeak_parent_start_idx": int(parent_start),
        "massive_subpeak_parent_end_idx": int(parent_end),
    }


def force_massive_subpeak_segments(child, scores, state, intervals, ends, widthPolicy, boundaryCost, minRunBins,
                                   splitQuantile=SPLIT_QUANTILE, minSplitZ=SPLIT_Z, maxDepth=MAX_DEPTH):
    """Drop-in for `_forceMassiveSubpeakSegments`: (the child's final segments from left to right, the five counters)."""
    threshold = None if widthPolicy is None else widthPolicy.get("width_threshold_bp")
    if threshold is None:
        return [dict(child)], {k: 0 for k in COUNTERS}
    threshold = float(threshold)
    s = np.asarray(scores, dtype=np.float64)
    x = np.asarray(state, dtype=np.float64)
    start, end = int(child["start_idx"]), int(child["end_idx"])
    if start < 0 or end < start or end >= s.size:
        raise ValueError("the child's bins are outside `scores`")
    edges, origin, step = _coords(intervals, ends, start, end)
    row = (threshold, contract_threshold(widthPolicy, threshold), float(splitQuantile), float(minSplitZ), float(boundaryCost),
           _i32(minRunBins), _i32(max(int(maxDepth), 0)))
    seg, cnt = plan(L.CLEANUP_OP_FORCE, s[start:end + 1], edges, origin, step, [(0, end - start)], row)
    own = bool(child.get("split_from_parent", False))
    out = [segment_dict(g, start, x, start, end, len(seg), bool(int(g["flags"]) & L.CLEANUP_SPLIT_FROM_PARENT) or own,
                        float(child.get("subpeak_objective", 0.0)), float(child.get("subpeak_boundary_penalty", 0.0))) for g in seg]
    return out, {k: int(cnt[0][k]) for k in COUNTERS}


# ---------------------------------------------------------------------------------------------------------------
# narrowPeak rows under a width policy, on host arrays
# ---------------------------------------------------------------------------------------------------------------
BATCH_CHILD = np.dtype([("start", "<i8"), ("end", "<i8"), ("edge_base", "<i8"), ("chain", "<i4"), ("reserved", "<i4")])


def count_details(details, cnt):
    """the five counters of a chain's children into its export details"""
    for key in COUNTERS:
        details[f"num_massive_subpeak_{key}"] = int(cnt[key].sum())


def finish_segments(done, seg, cnt, peaks):
    """What the finishing step per segment cannot know, into its records `done` (one per segment, in order): the segment count of
    the child as num_subpeaks, split_from_parent (the segment's flag OR the child's own), the child's parent, objective and boundary
    penalty.  `seg["child"]` indexes `peaks` and `cnt`.  Returns the segments by their first bin (they are disjoint)."""
    by_start = {}
    for g, p in zip(seg, done):
        kid = peaks[int(g["child"])]
        split = bool(int(g["flags"]) & L.CLEANUP_SPLIT_FROM_PARENT) or bool(int(kid["flags"]) & L.EXPORT_SPLIT_FROM_PARENT)
        p["flags"] = (int(p["flags"]) & ~L.EXPORT_SPLIT_FROM_PARENT) | (L.EXPORT_SPLIT_FROM_PARENT if split else 0)
        p["num_subpeaks"] = int(cnt[int(g["child"])]["n_segments"])
        p["parent"] = kid["parent"]
        p["subpeak_objective"], p["subpeak_boundary_penalty"] = kid["subpeak_objective"], kid["subpeak_boundary_penalty"]
        by_start[int(g["start"])] = g
    if len(by_start) != len(seg):
        raise RuntimeError("clean-up segments are not disjoint")
    return by_start


def fill_meta(meta, by_start, policy):
    """The clean-up's keys of a chain's meta dicts: the segment's fields where the clean-up ran (`by_start`: segments by their
    untrimmed first bin), and for every peak the width p value and the threshold the policy holds, active or not."""
    threshold = policy.get("width_threshold_bp")
    for m in meta:
        g = by_start.get(m["untrimmed_start_idx"])
        if g is not None:
            fl, hs = int(g["flags"]), bool(int(g["flags"]) & L.CLEANUP_HAS_SPLIT)
            m["massive_subpeak_cleanup_candidate"] = bool(fl & L.CLEANUP_CANDIDATE)
            m["massive_subpeak_cleanup_applied"] = bool(fl & L.CLEANUP_APPLIED)
            m["massive_subpeak_cleanup_mode"] = L.CLEANUP_MODES[int(g["mode"])]
            m["massive_subpeak_split_gain"] = float(g["gain"]) if hs else None
            m["massive_subpeak_split_z"] = float(g["z"]) if hs else None
            m["massive_subpeak_gap_bins"] = int(g["gap_bins"]) if hs else None
            m["massive_subpeak_core_width_bp"] = int(g["core_width_bp"]) if fl & L.CLEANUP_HAS_CORE_WIDTH else None
            m["massive_subpeak_core_score_floor"] = float(g["core_score_floor"]) if fl & L.CLEANUP_HAS_CORE_FLOOR else None
        m["massive_subpeak_width_p"] = massive_subpeak_width_pvalue(float(m["end"] - m["start"]), policy)[0]
        m["massive_subpeak_width_threshold_bp"] = None if threshold is None else int(threshold)


def policy_row(policy, cost, min_run, split_quantile=SPLIT_QUANTILE, min_split_z=SPLIT_Z, max_depth=MAX_DEPTH):
    """One csr_cleanup_policy row of a policy dict that has a threshold."""
    threshold = float(policy["width_threshold_bp"])
    return (threshold, contract_threshold(policy, threshold), float(split_quantile), float(min_split_z), float(cost), _i32(min_run),
            _i32(max(int(max_depth), 0)))


def _cleaned_children(peaks, s, intervals, ends, policy, cost, min_run, split_quantile, min_split_z):
    """The first pass's children through ONE plan call: (segment records in chain indices, per segment the index of its child, the
    per-child counts).  Only the children's own bins travel, one after the other with a separator bin between two children (its
    edges are the end of one child and the start of the next, so one edge array serves all of them)."""
    threshold = float(policy["width_threshold_bp"])
    parts, edges, kids, at = [], [], [], 0
    for k, p in enumerate(peaks):
        a, b = int(p["untrimmed_start"]), int(p["untrimmed_end"])
        if k:
            parts.append(np.zeros(1))
            at += 1
        parts.append(s[a:b + 1])
        edges += [intervals[a:b + 1], ends[b:b + 1]]
        kids.append((at, at + b - a))
        at += b - a + 1
    # (a child's edges are intervals[a .. b] and ends[b]; the separator bin after it is [ends[b], intervals[next a]))
    row = (threshold, contract_threshold(policy, threshold), float(split_quantile), float(min_split_z), float(cost), _i32(min_run),
           MAX_DEPTH)
    seg, cnt = plan(L.CLEANUP_OP_FORCE, np.concatenate(parts), np.ascontiguousarray(np.concatenate(edges), dtype=np.int64), 0, 0, kids, row)
    seg = seg.copy()
    shift = np.asarray([int(peaks[k]["untrimmed_start"]) - kids[k][0] for k in range(len(kids))], np.int64)[seg["child"]]
    seg["start"] += shift
    seg["end"] += shift
    return seg, cnt


def solution_to_chrom_narrowpeak_rows(chromosome, intervals, ends, state, scores, solution, prefix, nullScale, uncertainty=None,
                                      splitSubpeaks=True, trimScoreFloor=0.0, subpeakSelectionPenalty=None, subpeakBoundaryCost=None,
                                      minSubpeakBins=1, massiveSubpeakCleanup=False, massiveSubpeakWidthPolicy=None,
                                      massiveSubpeakSplitQuantile=SPLIT_QUANTILE, massiveSubpeakSplitZ=SPLIT_Z,
                                      dropMedianSignalBelowNegativeLocalP=True, exportFilterUncertaintyMultiplier=2.0,
                                      scoreFloor=250.0, scoreCeil=1000.0, nestedHierarchy=None, nestedDetails=None,
                                      returnExportDetails=False):
    """Drop-in for `_solutionToChromNarrowPeakRows` with the massive sub-peak clean-up (still without a hierarchy), on host arrays:
    (rows, meta) or (rows, meta, exportDetails).  Three device calls and no per-bin work on the host: the first pass's children
    (csr_export_peaks), their final segments (csr_cleanup_plan, if the policy is active), and the finishing step per SEGMENT --
    summit, trim, medians, maxima, filter flag -- which is csr_export_peaks again with the segments as parents that do not split."""
    from . import narrowpeak as P
    from .nested import run_bounds

    policy = massiveSubpeakWidthPolicy
    if policy is None:
        return P.solution_to_chrom_narrowpeak_rows(
            chromosome, intervals, ends, state, scores, solution, prefix, nullScale, uncertainty, splitSubpeaks, trimScoreFloor,
            subpeakSelectionPenalty, subpeakBoundaryCost, minSubpeakBins, massiveSubpeakCleanup, None, massiveSubpeakSplitQuantile,
            massiveSubpeakSplitZ, dropMedianSignalBelowNegativeLocalP, exportFilterUncertaintyMultiplier, scoreFloor, scoreCeil,
            nestedHierarchy, nestedDetails, returnExportDetails)
    if nestedHierarchy is not None or (nestedDetails is not None and any(
            k in nestedDetails for k in ("nestedHierarchy", "nested_hierarchy", "hierarchy"))):
        raise ValueError("`nestedHierarchy` is not supported: the export hierarchy is not built")
    intervals = np.asarray(intervals, dtype=np.int64).ravel()
    ends = np.asarray(ends, dtype=np.int64).ravel()
    x = np.ascontiguousarray(np.asarray(state, dtype=np.float64).ravel())
    s = np.ascontiguousarray(np.asarray(scores, dtype=np.float64).ravel())
    sol = np.asarray(solution, dtype=np.uint8).ravel()
    if intervals.size != x.size or ends.size != x.size or s.size != x.size or sol.size != x.size:
        raise ValueError("`intervals`, `ends`, `state`, `scores`, and `solution` must match length")
    u = None
    if uncertainty is not None:
        u = np.ascontiguousarray(np.asarray(uncertainty, dtype=np.float64).ravel())
        if u.size != x.size:
            raise ValueError("`uncertainty` must match `state` length")
    mult = P.validate_multiplier(exportFilterUncertaintyMultiplier)
    use_filter = bool(dropMedianSignalBelowNegativeLocalP and u is not None)
    active = bool(massiveSubpeakCleanup and bool(policy.get("active", False)))
    details = P.export_details(mult, use_filter)
    details["massive_subpeak_cleanup_active"] = active
    details["massive_subpeak_width_policy"] = dict(policy)
    starts, stops = run_bounds(sol)
    ps, pe, cuts = P.cut_parents(starts, stops, intervals, ends)
    details["num_coordinate_gap_splits"] = cuts
    rows, meta = [], []
    if ps.size:
        fallback = float(max(float(nullScale), 0.0))
        penalty = fallback if subpeakSelectionPenalty is None else float(subpeakSelectionPenalty)
        cost = fallback if subpeakBoundaryCost is None else float(subpeakBoundaryCost)
        if splitSubpeaks:
            if not np.all(np.isfinite(s[ps[0]:pe[0] + 1])):
                raise ValueError("`scores` contains non-finite values")
            if not math.isfinite(float(max(cost, 0.0))):
                raise ValueError("`boundaryCosts` must be finite and non-negative")
            if not math.isfinite(penalty):
                raise ValueError("`selectionPenalty` must be finite")
        row = P.chain_cfg(penalty, cost, trimScoreFloor, mult, minSubpeakBins, splitSubpeaks, use_filter)
        peaks = P._one_chain(x, s, u, row, list(zip(ps.tolist(), pe.tolist())))
        by_start = {}
        if active and policy.get("width_threshold_bp") is not None and peaks.size:
            seg, cnt = _cleaned_children(peaks, s, intervals, ends, policy, cost, int(max(int(minSubpeakBins), 1)),
                                         massiveSubpeakSplitQuantile, massiveSubpeakSplitZ)
            count_details(details, cnt)
            flat = P.chain_cfg(penalty, cost, trimScoreFloor, mult, minSubpeakBins, False, use_filter)
            done = P._one_chain(x, s, u, flat, list(zip(seg["start"].tolist(), seg["end"].tolist())))
            by_start = finish_segments(done, seg, cnt, peaks)
            peaks = done
        rows, meta = P.assemble(chromosome, intervals, ends, prefix, peaks, mult, trimScoreFloor, details, scoreFloor, scoreCeil)
        fill_meta(meta, by_start, policy)
    if not rows:
        if returnExportDetails:
            details["num_segments_kept"] = 0
            return [], [], details
        return [], []
    if returnExportDetails:
        return rows, meta, details
    return rows, meta
