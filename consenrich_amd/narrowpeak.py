"""narrowPeak rows from a solution mask on the device (csrc/csr_export.h), bit for bit the reference's
`_solutionToChromNarrowPeakRows` (peaks.py:5202-5567) without a width policy and without a hierarchy -- the first pass `solveRocco`
always makes -- with `_solveParentConditionedSubpeakSegments` (4507-4576) and `_trimChildSegmentAroundSummit` (4789-4824).

What runs where.  The DEVICE does everything per bin, for all parents of all chains in one call: per parent the required bin, the
min-run dynamic programme with a uniform boundary cost, its backtrace, the penalized objective and the boundary penalty; per child
the summit, the trim, np.median and np.max of the signal, np.max of the scores, np.median of the finite uncertainty values and the
median filter's flag.  The HOST works from compact records and the caller's coordinates only: it cuts the mask's runs at
coordinate gaps, and makes chromStart / chromEnd / summit / peak offset, the 200 bp filter, names, counters, the scaled score and
the row lists and meta dicts with the reference's keys, types and order.

One kind of chain is decided on the host: a non-finite signal value inside a selected run makes NumPy's maxima and medians
propagate NaN, which no order statistic reproduces.  The children of such a chain still come from the device (they depend on the
scores alone); its signal-dependent numbers are redone with NumPy on the chain's tracks.  STATS counts those chains.

Not offered: `_forceMassiveSubpeakSegments` / a width policy, a nested hierarchy, the blacklist and minPeakScore filters, broad
mode, writing a file."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib as L
from ._lib import _vp

MIN_PEAK_BP = 200
MULTIPLIER = 2.0
MAX_MIN_RUN = 255
STATS = {"calls": 0, "chains": 0, "parents": 0, "peaks": 0, "decided_on_host": 0}

CFG = np.dtype([("selection_penalty", "<f8"), ("boundary_cost", "<f8"), ("trim_floor", "<f8"), ("multiplier", "<f8"),
                ("min_run", "<i4"), ("split", "<i4"), ("trim", "<i4"), ("filter", "<i4")])
PARENT = np.dtype([("start", "<i8"), ("end", "<i8"), ("chain", "<i4"), ("reserved", "<i4")])
PEAK = np.dtype([("start", "<i8"), ("end", "<i8"), ("untrimmed_start", "<i8"), ("untrimmed_end", "<i8"), ("summit", "<i8"),
                 ("chain", "<i4"), ("parent", "<i4"), ("num_subpeaks", "<i4"), ("flags", "<i4"), ("median_state", "<f8"),
                 ("local_median_p", "<f8"), ("max_state", "<f8"), ("max_score", "<f8"), ("subpeak_objective", "<f8"),
                 ("subpeak_boundary_penalty", "<f8")])


def validate_multiplier(value):
    value = float(value)
    if not math.isfinite(value) or value < 0.0:
        raise ValueError("`exportFilterUncertaintyMultiplier` must be finite and non-negative")
    return value


def chain_cfg(selection_penalty, boundary_cost, trim_score_floor, multiplier, min_subpeak_bins, split, use_filter):
    """One csr_export_cfg row.  A trim floor of None or a non-finite one switches the trim off, as the reference does."""
    floor = None if trim_score_floor is None else float(trim_score_floor)
    trim = floor is not None and math.isfinite(floor)
    # (minSubpeakBins is an int of any size in the reference; beyond the device's limit it is refused there whatever the excess)
    min_run = int(min(max(int(min_subpeak_bins), 1), 1 << 30))
    return (float(selection_penalty), float(boundary_cost), floor if trim else 0.0, float(multiplier), min_run, int(bool(split)),
            int(trim), int(bool(use_filter)))


def cut_parents(starts, ends_idx, intervals, ends):
    """The mask's runs (inclusive bin indices) cut where ends[i] != intervals[i + 1]: (parent starts, parent ends, the number of
    cuts -- the reference's num_coordinate_gap_splits).  The gap positions come from the coordinates alone."""
    starts = np.asarray(starts, np.int64)
    ends_idx = np.asarray(ends_idx, np.int64)
    if starts.size == 0 or intervals.size < 2:
        return starts, ends_idx, 0
    gaps = np.flatnonzero(ends[:-1] != intervals[1:])       # a cut between bin g and bin g + 1
    if gaps.size == 0:
        return starts, ends_idx, 0
    lo = np.searchsorted(gaps, starts, "left")
    hi = np.searchsorted(gaps, ends_idx, "left")            # gaps g with start <= g < end
    if not np.any(hi > lo):
        return starts, ends_idx, 0
    ps, pe = [], []
    for a, b, i, j in zip(starts.tolist(), ends_idx.tolist(), lo.tolist(), hi.tolist()):
        cur = a
        for g in gaps[i:j].tolist():
            ps.append(cur)
            pe.append(g)
            cur = g + 1
        ps.append(cur)
        pe.append(b)
    return np.asarray(ps, np.int64), np.asarray(pe, np.int64), int(np.sum(hi - lo))


def redo_on_host(peaks, state, scores, uncertainty, cfg_row):
    """The signal-dependent numbers of one chain's children with the reference's NumPy steps (a chain with a non-finite signal
    value inside a selected run).  `peaks` is a writable view of that chain's records."""
    floor, mult = float(cfg_row["trim_floor"]), float(cfg_row["multiplier"])
    for p in peaks:
        a, b = int(p["untrimmed_start"]), int(p["untrimmed_end"])
        summit = a + int(np.argmax(state[a:b + 1]))
        s, e = a, b
        if cfg_row["trim"] and bool(scores[summit] > floor):
            keep = scores[a:b + 1] > floor
            s = e = summit
            while s > a and keep[s - 1 - a]:
                s -= 1
            while e < b and keep[e + 1 - a]:
                e += 1
        flags = int(p["flags"]) & L.EXPORT_SPLIT_FROM_PARENT
        if s != a or e != b:
            flags |= L.EXPORT_TRIMMED
        with np.errstate(invalid="ignore"):
            p["median_state"] = float(np.median(state[s:e + 1]))
            p["max_state"] = float(np.max(state[s:e + 1]))
        p["max_score"] = float(np.max(scores[s:e + 1]))
        p["local_median_p"] = 0.0
        if cfg_row["filter"] and uncertainty is not None:
            local = uncertainty[s:e + 1]
            local = local[np.isfinite(local)]
            if local.size:
                p["local_median_p"] = float(np.median(local))
                flags |= L.EXPORT_HAS_LOCAL_P
                if float(p["median_state"]) < float(-mult * float(p["local_median_p"])):
                    flags |= L.EXPORT_DROPPED_MEDIAN
        p["start"], p["end"], p["summit"], p["flags"] = s, e, summit, flags


def export_details(multiplier, filter_active):
    return {
        "num_candidate_segments": 0,
        "num_segments_dropped_median_signal_local_p": 0,
        "num_segments_dropped_min_peak_bp": 0,
        "min_peak_bp": int(MIN_PEAK_BP),
        "median_signal_local_p_multiplier": float(multiplier),
        "median_signal_local_p_filter_active": bool(filter_active),
        "massive_subpeak_cleanup_active": False,
        "massive_subpeak_width_policy": None,
        "num_massive_subpeak_candidates": 0,
        "num_massive_subpeak_splits": 0,
        "num_massive_subpeak_segments_added": 0,
        "num_massive_subpeak_evaluated": 0,
        "num_massive_subpeak_contracts": 0,
        "num_coordinate_gap_splits": 0,
    }


def assemble(chromosome, intervals, ends, prefix, peaks, multiplier, trim_score_floor, details, score_floor=250.0, score_ceil=1000.0):
    """The host half of `_solutionToChromNarrowPeakRows`: one chain's peak records, in the reference's order, to (rows, meta);
    counts into `details`."""
    raw, meta = [], []
    name_chrom = str(chromosome)
    for p in peaks:
        flags = int(p["flags"])
        details["num_candidate_segments"] += 1
        local_p = threshold = None
        if flags & L.EXPORT_HAS_LOCAL_P:
            local_p = float(p["local_median_p"])
            threshold = float(-multiplier * local_p)
            if flags & L.EXPORT_DROPPED_MEDIAN:
                details["num_segments_dropped_median_signal_local_p"] += 1
                continue
        s, e, summit = int(p["start"]), int(p["end"]), int(p["summit"])
        us, ue = int(p["untrimmed_start"]), int(p["untrimmed_end"])
        summit_abs = int(intervals[summit] + max(1, int((ends[summit] - intervals[summit]) // 2)))
        chrom_start, chrom_end = int(intervals[s]), int(ends[e])
        if chrom_end - chrom_start < MIN_PEAK_BP:
            details["num_segments_dropped_min_peak_bp"] += 1
            continue
        name = f"{prefix}_{chromosome}_{len(raw) + 1}"
        raw.append((chrom_start, chrom_end, str(name), float(p["max_score"]), float(p["max_state"]), int(max(0, summit_abs - chrom_start))))
        meta.append({
            "name": str(name),
            "chromosome": name_chrom,
            "start": chrom_start,
            "end": chrom_end,
            "summit": summit_abs,
            "start_idx": s,
            "end_idx": e,
            "summit_idx": summit,
            "untrimmed_start_idx": us,
            "untrimmed_end_idx": ue,
            "segment_length_bins": int(ue - us + 1),
            "median_state": float(p["median_state"]),
            "local_median_p": local_p,
            "median_signal_threshold": threshold,
            "max_state": float(p["max_state"]),
            "max_score": float(p["max_score"]),
            "num_subpeaks": int(p["num_subpeaks"]),
            "split_from_parent": bool(flags & L.EXPORT_SPLIT_FROM_PARENT),
            "subpeak_objective": float(p["subpeak_objective"]),
            "subpeak_boundary_penalty": float(p["subpeak_boundary_penalty"]),
            "massive_subpeak_cleanup_candidate": False,
            "massive_subpeak_cleanup_applied": False,
            "massive_subpeak_cleanup_mode": None,
            "massive_subpeak_width_p": None,
            "massive_subpeak_width_q": None,
            "massive_subpeak_width_threshold_bp": None,
            "massive_subpeak_split_gain": None,
            "massive_subpeak_split_z": None,
            "massive_subpeak_gap_bins": None,
            "massive_subpeak_core_width_bp": None,
            "massive_subpeak_core_score_floor": None,
            "trimmed_from_parent": bool(flags & L.EXPORT_TRIMMED),
            "trim_score_floor": None if trim_score_floor is None else float(trim_score_floor),
            "untrimmed_start": int(intervals[us]),
            "untrimmed_end": int(ends[ue]),
        })
    details["num_segments_kept"] = len(raw)
    if not raw:
        return [], []
    scores = np.asarray([r[3] for r in raw], dtype=np.float64)
    lo, hi = float(np.min(scores)), float(np.max(scores))
    span = max(hi - lo, 1.0e-12)
    rows = []
    for chrom_start, chrom_end, name, raw_score, signal, offset in raw:
        scaled = score_floor + (score_ceil - score_floor) * ((raw_score - lo) / span)
        rows.append([name_chrom, chrom_start, chrom_end, name, int(round(scaled)), ".", signal, -1, -1, offset])
    return rows, meta


# ---------------------------------------------------------------------------------------------------------------
# the pieces of the reference on their own
# ---------------------------------------------------------------------------------------------------------------
def _device_peaks(state, scores, uncertainty, cfg_row, parents):
    """csr_export_peaks of one chain on host arrays: (peak records, per-parent flags)"""
    cfg = np.asarray([cfg_row], CFG)
    par = np.zeros(len(parents), PARENT)
    for k, (a, b) in enumerate(parents):
        par[k] = (a, b, 0, 0)
    flags = np.zeros(par.size, np.int32)
    count = C.c_int64(0)
    lens = np.asarray([int(scores.size)], np.int64)
    lib = L.lib()
    L.check_value(lib.csr_export_peaks(1, lens.ctypes.data_as(L.I64P), L.dp(state), L.dp(scores), L.dp(uncertainty), _vp(cfg), par.size,
                                       _vp(par), _vp(flags), C.byref(count)))
    peaks = np.zeros(int(count.value), PEAK)
    L.check(lib.csr_export_fetch(None, peaks.size, _vp(peaks)))
    return peaks, flags


def _one_chain(state, scores, uncertainty, cfg_row, parents):
    """The peak records of one chain on host arrays, the host decision included."""
    peaks, flags = _device_peaks(state, scores, uncertainty, cfg_row, parents)
    host = int(bool(np.any(flags & L.EXPORT_NONFINITE_SIGNAL)))
    if host:
        redo_on_host(peaks, state, scores, uncertainty, np.asarray([cfg_row], CFG)[0])
    STATS["calls"] += 1
    STATS["chains"] += 1
    STATS["parents"] += len(parents)
    STATS["peaks"] += int(peaks.size)
    STATS["decided_on_host"] += host
    return peaks


def solve_parent_conditioned_subpeak_segments(segmentScores, segmentState, startIdx, endIdx, selectionPenalty, boundaryCost, minRunBins):
    """Drop-in for `_solveParentConditionedSubpeakSegments`: the list of child dicts of one parent."""
    s = np.ascontiguousarray(np.asarray(segmentScores, dtype=np.float64))
    x = np.ascontiguousarray(np.asarray(segmentState, dtype=np.float64))
    if s.size != x.size:
        raise ValueError("`segmentScores` and `segmentState` must match")
    if s.ndim != 1 or s.size == 0:
        raise ValueError("`scores` must be a non-empty one-dimensional array")
    if not np.all(np.isfinite(s)):
        raise ValueError("`scores` contains non-finite values")
    cost = float(max(float(boundaryCost), 0.0))
    if not math.isfinite(cost):
        raise ValueError("`boundaryCosts` must be finite and non-negative")
    if not math.isfinite(float(selectionPenalty)):
        raise ValueError("`selectionPenalty` must be finite")
    row = chain_cfg(selectionPenalty, cost, None, 0.0, minRunBins, True, False)
    peaks = _one_chain(x, s, None, row, [(0, int(s.size) - 1)])
    start, end = int(startIdx), int(endIdx)
    return [{
        "start_idx": int(start + int(p["untrimmed_start"])),
        "end_idx": int(start + int(p["untrimmed_end"])),
        "summit_idx": int(start + int(p["summit"])),
        "segment_length_bins": int(p["untrimmed_end"] - p["untrimmed_start"] + 1),
        "num_subpeaks": int(p["num_subpeaks"]),
        "split_from_parent": bool(int(p["flags"]) & L.EXPORT_SPLIT_FROM_PARENT),
        "subpeak_objective": float(p["subpeak_objective"]),
        "subpeak_boundary_penalty": float(p["subpeak_boundary_penalty"]),
        "massive_subpeak_cleanup_candidate": False,
        "massive_subpeak_cleanup_applied": False,
        "massive_subpeak_split_gain": None,
        "massive_subpeak_split_z": None,
        "massive_subpeak_gap_bins": None,
        "massive_subpeak_parent_start_idx": start,
        "massive_subpeak_parent_end_idx": end,
    } for p in peaks]


def trim_child_segment_around_summit(childStartIdx, childEndIdx, summitIdx, scores, trimScoreFloor):
    """Drop-in for `_trimChildSegmentAroundSummit`: (start, end, trimmed).  The device trims around a child's own summit (the arg-max
    of its signal); a summit given from outside is served by a signal that peaks there."""
    start, end = int(childStartIdx), int(childEndIdx)
    if trimScoreFloor is None or not math.isfinite(float(trimScoreFloor)):
        return start, end, False
    sc = np.ascontiguousarray(np.asarray(scores[start:end + 1], dtype=np.float64))
    if sc.size == 0:
        return start, end, False
    summit = int(np.clip(int(summitIdx), start, end)) - start
    signal = np.zeros(sc.size, np.float64)
    signal[summit] = 1.0
    row = chain_cfg(0.0, 0.0, float(trimScoreFloor), 0.0, 1, False, False)
    p = _one_chain(signal, sc, None, row, [(0, int(sc.size) - 1)])[0]
    return int(start + int(p["start"])), int(start + int(p["end"])), bool(int(p["flags"]) & L.EXPORT_TRIMMED)


def solution_to_chrom_narrowpeak_rows(chromosome, intervals, ends, state, scores, solution, prefix, nullScale, uncertainty=None,
                                      splitSubpeaks=True, trimScoreFloor=0.0, subpeakSelectionPenalty=None, subpeakBoundaryCost=None,
                                      minSubpeakBins=1, massiveSubpeakCleanup=False, massiveSubpeakWidthPolicy=None,
                                      massiveSubpeakSplitQuantile=0.25, massiveSubpeakSplitZ=2.0,
                                      dropMedianSignalBelowNegativeLocalP=True, exportFilterUncertaintyMultiplier=MULTIPLIER,
                                      scoreFloor=250.0, scoreCeil=1000.0, nestedHierarchy=None, nestedDetails=None,
                                      returnExportDetails=False):
    """Drop-in for `_solutionToChromNarrowPeakRows` with `massiveSubpeakWidthPolicy=None` and without a hierarchy: (rows, meta) or
    (rows, meta, exportDetails)."""
    if massiveSubpeakWidthPolicy is not None:
        raise ValueError("`massiveSubpeakWidthPolicy` is not supported: the massive sub-peak clean-up is not built")
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
    mult = validate_multiplier(exportFilterUncertaintyMultiplier)
    use_filter = bool(dropMedianSignalBelowNegativeLocalP and u is not None)
    details = export_details(mult, use_filter)
    from .nested import run_bounds

    starts, stops = run_bounds(sol)
    ps, pe, cuts = cut_parents(starts, stops, intervals, ends)
    details["num_coordinate_gap_splits"] = cuts
    rows, meta = [], []
    if ps.size:
        fallback = float(max(float(nullScale), 0.0))
        penalty = fallback if subpeakSelectionPenalty is None else float(subpeakSelectionPenalty)
        cost = fallback if subpeakBoundaryCost is None else float(subpeakBoundaryCost)
        if splitSubpeaks:
            # the first parent's checks, in the reference's order
            if not np.all(np.isfinite(s[ps[0]:pe[0] + 1])):
                raise ValueError("`scores` contains non-finite values")
            if not math.isfinite(float(max(cost, 0.0))):
                raise ValueError("`boundaryCosts` must be finite and non-negative")
            if not math.isfinite(penalty):
                raise ValueError("`selectionPenalty` must be finite")
        row = chain_cfg(penalty, cost, trimScoreFloor, mult, minSubpeakBins, splitSubpeaks, use_filter)
        peaks = _one_chain(x, s, u, row, list(zip(ps.tolist(), pe.tolist())))
        rows, meta = assemble(chromosome, intervals, ends, prefix, peaks, mult, trimScoreFloor, details, scoreFloor, scoreCeil)
    if not rows:
        if returnExportDetails:
            details["num_segments_kept"] = 0
            return [], [], details
        return [], []
    if returnExportDetails:
        return rows, meta, details
    return rows, meta
