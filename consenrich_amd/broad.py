"""Broad mode's bridging and broadPeak / gappedPeak rows with the per-bin arithmetic on the device (csrc/csr_broad.h), bit for bit
the reference's `_mergeBroadRunsByObjective` (peaks.py:1898-2005), `_solutionToChromBroadPeakRows` (5606-5818),
`_blocksForBroadParent` (5570-5603) and `_selectedCoordinateRunBounds` (1869-1895).

What runs where.  The DEVICE sums the scores of the gaps in NumPy's order, one lane per gap (the drop-in sends the gaps that are
left after the distance and blacklist tests; the resident form sums the gap behind every kept run that is short enough to pass
the distance test at all), and makes the numbers of every parent (one wavefront per parent): np.median, the leftmost arg-max, np.max and
np.mean of the signal, np.max and np.mean of the scores, np.median of the finite uncertainty values and the median filter's flag.
The HOST works from compact records and the caller's coordinates only: coordinate breaks, gapBP, the distance and blacklist tests
(vectorised), the gain decision, the merged runs, the counters and both forms of the details dict; child blocks (children are
assigned to parents by `searchsorted`), coordinates, summit, the minimum width, names, the scaled score, both row lists and the meta
dicts with the reference's keys, types and order.

In the reference every branch of the walk over the runs moves `activeEnd` to the next run's end, so each gap is decided on its own;
that is what lets all gaps go to the device in one call.

One kind of chain is decided on the host: a non-finite signal or score value inside a parent makes NumPy's maxima, medians and
means propagate NaN, which no order statistic reproduces.  Its parent numbers are redone with NumPy; STATS counts those chains.

The RESIDENT form (`batch_parents`, `batch_rows`: what `DeviceBatch.broad_parents` and `DeviceBatch.broadpeak_rows` run) takes
nothing per bin across the bus.  The support runs of scores >= threshold, cut at the coordinate breaks the host lists, the runs among
them that touch weak | strong (or, where none does, the runs of weak | strong) and the gap sum behind every kept run come from
`csr_batch_broad_runs` as one record per kept run; the parent records come from `csr_batch_broad_rows`, which reads the signal and
the uncertainty from the smoothed fit and fills the resident parent mask.

`driver.broad_peaks_batch` puts the weak budget and gamma (`solveRocco`'s 6743-6778) in front of the two.

Not offered: `peakMode="both"`, the blacklist filter on finished rows, the p and q columns, writing a gappedPeak file."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from ._lib import _vp
from .narrowpeak import MULTIPLIER, PARENT, cut_parents, validate_multiplier
from .nested import run_bounds

MIN_PEAK_BP = 1000
STATS = {"calls": 0, "parents": 0, "gaps": 0, "gaps_summed": 0, "decided_on_host": 0}

CFG = np.dtype([("multiplier", "<f8"), ("filter", "<i4"), ("reserved", "<i4")])
REC = np.dtype([("start", "<i8"), ("end", "<i8"), ("summit", "<i8"), ("chain", "<i4"), ("flags", "<i4"), ("median_state", "<f8"),
                ("local_median_p", "<f8"), ("max_state", "<f8"), ("max_score", "<f8"), ("mean_state", "<f8"), ("mean_score", "<f8")])
RUN_CFG = np.dtype([("threshold", "<f8"), ("selection_penalty", "<f8"), ("dip_fraction", "<f8"), ("max_gap_bins", "<i8")])
RUN_COUNTS = np.dtype([("support_runs", "<i8"), ("touching_runs", "<i8"), ("fallback", "<i4"), ("reserved", "<i4")])
RUN = np.dtype([("start", "<i8"), ("end", "<i8"), ("gap_sum", "<f8"), ("chain", "<i4"), ("reserved", "<i4")])
HAS_LOCAL_P, DROPPED_MEDIAN, NONFINITE = 1, 2, 4


# ---------------------------------------------------------------------------------------------------------------
# coordinate runs
# ---------------------------------------------------------------------------------------------------------------
def coordinate_runs(mask, intervals, ends):
    """The mask's runs cut where ends[i] != intervals[i + 1], as two int64 arrays of inclusive bin indices"""
    starts, stops = run_bounds(np.asarray(mask, dtype=bool))
    ps, pe, _ = cut_parents(starts, stops, intervals, ends)
    return ps, pe


def selected_coordinate_run_bounds(mask, intervals, ends):
    """Drop-in for `_selectedCoordinateRunBounds`: the list of (start, end) of the mask's coordinate runs."""
    mask = np.asarray(mask, dtype=bool)
    intervals = np.asarray(intervals, dtype=np.int64).ravel()
    ends = np.asarray(ends, dtype=np.int64).ravel()
    if intervals.size != mask.size or ends.size != mask.size:
        raise ValueError("`intervals`, `ends`, and `mask` must match length")
    ps, pe = coordinate_runs(mask, intervals, ends)
    return list(zip(ps.tolist(), pe.tolist()))


# ---------------------------------------------------------------------------------------------------------------
# bridging
# ---------------------------------------------------------------------------------------------------------------
def _device_gap_sums(scores, penalty, fraction, starts, lens):
    """csr_broad_gap_sums on host arrays"""
    sums = np.zeros(starts.size, np.float64)
    L.check_value(L.lib().csr_broad_gap_sums(int(scores.size), L.dp(scores), float(penalty), float(fraction), int(starts.size),
                                             L._i64p(starts), L._i64p(lens), L.dp(sums)))
    return sums


def overlaps_blacklist(blacklist, gap_start_bp, gap_end_bp):
    """`_intervalOverlapsBlacklist` of many intervals against one chromosome's (k, 2) array"""
    hit = np.zeros(gap_start_bp.size, bool)
    if blacklist is None or blacklist.size == 0 or hit.size == 0:
        return hit
    idx = np.searchsorted(blacklist[:, 0], gap_end_bp, side="left")
    last = np.asarray(blacklist[:, 1])[np.maximum(idx, 1) - 1].astype(np.int64)
    return (gap_end_bp > gap_start_bp) & (idx > 0) & (last > gap_start_bp)


def merge_details(fraction, max_gap_bp, run_penalty, counts=None, selection_penalty=None, boundary_cost=None):
    """The reference's details dict: the short form of an empty input (counts None), or the full one"""
    policy = "soft_dip_objective_delta" if fraction < 1.0 else "objective_delta"
    if counts is None:
        return {"policy": policy, "num_input_runs": 0, "num_output_runs": 0, "num_gaps_evaluated": 0, "num_gaps_merged": 0,
                "num_gaps_blocked_by_blacklist": 0, "num_gaps_blocked_by_distance": 0, "max_gap_bp": int(max_gap_bp),
                "run_penalty": float(run_penalty), "dip_penalty_fraction": float(fraction)}
    n_in, n_out, evaluated, merged, by_blacklist, by_distance = counts
    return {"policy": policy, "num_input_runs": int(n_in), "num_output_runs": int(n_out), "num_gaps_evaluated": int(evaluated),
            "num_gaps_merged": int(merged), "num_gaps_blocked_by_blacklist": int(by_blacklist),
            "num_gaps_blocked_by_distance": int(by_distance), "selection_penalty": float(selection_penalty),
            "boundary_cost": float(boundary_cost), "run_penalty": float(run_penalty), "max_gap_bp": int(max_gap_bp),
            "dip_penalty_fraction": float(fraction)}


def gap_tests(rs, re, intervals, ends, max_gap_bp, blacklist):
    """The host's tests of the gaps between consecutive runs: (blocked by distance, blocked by blacklist, first bin, bins) -- the
    distance test comes first, so a gap that fails both counts as distance"""
    gap_start_bp, gap_end_bp = ends[re[:-1]], intervals[rs[1:]]
    gap_bp = np.maximum(gap_end_bp - gap_start_bp, 0)
    far = gap_bp > max_gap_bp
    black = ~far & overlaps_blacklist(blacklist, gap_start_bp, gap_end_bp)
    lens = np.maximum(rs[1:] - re[:-1] - 1, 0)
    first = np.where(lens > 0, re[:-1] + 1, 0)
    return far, black, first.astype(np.int64), lens.astype(np.int64)


def decide_merges(sums, boundary_cost, run_penalty):
    """mergeGain > 0 with the reference's order of additions; a NaN gain does not merge"""
    return ((sums + 2.0 * boundary_cost) + run_penalty) > 0.0


def merged_runs(rs, re, merge):
    """Runs joined across the gaps that merge: a group keeps its first start and its last end"""
    head = np.concatenate(([True], ~merge))
    tail = np.concatenate((~merge, [True]))
    return rs[head], re[tail]


def merge_broad_runs_by_objective(runs, scores, intervals, ends, chromosome, selectionPenalty, boundaryCost, maxGapBP,
                                  blacklistByChrom, runPenalty=0.0, dipPenaltyFraction=1.0):
    """Drop-in for `_mergeBroadRunsByObjective`: (merged runs, details)."""
    fraction = float(np.clip(float(dipPenaltyFraction), 0.0, 1.0))
    if not runs:
        return [], merge_details(fraction, int(maxGapBP), float(max(float(runPenalty), 0.0)))
    s = np.ascontiguousarray(np.asarray(scores, dtype=np.float64).ravel())
    intervals = np.asarray(intervals, dtype=np.int64).ravel()
    ends = np.asarray(ends, dtype=np.int64).ravel()
    if s.size != intervals.size or s.size != ends.size:
        raise ValueError("`scores`, `intervals`, and `ends` must match length")
    penalty = float(max(float(selectionPenalty), 0.0))
    cost = float(max(float(boundaryCost), 0.0))
    run_penalty = float(max(float(runPenalty), 0.0))
    max_gap = int(max(int(maxGapBP), 0))
    rs = np.asarray([int(r[0]) for r in runs], np.int64)
    re = np.asarray([int(r[1]) for r in runs], np.int64)
    blacklist = blacklistByChrom.get(str(chromosome))
    far, black, first, lens = gap_tests(rs, re, intervals, ends, max_gap, None if blacklist is None else np.asarray(blacklist))
    open_ = np.flatnonzero(~far & ~black)
    sums = np.zeros(far.size, np.float64)
    if open_.size:
        sums[open_] = _device_gap_sums(s, penalty, fraction, np.ascontiguousarray(first[open_]), np.ascontiguousarray(lens[open_]))
    merge = ~far & ~black & decide_merges(sums, cost, run_penalty)
    ms, me = merged_runs(rs, re, merge)
    STATS["calls"] += 1
    STATS["gaps"] += int(far.size)
    STATS["gaps_summed"] += int(open_.size)
    counts = (rs.size, ms.size, far.size, int(np.sum(merge)), int(np.sum(black)), int(np.sum(far)))
    return list(zip(ms.tolist(), me.tolist())), merge_details(fraction, max_gap, run_penalty, counts, penalty, cost)


# ---------------------------------------------------------------------------------------------------------------
# rows
# ---------------------------------------------------------------------------------------------------------------
def blocks_for_broad_parent(parentStartIdx, parentEndIdx, childRuns, intervals, ends):
    """Drop-in for `_blocksForBroadParent` (pure host): the gappedPeak blocks of one parent, in bp."""
    ps, pe = int(parentStartIdx), int(parentEndIdx)
    start_bp, end_bp = int(intervals[ps]), int(ends[pe])
    blocks = []
    for a, b in childRuns:
        a, b = int(a), int(b)
        if b < ps or a > pe:
            continue
        lo, hi = int(max(int(intervals[max(a, ps)]), start_bp)), int(min(int(ends[min(b, pe)]), end_bp))
        if hi > lo:
            blocks.append((lo, hi))
    if not blocks:
        blocks = [(start_bp, end_bp)]
    blocks.sort()
    merged = []
    for lo, hi in blocks:
        if not merged or lo > merged[-1][1]:
            merged.append((lo, hi))
        else:
            merged[-1] = (merged[-1][0], max(merged[-1][1], hi))
    if merged[0][0] > start_bp:
        merged.insert(0, (start_bp, start_bp + 1))
    if merged[-1][1] < end_bp:
        merged.append((end_bp - 1, end_bp))
    return merged


def _device_records(state, scores, uncertainty, multiplier, ps, pe):
    """csr_broad_rows of one chain on host arrays: (parent records, parent mask)"""
    cfg = np.asarray([(float(multiplier), int(uncertainty is not None), 0)], CFG)
    par = np.zeros(ps.size, PARENT)
    par["start"], par["end"] = ps, pe
    rec = np.zeros(ps.size, REC)
    mask = np.zeros(scores.size, np.uint8)
    lens = np.asarray([int(scores.size)], np.int64)
    L.check_value(L.lib().csr_broad_rows(1, L._i64p(lens), L.dp(state), L.dp(scores), L.dp(uncertainty), _vp(cfg), par.size, _vp(par),
                                         mask.ctypes.data_as(C.POINTER(C.c_uint8)), _vp(rec)))
    return rec, mask


def redo_on_host(rec, state, scores, uncertainty, multiplier):
    """The parent numbers of one chain with the reference's NumPy steps (a chain with a non-finite signal or score value inside a
    parent).  `rec` is a writable array of that chain's records."""
    for r in rec:
        a, b = int(r["start"]), int(r["end"])
        x, s = state[a:b + 1], scores[a:b + 1]
        flags = int(r["flags"]) & NONFINITE
        with np.errstate(invalid="ignore"):
            r["median_state"] = float(np.median(x))
            r["max_state"], r["mean_state"] = float(np.max(x)), float(np.mean(x))
            r["max_score"], r["mean_score"] = float(np.max(s)), float(np.mean(s))
        r["summit"] = a + int(np.argmax(x))
        r["local_median_p"] = 0.0
        if uncertainty is not None:
            local = uncertainty[a:b + 1]
            local = local[np.isfinite(local)]
            if local.size:
                r["local_median_p"] = float(np.median(local))
                flags |= HAS_LOCAL_P
                if float(r["median_state"]) < float(-multiplier * float(r["local_median_p"])):
                    flags |= DROPPED_MEDIAN
        r["flags"] = flags


def export_details(min_peak_bp, multiplier, filter_active):
    return {
        "num_candidate_segments": 0,
        "num_segments_dropped_median_signal_local_p": 0,
        "num_segments_dropped_min_peak_bp": 0,
        "min_peak_bp": int(min_peak_bp),
        "median_signal_local_p_multiplier": float(multiplier),
        "median_signal_local_p_filter_active": bool(filter_active),
        "num_broad_parent_segments": 0,
        "num_gapped_peak_blocks": 0,
    }


def assemble(chromosome, intervals, ends, prefix, rec, cs, ce, multiplier, min_peak_bp, details, score_floor=250.0, score_ceil=1000.0):
    """The host half of `_solutionToChromBroadPeakRows`: one chain's parent records and the child mask's coordinate runs (cs, ce)
    to (broad rows, gapped rows, meta); counts into `details`."""
    raw, meta = [], []
    name_chrom = str(chromosome)
    # the children that reach into a parent: child runs ascend and are disjoint
    first = np.searchsorted(ce, rec["start"], "left").tolist()
    last = np.searchsorted(cs, rec["end"], "right").tolist()
    kids = list(zip(cs.tolist(), ce.tolist()))
    for r, k0, k1 in zip(rec, first, last):
        flags = int(r["flags"])
        details["num_candidate_segments"] += 1
        local_p = threshold = None
        if flags & HAS_LOCAL_P:
            local_p = float(r["local_median_p"])
            threshold = float(-multiplier * local_p)
            if flags & DROPPED_MEDIAN:
                details["num_segments_dropped_median_signal_local_p"] += 1
                continue
        s, e, summit = int(r["start"]), int(r["end"]), int(r["summit"])
        chrom_start, chrom_end = int(intervals[s]), int(ends[e])
        if chrom_end - chrom_start < min_peak_bp:
            details["num_segments_dropped_min_peak_bp"] += 1
            continue
        summit_abs = int(intervals[summit] + max(1, int((ends[summit] - intervals[summit]) // 2)))
        blocks = blocks_for_broad_parent(s, e, kids[k0:k1], intervals, ends)
        sizes = [int(b - a) for a, b in blocks]
        starts = [int(a - chrom_start) for a, _ in blocks]
        if starts[0] != 0:
            raise RuntimeError("gappedPeak first block must start at parent start")
        if starts[-1] + sizes[-1] != chrom_end - chrom_start:
            raise RuntimeError("gappedPeak final block must end at parent end")
        name = f"{prefix}_{chromosome}_{len(raw) + 1}"
        raw.append((chrom_start, chrom_end, str(name), float(r["mean_state"]), float(r["mean_score"]), sizes, starts))
        meta.append({
            "name": str(name),
            "chromosome": name_chrom,
            "start": chrom_start,
            "end": chrom_end,
            "summit": summit_abs,
            "start_idx": s,
            "end_idx": e,
            "summit_idx": summit,
            "median_state": float(r["median_state"]),
            "mean_state": float(r["mean_state"]),
            "max_state": float(r["max_state"]),
            "mean_score": float(r["mean_score"]),
            "max_score": float(r["max_score"]),
            "local_median_p": local_p,
            "median_signal_threshold": threshold,
            "block_count": int(len(blocks)),
            "block_sizes": list(sizes),
            "block_starts": list(starts),
        })
    details["num_segments_kept"] = len(raw)
    if not raw:
        return [], [], []
    scores = np.asarray([r[4] for r in raw], dtype=np.float64)
    lo, hi = float(np.min(scores)), float(np.max(scores))
    span = max(hi - lo, 1.0e-12)
    broad, gapped = [], []
    for chrom_start, chrom_end, name, signal, raw_score, sizes, starts in raw:
        scaled = score_floor + (score_ceil - score_floor) * ((raw_score - lo) / span)
        score = int(round(scaled))
        broad.append([name_chrom, chrom_start, chrom_end, name, score, ".", signal, -1, -1])
        gapped.append([name_chrom, chrom_start, chrom_end, name, score, ".", 0, 0, 0, int(len(sizes)),
                       ",".join(str(v) for v in sizes), ",".join(str(v) for v in starts), signal, -1, -1])
    details["num_broad_parent_segments"] = len(broad)
    details["num_gapped_peak_blocks"] = int(sum(int(row[9]) for row in gapped))
    return broad, gapped, meta


def solution_to_chrom_broadpeak_rows(chromosome, intervals, ends, state, scores, parentSolution, childSolution, prefix, uncertainty=None,
                                     exportFilterUncertaintyMultiplier=MULTIPLIER, minPeakBP=MIN_PEAK_BP, scoreFloor=250.0,
                                     scoreCeil=1000.0, returnExportDetails=False):
    """Drop-in for `_solutionToChromBroadPeakRows`: (broad rows, gapped rows, meta) or the same with the export details."""
    intervals = np.asarray(intervals, dtype=np.int64).ravel()
    ends = np.asarray(ends, dtype=np.int64).ravel()
    x = np.ascontiguousarray(np.asarray(state, dtype=np.float64).ravel())
    s = np.ascontiguousarray(np.asarray(scores, dtype=np.float64).ravel())
    parent = np.asarray(parentSolution, dtype=np.uint8).ravel()
    child = np.asarray(childSolution, dtype=np.uint8).ravel()
    if intervals.size != x.size or ends.size != x.size or s.size != x.size or parent.size != x.size or child.size != x.size:
        raise ValueError("`intervals`, `ends`, `state`, `scores`, and solutions must match length")
    u = None
    if uncertainty is not None:
        u = np.ascontiguousarray(np.asarray(uncertainty, dtype=np.float64).ravel())
        if u.size != x.size:
            raise ValueError("`uncertainty` must match `state` length")
    mult = validate_multiplier(exportFilterUncertaintyMultiplier)
    min_bp = int(max(int(minPeakBP), 1))
    details = export_details(min_bp, mult, u is not None)
    ps, pe = coordinate_runs(parent, intervals, ends)
    cs, ce = coordinate_runs(child, intervals, ends)
    broad, gapped, meta = [], [], []
    if ps.size:
        rec, _ = _device_records(x, s, u, mult, ps, pe)
        host = int(bool(np.any(rec["flags"] & NONFINITE)))
        if host:
            redo_on_host(rec, x, s, u, mult)
        STATS["calls"] += 1
        STATS["parents"] += int(ps.size)
        STATS["decided_on_host"] += host
        broad, gapped, meta = assemble(chromosome, intervals, ends, prefix, rec, cs, ce, mult, min_bp, details, scoreFloor, scoreCeil)
    if not broad:
        details["num_segments_kept"] = 0
        if returnExportDetails:
            return [], [], [], details
        return [], [], []
    if returnExportDetails:
        return broad, gapped, meta, details
    return broad, gapped, meta


# ---------------------------------------------------------------------------------------------------------------
# the resident form
# ---------------------------------------------------------------------------------------------------------------
def _per_chain(v, nc):
    if isinstance(v, (list, tuple, np.ndarray)):
        if len(v) != nc:
            raise ValueError("one value per chain")
        return list(v)
    return [v] * nc


def chain_coords(batch, take, intervals, ends, interval_bp):
    """Per taken chain its (intervals, ends) as int64 arrays: the caller's, or bins of interval_bp from 0"""
    nc = len(take)
    iv = [None] * nc if intervals is None else list(intervals)
    en = [None] * nc if ends is None else list(ends)
    if len(iv) != nc or len(en) != nc:
        raise ValueError("one intervals / ends entry per chain")
    for c in range(nc):
        if not take[c]:
            continue
        n = batch.chain_lens[c]
        if iv[c] is None or en[c] is None:
            if iv[c] is not None or en[c] is not None:
                raise ValueError("`intervals` and `ends` must be supplied together")
            if interval_bp is None:
                raise ValueError("`interval_bp` is needed where no coordinates are given")
            iv[c] = np.arange(n, dtype=np.int64) * int(interval_bp)
            en[c] = iv[c] + int(interval_bp)
        iv[c] = np.asarray(iv[c], dtype=np.int64).ravel()
        en[c] = np.asarray(en[c], dtype=np.int64).ravel()
        if iv[c].size != n or en[c].size != n:
            raise ValueError("`scores`, `intervals`, and `ends` must match length")
    return iv, en


def fuse_adjacent(rs, re):
    """Runs that touch (end + 1 == the next start) as one: what filling a mask with them and reading its runs back gives"""
    if rs.size < 2:
        return rs, re
    apart = rs[1:] != re[:-1] + 1
    return rs[np.concatenate(([True], apart))], re[np.concatenate((apart, [True]))]


def max_gap_bins(intervals, ends, max_gap_bp):
    """The most bins a gap of at most max_gap_bp can hold (-1: no bound).  Where the bins ascend without overlap a gap of k bins
    spans at least k times the narrowest bin, so a longer one fails the distance test whatever its sum."""
    if intervals.size == 0:
        return -1
    narrowest = int(np.min(ends - intervals))
    if narrowest <= 0 or (intervals.size > 1 and bool(np.any(intervals[1:] < ends[:-1]))):
        return -1
    return int(max_gap_bp) // narrowest


def _device_run_records(batch, cfg, mask, n_breaks, flat):
    """csr_batch_broad_runs and its fetch: (per-chain counts, the kept runs' records in chain order)"""
    counts = np.zeros(cfg.size, RUN_COUNTS)
    total = C.c_int64(0)
    lib = L.lib()
    L.check_value(lib.csr_batch_broad_runs(batch._ctx, _vp(cfg), mask, L._i64p(n_breaks), L._i64p(flat) if flat.size else None, _vp(counts),
                                           C.byref(total)))
    rec = np.zeros(int(total.value), RUN)
    L.check(lib.csr_batch_broad_runs_fetch(batch._ctx, rec.size, _vp(rec)))
    return counts, rec


def batch_parents(batch, thresholds, selection_penalties, boundary_costs, *, max_gap_bp, intervals=None, ends=None, interval_bp=None,
                  chroms=None, blacklist=None, dip_penalty_fraction=0.5, run_penalty=0.0, chains=None):
    import time

    t_start = time.perf_counter()
    take, mask = batch._chain_mask(chains)
    nc = len(take)
    thr, pen, cost, gap = (_per_chain(v, nc) for v in (thresholds, selection_penalties, boundary_costs, max_gap_bp))
    names = [f"chain{i}" for i in range(nc)] if chroms is None else [str(c) for c in chroms]
    if len(names) != nc:
        raise ValueError("one chroms entry per chain")
    iv, en = chain_coords(batch, take, intervals, ends, interval_bp)
    uniform = intervals is None and ends is None and int(interval_bp) > 0       # bins of interval_bp: no break, one width
    fraction = float(np.clip(float(dip_penalty_fraction), 0.0, 1.0))
    run_pen = float(max(float(run_penalty), 0.0))
    cfg = np.zeros(nc, RUN_CFG)
    breaks, n_breaks = [], np.zeros(nc, np.int64)
    for c in range(nc):
        if not take[c]:
            continue
        limit = int(max(int(gap[c]), 0))
        cfg[c] = (float(thr[c]), float(max(float(pen[c]), 0.0)), fraction,
                  limit // int(interval_bp) if uniform else max_gap_bins(iv[c], en[c], limit))
        b = np.zeros(0, np.int64) if uniform else np.flatnonzero(en[c][:-1] != iv[c][1:]).astype(np.int64)
        breaks.append(b)
        n_breaks[c] = b.size
    flat = np.ascontiguousarray(np.concatenate(breaks + [np.zeros(0, np.int64)]), np.int64)
    t_device = time.perf_counter()
    counts, rec = _device_run_records(batch, cfg, mask, n_breaks, flat)
    t_device = time.perf_counter() - t_device
    first = np.searchsorted(rec["chain"], np.arange(nc + 1), "left")       # (the records come in chain order)
    out = [None] * nc
    bl = {} if blacklist is None else blacklist
    for c in range(nc):
        if not take[c]:
            continue
        mine = rec[first[c]:first[c + 1]]
        rs, re = mine["start"].astype(np.int64), mine["end"].astype(np.int64)
        max_gap = int(max(int(gap[c]), 0))
        cost_c = float(max(float(cost[c]), 0.0))
        if rs.size == 0:
            details = merge_details(fraction, int(gap[c]), run_pen)
            ms = me = np.zeros(0, np.int64)
        else:
            b = bl.get(names[c])
            far, black, _, _ = gap_tests(rs, re, iv[c], en[c], max_gap, None if b is None else np.asarray(b))
            merge = ~far & ~black & decide_merges(mine["gap_sum"][:-1], cost_c, run_pen)
            ms, me = merged_runs(rs, re, merge)
            details = merge_details(fraction, max_gap, run_pen, (rs.size, ms.size, far.size, int(np.sum(merge)), int(np.sum(black)),
                                                                 int(np.sum(far))), float(cfg[c]["selection_penalty"]), cost_c)
        batch._broad_parents[c] = (ms, me)
        out[c] = {"starts": ms, "ends": me, "merge_details": details, "weak_support_threshold": float(thr[c]),
                  "weak_support_run_count": int(counts[c]["support_runs"]),
                  "weak_support_touching_run_count": int(counts[c]["touching_runs"]), "envelope_fallback": bool(counts[c]["fallback"]),
                  "broad_bridge_dip_penalty_fraction": fraction}
    batch.broad_stats = {"chains": int(sum(take)), "support_runs": int(counts["support_runs"].sum()), "kept_runs": int(rec.size),
                         "parents": int(sum(o["starts"].size for o in out if o is not None)), "decided_on_host": 0,
                         "device_seconds": t_device, "seconds": time.perf_counter() - t_start}
    return out


def batch_rows(batch, *, intervals=None, ends=None, interval_bp=None, chroms=None, prefix="consenrich", multiplier=MULTIPLIER,
               use_uncertainty=True, min_peak_bp=MIN_PEAK_BP, chains=None, signal="state"):
    import time

    t_start = time.perf_counter()
    take, mask = batch._chain_mask(chains)
    nc = len(take)
    names = [f"chain{i}" for i in range(nc)] if chroms is None else [str(c) for c in chroms]
    if len(names) != nc:
        raise ValueError("one chroms entry per chain")
    iv, en = chain_coords(batch, take, intervals, ends, interval_bp)
    mult = validate_multiplier(multiplier)
    min_bp = int(max(int(min_peak_bp), 1))
    cfg = np.zeros(nc, CFG)
    spans, parents, kids = [], [], {}
    for c in range(nc):
        if not take[c]:
            continue
        if c not in batch._broad_parents:
            raise L.ConsenrichAMDError(f"chain {c} has no broad parents: call broad_parents first")
        cfg[c] = (mult, int(bool(use_uncertainty)), 0)
        ps, pe, _ = cut_parents(*fuse_adjacent(*batch._broad_parents[c]), iv[c], en[c])
        cs, ce, _ = cut_parents(*batch.rocco_runs(c, 0), iv[c], en[c])
        kids[c] = (cs, ce)
        spans.append((c, len(parents), len(parents) + ps.size))
        parents += [(a, b, c, 0) for a, b in zip(ps.tolist(), pe.tolist())]
    par = np.asarray(parents, PARENT) if parents else np.zeros(0, PARENT)
    rec = np.zeros(par.size, REC)
    t_device = time.perf_counter()
    L.check_value(L.lib().csr_batch_broad_rows(batch._ctx, _vp(cfg), mask, par.size, _vp(par), _vp(rec)))
    t_device = time.perf_counter() - t_device
    out = [None] * nc
    hosts = 0
    for c, a, b in spans:
        mine = rec[a:b]
        host = bool(np.any(mine["flags"] & NONFINITE))
        if host:
            state = batch._signal_track(c, signal)
            unc = np.sqrt(batch.download(c, "Ps")[:, 0, 0]).astype(np.float64) if use_uncertainty else None
            with np.errstate(invalid="ignore"):
                redo_on_host(mine, state, batch.download_scores(c), unc, mult)
            hosts += 1
        details = export_details(min_bp, mult, bool(use_uncertainty))
        broad, gapped, meta = assemble(names[c], iv[c], en[c], prefix, mine, *kids[c], mult, min_bp, details)
        if not broad:
            details["num_segments_kept"] = 0
        out[c] = {"broad_rows": broad, "gapped_rows": gapped, "peak_meta": meta, "export_details": details, "decided_on_host": host}
    stats = dict(getattr(batch, "broad_stats", None) or {})
    stats.update({"rows_chains": len(spans), "row_parents": int(par.size), "rows": int(sum(len(o["broad_rows"]) for o in out if o)),
                  "decided_on_host": hosts, "rows_device_seconds": t_device, "rows_seconds": time.perf_counter() - t_start})
    batch.broad_stats = stats
    return out
