"""Pure-Python twin of broad mode's bridging and rows, in two forms.

  form="steps"   the reference's steps one after the other with NumPy: the walk over the runs with one np.sum per open gap, per
                 parent np.median / np.argmax / np.mean / np.max, the blocks by a loop over all children.  It is what the batch
                 tests feed with downloaded tracks.
  form="device"  the decomposition the library makes: every gap decided on its own from a sum in NumPy's order written out
                 (chunks, the pairwise tree, the eight accumulators: twin_peakscore.numpy_sum_device), the merged runs from the
                 decisions; per parent a sort for the medians, a scan for the leftmost arg-max, the written-out sum over the
                 count for the means, a stable compaction of the finite uncertainty values, the non-finite flag and the host
                 decision; children assigned to parents by bisection.  BRANCHES counts what the case table must take.

tests/test_broad_twin.py holds both forms equal to the fixtures made from the reference's own functions."""
import bisect
import math

import numpy as np

from twin_peakscore import numpy_sum_device

BRANCHES = {}


def reset_branches():
    BRANCHES.clear()


def took(name, k=1):
    BRANCHES[name] = BRANCHES.get(name, 0) + k


def coordinate_runs(mask, intervals, ends):
    """`_selectedCoordinateRunBounds`: the runs of the mask, cut where ends[i] != intervals[i + 1]"""
    m = np.asarray(mask, dtype=bool)
    iv, en = np.asarray(intervals, np.int64).ravel(), np.asarray(ends, np.int64).ravel()
    if iv.size != m.size or en.size != m.size:
        raise ValueError("`intervals`, `ends`, and `mask` must match length")
    runs, start, n = [], None, int(m.size)
    m, iv, en = m.tolist(), iv.tolist(), en.tolist()
    for i in range(n):
        if not m[i]:
            continue
        if start is None:
            start = i
        if i + 1 == n or not m[i + 1] or en[i] != iv[i + 1]:
            runs.append((start, i))
            start = None
    return runs


def _overlaps(blacklist, chrom, a, b):
    bl = blacklist.get(str(chrom))
    if bl is None or bl.size == 0 or b <= a:
        return False
    k = int(np.searchsorted(bl[:, 0], b, side="left"))
    return k > 0 and int(bl[k - 1, 1]) > a


def _details(fraction, counts, max_gap, run_penalty, penalty=None, cost=None):
    d = {"policy": "soft_dip_objective_delta" if fraction < 1.0 else "objective_delta", "num_input_runs": int(counts[0]),
         "num_output_runs": int(counts[1]), "num_gaps_evaluated": int(counts[2]), "num_gaps_merged": int(counts[3]),
         "num_gaps_blocked_by_blacklist": int(counts[4]), "num_gaps_blocked_by_distance": int(counts[5])}
    if penalty is not None:
        d.update({"selection_penalty": float(penalty), "boundary_cost": float(cost)})
        d.update({"run_penalty": float(run_penalty), "max_gap_bp": int(max_gap), "dip_penalty_fraction": float(fraction)})
    else:
        d.update({"max_gap_bp": int(max_gap), "run_penalty": float(run_penalty), "dip_penalty_fraction": float(fraction)})
    return d


def merge(runs, scores, intervals, ends, chromosome, selectionPenalty, boundaryCost, maxGapBP, blacklistByChrom, runPenalty=0.0,
          dipPenaltyFraction=1.0, form="steps", gap_sums=None):
    """`_mergeBroadRunsByObjective`: (merged runs, details).  gap_sums (device form): the sums a caller made of every gap in
    front of the tests, as the resident form does; a gap that reaches the gain decision reads its own"""
    f = float(np.clip(float(dipPenaltyFraction), 0.0, 1.0))
    if not runs:
        took("no_runs")
        return [], _details(f, (0,) * 6, int(maxGapBP), float(max(float(runPenalty), 0.0)))
    s = np.asarray(scores, np.float64).ravel()
    iv, en = np.asarray(intervals, np.int64).ravel(), np.asarray(ends, np.int64).ravel()
    if s.size != iv.size or s.size != en.size:
        raise ValueError("`scores`, `intervals`, and `ends` must match length")
    pen, cost, rp = (float(max(float(v), 0.0)) for v in (selectionPenalty, boundaryCost, runPenalty))
    max_gap = int(max(int(maxGapBP), 0))
    runs = [(int(a), int(b)) for a, b in runs]

    def gap_score(a, b):        # the bins a .. b - 1
        if b <= a:
            took("gap_without_bin")
            return 0.0
        ex = np.asarray(s[a:b] - pen, dtype=np.float64)
        w = np.where(ex < 0.0, f * ex, ex)
        if form == "steps":
            return float(np.sum(w))
        took(f"gap_len_{b - a}")
        return float(numpy_sum_device(w))

    # 0: merged, 1: distance, 2: blacklist, 3: no gain -- of every gap on its own
    verdict = []
    for k, ((_, pe), (ns, _)) in enumerate(zip(runs[:-1], runs[1:])):
        a_bp, b_bp = int(en[pe]), int(iv[ns])
        if max(b_bp - a_bp, 0) > max_gap:
            took("both_fail" if _overlaps(blacklistByChrom, chromosome, a_bp, b_bp) else "distance")
            verdict.append(1)
        elif _overlaps(blacklistByChrom, chromosome, a_bp, b_bp):
            verdict.append(2)
        else:
            with np.errstate(invalid="ignore"):
                gain = float((gap_score(pe + 1, ns) if gap_sums is None else gap_sums[k]) + 2.0 * cost + rp)
            took("gain_zero", int(gain == 0.0))
            took("gap_at_max", int(max(b_bp - a_bp, 0) == max_gap))
            verdict.append(0 if gain > 0.0 else 3)
    if form == "steps":         # the reference's walk
        merged, (cs, ce) = [], runs[0]
        for v, (ns, ne) in zip(verdict, runs[1:]):
            if v == 0:
                ce = ne
                continue
            merged.append((cs, ce))
            cs, ce = ns, ne
        merged.append((cs, ce))
    else:                       # a group keeps its first start and its last end
        heads = [0] + [k + 1 for k, v in enumerate(verdict) if v != 0]
        tails = [k for k, v in enumerate(verdict) if v != 0] + [len(runs) - 1]
        merged = [(runs[h][0], runs[t][1]) for h, t in zip(heads, tails)]
    counts = (len(runs), len(merged), len(verdict), verdict.count(0), verdict.count(2), verdict.count(1))
    return merged, _details(f, counts, max_gap, rp, pen, cost)


def blocks(parentStartIdx, parentEndIdx, childRuns, intervals, ends):
    """`_blocksForBroadParent`"""
    ps, pe = int(parentStartIdx), int(parentEndIdx)
    lo_bp, hi_bp = int(intervals[ps]), int(ends[pe])
    out = []
    for a, b in childRuns:
        if int(b) < ps or int(a) > pe:
            continue
        lo, hi = max(int(intervals[max(int(a), ps)]), lo_bp), min(int(ends[min(int(b), pe)]), hi_bp)
        if hi > lo:
            out.append((lo, hi))
    out = sorted(out) or [(lo_bp, hi_bp)]
    fused = []
    for lo, hi in out:
        if fused and lo <= fused[-1][1]:
            fused[-1] = (fused[-1][0], max(fused[-1][1], hi))
        else:
            fused.append((lo, hi))
    if fused[0][0] > lo_bp:
        took("sentinel_left")
        fused.insert(0, (lo_bp, lo_bp + 1))
    if fused[-1][1] < hi_bp:
        took("sentinel_right")
        fused.append((hi_bp - 1, hi_bp))
    return fused


def _median_sorted(w):
    m = len(w)
    return w[m // 2] if m & 1 else (w[m // 2 - 1] + w[m // 2]) / 2.0


def _parent_numbers(x, s, u, mult, form):
    """(median, local median or None, dropped, summit, mean state, max state, mean score, max score, decided on host)"""
    host = False
    if form == "device":
        took(f"parent_len_{x.size}")
        host = not (np.all(np.isfinite(x)) and np.all(np.isfinite(s)))
    if form == "steps" or host:
        with np.errstate(invalid="ignore"):
            med, summit = float(np.median(x)), int(np.argmax(x))
            nums = (float(np.mean(x)), float(np.max(x)), float(np.mean(s)), float(np.max(s)))
        local = None
        if u is not None:
            fin = u[np.isfinite(u)]
            if fin.size:
                local = float(np.median(fin))
    else:
        xs = [float(v) for v in x]
        med = float(_median_sorted(sorted(xs)))
        summit, best = 0, xs[0]
        for i, v in enumerate(xs):
            if v > best:
                summit, best = i, v
        took("argmax_tie", int(xs.count(best) > 1))
        nums = (float(numpy_sum_device(x) / float(x.size)), best, float(numpy_sum_device(s) / float(s.size)),
                float(max(float(v) for v in s)))
        local = None
        if u is not None:
            fin = [float(v) for v in u if math.isfinite(float(v))]
            took("uncertainty_some_nonfinite", int(0 < len(fin) < u.size))
            took("uncertainty_none_finite", int(not fin))
            if fin:
                local = float(_median_sorted(sorted(fin)))
    dropped = local is not None and med < float(-mult * local)
    if local is not None:
        took("median_equal_threshold", int(med == float(-mult * local)))
    return med, local, dropped, summit, nums, host


def rows(chromosome, intervals, ends, state, scores, parentSolution, childSolution, prefix, uncertainty=None,
         exportFilterUncertaintyMultiplier=2.0, minPeakBP=1000, scoreFloor=250.0, scoreCeil=1000.0, returnExportDetails=False,
         form="steps"):
    """`_solutionToChromBroadPeakRows`"""
    iv, en = np.asarray(intervals, np.int64).ravel(), np.asarray(ends, np.int64).ravel()
    x, s = np.asarray(state, np.float64).ravel(), np.asarray(scores, np.float64).ravel()
    pm, cm = np.asarray(parentSolution, np.uint8).ravel(), np.asarray(childSolution, np.uint8).ravel()
    if not (iv.size == en.size == s.size == pm.size == cm.size == x.size):
        raise ValueError("`intervals`, `ends`, `state`, `scores`, and solutions must match length")
    u = None
    if uncertainty is not None:
        u = np.asarray(uncertainty, np.float64).ravel()
        if u.size != x.size:
            raise ValueError("`uncertainty` must match `state` length")
    mult = float(exportFilterUncertaintyMultiplier)
    if not math.isfinite(mult) or mult < 0.0:
        raise ValueError("`exportFilterUncertaintyMultiplier` must be finite and non-negative")
    min_bp = int(max(int(minPeakBP), 1))
    d = {"num_candidate_segments": 0, "num_segments_dropped_median_signal_local_p": 0, "num_segments_dropped_min_peak_bp": 0,
         "min_peak_bp": min_bp, "median_signal_local_p_multiplier": mult, "median_signal_local_p_filter_active": u is not None,
         "num_broad_parent_segments": 0, "num_gapped_peak_blocks": 0}
    parents, kids = coordinate_runs(pm, iv, en), coordinate_runs(cm, iv, en)
    kid_starts, kid_ends = [k[0] for k in kids], [k[1] for k in kids]
    raw, meta, hosts = [], [], 0
    for a, b in parents:
        d["num_candidate_segments"] += 1
        med, local, dropped, summit, nums, host = _parent_numbers(x[a:b + 1], s[a:b + 1], None if u is None else u[a:b + 1], mult, form)
        hosts += int(host)
        if dropped:
            took("dropped_median")
            d["num_segments_dropped_median_signal_local_p"] += 1
            continue
        lo, hi = int(iv[a]), int(en[b])
        if hi - lo < min_bp:
            took("dropped_width")
            d["num_segments_dropped_min_peak_bp"] += 1
            continue
        k = a + summit
        mine = kids if form == "steps" else kids[bisect.bisect_left(kid_ends, a):bisect.bisect_right(kid_starts, b)]
        took("no_child", int(not any(q[1] >= a and q[0] <= b for q in mine)))
        bl = blocks(a, b, mine, iv, en)
        sizes, starts = [int(q[1] - q[0]) for q in bl], [int(q[0] - lo) for q in bl]
        if starts[0] != 0:
            raise RuntimeError("gappedPeak first block must start at parent start")
        if starts[-1] + sizes[-1] != hi - lo:
            raise RuntimeError("gappedPeak final block must end at parent end")
        name = f"{prefix}_{chromosome}_{len(raw) + 1}"
        raw.append((lo, hi, name, nums[0], nums[2], sizes, starts))
        meta.append({"name": name, "chromosome": str(chromosome), "start": lo, "end": hi,
                     "summit": int(iv[k] + max(1, int((en[k] - iv[k]) // 2))), "start_idx": int(a), "end_idx": int(b), "summit_idx": int(k),
                     "median_state": med, "mean_state": nums[0], "max_state": nums[1], "mean_score": nums[2], "max_score": nums[3],
                     "local_median_p": local, "median_signal_threshold": None if local is None else float(-mult * local),
                     "block_count": len(bl), "block_sizes": list(sizes), "block_starts": list(starts)})
    took("decided_on_host", int(hosts > 0))
    d["num_segments_kept"] = len(raw)
    if not raw:
        return ([], [], [], d) if returnExportDetails else ([], [], [])
    rs = np.asarray([r[4] for r in raw], np.float64)
    lo_s, hi_s = float(np.min(rs)), float(np.max(rs))
    span = max(hi_s - lo_s, 1.0e-12)
    took("span_floor", int(hi_s - lo_s < 1.0e-12))
    broad, gapped = [], []
    for lo, hi, name, signal, score, sizes, starts in raw:
        scaled = scoreFloor + (scoreCeil - scoreFloor) * ((score - lo_s) / span)
        took("half_way", int(abs(scaled - math.floor(scaled) - 0.5) == 0.0))
        q = int(round(scaled))
        broad.append([str(chromosome), lo, hi, name, q, ".", signal, -1, -1])
        gapped.append([str(chromosome), lo, hi, name, q, ".", 0, 0, 0, len(sizes), ",".join(map(str, sizes)), ",".join(map(str, starts)),
                       signal, -1, -1])
    d["num_broad_parent_segments"] = len(broad)
    d["num_gapped_peak_blocks"] = int(sum(r[9] for r in gapped))
    return (broad, gapped, meta, d) if returnExportDetails else (broad, gapped, meta)


def _device_kept_runs(s, env, threshold, breaks, n, envelope):
    """What the run kernels make of one chain: per bin a start and an end flag, their exclusive scan as the place of a run's
    bounds, per run the touch flag, the touching runs compacted in order.  Returns (support runs, kept runs)"""
    def pred(i):
        return bool(env[i]) if envelope else bool(s[i] >= threshold)

    def is_break(g):
        k = bisect.bisect_left(breaks, g)
        took("break_bisected", int(len(breaks) > 2))
        return k < len(breaks) and breaks[k] == g

    starts, ends = [], []
    for i in range(n):
        if not pred(i):
            continue
        if i == 0 or not pred(i - 1) or is_break(i - 1):
            starts.append(i)
            took("break_on_block_edge", int(i > 0 and i % 1024 == 0 and pred(i - 1)))
            took("fallback_run_cut_at_break", int(envelope and i > 0 and pred(i - 1)))
        if i == n - 1 or not pred(i + 1) or is_break(i):
            ends.append(i)
    runs = list(zip(starts, ends))
    touch = [True if envelope else bool(np.any(env[a:b + 1])) for a, b in runs]
    for k, ((a, b), t) in enumerate(zip(runs, touch)):
        cut_left = a > 0 and pred(a - 1)
        cut_right = b < n - 1 and pred(b + 1)
        took("piece_touching" if t else "piece_not_touching", int(cut_left or cut_right))
        took("support_not_touching", int(not t and not cut_left and not cut_right))
        took("run_from_bin_0", int(t and a == 0))
        took("run_to_last_bin", int(t and b == n - 1))
        took("run_across_block_edge", int(t and a // 1024 != b // 1024))
    # the second level of the launches and scans (tests/second_level_cases.py): a second workgroup of the passes over the runs, of the
    # gap sums (64 kept runs each), a second round of the scan of the bins' block sums, a break list longer than a block of runs
    kept = sum(touch)
    took("support_runs_over_block", int(len(runs) > 1024))
    took("kept_runs_over_wave", int(kept > 64))
    took("kept_runs_over_block", int(kept > 1024))
    took("bins_over_carry_round", int(n > 1024 * 1024))
    took("breaks_over_block", int(len(breaks) > 1024))
    return runs, [r for r, t in zip(runs, touch) if t]


def parents(scores, strong, weak, threshold, intervals, ends, chromosome, selection_penalty, boundary_cost, max_gap_bp, blacklist=None,
            dip_penalty_fraction=0.5, run_penalty=0.0, form="steps"):
    """peaks.py:6884-6932: the envelope, the support runs that touch it (or the envelope's own runs), the bridging, the parent
    mask.  Returns a dict like DeviceBatch.broad_parents' with the mask.  form="device": the runs from per-bin flags and scans
    with the breaks as a bisected list, the gap sum behind every kept run unless the gap holds more bins than a gap within
    max_gap_bp can, every gap decided on its own from those sums."""
    s = np.asarray(scores, np.float64)
    iv, en = np.asarray(intervals, np.int64), np.asarray(ends, np.int64)
    env = (np.asarray(weak, np.uint8) > 0) | (np.asarray(strong, np.uint8) > 0)
    bl = {} if blacklist is None else blacklist
    if form == "steps":
        support = coordinate_runs(s >= float(threshold), iv, en)
        touching = [(a, b) for a, b in support if np.any(env[a:b + 1])]
        fallback = not touching
        if fallback:
            touching = coordinate_runs(env, iv, en)
        merged, details = merge(touching, s, iv, en, chromosome, selection_penalty, boundary_cost, max_gap_bp, bl, run_penalty,
                                dip_penalty_fraction)
    else:
        n = int(s.size)
        breaks = np.flatnonzero(en[:-1] != iv[1:]).tolist()
        support, touching = _device_kept_runs(s, env, float(threshold), breaks, n, False)
        fallback = not touching
        if fallback:
            took("envelope_fallback")
            _, touching = _device_kept_runs(s, env, float(threshold), breaks, n, True)
            took("empty_envelope", int(not touching))
        # the bound on a summed gap: k bins span at least k times the narrowest bin
        narrowest = int(np.min(en - iv)) if n else 0
        bound = int(max(int(max_gap_bp), 0)) // narrowest if narrowest > 0 and not np.any(iv[1:] < en[:-1]) else -1
        f = float(np.clip(float(dip_penalty_fraction), 0.0, 1.0))
        pen = float(max(float(selection_penalty), 0.0))
        sums = []
        for (_, pe), (ns, _) in zip(touching[:-1], touching[1:]):
            k = ns - pe - 1
            took("kept_gap_over_chunk", int(k > 8192))
            took("kept_gap_without_bin", int(k <= 0))
            if k <= 0 or (bound >= 0 and k > bound):
                took("gap_beyond_bound", int(k > 0))
                sums.append(0.0)
                continue
            ex = np.asarray(s[pe + 1:ns] - pen, dtype=np.float64)
            with np.errstate(invalid="ignore"):
                sums.append(float(numpy_sum_device(np.where(ex < 0.0, f * ex, ex))))
        merged, details = merge(touching, s, iv, en, chromosome, selection_penalty, boundary_cost, max_gap_bp, bl, run_penalty,
                                dip_penalty_fraction, form="device", gap_sums=sums)
    mask = np.zeros(s.size, np.uint8)
    for a, b in merged:
        mask[a:b + 1] = 1
    return {"starts": [a for a, _ in merged], "ends": [b for _, b in merged], "merge_details": details,
            "weak_support_run_count": len(support), "weak_support_touching_run_count": len(touching), "envelope_fallback": fallback,
            "mask": mask}
