"""Pure-Python twin of the reference's nested ROCCO refinement (peaks.py `_solveParentConditionedSubpeaks`,
`_parentConditionedSubpeakObjective`, `_nestedSoftSelectionPenalty`, `_refineNestedROCCOSolution`), in two forms that the tests
hold equal bit for bit:

  the reference's steps restated (`form="steps"`): all `minRun + 1` states of the dynamic programme with a full back-pointer
  table, NumPy's own quantile and sum, masks compared bin by bin;

  the device's decomposition (`form="device"`, csrc/csr_nested.h): order statistics read at ranks of ONE sort per region (the
  solver scores `x - floor` are monotone in x, so their positives are a suffix of the same order), both branches of NumPy's
  `_lerp` spelled out, the middle states as a shift register, two back-pointer bits per bin packed 32 bins to a word, the
  selected scores compacted and summed over the leaves of NumPy's pairwise tree in chunks of 8192, the per-chain objective from
  the leaf runs, the Jaccard index from counts.

COUNTERS (device form) tells the fixture maker which tie-break branches a case took, how many values its quantiles were
taken of and how many strictly positive solver scores its processed regions held.  Nothing here imports the product."""
import math

import numpy as np

from twin_peakscore import numpy_sum_device

EDGE = 1.0e-12          # cost of a region's two outer boundaries
EPS = 1.0e-12           # tolerance of the value comparison
WORD = 32               # bins per back-pointer word
POLICY = "soft_selection_penalty"
MODE = "parent_conditioned_min_run_dp"
COUNTERS = dict(count_tie=0, tolerance=0, quantile_of_1=0, quantile_of_2=0, positives_0=0, positives_1=0, positives_2=0,
                positives_more=0)


def reset_counters():
    for k in COUNTERS:
        COUNTERS[k] = 0


def bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float64)).view(np.uint64)


def run_bounds(mask):
    m = np.asarray(mask, bool).astype(np.int8)
    d = np.diff(np.concatenate(([0], m, [0])))
    return list(zip(np.flatnonzero(d == 1).tolist(), (np.flatnonzero(d == -1) - 1).tolist()))


def full_costs(costs, n):
    c = np.asarray(costs, np.float64).ravel()
    if c.size == 1:
        c = np.full(n + 1, float(c[0]))
    elif c.size != n + 1:
        raise ValueError("`boundaryCosts` must be scalar or have length len(scores) + 1")
    if not np.all(np.isfinite(c)) or np.any(c < 0.0):
        raise ValueError("`boundaryCosts` must be finite and non-negative")
    return c.astype(np.float64)


def _wins(v, c, bv, bc, count=False):
    if v > bv + EPS:
        return True
    near = abs(v - bv) <= EPS
    if count and near and v != bv:
        COUNTERS["tolerance"] += 1
    if near and c < bc:
        if count and v == bv:
            COUNTERS["count_tie"] += 1
        return True
    return False


# ---------------------------------------------------------------------------------------------------------------
# the dynamic programme
# ---------------------------------------------------------------------------------------------------------------
def _dp_steps(s, costs, penalty, M, required, run_penalty):
    n, NEG, big = s.size, -math.inf, s.size + 1
    val, cnt = [NEG] * (M + 1), [big] * (M + 1)
    val[0], cnt[0] = 0.0, 0
    back = np.full((n, M + 1), -1, np.int16)
    for i in range(n):
        adj, tc = float(s[i] - penalty), float(costs[i])
        nv, nc = [NEG] * (M + 1), [big] * (M + 1)

        def offer(to, v, c, frm):
            if _wins(v, c, nv[to], nc[to]):
                nv[to], nc[to], back[i, to] = v, c, frm

        if i != required:
            if math.isfinite(val[0]):
                offer(0, val[0], cnt[0], 0)
            if math.isfinite(val[M]):
                offer(0, val[M] - tc, cnt[M], M)
        if math.isfinite(val[0]):
            offer(1, val[0] - tc - run_penalty + adj, cnt[0] + 1, 0)
        for k in range(1, M):
            if math.isfinite(val[k]):
                offer(k + 1, val[k] + adj, cnt[k] + 1, k)
        if math.isfinite(val[M]):
            offer(M, val[M] + adj, cnt[M] + 1, M)
        val, cnt = nv, nc
    last = float(val[M] - costs[n])
    state = M if (last, -cnt[M]) > (val[0], -cnt[0]) else 0
    if not math.isfinite(last if state else val[0]):
        raise RuntimeError("parent-conditioned subpeak DP found no feasible path")
    mask = np.zeros(n, bool)
    for i in range(n - 1, -1, -1):
        mask[i] = state > 0
        state = int(back[i, state])
        if state < 0:
            break
    return mask


def _dp_device(s, costs, penalty, M, required, run_penalty):
    """v[0], v[1..M] with the middle states a shift register; per bin bit 0 = state 0 came from state M, bit 1 = state M came
    from itself; every other state has one predecessor."""
    n, NEG, big = s.size, -math.inf, s.size + 1
    v, c = [NEG] * (M + 1), [big] * (M + 1)
    v[0], c[0] = 0.0, 0
    words = [0] * ((n + WORD - 1) // WORD)
    for i in range(n):
        adj, tc = float(s[i] - penalty), float(costs[i])
        p0, c0, pM, cM = v[0], c[0], v[M], c[M]
        n0v, n0c, b0 = NEG, big, 0
        if i != required:
            if math.isfinite(p0):
                n0v, n0c = p0, c0
            if math.isfinite(pM) and _wins(pM - tc, cM, n0v, n0c, True):
                n0v, n0c, b0 = pM - tc, cM, 1
        for k in range(M, 1, -1):                   # the shift, top down so that it can run in place
            v[k], c[k] = (v[k - 1] + adj, c[k - 1] + 1) if math.isfinite(v[k - 1]) else (NEG, big)
        v[1], c[1] = (p0 - tc - run_penalty + adj, c0 + 1) if math.isfinite(p0) else (NEG, big)
        b1 = 0
        if math.isfinite(pM) and _wins(pM + adj, cM + 1, v[M], c[M], True):
            v[M], c[M], b1 = pM + adj, cM + 1, 1
        v[0], c[0] = n0v, n0c
        words[i // WORD] |= (b0 | (b1 << 1)) << (2 * (i % WORD))
    last = v[M] - float(costs[n])
    state = M if (last > v[0] or (last == v[0] and c[M] < c[0])) else 0
    if not math.isfinite(last if state else v[0]):
        raise RuntimeError("parent-conditioned subpeak DP found no feasible path")
    mask = np.zeros(n, bool)
    for i in range(n - 1, -1, -1):
        mask[i] = state > 0
        w = (words[i // WORD] >> (2 * (i % WORD))) & 3
        if state == 0:
            state = M if w & 1 else 0
        elif state == M:
            state = M if w & 2 else M - 1
        else:
            state -= 1
    return mask


def objective_parts(s, mask, costs, penalty, run_penalty, form):
    """(objective, penalised objective, boundary penalty, run penalty total, runs, selected count)"""
    sel = s[mask]
    total = float(np.sum(sel)) if form == "steps" else float(numpy_sum_device(sel))
    bp, runs, prev = 0.0, 0, False
    for i, cur in enumerate(mask.tolist()):
        if cur != prev:
            bp += float(costs[i])
            runs += int(cur)
        prev = cur
    if prev:
        bp += float(costs[mask.size])
    rpt = float(run_penalty * float(runs))
    obj = float(total - bp - rpt)
    return obj, float(obj - float(penalty) * float(int(sel.size))), bp, rpt, runs, int(sel.size)


def solve(scores, boundaryCosts, selectionPenalty, minRunBins, requiredIndex=None, runPenalty=0.0, form="steps"):
    """`_solveParentConditionedSubpeaks`: (mask, objective, details)"""
    s = np.asarray(scores, np.float64)
    if s.ndim != 1 or s.size == 0:
        raise ValueError("`scores` must be a non-empty one-dimensional array")
    if not np.all(np.isfinite(s)):
        raise ValueError("`scores` contains non-finite values")
    costs = full_costs(boundaryCosts, s.size)
    penalty, rp = float(selectionPenalty), float(runPenalty)
    if not math.isfinite(penalty):
        raise ValueError("`selectionPenalty` must be finite")
    if not math.isfinite(rp) or rp < 0.0:
        raise ValueError("`runPenalty` must be finite and non-negative")
    n = int(s.size)
    req = None if requiredIndex is None else int(requiredIndex)
    if req is not None and not 0 <= req < n:
        raise ValueError("`requiredIndex` is outside `scores`")
    M = min(max(int(minRunBins), 1), n)
    mask = (_dp_steps if form == "steps" else _dp_device)(s, costs, penalty, M, -1 if req is None else req, rp)
    obj, pen, bp, rpt, runs, count = objective_parts(s, mask, costs, penalty, rp, form)
    if req is not None and not mask[req]:
        raise RuntimeError("parent-conditioned subpeak DP violated required bin constraint")
    return mask, obj, {
        "mode": MODE, "penalized_objective": pen, "selected_count": count, "selected_fraction": float(count / max(n, 1)),
        "selection_penalty": penalty, "run_penalty": rp, "run_penalty_total": rpt, "boundary_cost_min": float(np.min(costs)),
        "boundary_cost_max": float(np.max(costs)), "boundary_penalty": bp, "min_run_bins": int(M), "num_runs": int(runs),
        "required_index": req, "required_selected": bool(True if req is None else mask[req]), "required_fallback_window": False,
    }


# ---------------------------------------------------------------------------------------------------------------
# quantiles and the soft penalty
# ---------------------------------------------------------------------------------------------------------------
def quantile_sorted(sorted_vals, lo, m, q):
    """np.quantile(x, q) (method "linear", q a multiple of 1/4) of the m values sorted_vals[lo : lo + m]"""
    if m <= 2:
        COUNTERS[f"quantile_of_{m}"] += 1
    vi = m * q + (1.0 + q * -1.0) - 1.0
    if vi >= m - 1:             # (one value: NumPy's weight is then 1 and the upper branch returns the value itself)
        return float(sorted_vals[lo + m - 1])
    k = int(math.floor(vi))
    a, b = float(sorted_vals[lo + k]), float(sorted_vals[lo + k + 1])
    t = vi - math.floor(vi)
    d = b - a
    return b - d * (1.0 - t) if t >= 0.5 else a + d * t


def soft_penalty(solver, base, scale, form, floor_sorted=None):
    """`_nestedSoftSelectionPenalty` without the diagnostics-only scale: (penalty, extra)"""
    scale = float(np.clip(float(scale), 0.0, 1.0))
    base = float(max(float(base), 0.0))
    spread = 0.0
    if form == "steps":
        pos = solver[solver > 0.0]
        if pos.size > 1:
            spread = float(np.quantile(pos, 0.75) - np.quantile(pos, 0.25))
    else:
        srt, floor = floor_sorted               # the region's sorted raw values and the floor taken off them
        shifted = srt - floor
        P = int(np.count_nonzero(shifted > 0.0))
        COUNTERS[f"positives_{P}" if P <= 2 else "positives_more"] += 1
        if P > 1:
            lo = srt.size - P
            spread = float(quantile_sorted(shifted, lo, P, 0.75) - quantile_sorted(shifted, lo, P, 0.25))
    if not math.isfinite(spread) or spread < 0.0:
        spread = 0.0
    extra = float((1.0 - scale) * spread)
    return float(base + extra), extra


# ---------------------------------------------------------------------------------------------------------------
# the refinement
# ---------------------------------------------------------------------------------------------------------------
def min_child_bins(start, end, intervals, ends, min_bp, min_bins):
    region, bins = max(end - start + 1, 1), max(int(min_bins), 1)
    if min_bp is not None and intervals is not None:
        w = np.asarray(ends[start:end + 1] - intervals[start:end + 1], np.int64)
        w = w[w > 0]
        if w.size:
            step = max(int(np.median(w)), 1)
            bins = max(1, math.ceil(float(min_bp) / float(step)))
    return min(region, max(bins, 1))


def rocco_objective(scores, mask, gamma, form):
    sel = scores[mask]
    total = float(np.sum(sel)) if form == "steps" else float(numpy_sum_device(sel))
    if mask.size > 1:
        if form == "steps":
            switches = int(np.sum(np.diff(mask.astype(np.uint8)) != 0))
        else:
            runs = run_bounds(mask)
            switches = 2 * len(runs) - int(bool(mask[0])) - int(bool(mask[-1]))
        total -= float(max(float(gamma), 0.0)) * float(switches)
    return total


def refine(scores, solution, gamma, selectionPenalty, nestedRoccoIters=3, nestedRoccoBudgetScale=0.75, jaccardThreshold=0.999,
           intervals=None, ends=None, rawScores=None, minRegionBP=None, minRegionBins=5, form="steps"):
    """`_refineNestedROCCOSolution` without its diagnostics: (uint8 solution, details)"""
    def vector(name, x):
        a = np.asarray(x, np.float64)
        if a.ndim != 1:
            raise ValueError(f"`{name}` must be one-dimensional")
        if a.size == 0:
            raise ValueError(f"`{name}` must be non-empty")
        if not np.all(np.isfinite(a)):
            raise ValueError(f"`{name}` contains non-finite values")
        return a

    s = vector("scores", scores)
    raw = s
    if rawScores is not None:
        raw = vector("rawScores", rawScores)
        if raw.size != s.size:
            raise ValueError("`rawScores` must match `scores` length")
    current = np.asarray(solution, np.uint8).ravel() > 0
    if current.size != s.size:
        raise ValueError("`solution` must match `scores` length")
    first = current.copy()
    iv = en = None
    if intervals is not None or ends is not None:
        if intervals is None or ends is None:
            raise ValueError("`intervals` and `ends` must be supplied together")
        iv, en = np.asarray(intervals, np.int64).ravel(), np.asarray(ends, np.int64).ravel()
        if iv.size != s.size or en.size != s.size:
            raise ValueError("`intervals` and `ends` must match `scores` length")
    iters = max(int(nestedRoccoIters), 0)
    g = float(gamma)
    if not math.isfinite(g) or g < 0.0:
        raise ValueError("`gamma` must be finite and non-negative")
    local_gamma = 0.25 * g
    pen = float(selectionPenalty)
    if not math.isfinite(pen):
        raise ValueError("`selectionPenalty` must be finite")
    scale = float(nestedRoccoBudgetScale)
    if not math.isfinite(scale):
        raise ValueError("`nestedRoccoBudgetScale` must be finite")
    scale = float(np.clip(scale, 0.0, 1.0))
    jt = float(np.clip(jaccardThreshold, 0.0, 1.0))
    mbins = max(int(minRegionBins), 1)
    mbp = None if minRegionBP is None else max(int(minRegionBP), 0)

    nodes, by_id, leaves, frontier, roots, layers, history = [], {}, set(), [], [], [], []

    def add(layer, parent, a, b):
        nid = len(nodes) + 1
        k = int(np.argmax(raw[a:b + 1]))
        total = float(np.sum(s[a:b + 1])) if form == "steps" else float(numpy_sum_device(s[a:b + 1]))
        node = {
            "id": nid, "layer": int(layer), "parent_id": parent, "start_idx": int(a), "end_idx": int(b),
            "range_start": int(iv[a]) if iv is not None else int(a), "range_end": int(en[b]) if iv is not None else int(b + 1),
            "length_bins": int(b - a + 1), "selected_count": int(b - a + 1), "required_idx": int(a + k), "summit_idx": int(a + k),
            "raw_score_max": float(raw[a + k]), "score_sum": total, "child_ids": [], "direct_child_count": 0, "child_count": 1,
            "leaf_count": 1, "candidate_child_count": 1, "child_widths_bins": [], "split_gain": 0.0, "split_gate": False,
            "decision": "leaf", "objective": None, "penalized_objective": None, "parent_penalized_objective": None,
            "boundary_penalty": None, "run_penalty": None, "run_penalty_total": None, "selection_penalty": None,
            "min_child_bins": int(mbins),
        }
        nodes.append(node)
        by_id[nid] = node
        return nid

    def flat():
        out = np.zeros(s.size, bool)
        for nid in leaves:
            out[by_id[nid]["start_idx"]:by_id[nid]["end_idx"] + 1] = True
        return out

    def refresh_layers():
        layers.clear()
        for L in range(max((n["layer"] for n in nodes), default=-1) + 1):
            ns = [n for n in nodes if n["layer"] == L]
            layers.append({
                "layer": L, "node_count": len(ns), "root_count": sum(n["parent_id"] is None for n in ns), "parent_count": len(ns),
                "split_count": sum(n["decision"] == "split" for n in ns), "unsplit_count": sum(n["decision"] != "split" for n in ns),
                "leaf_count": sum(n["id"] in leaves for n in ns), "child_count": sum(n["child_count"] for n in ns),
                "selected_count": sum(n["selected_count"] for n in ns),
            })

    for a, b in run_bounds(current):
        nid = add(0, None, a, b)
        roots.append(nid)
        leaves.add(nid)
        frontier.append(nid)
    refresh_layers()
    count0 = int(np.count_nonzero(current))
    details = {
        "enabled": iters > 0, "requested_iters": iters, "completed_iters": 0, "stop_reason": "disabled" if iters == 0 else "not_started",
        "jaccard_threshold": jt, "parent_gamma": g, "local_gamma": float(local_gamma), "selection_penalty": pen, "budget_scale": scale,
        "budget_policy": POLICY, "score_shift": pen, "subproblem_mode": MODE, "subproblem_max_iter": 5,
        "parent_edge_boundary_cost": EDGE, "min_region_bins": mbins, "min_region_bp": mbp, "min_child_bins": mbins,
        "required_bin_policy": "argmax_raw_score_leftmost", "diagnostic_detail_path": None, "initial_selected_count": count0,
        "final_selected_count": count0, "root_ids": roots, "leaf_node_ids": sorted(leaves), "hierarchy": nodes, "layers": layers,
        "history": history,
    }
    if iters == 0:
        return current.astype(np.uint8), details

    internal = float(max(float(local_gamma), 1000.0 * EDGE))
    for it in range(iters):
        previous, parents, frontier = current, list(frontier), []
        it_scale = scale if it == 0 else 1.0
        n_skip = n_split = n_shrink = n_keep = n_soft = 0
        extra_total = extra_max = 0.0
        for pid in parents:
            node = by_id[pid]
            a, b = node["start_idx"], node["end_idx"]
            length_bp = (b - a + 1) if iv is None else max(int(en[b]) - int(iv[a]), 0)
            if (mbp is not None and length_bp < mbp) or (mbp is None and (b - a + 1) < mbins):
                node.update(decision="skipped_short", child_count=1, leaf_count=1)
                n_keep += 1
                n_skip += 1
                continue
            local = s[a:b + 1]
            M = min_child_bins(a, b, iv, en, mbp, mbins)
            req = int(np.argmax(raw[a:b + 1]))
            floor, solver, srt = 0.0, local, None
            if form == "device":
                srt = np.sort(local)
            if it > 0:
                floor = float(np.quantile(local, 0.25)) if form == "steps" else float(quantile_sorted(srt, 0, srt.size, 0.25))
                solver = np.asarray(local - floor, np.float64)
            lpen, extra = soft_penalty(solver, 0.0 if it > 0 else pen, it_scale, form, (srt, floor))
            n_soft += it_scale < 1.0
            nl = b - a + 1
            costs = np.full(nl + 1, internal)
            costs[0] = costs[-1] = EDGE
            sel, obj, d = solve(solver, costs, lpen, M, req, internal, form)
            extra_total += extra
            extra_max = float(max(extra_max, extra))
            if not sel.any():
                raise RuntimeError("parent-conditioned subpeak solve selected no bins")
            runs = run_bounds(sel)
            widths = [r - l + 1 for l, r in runs]
            ok = len(runs) >= 1 and all(w >= M for w in widths)
            kept = objective_parts(solver, np.ones(nl, bool), costs, lpen, internal, form)[1]
            gain = float(float(d["penalized_objective"]) - float(kept))
            split = len(runs) >= 2 and ok and gain > 0.0
            shrink = len(runs) == 1 and ok and (not sel.all()) and gain > 0.0
            node.update(decision="split" if split else ("shrink" if shrink else "keep_parent"), candidate_child_count=len(runs),
                        child_widths_bins=widths, split_gain=gain, split_gate=bool(split), objective=float(obj),
                        penalized_objective=float(d["penalized_objective"]), parent_penalized_objective=float(kept),
                        boundary_penalty=float(d["boundary_penalty"]), run_penalty=float(d["run_penalty"]),
                        run_penalty_total=float(d["run_penalty_total"]), selection_penalty=float(lpen), local_score_floor=float(floor),
                        min_child_bins=int(M))
            if split or shrink:
                kids = []
                for l, r in runs:
                    kid = add(it + 1, pid, a + l, a + r)
                    kids.append(kid)
                    leaves.add(kid)
                    frontier.append(kid)
                leaves.remove(pid)
                node.update(child_ids=kids, direct_child_count=len(kids), child_count=len(kids), leaf_count=len(kids))
                n_split += split
                n_shrink += shrink
            else:
                node.update(child_ids=[], direct_child_count=0, child_count=1, leaf_count=1)
                n_keep += 1
        new = flat()
        if np.any(new & ~first):
            raise RuntimeError("nested ROCCO selection left the input solution")
        before, after = int(np.count_nonzero(previous)), int(np.count_nonzero(new))
        if form == "steps":
            union = int(np.sum(previous | new))
            jac = 1.0 if union == 0 else float(np.sum(previous & new) / union)
        else:
            jac = 1.0 if before == 0 else float(after / before)        # new is a subset of previous
        o_prev, o_new = rocco_objective(s, previous, g, form), rocco_objective(s, new, g, form)
        runs_prev, runs_new = run_bounds(previous), run_bounds(new)
        refresh_layers()
        details["leaf_node_ids"] = sorted(leaves)
        history.append({
            "iter": it + 1, "layer": it + 1, "num_parent_peaks": len(parents), "num_parent_peaks_after": len(runs_new),
            "num_input_regions": len(parents), "num_next_parent_nodes": len(frontier), "num_split_parent_nodes": int(n_split),
            "num_refined_parent_nodes": int(n_shrink), "num_retained_parent_nodes": int(n_keep), "num_skipped_short_regions": int(n_skip),
            "num_budget_constrained_regions": int(n_soft), "num_soft_budget_penalty_regions": int(n_soft),
            "num_empty_local_solutions": 0, "num_budget_fallback_windows": 0, "num_required_fallback_windows": 0,
            "num_parent_erasure_violations": 0, "num_required_bin_violations": 0,
            "num_peak_count_monotonicity_violations": max(len(runs_prev) - len(runs_new), 0),
            "num_coverage_expansion_violations": max(after - before, 0), "num_short_child_runs_expanded": 0,
            "num_short_child_bins_added": 0, "local_penalty_extra_mean": float(extra_total / max(len(parents) - n_skip, 1)),
            "local_penalty_extra_max": float(extra_max), "budget_scale": float(it_scale), "budget_policy": POLICY,
            "selected_count_before": before, "selected_count_after": after, "selected_count_delta": after - before,
            "objective": float(o_new), "objective_previous": float(o_prev), "objective_delta": float(o_new - o_prev),
            "jaccard": float(jac),
        })
        details["completed_iters"] = it + 1
        current = new
        details["final_selected_count"] = after
        if np.array_equal(new, previous):
            details["stop_reason"] = "mask_equal"
            break
        if not frontier:
            details["stop_reason"] = "no_splits"
            break
        if jac >= jt:
            details["stop_reason"] = "jaccard"
            break
    else:
        details["stop_reason"] = "max_iter"
    return current.astype(np.uint8), details


# ---------------------------------------------------------------------------------------------------------------
# comparison and flattening (fixtures hold arrays only)
# ---------------------------------------------------------------------------------------------------------------
def differences(got, want, path=""):
    """Paths at which two results differ: floats by bit pattern, everything else exactly."""
    out = []
    if isinstance(want, dict):
        if not isinstance(got, dict) or set(got) != set(want):
            return [f"{path}: keys {sorted(set(got) ^ set(want)) if isinstance(got, dict) else type(got)}"]
        for k in want:
            out += differences(got[k], want[k], f"{path}/{k}")
    elif isinstance(want, (list, tuple)):
        if not isinstance(got, (list, tuple)) or len(got) != len(want):
            return [f"{path}: length"]
        for i, (a, b) in enumerate(zip(got, want)):
            out += differences(a, b, f"{path}[{i}]")
    elif isinstance(want, np.ndarray):
        if not isinstance(got, np.ndarray) or got.dtype != want.dtype or not np.array_equal(got, want):
            out.append(f"{path}: array")
    elif isinstance(want, float):
        if not isinstance(got, float) or bits(got)[()] != bits(want)[()]:
            out.append(f"{path}: {got!r} != {want!r}")
    elif type(got) is not type(want) or got != want:
        out.append(f"{path}: {got!r} != {want!r}")
    return out


NODE_FLOATS = ("raw_score_max", "score_sum", "split_gain", "objective", "penalized_objective", "parent_penalized_objective",
               "boundary_penalty", "run_penalty", "run_penalty_total", "selection_penalty", "local_score_floor")
NODE_INTS = ("id", "layer", "parent_id", "start_idx", "end_idx", "range_start", "range_end", "required_idx", "candidate_child_count",
             "min_child_bins", "child_count")
DECISIONS = ("leaf", "split", "shrink", "keep_parent", "skipped_short")
STOPS = ("disabled", "not_started", "mask_equal", "no_splits", "jaccard", "max_iter")
HISTORY_FLOATS = ("objective", "objective_previous", "objective_delta", "jaccard", "local_penalty_extra_mean",
                  "local_penalty_extra_max", "budget_scale")
HISTORY_INTS = ("num_parent_peaks", "num_parent_peaks_after", "num_next_parent_nodes", "num_split_parent_nodes",
                "num_refined_parent_nodes", "num_retained_parent_nodes", "num_skipped_short_regions",
                "num_soft_budget_penalty_regions", "selected_count_before", "selected_count_after")


def flatten_refine(mask, details):
    """What a fixture keeps of a refinement: every number that is not a function of the others, as arrays."""
    nan = float("nan")
    h = details["hierarchy"]
    out = {"mask": np.asarray(mask, np.uint8), "stop": np.asarray([STOPS.index(details["stop_reason"])], np.int64),
           "completed": np.asarray([details["completed_iters"], details["final_selected_count"]], np.int64),
           "leaves": np.asarray(details["leaf_node_ids"], np.int64),
           "decision": np.asarray([DECISIONS.index(n["decision"]) for n in h], np.int64)}
    out["node_f"] = np.asarray([[nan if n.get(k) is None else float(n[k]) for k in NODE_FLOATS] for n in h], np.float64).reshape(
        len(h), len(NODE_FLOATS))
    out["node_i"] = np.asarray([[-1 if n[k] is None else int(n[k]) for k in NODE_INTS] for n in h], np.int64).reshape(
        len(h), len(NODE_INTS))
    hist = details["history"]
    out["hist_f"] = np.asarray([[float(r[k]) for k in HISTORY_FLOATS] for r in hist], np.float64).reshape(len(hist), len(HISTORY_FLOATS))
    out["hist_i"] = np.asarray([[int(r[k]) for k in HISTORY_INTS] for r in hist], np.int64).reshape(len(hist), len(HISTORY_INTS))
    return out


SOLVE_FLOATS = ("penalized_objective", "selected_fraction", "selection_penalty", "run_penalty", "run_penalty_total",
                "boundary_cost_min", "boundary_cost_max", "boundary_penalty")


def flatten_solve(mask, objective, d):
    return {"mask": np.asarray(mask, np.uint8),
            "f": np.asarray([float(objective)] + [float(d[k]) for k in SOLVE_FLOATS], np.float64),
            "i": np.asarray([d["selected_count"], d["min_run_bins"], d["num_runs"],
                             -1 if d["required_index"] is None else d["required_index"], int(d["required_selected"])], np.int64)}


def same_flat(a, b):
    """Names of the arrays at which two flattened results differ (floats by bit pattern)."""
    bad = [k for k in set(a) ^ set(b)]
    for k in set(a) & set(b):
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if x.shape != y.shape or x.dtype != y.dtype:
            bad.append(k)
        elif x.dtype == np.float64:
            if not np.array_equal(bits(x), bits(y)):
                bad.append(k)
        elif not np.array_equal(x, y):
            bad.append(k)
    return sorted(bad)
