"""Nested ROCCO refinement on the device (csrc/csr_nested.h), bit for bit the reference's `_solveParentConditionedSubpeaks` and
`_refineNestedROCCOSolution` (peaks.py:3519-3720, 3763-4388).

What runs where.  Per region and layer the DEVICE does peaks.py:4042-4172: the required bin, the 25 % floor, the soft selection
penalty, the dynamic programme with its backtrace, both objectives, split gain, gates, decision, and per new node the arg-max,
raw maximum and score sum; per chain and layer the NumPy-order sum of the selected scores.  The HOST keeps the hierarchy (node
dicts and their ids in the reference's creation order, `layers`, `history`, `leaf_node_ids`), applies the stop rule, and decides
the geometry from `intervals` / `ends` (host arrays): which regions are too short and `_minimumChildBinsForRegion`.  It works from
compact per-region records, never from per-bin data.  The reference's diagnostics (logging, the JSONL file) are not offered."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib as L
from ._lib import _vp

EDGE = 1.0e-12
POLICY = "soft_selection_penalty"
MODE = "parent_conditioned_min_run_dp"
MAX_MIN_RUN = 255
DECISIONS = {0: "keep_parent", 1: "split", 2: "shrink"}

REGION = np.dtype([("start", "<i8"), ("end", "<i8"), ("chain", "<i4"), ("min_run", "<i4")])
CFG = np.dtype([("gamma", "<f8"), ("selection_penalty", "<f8"), ("budget_scale", "<f8"), ("subtract_floor", "<i4"), ("reserved", "<i4")])
REC = np.dtype([("required", "<i8"), ("selected_count", "<i8"), ("child_base", "<i8"), ("n_runs", "<i4"), ("decision", "<i4"),
                ("widths_ok", "<i4"), ("reserved", "<i4"), ("floor", "<f8"), ("selection_penalty", "<f8"), ("extra_penalty", "<f8"),
                ("objective", "<f8"), ("penalized", "<f8"), ("boundary_penalty", "<f8"), ("run_penalty_total", "<f8"),
                ("parent_penalized", "<f8"), ("split_gain", "<f8")])
NODE = np.dtype([("start", "<i8"), ("end", "<i8"), ("required", "<i8"), ("raw_score_max", "<f8"), ("score_sum", "<f8")])


def _float_vector(name, values):
    arr = np.asarray(values, dtype=np.float64)
    if arr.ndim != 1:
        raise ValueError(f"`{name}` must be one-dimensional")
    if arr.size == 0:
        raise ValueError(f"`{name}` must be non-empty")
    if not np.all(np.isfinite(arr)):
        raise ValueError(f"`{name}` contains non-finite values")
    return np.ascontiguousarray(arr)


def run_bounds(mask):
    m = (np.asarray(mask).ravel() > 0).astype(np.int8)
    d = np.diff(np.concatenate(([0], m, [0])))
    return np.flatnonzero(d == 1).astype(np.int64), (np.flatnonzero(d == -1) - 1).astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------
# `_solveParentConditionedSubpeaks`
# ---------------------------------------------------------------------------------------------------------------
def solve_parent_conditioned_subpeaks(scores, boundaryCosts, selectionPenalty, minRunBins, requiredIndex=None, runPenalty=0.0):
    """Drop-in for `_solveParentConditionedSubpeaks`: (bool mask, objective, details)."""
    s = np.asarray(scores, dtype=np.float64)
    if s.ndim != 1 or s.size == 0:
        raise ValueError("`scores` must be a non-empty one-dimensional array")
    if not np.all(np.isfinite(s)):
        raise ValueError("`scores` contains non-finite values")
    s = np.ascontiguousarray(s)
    n = int(s.size)
    costs = np.asarray(boundaryCosts, dtype=np.float64).ravel()
    if costs.size == 1:
        costs = np.full(n + 1, float(costs[0]), dtype=np.float64)
    elif costs.size == n + 1:
        costs = np.ascontiguousarray(costs, dtype=np.float64)
    else:
        raise ValueError("`boundaryCosts` must be scalar or have length len(scores) + 1")
    if not np.all(np.isfinite(costs)) or np.any(costs < 0.0):
        raise ValueError("`boundaryCosts` must be finite and non-negative")
    penalty = float(selectionPenalty)
    if not math.isfinite(penalty):
        raise ValueError("`selectionPenalty` must be finite")
    rp = float(runPenalty)
    if not math.isfinite(rp) or rp < 0.0:
        raise ValueError("`runPenalty` must be finite and non-negative")
    req = None if requiredIndex is None else int(requiredIndex)
    if req is not None and (req < 0 or req >= n):
        raise ValueError("`requiredIndex` is outside `scores`")
    min_run = int(min(max(int(minRunBins), 1), n))
    mask = np.zeros(n, np.uint8)
    rec = np.zeros(1, REC)
    L.check_value(L.lib().csr_nested_solve(L.dp(s), n, L.dp(costs), penalty, min_run, -1 if req is None else req, rp,
                                           mask.ctypes.data_as(C.POINTER(C.c_uint8)), _vp(rec)))
    r = rec[0]
    mask = mask.astype(bool)
    if req is not None and not bool(mask[req]):
        raise RuntimeError("parent-conditioned subpeak DP violated required bin constraint")
    count = int(r["selected_count"])
    return mask, float(r["objective"]), {
        "mode": MODE,
        "penalized_objective": float(r["penalized"]),
        "selected_count": count,
        "selected_fraction": float(count / max(n, 1)),
        "selection_penalty": penalty,
        "run_penalty": rp,
        "run_penalty_total": float(r["run_penalty_total"]),
        "boundary_cost_min": float(np.min(costs)),
        "boundary_cost_max": float(np.max(costs)),
        "boundary_penalty": float(r["boundary_penalty"]),
        "min_run_bins": min_run,
        "num_runs": int(r["n_runs"]),
        "required_index": req,
        "required_selected": bool(True if req is None else mask[req]),
        "required_fallback_window": False,
    }


# ---------------------------------------------------------------------------------------------------------------
# the refinement of any number of chains, over a backend that holds their scores and masks
# ---------------------------------------------------------------------------------------------------------------
class HostBackend:
    """Host arrays, one chain after the other (the default context of the library)."""

    def __init__(self, scores, raws, solutions):
        self.lens = np.asarray([s.size for s in scores], np.int64)
        self.scores = np.ascontiguousarray(np.concatenate(scores), np.float64)
        self.raw = None if all(r is None for r in raws) else np.ascontiguousarray(
            np.concatenate([s if r is None else r for s, r in zip(scores, raws)]), np.float64)
        self.solution = np.ascontiguousarray(np.concatenate(solutions), np.uint8)
        self.offsets = np.concatenate(([0], np.cumsum(self.lens)))
        self._lib = L.lib()

    def initial_runs(self, chain):
        return run_bounds(self.solution[self.offsets[chain]:self.offsets[chain + 1]])

    def nodes(self, regions):
        out = np.zeros(regions.size, NODE)
        L.check_value(self._lib.csr_nested_nodes(len(self.lens), self.lens.ctypes.data_as(L.I64P), L.dp(self.scores), L.dp(self.raw),
                                                 regions.size, _vp(regions), _vp(out)))
        return out

    def layer(self, cfg, take, regions):
        rec, count = np.zeros(regions.size, REC), C.c_int64(0)
        L.check_value(self._lib.csr_nested_layer(len(self.lens), self.lens.ctypes.data_as(L.I64P), L.dp(self.scores), L.dp(self.raw),
                                                 self.solution.ctypes.data_as(C.POINTER(C.c_uint8)), _vp(cfg), regions.size,
                                                 _vp(regions), _vp(rec), C.byref(count)))
        kids = np.zeros(int(count.value), NODE)
        L.check(self._lib.csr_nested_children(None, kids.size, _vp(kids)))
        return rec, kids

    def selected_sums(self, take, n_runs, starts, ends):
        out = np.zeros(len(self.lens), np.float64)
        L.check_value(self._lib.csr_nested_selected_sum(len(self.lens), self.lens.ctypes.data_as(L.I64P), L.dp(self.scores),
                                                        n_runs.ctypes.data_as(L.I64P), starts.ctypes.data_as(L.I64P),
                                                        ends.ctypes.data_as(L.I64P), L.dp(out)))
        return out

    def mask(self, chain):
        return self.solution[self.offsets[chain]:self.offsets[chain + 1]].copy()


class _Chain:
    """The reference's bookkeeping of one chain: nodes, leaves, frontier, layers, history."""

    def __init__(self, index, n, gamma, penalty, iters, scale, jaccard, intervals, ends, min_bp, min_bins):
        self.index, self.n = index, int(n)
        self.iv = self.en = None
        if intervals is not None or ends is not None:
            if intervals is None or ends is None:
                raise ValueError("`intervals` and `ends` must be supplied together")
            self.iv = np.asarray(intervals, dtype=np.int64).ravel()
            self.en = np.asarray(ends, dtype=np.int64).ravel()
            if self.iv.size != self.n or self.en.size != self.n:
                raise ValueError("`intervals` and `ends` must match `scores` length")
        self.iters = max(int(iters), 0)
        self.gamma = float(gamma)
        if not math.isfinite(self.gamma) or self.gamma < 0.0:
            raise ValueError("`gamma` must be finite and non-negative")
        self.penalty = float(selectionPenalty_check(penalty))
        scale = float(scale)
        if not math.isfinite(scale):
            raise ValueError("`nestedRoccoBudgetScale` must be finite")
        self.scale = float(np.clip(scale, 0.0, 1.0))
        self.jt = float(np.clip(jaccard, 0.0, 1.0))
        self.mbins = max(int(min_bins), 1)
        self.mbp = None if min_bp is None else max(int(min_bp), 0)
        self.nodes, self.by_id, self.leaves, self.frontier, self.roots, self.layers, self.history = [], {}, set(), [], [], [], []
        self.done = self.iters == 0
        self.details = None
        self.objective = None
        # one bin width for the whole chain: `_minimumChildBinsForRegion` is then one expression for all regions
        self.step = None
        if self.iv is not None and self.mbp is not None and self.n:
            w = self.en - self.iv
            if w.min() == w.max() and w[0] > 0:
                self.step = int(w[0])

    def add(self, layer, parent, nd):
        nid = len(self.nodes) + 1
        a, b = int(nd["start"]), int(nd["end"])
        node = {
            "id": nid, "layer": int(layer), "parent_id": parent, "start_idx": a, "end_idx": b,
            "range_start": int(self.iv[a]) if self.iv is not None else a,
            "range_end": int(self.en[b]) if self.iv is not None else b + 1,
            "length_bins": b - a + 1, "selected_count": b - a + 1, "required_idx": int(nd["required"]),
            "summit_idx": int(nd["required"]), "raw_score_max": float(nd["raw_score_max"]), "score_sum": float(nd["score_sum"]),
            "child_ids": [], "direct_child_count": 0, "child_count": 1, "leaf_count": 1, "candidate_child_count": 1,
            "child_widths_bins": [], "split_gain": 0.0, "split_gate": False, "decision": "leaf", "objective": None,
            "penalized_objective": None, "parent_penalized_objective": None, "boundary_penalty": None, "run_penalty": None,
            "run_penalty_total": None, "selection_penalty": None, "min_child_bins": int(self.mbins),
        }
        self.nodes.append(node)
        self.by_id[nid] = node
        return nid

    def refresh_layers(self):
        self.layers.clear()
        for k in range(max((n["layer"] for n in self.nodes), default=-1) + 1):
            ns = [n for n in self.nodes if n["layer"] == k]
            self.layers.append({
                "layer": k, "node_count": len(ns), "root_count": sum(n["parent_id"] is None for n in ns), "parent_count": len(ns),
                "split_count": sum(n["decision"] == "split" for n in ns), "unsplit_count": sum(n["decision"] != "split" for n in ns),
                "leaf_count": sum(n["id"] in self.leaves for n in ns), "child_count": sum(n["child_count"] for n in ns),
                "selected_count": sum(n["selected_count"] for n in ns),
            })

    def leaf_runs(self):
        runs = sorted((self.by_id[i]["start_idx"], self.by_id[i]["end_idx"]) for i in self.leaves)
        return runs

    def selected(self):
        return sum(self.by_id[i]["length_bins"] for i in self.leaves)

    def rocco_objective(self, total, runs):
        return rocco_objective(total, runs, self.n, self.gamma)

    def check_min_run(self, a, b):
        """Refuses, before any launch, a first-pass run [a, b] in which a region could ask for more states than the device has.  One
        bin width (or bin mode): the run's own minimum child run, which no child's exceeds.  Mixed widths: a bound, the minimum
        child run at the smallest positive width inside the run."""
        if self.too_short(a, b):
            return
        bins = self.min_child_bins(a, b)
        if self.mbp is not None and self.iv is not None and self.step is None:
            w = np.asarray(self.en[a:b + 1] - self.iv[a:b + 1], dtype=np.int64)
            w = w[w > 0]
            if w.size:
                bins = max(bins, min(b - a + 1, int(max(1, math.ceil(float(self.mbp) / float(max(int(w.min()), 1)))))))
        if bins > MAX_MIN_RUN:
            raise ValueError(f"`minRunBins` {bins} exceeds the supported maximum {MAX_MIN_RUN}")

    def min_child_bins(self, a, b):
        region, bins = max(b - a + 1, 1), self.mbins
        if self.mbp is not None and self.iv is not None:
            step = self.step
            if step is None:
                w = np.asarray(self.en[a:b + 1] - self.iv[a:b + 1], dtype=np.int64)
                w = w[w > 0]
                step = int(max(int(np.median(w)), 1)) if w.size else None
            if step is not None:
                bins = int(max(1, math.ceil(float(self.mbp) / float(max(step, 1)))))
        return int(min(region, max(bins, 1)))

    def too_short(self, a, b):
        if self.mbp is not None:
            length = (b - a + 1) if self.iv is None else max(int(self.en[b]) - int(self.iv[a]), 0)
            return length < self.mbp
        return (b - a + 1) < self.mbins


def rocco_objective(total, runs, n, gamma):
    """`_roccoObjectiveForSolution` from the NumPy-order sum of the selected scores and the runs of the mask"""
    if n > 1:
        switches = 2 * len(runs) - int(bool(runs) and runs[0][0] == 0) - int(bool(runs) and runs[-1][1] == n - 1)
        total -= float(max(float(gamma), 0.0)) * float(switches)
    return total


def selectionPenalty_check(value):
    value = float(value)
    if not math.isfinite(value):
        raise ValueError("`selectionPenalty` must be finite")
    return value


def refine_chains(backend, chains):
    """Runs the refinement of every chain of `chains` (a list of _Chain) layer by layer, all chains side by side."""
    nc = len(backend.lens)
    # roots
    regions = []
    for ch in chains:
        st, en = backend.initial_runs(ch.index)
        regions += [(int(a), int(b), ch.index, 1) for a, b in zip(st, en)]
        if not ch.done:
            for a, b in zip(st, en):
                ch.check_min_run(int(a), int(b))
    roots = backend.nodes(np.asarray(regions, REGION)) if regions else np.zeros(0, NODE)
    k = 0
    for ch in chains:
        while k < len(regions) and regions[k][2] == ch.index:
            nid = ch.add(0, None, roots[k])
            ch.roots.append(nid)
            ch.leaves.add(nid)
            ch.frontier.append(nid)
            k += 1
        ch.refresh_layers()
        count0 = ch.selected()
        internal = float(max(0.25 * ch.gamma, 1000.0 * EDGE))
        ch.internal = internal
        ch.details = {
            "enabled": ch.iters > 0, "requested_iters": ch.iters, "completed_iters": 0,
            "stop_reason": "disabled" if ch.iters == 0 else "not_started", "jaccard_threshold": ch.jt, "parent_gamma": ch.gamma,
            "local_gamma": float(0.25 * ch.gamma), "selection_penalty": ch.penalty, "budget_scale": ch.scale, "budget_policy": POLICY,
            "score_shift": ch.penalty, "subproblem_mode": MODE, "subproblem_max_iter": 5, "parent_edge_boundary_cost": EDGE,
            "min_region_bins": ch.mbins, "min_region_bp": ch.mbp, "min_child_bins": ch.mbins,
            "required_bin_policy": "argmax_raw_score_leftmost", "diagnostic_detail_path": None, "initial_selected_count": count0,
            "final_selected_count": count0, "root_ids": ch.roots, "leaf_node_ids": sorted(ch.leaves), "hierarchy": ch.nodes,
            "layers": ch.layers, "history": ch.history,
        }

    def objectives(live):
        """`_roccoObjectiveForSolution` of the current leaves of the live chains"""
        take = np.zeros(nc, np.uint8)
        n_runs, st, en, runs_of = np.zeros(nc, np.int64), [], [], {}
        for ch in live:
            runs = ch.leaf_runs()
            runs_of[ch.index] = runs
            take[ch.index] = 1
            n_runs[ch.index] = len(runs)
        for i in range(nc):        # (the runs go in chain order)
            for a, b in runs_of.get(i, ()):
                st.append(a)
                en.append(b)
        sums = backend.selected_sums(take, n_runs, np.asarray(st, np.int64), np.asarray(en, np.int64))
        return {ch.index: ch.rocco_objective(float(sums[ch.index]), runs_of[ch.index]) for ch in live}

    live = [ch for ch in chains if not ch.done]
    if live:
        for i, v in objectives(live).items():
            next(ch for ch in live if ch.index == i).objective = v
    it = 0
    while live:
        cfg = np.zeros(nc, CFG)
        take = np.zeros(nc, np.uint8)
        regions, owners = [], []
        stats = {}
        for ch in sorted(live, key=lambda c: c.index):
            take[ch.index] = 1
            cfg[ch.index] = (ch.gamma, 0.0 if it > 0 else ch.penalty, ch.scale if it == 0 else 1.0, int(it > 0), 0)
            ch.parents, ch.frontier = list(ch.frontier), []
            ch.before = ch.selected()
            ch.runs_before = len(ch.leaves)
            stats[ch.index] = dict(skip=0, split=0, shrink=0, keep=0, soft=0, extra_total=0.0, extra_max=0.0)
            # the device takes regions in ascending order of start; the parents are visited in the reference's order afterwards
            todo = []
            for pid in ch.parents:
                node = ch.by_id[pid]
                a, b = node["start_idx"], node["end_idx"]
                if not ch.too_short(a, b):
                    todo.append((a, b, ch.index, ch.min_child_bins(a, b), pid))
            todo.sort()
            for a, b, ci, m, pid in todo:
                if min(m, b - a + 1) > MAX_MIN_RUN:
                    raise ValueError(f"`minRunBins` {min(m, b - a + 1)} exceeds the supported maximum {MAX_MIN_RUN}")
                regions.append((a, b, ci, m))
                owners.append((ch, pid))
        if regions:
            rec, kids = backend.layer(cfg, take, np.asarray(regions, REGION))
        else:
            rec, kids = np.zeros(0, REC), np.zeros(0, NODE)
        by_parent = {(ch.index, pid): k for k, (ch, pid) in enumerate(owners)}
        for ch in live:
            s = stats[ch.index]
            it_scale = ch.scale if it == 0 else 1.0
            for pid in ch.parents:
                node = ch.by_id[pid]
                k = by_parent.get((ch.index, pid))
                if k is None:
                    node.update(decision="skipped_short", child_count=1, leaf_count=1)
                    s["keep"] += 1
                    s["skip"] += 1
                    continue
                r = rec[k]
                s["soft"] += it_scale < 1.0
                extra = float(r["extra_penalty"])
                s["extra_total"] += extra
                s["extra_max"] = float(max(s["extra_max"], extra))
                if int(r["selected_count"]) == 0:
                    raise RuntimeError("parent-conditioned subpeak solve selected no bins")
                runs = kids[int(r["child_base"]):int(r["child_base"]) + int(r["n_runs"])]
                decision = DECISIONS[int(r["decision"])]
                node.update(decision=decision, candidate_child_count=int(r["n_runs"]),
                            child_widths_bins=[int(e - a + 1) for a, e in zip(runs["start"], runs["end"])],
                            split_gain=float(r["split_gain"]), split_gate=decision == "split", objective=float(r["objective"]),
                            penalized_objective=float(r["penalized"]), parent_penalized_objective=float(r["parent_penalized"]),
                            boundary_penalty=float(r["boundary_penalty"]), run_penalty=float(ch.internal),
                            run_penalty_total=float(r["run_penalty_total"]), selection_penalty=float(r["selection_penalty"]),
                            local_score_floor=float(r["floor"]), min_child_bins=int(regions[k][3]))
                if decision in ("split", "shrink"):
                    ids = []
                    for nd in runs:
                        kid = ch.add(it + 1, pid, nd)
                        ids.append(kid)
                        ch.leaves.add(kid)
                        ch.frontier.append(kid)
                    ch.leaves.remove(pid)
                    node.update(child_ids=ids, direct_child_count=len(ids), child_count=len(ids), leaf_count=len(ids))
                    s["split" if decision == "split" else "shrink"] += 1
                else:
                    node.update(child_ids=[], direct_child_count=0, child_count=1, leaf_count=1)
                    s["keep"] += 1
        after_obj = objectives(live)
        still = []
        for ch in live:
            s = stats[ch.index]
            before, after = ch.before, ch.selected()
            # the new mask is made of children inside their parents: a subset of the previous one, so the Jaccard index is a ratio
            # of counts (reported: coverage expansion would show as after > before)
            jac = 1.0 if before == 0 else float(after / before)
            o_prev, o_new = ch.objective, after_obj[ch.index]
            ch.objective = o_new
            runs_after = len(ch.leaves)
            ch.refresh_layers()
            ch.details["leaf_node_ids"] = sorted(ch.leaves)
            ch.history.append({
                "iter": it + 1, "layer": it + 1, "num_parent_peaks": len(ch.parents), "num_parent_peaks_after": runs_after,
                "num_input_regions": len(ch.parents), "num_next_parent_nodes": len(ch.frontier),
                "num_split_parent_nodes": s["split"], "num_refined_parent_nodes": s["shrink"], "num_retained_parent_nodes": s["keep"],
                "num_skipped_short_regions": s["skip"], "num_budget_constrained_regions": int(s["soft"]),
                "num_soft_budget_penalty_regions": int(s["soft"]), "num_empty_local_solutions": 0, "num_budget_fallback_windows": 0,
                "num_required_fallback_windows": 0, "num_parent_erasure_violations": 0, "num_required_bin_violations": 0,
                "num_peak_count_monotonicity_violations": max(ch.runs_before - runs_after, 0),
                "num_coverage_expansion_violations": max(after - before, 0), "num_short_child_runs_expanded": 0,
                "num_short_child_bins_added": 0,
                "local_penalty_extra_mean": float(s["extra_total"] / max(len(ch.parents) - s["skip"], 1)),
                "local_penalty_extra_max": float(s["extra_max"]), "budget_scale": float(ch.scale if it == 0 else 1.0),
                "budget_policy": POLICY, "selected_count_before": before, "selected_count_after": after,
                "selected_count_delta": after - before, "objective": float(o_new), "objective_previous": float(o_prev),
                "objective_delta": float(o_new - o_prev), "jaccard": float(jac),
            })
            ch.details["completed_iters"] = it + 1
            ch.details["final_selected_count"] = after
            changed = s["split"] + s["shrink"] > 0     # a split or a shrink always drops at least one bin
            if not changed:
                ch.details["stop_reason"] = "mask_equal"
            elif not ch.frontier:
                ch.details["stop_reason"] = "no_splits"
            elif jac >= ch.jt:
                ch.details["stop_reason"] = "jaccard"
            elif it + 1 >= ch.iters:
                ch.details["stop_reason"] = "max_iter"
            else:
                still.append(ch)
                continue
            ch.done = True
        live = still
        it += 1
    return [ch.details for ch in chains]


def refine_nested_rocco_solution(scores, solution, gamma, selectionPenalty, nestedRoccoIters=3, nestedRoccoBudgetScale=0.75,
                                 jaccardThreshold=0.999, intervals=None, ends=None, rawScores=None, minRegionBP=None, minRegionBins=5):
    """Drop-in for `_refineNestedROCCOSolution` (without its three diagnostics arguments): (uint8 solution, details)."""
    s = _float_vector("scores", scores)
    raw = None
    if rawScores is not None:
        raw = _float_vector("rawScores", rawScores)
        if raw.size != s.size:
            raise ValueError("`rawScores` must match `scores` length")
    current = (np.asarray(solution, dtype=np.uint8).ravel() > 0).astype(np.uint8)
    if current.size != s.size:
        raise ValueError("`solution` must match `scores` length")
    ch = _Chain(0, s.size, gamma, selectionPenalty, nestedRoccoIters, nestedRoccoBudgetScale, jaccardThreshold, intervals, ends,
                minRegionBP, minRegionBins)
    backend = HostBackend([s], [raw], [current])
    details = refine_chains(backend, [ch])[0]
    return backend.mask(0), details
