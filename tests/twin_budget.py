"""Pure NumPy / Python twin of the ROCCO budget's device path (TEST INFRASTRUCTURE).

* `cEstimateEffectiveSampleSize`: the reference's native (pyx:9160-9279) restated.  Every sum of the native is a sequential walk
  with a separate multiply and add; here `np.cumsum(...)[-1]` walks (NumPy's cumulative sum adds in index order), everything
  else is Python floats -- the same IEEE operations.
* `series`: the three per-bin series of peaks.py:1414-1434 with the reference's own NumPy calls.
* `budget`: the scalar policy of `_estimateBudgetForPreparedROCCOScore` (peaks.py:1294-1516) restated step by step on a panel
  given as the per-z dicts of `dwb_panel` (the reference's `peaks` module does not import where fixtures are made).
"""
from __future__ import annotations

import math

import numpy as np

TINY = float(np.finfo(np.float64).tiny)
DBL_MIN = 2.2250738585072014e-308
BUDGET_MIN, BUDGET_MAX = 0.001, 0.25            # the reference's ROCCO_BUDGET_MIN / ROCCO_BUDGET_MAX


def walk(v) -> float:
    """0.0 + v[0] + v[1] + ... in index order."""
    v = np.asarray(v, np.float64)
    return float(np.cumsum(np.concatenate(([0.0], v)))[-1])


def _c_int(v) -> int:
    v = int(v)
    if not -(1 << 31) <= v < (1 << 31):
        raise OverflowError("value too large to convert to int")
    return v


def cEstimateEffectiveSampleSize(values, maxLag, activeMask=None, logPositive=False, windowIntervals=0):
    with np.errstate(invalid="ignore", over="ignore"):      # (a NaN, an inf or an overflow is data here, as in C)
        return _ess(values, maxLag, activeMask, logPositive, windowIntervals)


def _ess(values, maxLag, activeMask, logPositive, windowIntervals):
    maxLag, window = _c_int(maxLag), _c_int(windowIntervals)
    x = np.array(np.asarray(values, dtype=np.float64).reshape(-1), dtype=np.float64)      # (a copy: the native centres in place)
    n = x.shape[0]
    if window < 0:
        raise ValueError("windowIntervals must be nonnegative")
    if activeMask is None and not logPositive and window == 0:
        if n < 2:
            return float(n), 1.0, 0
        mean = walk(x) / float(n)
        x = x - mean
        var = walk(x * x) / float(max(n, 1))
        if not math.isfinite(var) or var <= DBL_MIN:
            return float(n), 1.0, 0
        max_lag = max(1, min(maxLag, n - 1))
        tau, used = 1.0, 0
        for lag in range(1, max_lag + 1):
            cov = walk(x[: n - lag] * x[lag:]) / float(max(n - lag, 1))
            rho = cov / var
            if not math.isfinite(rho) or rho <= 0.0:
                break
            tau += 2.0 * rho
            used = lag
        tau = max(tau, 1.0)
        return float(n / tau), float(tau), int(used)
    active = np.ones(n, bool)
    if activeMask is not None:
        m = np.asarray(activeMask, dtype=np.uint8).reshape(-1)
        if m.shape[0] != n:
            raise ValueError("activeMask length must match values length")
        active = m != 0
    for i in np.flatnonzero(active):
        v = float(x[i])
        if logPositive:
            if not math.isfinite(v) or v <= 0.0:
                raise ValueError("active values must be positive finite")
            x[i] = math.log(v)
        elif not math.isfinite(v):
            raise ValueError("active values must be finite")
    count = int(np.count_nonzero(active))
    if count < 2:
        return float(count), 1.0, 0
    mean = walk(x[active]) / float(count)
    x = np.where(active, x - mean, x)
    var = walk((x * x)[active]) / float(count)
    if not math.isfinite(var):
        raise ValueError("variance estimate must be finite")
    if var <= DBL_MIN:
        return float(count), 1.0, 0
    max_lag = max(1, min(maxLag, n - 1))
    if window > 0 and window - 1 < max_lag:
        max_lag = window - 1
    tau, used = 1.0, 0
    for lag in range(1, max_lag + 1):
        pair = active[: n - lag] & active[lag:]
        pairs = int(np.count_nonzero(pair))
        if pairs <= 0:
            continue
        cov = walk((x[: n - lag] * x[lag:])[pair]) / float(pairs)
        rho = cov / var
        if not math.isfinite(rho):
            raise ValueError("autocorrelation estimate must be finite")
        if window <= 0:
            if rho <= 0.0:
                break
            tau += 2.0 * rho
            used = lag
        elif rho > 0.0:
            taper = 1.0 - (float(lag) / float(window))
            if taper > 0.0:
                tau += 2.0 * taper * rho
                used = lag
    tau = max(tau, 1.0)
    if window > 0 and tau > float(window):
        tau = float(window)
    return float(count / tau), float(tau), int(used)


def soft_series(score, threshold, scale):
    return np.clip((score - float(threshold)) / max(float(scale), TINY), 0.0, None)


def series(kind, score, thresholds, scales):
    """peaks.py:1391-1434 on one score track; thresholds / scales: one value, or the grid's for "integrated"."""
    score = np.asarray(score, np.float64)
    thr, sc = np.atleast_1d(thresholds), np.atleast_1d(scales)
    if kind == "occupancy":
        return (score > float(thr[0])).astype(np.float64)
    if kind == "soft":
        return soft_series(score, thr[0], sc[0])
    return np.mean(np.vstack([soft_series(score, t, s) for t, s in zip(thr, sc)]), axis=0)


def integrated_in_order(score, thresholds, scales):
    """What the device evaluates: the soft series added in grid order, then divided by their number."""
    acc = soft_series(score, thresholds[0], scales[0])
    for t, s in zip(thresholds[1:], scales[1:]):
        acc = acc + soft_series(score, t, s)
    return acc / float(len(thresholds))


def z_key(z):
    z = float(z)
    return f"{z:.6f}".rstrip("0").rstrip(".")


def resolve_z_grid(threshold_z, grid):
    values, seen = [], set()
    for value in [threshold_z, *grid]:
        value_ = float(max(float(value), 0.0))
        key = z_key(value_)
        if key not in seen:
            seen.add(key)
            values.append(value_)
    values.sort()
    return values


def budget(score, views, *, statistic="occupancy", threshold_z, threshold_z_grid, dependence_span, budget_min=BUDGET_MIN,
           budget_max=BUDGET_MAX, ess=cEstimateEffectiveSampleSize):
    """peaks.py:1294-1516 for one chain; views: the per-z dicts of the panel (threshold views and metrics in one)."""
    score = np.asarray(score, np.float64)
    z_grid = resolve_z_grid(threshold_z, threshold_z_grid)
    budget_min_ = float(max(budget_min, 0.0))
    budget_max_ = float(max(budget_max, budget_min_))
    primary_key = z_key(float(max(threshold_z, 0.0)))
    statistic_ = str(statistic).strip().lower().replace("-", "_")
    if statistic_ in {"integrated", "integrated_excess", "integrated_excess_tail", "excess"}:
        selected = "integrated_excess_tail"
    elif statistic_ in {"occupancy", "calibrated_occupancy", "calibrated_tail_occupancy", "tail_fraction", "fraction", "tail",
                        "tail_occupancy"}:
        selected = "tail_occupancy"
    elif statistic_ in {"soft", "soft_occupancy", "soft_tail"}:
        selected = "soft"
    else:
        raise ValueError(f"Unknown budget statistic: {statistic}")
    threshold_views = {z_key(v["threshold_z"]): v for v in views}
    primary = threshold_views.get(primary_key)
    if primary is None:
        primary = threshold_views[z_key(z_grid[0])]
    integrated_raw = float(np.mean([float(m["budget_soft_raw"]) for m in threshold_views.values()]))
    occ_raw, soft_raw = float(primary["budget_occupancy_raw"]), float(primary["budget_soft_raw"])
    b_occ = float(np.clip(occ_raw, budget_min_, budget_max_))
    b_soft = float(np.clip(soft_raw, budget_min_, budget_max_))
    b_int = float(np.clip(integrated_raw, budget_min_, budget_max_))
    if selected == "tail_occupancy":
        b, raw = b_occ, occ_raw
        ess_series = (score > float(primary["threshold"])).astype(np.float64)
    elif selected == "soft":
        b, raw = b_soft, soft_raw
        ess_series = soft_series(score, primary["threshold"], primary["null_scale"])
    else:
        b, raw = b_int, integrated_raw
        parts = [soft_series(score, threshold_views[z_key(z)]["threshold"], threshold_views[z_key(z)]["null_scale"]) for z in z_grid]
        ess_series = np.mean(np.vstack(parts), axis=0)
    n_eff, tau, lags = ess(ess_series, max(4 * int(dependence_span), int(dependence_span)))
    d = {"statistic": selected, "num_bootstrap": int(primary["num_bootstrap"]), "null_quantile": float(primary["null_quantile"]),
         "dependence_span": int(dependence_span), "threshold": float(primary["threshold"]), "threshold_z": float(threshold_z),
         "threshold_z_grid": [float(z) for z in z_grid], "null_center": float(primary["null_center"]),
         "null_scale": float(primary["null_scale"])}
    for k in ("observed_tail_occupancy", "null_tail_occupancy", "null_tail_occupancy_calibrated", "null_tail_occupancy_sd",
              "observed_soft_tail", "null_soft_tail", "null_soft_tail_calibrated", "null_soft_tail_sd"):
        d[k] = float(primary[k])
    d.update(budget_min=budget_min_, budget_max=budget_max_, budget_raw=float(raw), budget_clipped=bool(abs(b - raw) > 1.0e-12),
             budget_occupancy_raw=occ_raw, budget_soft_raw=soft_raw, budget_integrated_raw=integrated_raw, budget_occupancy=b_occ,
             budget_soft=b_soft, budget_integrated=b_int, effective_count=float(b * n_eff), effective_total_count=float(n_eff),
             autocorrelation_time=float(tau), ess_lags_used=int(lags), budget=float(b))
    return d


def same_details(a: dict, b: dict):
    """Keys whose values differ: floats by their 64-bit patterns, everything else with ==."""
    bad = [k for k in set(a) ^ set(b)]
    for k in set(a) & set(b):
        if isinstance(a[k], float) and isinstance(b[k], float):
            if np.float64(a[k]).view(np.uint64) != np.float64(b[k]).view(np.uint64):
                bad.append(k)
        elif a[k] != b[k]:
            bad.append(k)
    return sorted(bad)


# ---------------------------------------------------------------------------------------------------------------
# gamma (peaks.py:1694-1780) and the wrapper of the solve (peaks.py:1783-1849), restated
# ---------------------------------------------------------------------------------------------------------------
def estimate_gamma(score, *, dependence_span, gamma_span=None, gamma=0.5, gamma_scale=0.5, clip_min=0.5, clip_max=50.0,
                   null_center=None, threshold=None):
    """(gamma, details) with the span given (`_resolveRoccoDependenceSpanDetails`: point = lower = upper = max(span, 2))."""
    if gamma is None:
        return 0.5, {"method": "fixed", "gamma": 0.5}
    gamma_ = float(gamma)
    if not np.isfinite(gamma_):
        raise ValueError("`gamma` must be finite")
    if gamma_ >= 0.0:
        return gamma_, {"method": "fixed", "gamma": float(gamma_)}
    scores = np.asarray(score, np.float64)
    span = max(int(dependence_span), 2)
    gamma_span_ = max(int(gamma_span), 2) if gamma_span is not None else span
    level, method = 0.0, "zero"
    if threshold is not None and np.isfinite(float(threshold)):
        level, method = float(threshold), "threshold"
    elif null_center is not None and np.isfinite(float(null_center)):
        level, method = float(null_center), "null_center"
    positive = scores - level
    positive = positive[positive > 0.0]
    scale = float(np.median(positive)) if positive.size > 0 else 1.0
    raw = float(max(float(gamma_scale), 0.0) * float(gamma_span_) * scale)
    gamma_ = float(max(raw, float(max(clip_min, 0.0))))
    if clip_max is not None:
        gamma_ = float(min(gamma_, float(max(clip_max, clip_min))))
    details = {"method": "dependence_span_lower_score_scale", "dependence_span": span, "gamma_span": gamma_span_,
               "dependence_span_lower": span, "dependence_span_upper": span, "reference_method": method,
               "reference_level": float(level), "positive_score_median": float(scale), "gamma_scale": float(gamma_scale),
               "gamma_raw": float(raw), "gamma": float(gamma_)}
    if clip_max is not None:
        details["gamma_clip_max"] = float(max(clip_max, clip_min))
    details["gamma_clip_min"] = float(max(clip_min, 0.0))
    return gamma_, details


def best_window(scores, target_count, selection_penalty, gamma, max_relative_range=None):
    """peaks.py:3723-3760 with its loop."""
    scores_ = np.asarray(scores, dtype=np.float64)
    n = int(scores_.size)
    target = int(min(max(int(target_count), 1), n))
    out = np.zeros(n, dtype=bool)
    if n == 0 or target <= 0:
        return out, False
    adjusted = scores_ - float(selection_penalty)
    cumsum = np.concatenate(([0.0], np.cumsum(adjusted, dtype=np.float64)))
    best_objective, best_start = -math.inf, 0
    for start in range(0, n - target + 1):
        end = start + target - 1
        window_score = float(cumsum[end + 1] - cumsum[start])
        switch_count = int(start > 0) + int(end < n - 1)
        objective = window_score - float(max(float(gamma), 0.0)) * float(switch_count)
        if objective > best_objective:
            best_objective, best_start = objective, start
    if not np.isfinite(best_objective) or best_objective <= 0.0:
        return out, False
    if max_relative_range is not None:
        window = scores_[best_start: best_start + target]
        window_range = float(np.max(window) - np.min(window))
        window_scale = float(max(np.max(np.abs(window)), 1.0e-6))
        if window_range > float(max(float(max_relative_range), 0.0)) * window_scale:
            return out, False
    out[best_start: best_start + target] = True
    return out, True


def objective_for_solution(scores, solution, gamma):
    scores_, solution_ = np.asarray(scores, np.float64), np.asarray(solution, np.uint8)
    objective = float(np.sum(scores_[solution_ > 0]))
    if solution_.size > 1:
        objective -= float(max(float(gamma), 0.0)) * float(np.sum(np.diff(solution_) != 0))
    return objective


def solve_chrom(scores, budget, gamma, selection_penalty=None, max_iter=60, solver=None):
    """`solveChromROCCO`: (solution, dict of the numeric results).  solver: a `csolveChromROCCOExact`."""
    if solver is None:
        import twin_rocco

        solver = twin_rocco.csolveChromROCCOExact
    scores_ = np.asarray(scores, np.float64)
    solution, objective, penalized, count, penalty = solver(scores_, budget=budget, gamma=float(gamma),
                                                            selectionPenalty=selection_penalty, maxIter=int(max_iter))
    used, target = False, None
    if budget is not None and selection_penalty is None:
        budget_ = float(budget)
        if np.isfinite(budget_):
            target = int(min(max(math.floor(scores_.size * budget_), 0), scores_.size))
        if int(count) == 0 and target is not None and target > 0:
            mask, ok = best_window(scores_, target, 0.0, gamma, max_relative_range=0.05)
            if ok:
                solution = mask.astype(np.uint8)
                count = int(np.sum(solution))
                objective = objective_for_solution(scores_, solution, gamma)
                penalized = float(objective) - float(penalty) * float(count)
                used = True
    return np.asarray(solution, np.uint8), {"objective": float(objective), "penalized_objective": float(penalized),
                                            "selected_count": int(count), "selection_penalty": float(penalty),
                                            "budget_target_count": target, "budget_fallback_window": bool(used)}


def first_pass(score, *, dependence_span, threshold_z, threshold_z_grid, num_bootstrap, random_seed, gamma, gamma_scale,
               selection_penalty=None, max_gap_bins=0, floors=None):
    """peaks.py:6700-6833 for one chromosome's score track up to the first-pass solution, composed of the twins: the null
    (twin_null), the panel (twin_dwb), the budget, gamma, the wrapped solve (twin_rocco) and the run bounds."""
    import twin_dwb
    import twin_null
    import twin_rocco

    score = np.asarray(score, np.float64)
    span = max(int(dependence_span), 2)
    null = twin_null.plain_all(score)
    grid = resolve_z_grid(threshold_z, threshold_z_grid)
    views = twin_dwb.panel(score, null["template"], null["null_center"], null["null_scale"], z_grid=grid, bandwidth=span,
                           num_bootstrap=num_bootstrap, seed=random_seed, cal_q=0.9, floors=floors, fast=True)
    b = budget(score, views, statistic="occupancy", threshold_z=threshold_z, threshold_z_grid=grid, dependence_span=span)
    g, gd = estimate_gamma(score, dependence_span=span, gamma_span=span, gamma=gamma, gamma_scale=gamma_scale,
                           null_center=b["null_center"], threshold=b["threshold"])
    solution, d = solve_chrom(score, b["budget"], g, selection_penalty)
    starts, ends = twin_rocco.cBooleanRunBounds(solution, max_gap_bins)
    d.update(gamma=g, budget=b["budget"], budget_details=b, gamma_details=gd, solution=solution,
             starts=np.asarray(starts, np.int64), ends=np.asarray(ends, np.int64), panel=views)
    return d
