"""The effective sample size scan behind the ROCCO budget on the device: a drop-in for the reference's
`cEstimateEffectiveSampleSize` (pyx:9160-9279), the budget policy that calls it (`_estimateBudgetForPreparedROCCOScore`,
peaks.py:1275-1516) and the scalar part of the gamma rule (`estimateROCCOGamma`, peaks.py:1694-1780) for the chains of a batch
whose score tracks are resident (`DeviceBatch.ess` / `rocco_budget` / `rocco_gamma`).

Same argument names, coercions, return tuple and `ValueError` texts as the original.  The mean, the variance sum and the
covariance sum of every lag are sequential walks on the device (csrc/csr_ess.h), in the reference's order with a separate multiply
and add; rho, the break / taper rule, tau and the clamps are composed from them by the C ABI (`csr_ess_scan`, `csr_batch_ess`) in
doubles.  Every number equals the reference's bit for bit.  No CPU fallback.

logPositive.  The logarithm is taken on the host, `math.log` per element -- the C library's `log`, which is what the reference's
native calls; NumPy's vectorised log is not guaranteed to round like it in the last bit.  The active values are validated in
index order on the way, with the reference's messages, before anything is uploaded.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib as L
from ._lib import _c_int

TINY = float(np.finfo(np.float64).tiny)         # peaks.py:73 `_TINY`
BUDGET_MIN, BUDGET_MAX = 0.001, 0.25            # constants.py `ROCCO_BUDGET_MIN`, `ROCCO_BUDGET_MAX` (peaks.py:74-75)
MAX_Z = 16
KINDS = {"occupancy": L.ESS_OCCUPANCY, "soft": L.ESS_SOFT, "integrated": L.ESS_INTEGRATED}


def cEstimateEffectiveSampleSize(values, maxLag, activeMask=None, logPositive=False, windowIntervals=0):
    """pyx:9160-9279: (n_eff, tau, lags_used) of the positive-autocorrelation scan.  Without a mask, a log and a window the
    reference's fast path runs (no finiteness checks); otherwise its general path (pair counts under the mask, Bartlett taper
    and clamp with a window).  With logPositive the logarithm is `math.log` per element on the host (see the module text)."""
    maxLag, windowIntervals = _c_int(maxLag), _c_int(windowIntervals)
    logPositive = bool(logPositive)
    x = np.ascontiguousarray(np.asarray(values, dtype=np.float64).reshape(-1), dtype=np.float64)
    n = x.shape[0]
    if windowIntervals < 0:
        raise ValueError("windowIntervals must be nonnegative")
    general = activeMask is not None or logPositive or windowIntervals != 0
    mask = None
    if general:
        if activeMask is not None:
            mask = np.ascontiguousarray(np.asarray(activeMask, dtype=np.uint8).reshape(-1), dtype=np.uint8)
            if mask.shape[0] != n:
                raise ValueError("activeMask length must match values length")
        if logPositive:
            x = x.copy()
            for i in (range(n) if mask is None else np.flatnonzero(mask)):
                v = float(x[i])
                if not math.isfinite(v) or v <= 0.0:
                    raise ValueError("active values must be positive finite")
                x[i] = math.log(v)
        else:
            live = x if mask is None else x[mask != 0]
            if not np.all(np.isfinite(live)):
                raise ValueError("active values must be finite")
        if (n if mask is None else int(np.count_nonzero(mask))) < 2:
            return float(n if mask is None else int(np.count_nonzero(mask))), 1.0, 0
    elif n < 2:
        return float(n), 1.0, 0
    L.require_gpu()
    out = L.EssOut()
    mp = None if mask is None else mask.ctypes.data_as(C.POINTER(C.c_uint8))
    L.check_value(L.lib().csr_ess_scan(L.dp(x), n, maxLag, mp, int(general), windowIntervals, C.byref(out)))
    return float(out.n_eff), float(out.tau), int(out.lags_used)


# ---------------------------------------------------------------------------------------------------------------
# the budget policy (peaks.py:1275-1516), scalar work on what dwb_panel returned
# ---------------------------------------------------------------------------------------------------------------
_INTEGRATED = {"integrated", "integrated_excess", "integrated_excess_tail", "excess"}
_OCCUPANCY = {"occupancy", "calibrated_occupancy", "calibrated_tail_occupancy", "tail_fraction", "fraction", "tail",
              "tail_occupancy"}
_SOFT = {"soft", "soft_occupancy", "soft_tail"}


def resolve_statistic(statistic) -> str:
    """peaks.py:1305-1326: the reference's name of the statistic an alias selects."""
    s = str(statistic).strip().lower().replace("-", "_")
    if s in _INTEGRATED:
        return "integrated_excess_tail"
    if s in _OCCUPANCY:
        return "tail_occupancy"
    if s in _SOFT:
        return "soft"
    raise ValueError(f"Unknown budget statistic: {statistic}")


SERIES_OF = {"tail_occupancy": "occupancy", "soft": "soft", "integrated_excess_tail": "integrated"}


def z_key(z) -> str:
    """peaks.py:288-290 `_thresholdZKey`."""
    return f"{float(z):.6f}".rstrip("0").rstrip(".")


def resolve_z_grid(threshold_z, threshold_z_grid) -> list:
    """peaks.py:293-309 `_resolveThresholdZGrid` (the grid is an argument here: the reference's default is its constant)."""
    values, seen = [], set()
    for value in [threshold_z, *threshold_z_grid]:
        v = float(max(float(value), 0.0))
        if z_key(v) not in seen:
            seen.add(z_key(v))
            values.append(v)
    values.sort()
    return values


def budget_policy(views, *, statistic, threshold_z, threshold_z_grid, budget_min, budget_max) -> dict:
    """The scalar part of peaks.py:1294-1434 for ONE chain.  views: the chain's list of per-z dicts as `dwb_panel` returns it (its
    order is the order of the reference's `thresholdMetrics`).  Returns the selected statistic, the primary view (the view of
    threshold_z, else that of the first z of the resolved grid), the views whose excess the integrated series averages (grid
    order), the three raw and clipped budgets and the budget of the statistic."""
    selected = resolve_statistic(statistic)
    grid = resolve_z_grid(threshold_z, threshold_z_grid)
    by_key = {z_key(v["threshold_z"]): v for v in views}
    lo = float(max(budget_min, 0.0))
    hi = float(max(budget_max, lo))
    primary = by_key.get(z_key(float(max(threshold_z, 0.0))))
    if primary is None:
        primary = by_key[z_key(grid[0])]
    integrated_raw = float(np.mean([float(v["budget_soft_raw"]) for v in views]))
    occ_raw, soft_raw = float(primary["budget_occupancy_raw"]), float(primary["budget_soft_raw"])
    out = {"statistic": selected, "primary": primary, "grid": grid,
           "budget_min": lo, "budget_max": hi, "budget_occupancy_raw": occ_raw, "budget_soft_raw": soft_raw,
           "budget_integrated_raw": integrated_raw, "budget_occupancy": float(np.clip(occ_raw, lo, hi)),
           "budget_soft": float(np.clip(soft_raw, lo, hi)), "budget_integrated": float(np.clip(integrated_raw, lo, hi))}
    name = SERIES_OF[selected]
    out["budget"], out["budget_raw"] = out[f"budget_{name}"], out[f"budget_{name}_raw"]
    # the integrated series reads the view of EVERY z of the grid (a KeyError in the reference if one is missing)
    out["series_views"] = [by_key[z_key(z)] for z in grid] if selected == "integrated_excess_tail" else [primary]
    return out


def gamma_reference_level(threshold, null_center):
    """peaks.py:1732-1739: the level the positive excess is measured from -- threshold, then null_center, then zero."""
    if threshold is not None and np.isfinite(float(threshold)):
        return float(threshold), "threshold"
    if null_center is not None and np.isfinite(float(null_center)):
        return float(null_center), "null_center"
    return 0.0, "zero"


def gamma_from_scale(positive_scale: float, *, span: int, gamma_span, gamma_scale, clip_min, clip_max, level, method) -> tuple:
    """peaks.py:1727-1780 after the median: (gamma, the numeric details and the two method names)."""
    span_ = max(int(span), 2)
    gamma_span_ = max(int(gamma_span), 2) if gamma_span is not None else span_
    raw = float(max(float(gamma_scale), 0.0) * float(gamma_span_) * positive_scale)
    g = float(max(raw, float(max(clip_min, 0.0))))
    if clip_max is not None:
        g = float(min(g, float(max(clip_max, clip_min))))
    d = {"method": "dependence_span_lower_score_scale", "dependence_span": span_, "gamma_span": gamma_span_,
         "dependence_span_lower": span_, "dependence_span_upper": span_, "reference_method": method,
         "reference_level": float(level), "positive_score_median": float(positive_scale), "gamma_scale": float(gamma_scale),
         "gamma_raw": raw, "gamma": g}
    if clip_max is not None:
        d["gamma_clip_max"] = float(max(clip_max, clip_min))
    d["gamma_clip_min"] = float(max(clip_min, 0.0))
    return g, d


def budget_details(policy: dict, threshold_z, span: int, ess) -> dict:
    """The numeric fields of the reference's `details` (peaks.py:1452-1510) from `statistic` through `ess_lags_used`, plus
    `budget`; the string-valued bookkeeping of the calibration is not reproduced."""
    p, m = policy, policy["primary"]
    n_eff, tau, lags = ess
    d = {"statistic": p["statistic"], "num_bootstrap": int(m["num_bootstrap"]), "null_quantile": float(m["null_quantile"]),
         "dependence_span": int(span), "threshold": float(m["threshold"]), "threshold_z": float(threshold_z),
         "threshold_z_grid": [float(z) for z in p["grid"]], "null_center": float(m["null_center"]),
         "null_scale": float(m["null_scale"])}
    for k in ("observed_tail_occupancy", "null_tail_occupancy", "null_tail_occupancy_calibrated", "null_tail_occupancy_sd",
              "observed_soft_tail", "null_soft_tail", "null_soft_tail_calibrated", "null_soft_tail_sd"):
        d[k] = float(m[k])
    d.update(budget_min=p["budget_min"], budget_max=p["budget_max"], budget_raw=float(p["budget_raw"]),
             budget_clipped=bool(abs(p["budget"] - p["budget_raw"]) > 1.0e-12),
             budget_occupancy_raw=p["budget_occupancy_raw"], budget_soft_raw=p["budget_soft_raw"],
             budget_integrated_raw=p["budget_integrated_raw"], budget_occupancy=p["budget_occupancy"],
             budget_soft=p["budget_soft"], budget_integrated=p["budget_integrated"],
             effective_count=float(p["budget"] * n_eff), effective_total_count=float(n_eff),
             autocorrelation_time=float(tau), ess_lags_used=int(lags), budget=float(p["budget"]))
    return d
