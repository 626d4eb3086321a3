"""Budgeted chain peak selection (ROCCO) on the device: drop-ins for the reference natives `csolvePenalizedChainROCCO`,
`ccalibrateSelectionPenaltyROCCO` (pyx:8719-8874) and `csolveChromROCCOExact` (pyx:8877-8958).

Same argument names, coercions (`ravel`, float64), return tuples (Python float / int, uint8 array) and `ValueError` texts as
the Cython originals; every check runs before any GPU call.  The arithmetic is one C-ABI call (`csr_rocco_solve`): each value
returned equals the reference's bit for bit (csrc/csr_rocco.h says why that rules out a scan over time and where the
parallelism comes from instead).  No CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib as L
from ._lib import _c_int, _f64

_I64_MAX = (1 << 63) - 1


def set_depth(depth: int) -> None:
    """Speculation depth D of the calibration for the calls of this module (1..8, 0 = default): 2^D - 1 penalties run side by
    side per round.  Changes speed only."""
    L.check(L.lib().csr_set_rocco_depth(None, int(depth)))


def _clip_i64(v) -> int:
    return max(-_I64_MAX, min(_I64_MAX, int(v)))


def target_count(n: int, budget: float) -> int:
    """`<Py_ssize_t>floor(n * budget)` of pyx:8929."""
    return _clip_i64(math.floor(n * budget))


def config(*, penalty=None, target=None, gamma=0.0, max_iter=60) -> L.RoccoCfg:
    """One chain's csr_rocco_cfg: a fixed penalty, or a target count to calibrate the penalty for."""
    g = L.RoccoCfg()
    g.max_iter = _c_int(max_iter)
    g.gamma = float(gamma)
    if target is None:
        g.mode, g.penalty, g.target_count = L.ROCCO_FIXED_PENALTY, float(penalty), 0
    else:
        g.mode, g.penalty, g.target_count = L.ROCCO_TARGET_COUNT, 0.0, _clip_i64(target)
    return g


def _solve_one(scores, costs, cfg):
    """(solution, csr_rocco_out) of one chain on host arrays; costs None = the constant cfg.gamma."""
    L.require_gpu()
    n = np.array([scores.size], np.int64)
    out = L.RoccoOut()
    sol = np.empty(scores.size, np.uint8)
    L.check(L.lib().csr_rocco_solve(1, n.ctypes.data_as(L.I64P), L.dp(scores), None if costs is None else L.dp(costs),
                                    C.byref(cfg), C.byref(out), sol.ctypes.data_as(C.POINTER(C.c_uint8))))
    return sol, out


def _check_chain(scoresArr, switchCostsArr):  # pyx:8732-8739 / 8861-8868
    if scoresArr.size == 0:
        raise ValueError("`scores` cannot be empty")
    if not np.all(np.isfinite(scoresArr)):
        raise ValueError("`scores` contains non-finite values")
    if not np.all(np.isfinite(switchCostsArr)):
        raise ValueError("`switchCosts` contains non-finite values")
    if scoresArr.size > 1 and switchCostsArr.size != scoresArr.size - 1:
        raise ValueError("`switchCosts` must have length len(scores) - 1")


def csolvePenalizedChainROCCO(scores, switchCosts, selectionPenalty):
    """pyx:8719-8740: (solution uint8, penalizedObjective, selectedCount)."""
    scoresArr, switchCostsArr = _f64(scores), _f64(switchCosts)
    selectionPenalty = float(selectionPenalty)
    _check_chain(scoresArr, switchCostsArr)
    costs = switchCostsArr if scoresArr.size > 1 else None       # a single bin has no transition (pyx:8643-8647)
    sol, out = _solve_one(scoresArr, costs, config(penalty=selectionPenalty))
    return sol, float(out.penalized_objective), int(out.selected_count)


def ccalibrateSelectionPenaltyROCCO(scores, switchCosts, targetCount, maxIter=60):
    """pyx:8847-8874: (selectionPenalty, solution uint8, penalizedObjective, selectedCount)."""
    scoresArr, switchCostsArr = _f64(scores), _f64(switchCosts)
    targetCount, maxIter = _c_int(targetCount), _c_int(maxIter)
    _check_chain(scoresArr, switchCostsArr)
    costs = switchCostsArr if scoresArr.size > 1 else None
    sol, out = _solve_one(scoresArr, costs, config(target=targetCount, max_iter=maxIter))
    return float(out.selection_penalty), sol, float(out.penalized_objective), int(out.selected_count)


def chrom_config(n, budget=None, gamma=0.5, selectionPenalty=None, maxIter=60) -> L.RoccoCfg:
    """The three modes of `csolveChromROCCOExact` (pyx:8917-8944) as one chain's config, with its checks."""
    gamma = float(gamma)
    if (not math.isfinite(gamma)) or gamma < 0.0:
        raise ValueError("`gamma` must be finite and non-negative")
    if selectionPenalty is not None:
        return config(penalty=float(selectionPenalty), gamma=gamma, max_iter=maxIter)
    if budget is None:
        return config(penalty=0.0, gamma=gamma, max_iter=maxIter)
    budget_ = float(budget)
    if not math.isfinite(budget_):
        raise ValueError("`budget` must be finite")
    return config(target=target_count(int(n), budget_), gamma=gamma, max_iter=maxIter)


def csolveChromROCCOExact(scores, budget=None, gamma=0.5, selectionPenalty=None, maxIter=60):
    """pyx:8877-8958: (solution uint8, objective, penalizedObjective, selectedCount, selectionPenalty)."""
    scoresArr = _f64(scores)
    gamma, maxIter = float(gamma), _c_int(maxIter)
    if scoresArr.size == 0:
        raise ValueError("`scores` cannot be empty")
    if not np.all(np.isfinite(scoresArr)):
        raise ValueError("`scores` contains non-finite values")
    cfg = chrom_config(scoresArr.size, budget, gamma, selectionPenalty, maxIter)
    sol, out = _solve_one(scoresArr, None, cfg)
    return (sol, float(out.objective), float(out.penalized_objective), int(out.selected_count),
            float(out.selection_penalty))


# ------------------------------------------------------------------------------------------------------------------
# the wrapper `solveChromROCCO` puts around the native (peaks.py:1804-1835): host steps of the rare chain that selected nothing
# ------------------------------------------------------------------------------------------------------------------
def budget_target_count(n: int, budget) -> int | None:
    """peaks.py:1806-1811: None when the budget is not finite."""
    b = float(budget)
    if not np.isfinite(b):
        return None
    return int(min(max(math.floor(int(n) * b), 0), int(n)))


def best_contiguous_budget_fallback_mask(scores, targetCount, selectionPenalty, gamma, maxRelativeRange=None):
    """peaks.py:3723-3760 `_bestContiguousBudgetFallbackMask` with the reference's NumPy steps: (mask, used)."""
    scores_ = np.asarray(scores, dtype=np.float64)
    n = int(scores_.size)
    target = int(min(max(int(targetCount), 1), n))
    out = np.zeros(n, dtype=bool)
    if n == 0 or target <= 0:
        return out, False
    adjusted = scores_ - float(selectionPenalty)
    cumsum = np.concatenate(([0.0], np.cumsum(adjusted, dtype=np.float64)))
    # the reference's loop keeps the FIRST start of the largest objective (strict '>'): np.argmax of the same floats
    window = cumsum[target:] - cumsum[: n - target + 1]
    starts = np.arange(n - target + 1)
    switches = (starts > 0).astype(np.float64) + (starts + target - 1 < n - 1).astype(np.float64)
    objective = window - float(max(float(gamma), 0.0)) * switches
    if np.any(np.isnan(objective)):
        finite = np.where(np.isnan(objective), -np.inf, objective)       # (a NaN never wins a '>' comparison)
    else:
        finite = objective
    bestStart = int(np.argmax(finite))
    bestObjective = float(finite[bestStart])
    if not np.isfinite(bestObjective) or bestObjective <= 0.0:
        return out, False
    if maxRelativeRange is not None:
        bestWindow = scores_[bestStart: bestStart + target]
        windowRange = float(np.max(bestWindow) - np.min(bestWindow))
        windowScale = float(max(np.max(np.abs(bestWindow)), 1.0e-6))
        if windowRange > float(max(float(maxRelativeRange), 0.0)) * windowScale:
            return out, False
    out[bestStart: bestStart + target] = True
    return out, True


def objective_for_solution(scores, solution, gamma) -> float:
    """peaks.py:2017-2031 `_roccoObjectiveForSolution`."""
    scores_ = np.asarray(scores, dtype=np.float64)
    solution_ = np.asarray(solution, dtype=np.uint8)
    objective = float(np.sum(scores_[solution_ > 0]))
    if solution_.size > 1:
        objective -= float(max(float(gamma), 0.0)) * float(np.sum(np.diff(solution_) != 0))
    return objective
