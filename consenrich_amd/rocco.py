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

_I64_MAX = (1 << 63) - 1


def set_depth(depth: int) -> None:
    """Speculation depth D of the calibration for the calls of this module (1..8, 0 = default): 2^D - 1 penalties run side by
    side per round.  Changes speed only."""
    L.check(L.lib().csr_set_rocco_depth(None, int(depth)))


def _f64(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64).ravel(), dtype=np.float64)


def _c_int(v) -> int:
    """A Cython `int` argument: truncated like C, OverflowError outside int32 (pyx:8850-8851, 8882)."""
    v = int(v)
    if not -(1 << 31) <= v < (1 << 31):
        raise OverflowError("value too large to convert to int")
    return v


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
