"""CPU twin of the ROCCO natives: a pure-Python restatement of `csolvePenalizedChainROCCO`,
`ccalibrateSelectionPenaltyROCCO`, `csolveChromROCCOExact` (pyx:8603-8958), `cBooleanRunBounds` (pyx:9427-9457) and
`consenrichStateScoreTrack` (peaks.py:342-393).  Python floats are IEEE float64 and every operation below is written in the
reference's order, so the twin equals the compiled reference bit for bit (tests/golden/make_rocco_golden.py requires that
before it writes a fixture).  The GPU tests compare against this: the reference itself does not exist on the GPU machine."""
import math

import numpy as np


def _c_int(v):
    v = int(v)
    if not -(1 << 31) <= v < (1 << 31):
        raise OverflowError("value too large to convert to int")
    return v


def _f64(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64).ravel(), dtype=np.float64)


def _solve(s, cost, p):
    """`_solvePenalizedChainROCCO_F64`; s, cost: Python lists of floats."""
    n = len(s)
    if n == 1:
        v = s[0] - p
        if v > 0.0:
            return np.asarray([1], dtype=np.uint8), float(v), 1
        return np.asarray([0], dtype=np.uint8), 0.0, 0
    bt0 = bytearray(n)
    bt1 = bytearray(n)
    v0, c0 = 0.0, 0
    v1, c1 = s[0] - p, 1
    for i in range(1, n):
        c = cost[i - 1]
        sw0 = v1 - c
        if sw0 > v0 or (sw0 == v0 and c1 < c0):
            n0v, n0c = sw0, c1
            bt0[i] = 1
        else:
            n0v, n0c = v0, c0
        st1 = v1 + s[i] - p
        sw1 = v0 - c + s[i] - p
        if sw1 > st1 or (sw1 == st1 and c0 + 1 < c1 + 1):
            n1v, n1c = sw1, c0 + 1
        else:
            n1v, n1c = st1, c1 + 1
            bt1[i] = 1
        v0, c0, v1, c1 = n0v, n0c, n1v, n1c
    if v1 > v0 or (v1 == v0 and c1 < c0):
        best, cnt, state = v1, c1, 1
    else:
        best, cnt, state = v0, c0, 0
    sol = np.zeros(n, dtype=np.uint8)
    sol[n - 1] = state
    for i in range(n - 1, 0, -1):
        state = bt0[i] if state == 0 else bt1[i]
        sol[i - 1] = state
    return sol, float(best), int(cnt)


def _check(scores, costs):
    if scores.size == 0:
        raise ValueError("`scores` cannot be empty")
    if not np.all(np.isfinite(scores)):
        raise ValueError("`scores` contains non-finite values")
    if not np.all(np.isfinite(costs)):
        raise ValueError("`switchCosts` contains non-finite values")
    if scores.size > 1 and costs.size != scores.size - 1:
        raise ValueError("`switchCosts` must have length len(scores) - 1")


def csolvePenalizedChainROCCO(scores, switchCosts, selectionPenalty):
    scores, costs = _f64(scores), _f64(switchCosts)
    _check(scores, costs)
    return _solve(scores.tolist(), costs.tolist(), float(selectionPenalty))


def _calibrate(s, cost, target, maxIter):
    n = len(s)
    target = 0 if target < 0 else (n if target > n else target)
    if target == n:
        sol, val, cnt = _solve(s, cost, 0.0)
        return 0.0, sol, val, cnt
    lo = hi = s[0]
    ssum = 0.0
    for i in range(n):
        if s[i] < lo:
            lo = s[i]
        if s[i] > hi:
            hi = s[i]
        if i < n - 1:
            ssum += cost[i]
    lower = lo - ssum - 1.0
    upper = hi + ssum + 1.0
    _, _, lcnt = _solve(s, cost, lower)
    while lcnt <= target:
        lower -= max(1.0, abs(lower))
        _, _, lcnt = _solve(s, cost, lower)
    bsol, bval, bcnt = _solve(s, cost, upper)
    while bcnt > target:
        upper += max(1.0, abs(upper))
        bsol, bval, bcnt = _solve(s, cost, upper)
    for _ in range(max(maxIter, 1)):
        mid = (lower + upper) / 2.0
        sol, val, cnt = _solve(s, cost, mid)
        if cnt > target:
            lower = mid
        else:
            upper = mid
            bsol, bval, bcnt = sol, val, cnt
    return float(upper), bsol, float(bval), int(bcnt)


def ccalibrateSelectionPenaltyROCCO(scores, switchCosts, targetCount, maxIter=60):
    scores, costs = _f64(scores), _f64(switchCosts)
    targetCount, maxIter = _c_int(targetCount), _c_int(maxIter)
    _check(scores, costs)
    return _calibrate(scores.tolist(), costs.tolist(), targetCount, maxIter)


def csolveChromROCCOExact(scores, budget=None, gamma=0.5, selectionPenalty=None, maxIter=60):
    scores = _f64(scores)
    gamma, maxIter = float(gamma), _c_int(maxIter)
    if scores.size == 0:
        raise ValueError("`scores` cannot be empty")
    if not np.all(np.isfinite(scores)):
        raise ValueError("`scores` contains non-finite values")
    if (not math.isfinite(gamma)) or gamma < 0.0:
        raise ValueError("`gamma` must be finite and non-negative")
    n = scores.size
    s = scores.tolist()
    cost = [gamma] * (n - 1)
    if selectionPenalty is None:
        if budget is None:
            pen = 0.0
            sol, pval, cnt = _solve(s, cost, pen)
        else:
            budget_ = float(budget)
            if not math.isfinite(budget_):
                raise ValueError("`budget` must be finite")
            pen, sol, pval, cnt = _calibrate(s, cost, int(math.floor(n * budget_)), int(maxIter))
    else:
        pen = float(selectionPenalty)
        sol, pval, cnt = _solve(s, cost, pen)
    obj = 0.0
    sl = sol.tolist()
    for i in range(n):
        obj += s[i] * float(sl[i])
        if i < n - 1 and sl[i] != sl[i + 1]:
            obj -= cost[i]
    return sol, float(obj), float(pval), int(cnt), float(pen)


def cBooleanRunBounds(above, maxGapBins=0):
    arr = np.asarray(above, dtype=np.uint8).reshape(-1).tolist()
    starts, ends = [], []
    run, last = -1, -1
    gap = maxGapBins if maxGapBins > 0 else 0
    for i, a in enumerate(arr):
        if a != 0:
            if run < 0:
                run = i
            elif i - last > gap + 1:
                starts.append(run)
                ends.append(last)
                run = i
            last = i
    if run >= 0:
        starts.append(run)
        ends.append(last)
    return np.asarray(starts, dtype=np.int64), np.asarray(ends, dtype=np.int64)


def score_track(state, uncertainty=None, mode="state", z=1.0):
    """`consenrichStateScoreTrack` without its details record; state / uncertainty are widened to float64 first."""
    st = np.asarray(state, dtype=np.float64).ravel()
    if mode == "state":
        return st
    un = np.asarray(uncertainty, dtype=np.float64).ravel()
    if np.any(un < 0.0):
        raise ValueError("`uncertainty` must be non-negative for lower_confidence")
    raw = st - float(z) * un
    mx = float(np.max(st))
    if np.isfinite(mx) and mx > 0.0:
        return np.maximum(raw, float(-2.0 * mx))
    return raw
