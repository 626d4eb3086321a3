"""Pure NumPy / Python twin of the dense observation-variance seed natives and of the seed loop's per-cell glue.

Two forms, like the other twins:
  * the reference's steps -- `cMuncObservationMomentSeedPass` (pyx:4767-5351) and `cMuncSmoothDenseLocalEvidence` (pyx:5547-5741)
    restated cell by cell in Python floats (IEEE doubles) with float32 casts where the reference casts;
  * the device's decomposition (csrc/csr_munc.h) -- `seed_pass_device`: one lane per interval, vectorised over the intervals,
    tracks in order, the float32-rounded (moment, rho) pair carried from the first sweep to the second; `smooth_device`: rows cut
    into blocks of ROLL_BLOCK intervals that start from the in-order window sum, every add and subtract checked with the TwoSum
    residual, and the rows with an inexact block redone whole through the closed form of the reference's walk.  It returns the
    rows redone.
tests/test_munc_twin.py holds the two forms to each other and the first to the compiled reference's fixtures."""
from __future__ import annotations

import math

import numpy as np

F32 = np.float32
F32_MAX = 3.4028234663852886e38
ROLL_BLOCK = 128
SEED_INVALID = "active MUNC seed cells must be finite with positive denominators"
LOCAL_INVALID = "active local evidence cells must be positive and finite"


def _f32(x):
    return float(F32(x))


def _typed(a, ndim):
    if not isinstance(a, np.ndarray) or a.dtype != np.float32 or a.ndim != ndim or not a.flags.c_contiguous:
        raise ValueError("typed buffer mismatch")
    return a


# ---------------------------------------------------------------------------------------------------------------
# the wrapper of pyx:5042-5232: coercions and ValueErrors in the reference's order
# ---------------------------------------------------------------------------------------------------------------
def _seed_arguments(matrixData, matrixMunc, stateMean, stateVariance, background, gVariance, countFloor, omegaIn, rhoIn, pad,
                    studentTdf, useSeedWeights, updateWeights, omegaMin, omegaMax, varianceFloor, varianceCap, enabled, studentT,
                    dOmega, activeMask):
    data, munc = _typed(matrixData, 2), _typed(matrixMunc, 2)
    mean, var = _typed(stateMean, 1), _typed(stateVariance, 1)
    m, n = data.shape
    p = dict(pad=_f32(pad), dS=_f32(studentTdf), dOmega=_f32(dOmega), omegaMin=_f32(omegaMin), omegaMax=_f32(omegaMax),
             floor=_f32(varianceFloor), cap=_f32(varianceCap), useWeights=bool(enabled) and bool(useSeedWeights),
             studentT=bool(studentT), updateWeights=bool(updateWeights))
    if munc.shape != (m, n):
        raise ValueError("matrixMunc shape must match matrixData shape")
    if mean.shape[0] != n:
        raise ValueError("stateMean length must match interval count")
    if var.shape[0] != n:
        raise ValueError("stateVariance length must match interval count")
    if p["pad"] < 0.0 or not math.isfinite(p["pad"]):
        raise ValueError("pad must be finite and nonnegative")
    if p["floor"] <= 0.0 or not math.isfinite(p["floor"]):
        raise ValueError("varianceFloor must be positive and finite")
    if not math.isfinite(p["cap"]) or p["cap"] < p["floor"]:
        raise ValueError("varianceCap must be greater than or equal to varianceFloor")
    if p["useWeights"] and p["studentT"] and (
            p["dS"] <= 0.0 or p["dOmega"] <= 0.0 or not math.isfinite(p["dS"]) or not math.isfinite(p["dOmega"])
            or p["omegaMin"] <= 0.0 or p["omegaMax"] < p["omegaMin"] or not math.isfinite(p["omegaMin"])
            or not math.isfinite(p["omegaMax"])):
        raise ValueError("seed weight parameters are invalid")
    bg = gv = cf = om = rho = mask = None
    mode = 0
    if background is not None:
        bg = np.ascontiguousarray(background, dtype=F32).reshape(-1)
        if bg.shape[0] != n:
            raise ValueError("background length must match interval count")
    if gVariance is not None:
        gv = np.ascontiguousarray(gVariance, dtype=F32).reshape(-1)
        if gv.shape[0] != n:
            raise ValueError("gVariance length must match interval count")
    if countFloor is not None:
        cf = np.ascontiguousarray(countFloor, dtype=F32)
        if cf.shape != (m, n):
            raise ValueError("countFloor shape must match matrixData shape")
    if omegaIn is not None:
        om = np.ascontiguousarray(omegaIn, dtype=F32)
        if om.ndim != 1:
            raise ValueError("omegaIn must be one-dimensional")
        if om.shape[0] != n:
            raise ValueError("omegaIn length must match interval count")
    weighted = p["useWeights"] and p["studentT"]
    if rhoIn is None and weighted and not p["updateWeights"]:
        rho = np.ones((m, n), F32)
    elif rhoIn is not None:
        rho = np.ascontiguousarray(rhoIn, dtype=F32)
        if rho.shape != (m, n):
            raise ValueError("rhoIn shape must match matrixData shape")
    if activeMask is not None:
        mask = np.ascontiguousarray(activeMask, dtype=np.uint8)
        if mask.ndim == 1:
            if mask.shape[0] != n:
                raise ValueError("activeMask length must match interval count")
            mode = 1
        elif mask.ndim == 2:
            if mask.shape != (m, n):
                raise ValueError("activeMask shape must match matrixData shape")
            mode = 2
        else:
            raise ValueError("activeMask must be one- or two-dimensional")
    active = np.ones((m, n), bool) if mode == 0 else (np.broadcast_to(mask != 0, (m, n)) if mode == 1 else mask != 0)
    p["weighted"] = weighted
    return data, munc, mean, var, bg, gv, cf, om, rho, np.ascontiguousarray(active), p


def _seed_validate(data, munc, mean, var, bg, gv, cf, om, rho, active, p):
    """pyx:4767-4840 as one predicate over the active cells (the text carries no index)."""
    fin = np.isfinite
    with np.errstate(all="ignore"):
        per_interval = fin(mean.astype(np.float64)) & fin(var.astype(np.float64))
        if bg is not None:
            per_interval &= fin(bg)
        if gv is not None:
            per_interval &= fin(gv)
        base = munc.astype(np.float64) + p["pad"]
        ok = per_interval[None, :] & fin(data) & fin(base) & (base > 0.0)
        if cf is not None:
            ok &= fin(cf) & (cf >= 0.0)
        if p["weighted"]:
            if om is not None:
                ok &= (fin(om) & (om > 0.0))[None, :]
            if not p["updateWeights"]:
                ok &= fin(rho) & (rho > 0.0)
    if np.any(active & ~ok):
        raise ValueError(SEED_INVALID)


def _clamp(v, lo, hi):
    return lo if v < lo else (hi if v > hi else v)


def _cascade(local, count, floor, cap, floor_first):
    if floor_first:
        total = local + count
        if local < floor:
            local = floor
            total = local + count
    else:
        if local < floor:
            local = floor
        total = local + count
    if total > cap:
        total = cap
        local = total - count
        if local < floor:
            local = floor
            total = local + count
    return local, total


def cMuncObservationMomentSeedPass(matrixData, matrixMunc, stateMean, stateVariance, background=None, gVariance=None,
                                   countFloor=None, omegaIn=None, rhoIn=None, pad=1.0e-4, studentTdf=8.0, useSeedWeights=True,
                                   updateWeights=True, omegaMin=0.01, omegaMax=100.0, varianceFloor=1.0e-12,
                                   varianceCap=F32_MAX, enabled=True, studentT=True, dOmega=8.0, activeMask=None):
    """The reference's steps (pyx:4843-5039), cell by cell."""
    args = _seed_arguments(matrixData, matrixMunc, stateMean, stateVariance, background, gVariance, countFloor, omegaIn, rhoIn,
                           pad, studentTdf, useSeedWeights, updateWeights, omegaMin, omegaMax, varianceFloor, varianceCap,
                           enabled, studentT, dOmega, activeMask)
    _seed_validate(*args)
    data, munc, mean, var, bg, gv, cf, om, rho, active, p = args
    m, n = data.shape
    moment, rhoOut = np.empty((m, n), F32), np.empty((m, n), F32)
    omegaRaw, omegaOut = np.empty(n, F32), np.empty(n, F32)
    local, variance = np.empty((m, n), F32), np.empty((m, n), F32)
    padv, dS, dOm, floor, cap = p["pad"], p["dS"], p["dOmega"], p["floor"], p["cap"]
    weighted = p["weighted"]
    with np.errstate(all="ignore"):
        for k in range(n):
            state = float(mean[k])
            mvb = float(var[k])
            bgv = float(bg[k]) if bg is not None else 0.0
            if gv is not None:
                mvb += float(gv[k])
            if mvb < 0.0:
                mvb = 0.0
            omega = 1.0
            if weighted:
                omega_in = float(om[k]) if om is not None else 1.0
                if p["updateWeights"]:
                    dbar, cnt = 0.0, 0
                    for j in range(m):
                        if not active[j, k]:
                            moment[j, k], rhoOut[j, k] = 0.0, 1.0
                            continue
                        base = float(munc[j, k]) + padv
                        if base < floor:
                            base = floor
                        r = float(data[j, k]) - bgv - state
                        mo = r * r + mvb
                        moment[j, k] = F32(mo)
                        rhoOut[j, k] = F32((dS + 1.0) / (dS + omega_in * mo / base))
                        dbar += mo / base
                        cnt += 1
                    if cnt > 0:
                        dbar = dbar / float(cnt)
                        raw = (dOm + 1.0) / (dOm + dbar)
                        omega = _clamp(raw, p["omegaMin"], p["omegaMax"])
                    else:
                        raw, omega = 1.0, 1.0
                else:
                    raw = omega_in
                    omega = _clamp(raw, p["omegaMin"], p["omegaMax"])
                    for j in range(m):
                        if not active[j, k]:
                            moment[j, k], rhoOut[j, k] = 0.0, 1.0
                            continue
                        r = float(data[j, k]) - bgv - state
                        moment[j, k] = F32(r * r + mvb)
                        rhoOut[j, k] = rho[j, k]
                omegaRaw[k], omegaOut[k] = F32(raw), F32(omega)
            else:
                omegaRaw[k], omegaOut[k] = 1.0, 1.0
            for j in range(m):
                count = float(cf[j, k]) if cf is not None else 0.0
                if active[j, k]:
                    if not weighted:
                        r = float(data[j, k]) - bgv - state
                        mo = r * r + mvb
                        moment[j, k], rhoOut[j, k] = F32(mo), 1.0
                        lv = mo - padv - count
                    else:       # the float32 values just written are read back
                        lv = omega * float(rhoOut[j, k]) * float(moment[j, k]) - padv - count
                    lv, tv = _cascade(lv, count, floor, cap, True)
                else:
                    lv, tv = _cascade(float(munc[j, k]) - count, count, floor, cap, False)
                    moment[j, k], rhoOut[j, k] = 0.0, 1.0
                local[j, k], variance[j, k] = F32(lv), F32(tv)
    return moment, rhoOut, omegaRaw, omegaOut, local, variance


def seed_pass_device(matrixData, matrixMunc, stateMean, stateVariance, **kw):
    """The device's decomposition: every interval at once, the tracks in order, float64 arrays for the lanes' doubles."""
    names = ("background", "gVariance", "countFloor", "omegaIn", "rhoIn", "pad", "studentTdf", "useSeedWeights", "updateWeights",
             "omegaMin", "omegaMax", "varianceFloor", "varianceCap", "enabled", "studentT", "dOmega", "activeMask")
    defaults = (None, None, None, None, None, 1.0e-4, 8.0, True, True, 0.01, 100.0, 1.0e-12, F32_MAX, True, True, 8.0, None)
    full = [kw.get(k, d) for k, d in zip(names, defaults)]
    args = _seed_arguments(matrixData, matrixMunc, stateMean, stateVariance, *full)
    _seed_validate(*args)
    data, munc, mean, var, bg, gv, cf, om, rho, active, p = args
    m, n = data.shape
    f64 = np.float64
    padv, dS, dOm, floor, cap = p["pad"], p["dS"], p["dOmega"], p["floor"], p["cap"]
    weighted, update = p["weighted"], p["updateWeights"]
    moment, rhoOut = np.zeros((m, n), F32), np.ones((m, n), F32)
    local, variance = np.empty((m, n), F32), np.empty((m, n), F32)
    with np.errstate(all="ignore"):
        state = mean.astype(f64)
        mvb = var.astype(f64)
        bgv = bg.astype(f64) if bg is not None else np.zeros(n)
        if gv is not None:
            mvb = mvb + gv.astype(f64)
        mvb = np.where(mvb < 0.0, 0.0, mvb)
        omega = np.ones(n)
        raw = np.ones(n)
        if weighted:
            omega_in = om.astype(f64) if om is not None else np.ones(n)
            if update:
                dbar, cnt = np.zeros(n), np.zeros(n, np.int64)
                for j in range(m):
                    base = munc[j].astype(f64) + padv
                    base = np.where(base < floor, floor, base)
                    r = data[j].astype(f64) - bgv - state
                    mo = r * r + mvb
                    rh = (dS + 1.0) / (dS + omega_in * mo / base)
                    a = active[j]
                    moment[j] = np.where(a, mo.astype(F32), F32(0.0))
                    rhoOut[j] = np.where(a, rh.astype(F32), F32(1.0))
                    dbar = np.where(a, dbar + mo / base, dbar)
                    cnt += a
                some = cnt > 0
                dbar = dbar / np.where(some, cnt, 1).astype(f64)
                raw = np.where(some, (dOm + 1.0) / (dOm + dbar), 1.0)
                omega = np.where(some, np.where(raw < p["omegaMin"], p["omegaMin"], np.where(raw > p["omegaMax"], p["omegaMax"], raw)),
                                 1.0)
            else:
                raw = omega_in
                omega = np.where(raw < p["omegaMin"], p["omegaMin"], np.where(raw > p["omegaMax"], p["omegaMax"], raw))
        for j in range(m):
            a = active[j]
            count = cf[j].astype(f64) if cf is not None else np.zeros(n)
            r = data[j].astype(f64) - bgv - state
            mo64 = r * r + mvb
            if not weighted:
                mo32, rh32 = mo64.astype(F32), np.ones(n, F32)
                lv = mo64 - padv - count
            else:
                mo32 = moment[j] if update else mo64.astype(F32)
                rh32 = rhoOut[j] if update else rho[j]
                lv = omega * rh32.astype(f64) * mo32.astype(f64) - padv - count
            # active: floor first; inactive: munc - count, floor, then the sum
            lv = np.where(a, lv, munc[j].astype(f64) - count)
            lv = np.where(lv < floor, floor, lv)
            tv = lv + count
            over = tv > cap
            tv = np.where(over, cap, tv)
            lv2 = np.where(over, tv - count, lv)
            refl = over & (lv2 < floor)
            lv2 = np.where(refl, floor, lv2)
            tv = np.where(refl, lv2 + count, tv)
            moment[j] = np.where(a, mo32, F32(0.0))
            rhoOut[j] = np.where(a, rh32, F32(1.0))
            local[j], variance[j] = lv2.astype(F32), tv.astype(F32)
    return moment, rhoOut, raw.astype(F32), omega.astype(F32), local, variance


# ---------------------------------------------------------------------------------------------------------------
# rolling mean
# ---------------------------------------------------------------------------------------------------------------
def _smooth_arguments(localEvidence, windowIntervals, excludeMask, eps):
    local = _typed(localEvidence, 2)
    window, eps = int(windowIntervals), _f32(eps)
    m, n = local.shape
    if window < 1:
        raise ValueError("windowIntervals must be positive")
    if eps <= 0.0 or not math.isfinite(eps):
        raise ValueError("eps must be positive and finite")
    excluded = np.zeros((m, n), bool)
    if excludeMask is not None:
        mask = np.ascontiguousarray(excludeMask, dtype=np.uint8)
        if mask.ndim == 1:
            if mask.shape[0] != n:
                raise ValueError("excludeMask length must match interval count")
            excluded = np.broadcast_to(mask != 0, (m, n))
        elif mask.ndim == 2:
            if mask.shape != (m, n):
                raise ValueError("excludeMask shape must match localEvidence shape")
            excluded = mask != 0
        else:
            raise ValueError("excludeMask must be one- or two-dimensional")
    with np.errstate(all="ignore"):
        if np.any(~excluded & ~(np.isfinite(local) & (local > 0.0))):
            raise ValueError(LOCAL_INVALID)
    return local, window, np.ascontiguousarray(excluded), eps


def _window(i, n, window):
    half = window // 2
    left = i - half if i >= half else 0
    right = left + window
    if right > n:
        right = n
        left = right - window if right >= window else 0
    return left, right


def _walk(row, ex, out, n, window, eps, i0, i1, left, right, s, count, check):
    """pyx:5600-5639 over [i0, i1) from the given state; check: count the inexact operations (TwoSum residual != 0)."""
    inexact = 0
    for i in range(i0, i1):
        tl, tr = _window(i, n, window)
        while right < tr:
            if not ex[right]:
                s, e = _two_sum(s, float(row[right]))
                inexact += check and e != 0.0
                count += 1
            right += 1
        while left < tl:
            if not ex[left]:
                s, e = _two_sum(s, -float(row[left]))
                inexact += check and e != 0.0
                count -= 1
            left += 1
        value = s / float(count) if count > 0 else float(row[i])
        if value < eps:
            value = eps
        out[i] = F32(value)
    return inexact


def _two_sum(a, b):
    t = a + b
    bb = t - a
    return t, (a - (t - bb)) + (b - bb)


def _entry(row, ex, n, window, i0):
    left, right = _window(i0 - 1, n, window)
    s, count, inexact = 0.0, 0, 0
    for k in range(left, right):
        if not ex[k]:
            s, e = _two_sum(s, float(row[k]))
            inexact += e != 0.0
            count += 1
    return left, right, s, count, inexact


def cMuncSmoothDenseLocalEvidence(localEvidence, windowIntervals, excludeMask=None, eps=1.0e-12):
    """The reference's steps: one running sum per row."""
    local, window, excluded, eps = _smooth_arguments(localEvidence, windowIntervals, excludeMask, eps)
    m, n = local.shape
    out = np.empty((m, n), F32)
    for j in range(m):
        _walk(local[j], excluded[j], out[j], n, window, eps, 0, n, 0, 0, 0.0, 0, False)
    return out


def _redo_row(row, ex, out, n, window, eps):
    """k_munc_roll_fix: the reference's walk in its closed form.  S_0 = the first window [0, min(W, n)) summed in index order, the
    value of intervals 0 .. W // 2; then n - W steps s = 1.. add cell s + W - 1 and subtract cell s - 1, in that order, the value
    of interval s + W // 2; the last sum stays to the row's end.  An excluded cell adds an exact + 0.0 and counts 0."""
    half = window // 2
    w0, steps = min(window, n), max(n - window, 0)
    x = np.where(ex, 0.0, row.astype(np.float64))
    live = (~ex).astype(np.int64)

    def store(i, s, c):
        value = s / float(c) if c > 0 else float(row[i])
        out[i] = F32(eps if value < eps else value)

    s, c = 0.0, 0
    for k in range(w0):
        s = s + float(x[k])
        c += int(live[k])
    for i in range(0, (min(half, n - 1) if steps > 0 else n - 1) + 1):
        store(i, s, c)
    for step in range(1, steps + 1):
        s = s + float(x[step + window - 1])
        s = s - float(x[step - 1])
        c += int(live[step + window - 1]) - int(live[step - 1])
        store(step + half, s, c)
    if steps > 0:
        for i in range(steps + half + 1, n):
            store(i, s, c)


def smooth_device(localEvidence, windowIntervals, excludeMask=None, eps=1.0e-12, block=ROLL_BLOCK):
    """The device's decomposition.  Returns (out, rows redone, non-zero residuals seen by the speculative blocks)."""
    local, window, excluded, eps = _smooth_arguments(localEvidence, windowIntervals, excludeMask, eps)
    m, n = local.shape
    out = np.empty((m, n), F32)
    redone = residuals = 0
    for j in range(m):
        row, ex = local[j], excluded[j]
        dirty = 0
        for b in range((n + block - 1) // block):
            i0, i1 = b * block, min((b + 1) * block, n)
            left, right, s, count, e_in = (0, 0, 0.0, 0, 0) if b == 0 else _entry(row, ex, n, window, i0)
            dirty += e_in + _walk(row, ex, out[j], n, window, eps, i0, i1, left, right, s, count, True)
        residuals += dirty
        if dirty:
            _redo_row(row, ex, out[j], n, window, eps)
            redone += 1
    return out, redone, residuals


# ---------------------------------------------------------------------------------------------------------------
# the per-cell glue of the loop, as the reference writes it
# ---------------------------------------------------------------------------------------------------------------
def seed_working_munc(total, omega, rho, g_variance, pad, use_weights):
    """consenrich.py:7482-7503."""
    base = np.asarray(total, dtype=np.float64) + float(pad)
    if use_weights:
        denom = np.maximum(np.asarray(omega, dtype=np.float64).reshape(1, -1) * np.asarray(rho, dtype=np.float64), 1.0e-12)
        working = base / denom
    else:
        working = base
    working = working + np.asarray(g_variance, dtype=np.float64).reshape(1, -1)
    working -= float(pad)
    return np.ascontiguousarray(np.maximum(working, 1.0e-12), dtype=F32)


def local_to_total_variance(local, count_floor, cap):
    """consenrich.py:7557-7576 (cap: None or <= 0 for none)."""
    total = np.asarray(local, dtype=F32)
    total = total.copy() if count_floor is None else np.ascontiguousarray(total + np.asarray(count_floor, dtype=F32), dtype=F32)
    if cap is not None and cap > 0.0:
        total = np.minimum(total, F32(float(cap)))
    return np.ascontiguousarray(np.maximum(total, F32(1.0e-12)), dtype=F32)


def response_weight(rho, omega, use_weights):
    """consenrich.py:7938-7945."""
    if not use_weights:
        return np.ones(np.asarray(rho).shape, F32)
    return np.ascontiguousarray(np.asarray(rho, dtype=F32) * np.asarray(omega, dtype=F32).reshape(1, -1), dtype=F32)


# ---------------------------------------------------------------------------------------------------------------
# the plain-C restatement (scripts/ubench/munc_cpu.c) behind the natives' signatures: the one-core yardstick of
# scripts/munc_seed_bench.py, held to the fixtures by tests/test_munc_twin.py
# ---------------------------------------------------------------------------------------------------------------
class CPort:
    def __init__(self, workdir):
        import ctypes as C
        import os
        import subprocess

        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        so = os.path.join(str(workdir), "libmunc_cpu.so")
        subprocess.check_call(["gcc", "-O3", "-fno-trapping-math", "-fno-math-errno", "-mtune=generic", "-ffp-contract=off", "-shared",
                               "-fPIC", "-o", so, os.path.join(root, "scripts", "ubench", "munc_cpu.c"), "-lm"])
        self.C, self.lib = C, C.CDLL(so)
        FP, UP, D = C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.c_double
        self.FP, self.UP = FP, UP
        self.lib.munc_cpu_seed_pass.argtypes = [C.c_long, C.c_long] + [FP] * 9 + [UP, C.c_int] + [D] * 7 + [C.c_int, C.c_int] + [FP] * 6
        self.lib.munc_cpu_smooth.argtypes = [C.c_long, C.c_long, FP, C.c_long, UP, C.c_int, D, FP]
        self.__name__ = "munc_cpu.c"

    def _fp(self, a):
        return None if a is None else a.ctypes.data_as(self.FP)

    def cMuncObservationMomentSeedPass(self, matrixData, matrixMunc, stateMean, stateVariance, background=None, gVariance=None,
                                       countFloor=None, omegaIn=None, rhoIn=None, pad=1.0e-4, studentTdf=8.0, useSeedWeights=True,
                                       updateWeights=True, omegaMin=0.01, omegaMax=100.0, varianceFloor=1.0e-12,
                                       varianceCap=F32_MAX, enabled=True, studentT=True, dOmega=8.0, activeMask=None):
        data, munc, mean, var, bg, gv, cf, om, rho, _active, p = _seed_arguments(
            matrixData, matrixMunc, stateMean, stateVariance, background, gVariance, countFloor, omegaIn, rhoIn, pad, studentTdf,
            useSeedWeights, updateWeights, omegaMin, omegaMax, varianceFloor, varianceCap, enabled, studentT, dOmega, activeMask)
        m, n = data.shape
        mask = None if activeMask is None else np.ascontiguousarray(activeMask, dtype=np.uint8)
        outs = [np.empty((m, n), F32), np.empty((m, n), F32), np.empty(n, F32), np.empty(n, F32), np.empty((m, n), F32),
                np.empty((m, n), F32)]
        rc = self.lib.munc_cpu_seed_pass(m, n, self._fp(data), self._fp(munc), self._fp(mean), self._fp(var), self._fp(bg), self._fp(gv),
                                         self._fp(cf), self._fp(om), self._fp(rho), None if mask is None else mask.ctypes.data_as(self.UP),
                                         0 if mask is None else mask.ndim, p["pad"], p["dS"], p["dOmega"], p["omegaMin"], p["omegaMax"],
                                         p["floor"], p["cap"], int(p["weighted"]), int(p["updateWeights"]), *(self._fp(o) for o in outs))
        if rc:
            raise ValueError(SEED_INVALID)
        return tuple(outs)

    def cMuncSmoothDenseLocalEvidence(self, localEvidence, windowIntervals, excludeMask=None, eps=1.0e-12):
        local = _typed(localEvidence, 2)
        window, eps = int(windowIntervals), _f32(eps)
        if window < 1:
            raise ValueError("windowIntervals must be positive")
        if eps <= 0.0 or not math.isfinite(eps):
            raise ValueError("eps must be positive and finite")
        m, n = local.shape
        mask = None if excludeMask is None else np.ascontiguousarray(excludeMask, dtype=np.uint8)
        out = np.empty((m, n), F32)
        if self.lib.munc_cpu_smooth(m, n, self._fp(local), window, None if mask is None else mask.ctypes.data_as(self.UP),
                                    0 if mask is None else mask.ndim, eps, self._fp(out)):
            raise ValueError(LOCAL_INVALID)
        return out


# ---------------------------------------------------------------------------------------------------------------
# `_updateSeedBackground` (consenrich.py:7688-7777) on top of the oracle's background natives and solve (oracle/background.py)
# ---------------------------------------------------------------------------------------------------------------
def seed_background_inputs(data, mean, total, omega, rho, pad, use_weights):
    """(float32 invVar, float32 residual, float64 invVar) as the reference forms them."""
    base = np.asarray(total, dtype=np.float64) + float(pad)
    if use_weights:
        inv = np.asarray(omega, dtype=np.float64).reshape(1, -1) * np.asarray(rho, dtype=np.float64) / np.maximum(base, 1.0e-12)
    else:
        inv = 1.0 / np.maximum(base, 1.0e-12)
    res = np.asarray(data, dtype=F32) - np.asarray(mean, dtype=F32).reshape(1, -1)
    return np.ascontiguousarray(inv, dtype=F32), np.ascontiguousarray(res, dtype=F32), inv


def penalty_diagonal(n, lam_first, lam_second):
    """core.py:7506-7528 `_backgroundPenaltyDiagonal`."""
    diag = np.zeros(n, dtype=np.float64)
    if n >= 2 and lam_first > 0.0:
        diag[0] += lam_first
        diag[-1] += lam_first
        if n > 2:
            diag[1:-1] += 2.0 * lam_first
    if n >= 3 and lam_second > 0.0:
        if n == 3:
            diag += np.asarray([1.0, 4.0, 1.0], dtype=np.float64) * lam_second
        else:
            diag[0] += lam_second
            diag[-1] += lam_second
            diag[1] += 5.0 * lam_second
            diag[-2] += 5.0 * lam_second
            if n > 4:
                diag[2:-2] += 6.0 * lam_second
    return diag


def seed_g_variance(inv64, total, background, lam_first, lam_second, use_nonnegative, multiplier, mode):
    """consenrich.py:7723-7773: G given the new background."""
    n = inv64.shape[1]
    if mode == "disabled":
        nxt = np.zeros(n, dtype=F32)
    else:
        weight = np.sum(inv64, axis=0, dtype=np.float64)
        diagonal = weight + penalty_diagonal(n, float(lam_first), float(lam_second))
        mult = multiplier if use_nonnegative else None
        if mult is not None and float(mult) > 0.0:
            pos = weight[weight > 0.0]
            scale = float(np.median(pos)) if pos.size else 1.0
            diagonal[np.asarray(background) < 0.0] += float(mult) * max(scale, 1.0e-12)
        nxt = (1.0 / np.maximum(diagonal, 1.0e-12)).astype(F32)
    cap = float(np.quantile(np.asarray(total, dtype=np.float64), 0.99))
    if not np.isfinite(cap) or cap <= 0.0:
        cap = 1.0
    return np.minimum(np.maximum(np.asarray(nxt, dtype=F32), 0.0), F32(cap))


def update_seed_background(data, mean, total, omega, rho, pad, use_weights, *, lam_first, lam, zero_center=False, use_nonnegative=True,
                           negative_penalty_multiplier=1.0, g_uncertainty="proxy"):
    """(g float32, G float32, weight, rhs, info) of one chain; the solve is oracle.background.solve_background."""
    from oracle import background as bgo
    from oracle import oracle as orc

    inv32, res, inv64 = seed_background_inputs(data, mean, total, omega, rho, pad, use_weights)
    w, r, _support = orc.cbackgroundWeightedStatsWithSupport(res, inv32)
    g, info = bgo.solve_background(w, r, 0, zero_center=zero_center, use_nonnegative=use_nonnegative,
                                   multiplier=negative_penalty_multiplier, penalties_override=(lam_first, lam), return_info=True)
    g = np.ascontiguousarray(g, dtype=F32)
    G = seed_g_variance(inv64, total, g, lam_first, lam, use_nonnegative, negative_penalty_multiplier, g_uncertainty)
    return g, G, w, r, info
