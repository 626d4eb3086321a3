"""The dense observation-variance ("munc") seed natives on the device: drop-ins for the reference's
`cMuncObservationMomentSeedPass` (pyx:5042-5351) and `cMuncSmoothDenseLocalEvidence` (pyx:5642-5741).

Same argument names, defaults, coercions, return forms and `ValueError` texts (in the reference's order) as the originals.  The
kernels (csrc/csr_munc.h) use float64 + - * /, comparisons and float32 casts only, so every output element equals the reference's
bit for bit.  Invalid cells are found by the kernel (a flag reduction) and answered with the reference's text.  No CPU fallback.

The drop-ins move whole (m, n) arrays over the bus and are the pinning device for the kernels; the product is the resident form
(`DeviceBatch.munc_seed_*`), which runs the same kernels on arrays that stay on the device between the rounds of the seed loop.
`last_smooth_fallback_rows` says how many rows of the last `cMuncSmoothDenseLocalEvidence` call were redone whole, a wavefront per row
(an add or subtract of the running sum was inexact; csrc/csr_munc.h)."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib as L

F32_MAX = 3.4028234663852886e38
last_smooth_fallback_rows = 0


def _f32(x) -> float:
    """A Cython `float` argument: the Python float rounded to float32 (pyx:5052-5062)."""
    return float(np.float32(x))


def _u8p(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint8))


def seed_cfg(pad, studentTdf, dOmega, omegaMin, omegaMax, varianceFloor, varianceCap, useWeights, studentT, updateWeights):
    """The parameter checks of pyx:5116-5132 in their order, and the C record."""
    if pad < 0.0 or not math.isfinite(pad):
        raise ValueError("pad must be finite and nonnegative")
    if varianceFloor <= 0.0 or not math.isfinite(varianceFloor):
        raise ValueError("varianceFloor must be positive and finite")
    if not math.isfinite(varianceCap) or varianceCap < varianceFloor:
        raise ValueError("varianceCap must be greater than or equal to varianceFloor")
    if useWeights and studentT and (studentTdf <= 0.0 or dOmega <= 0.0 or not math.isfinite(studentTdf)
                                    or not math.isfinite(dOmega) or omegaMin <= 0.0 or omegaMax < omegaMin
                                    or not math.isfinite(omegaMin) or not math.isfinite(omegaMax)):
        raise ValueError("seed weight parameters are invalid")
    return L.MuncSeedCfg(pad, studentTdf, dOmega, omegaMin, omegaMax, varianceFloor, varianceCap, int(bool(useWeights)),
                         int(bool(studentT)), int(bool(updateWeights)), 0)


def cMuncObservationMomentSeedPass(matrixData, matrixMunc, stateMean, stateVariance, background=None, gVariance=None,
                                   countFloor=None, omegaIn=None, rhoIn=None, pad=1.0e-4, studentTdf=8.0, useSeedWeights=True,
                                   updateWeights=True, omegaMin=0.01, omegaMax=100.0, varianceFloor=1.0e-12,
                                   varianceCap=F32_MAX, enabled=True, studentT=True, dOmega=8.0, activeMask=None):
    """pyx:5042-5351: (moment, rhoOut, omegaRaw, omegaOut, local, variance) of one seed pass."""
    from .cconsenrich import _typed

    matrixData = _typed(matrixData, "matrixData", np.float32, 2)
    matrixMunc = _typed(matrixMunc, "matrixMunc", np.float32, 2)
    stateMean = _typed(stateMean, "stateMean", np.float32, 1)
    stateVariance = _typed(stateVariance, "stateVariance", np.float32, 1)
    pad, studentTdf, omegaMin, omegaMax = _f32(pad), _f32(studentTdf), _f32(omegaMin), _f32(omegaMax)
    varianceFloor, varianceCap, dOmega = _f32(varianceFloor), _f32(varianceCap), _f32(dOmega)
    m, n = matrixData.shape
    useWeights = bool(enabled) and bool(useSeedWeights)
    studentT, updateWeights = bool(studentT), bool(updateWeights)
    if matrixMunc.shape[0] != m or matrixMunc.shape[1] != n:
        raise ValueError("matrixMunc shape must match matrixData shape")
    if stateMean.shape[0] != n:
        raise ValueError("stateMean length must match interval count")
    if stateVariance.shape[0] != n:
        raise ValueError("stateVariance length must match interval count")
    cfg = seed_cfg(pad, studentTdf, dOmega, omegaMin, omegaMax, varianceFloor, varianceCap, useWeights, studentT, updateWeights)
    bg = gv = cf = om = rho = mask = None
    mode = 0
    if background is not None:
        bg = np.ascontiguousarray(background, dtype=np.float32).reshape(-1)
        if bg.shape[0] != n:
            raise ValueError("background length must match interval count")
    if gVariance is not None:
        gv = np.ascontiguousarray(gVariance, dtype=np.float32).reshape(-1)
        if gv.shape[0] != n:
            raise ValueError("gVariance length must match interval count")
    if countFloor is not None:
        cf = np.ascontiguousarray(countFloor, dtype=np.float32)
        if cf.ndim != 2:
            raise ValueError(f"Buffer has wrong number of dimensions (expected 2, got {cf.ndim})")
        if cf.shape[0] != m or cf.shape[1] != n:
            raise ValueError("countFloor shape must match matrixData shape")
    if omegaIn is not None:
        om = np.ascontiguousarray(omegaIn, dtype=np.float32)
        if om.ndim != 1:
            raise ValueError("omegaIn must be one-dimensional")
        if om.shape[0] != n:
            raise ValueError("omegaIn length must match interval count")
    if rhoIn is not None:
        rho = np.ascontiguousarray(rhoIn, dtype=np.float32)
        if rho.ndim != 2:
            raise ValueError(f"Buffer has wrong number of dimensions (expected 2, got {rho.ndim})")
        if rho.shape[0] != m or rho.shape[1] != n:
            raise ValueError("rhoIn shape must match matrixData shape")
    if activeMask is not None:
        mask = np.ascontiguousarray(activeMask, dtype=np.uint8)
        if mask.ndim == 1:
            if mask.shape[0] != n:
                raise ValueError("activeMask length must match interval count")
            mode = 1
        elif mask.ndim == 2:
            if mask.shape[0] != m or mask.shape[1] != n:
                raise ValueError("activeMask shape must match matrixData shape")
            mode = 2
        else:
            raise ValueError("activeMask must be one- or two-dimensional")
    moment, rhoOut = np.empty((m, n), np.float32), np.empty((m, n), np.float32)
    omegaRaw, omegaOut = np.empty(n, np.float32), np.empty(n, np.float32)
    local, variance = np.empty((m, n), np.float32), np.empty((m, n), np.float32)
    if m == 0 or n == 0:
        return moment, rhoOut, omegaRaw, omegaOut, local, variance
    L.require_gpu()
    L.check_value(L.lib().csr_munc_seed_pass(m, n, L.fp(matrixData), L.fp(matrixMunc), L.fp(stateMean), L.fp(stateVariance),
                                             L.fp(bg), L.fp(gv), L.fp(cf), L.fp(om), L.fp(rho), _u8p(mask), mode, C.byref(cfg),
                                             L.fp(moment), L.fp(rhoOut), L.fp(omegaRaw), L.fp(omegaOut), L.fp(local),
                                             L.fp(variance)))
    return moment, rhoOut, omegaRaw, omegaOut, local, variance


def cMuncSmoothDenseLocalEvidence(localEvidence, windowIntervals, excludeMask=None, eps=1.0e-12):
    """pyx:5642-5741: the rolling mean of every row over the non-excluded cells of a clamped window."""
    global last_smooth_fallback_rows
    from .cconsenrich import _typed

    localEvidence = _typed(localEvidence, "localEvidence", np.float32, 2)
    windowIntervals = int(windowIntervals)
    if not -(1 << 63) <= windowIntervals < (1 << 63):
        raise OverflowError("Python int too large to convert to C ssize_t")
    eps = _f32(eps)
    m, n = localEvidence.shape
    if windowIntervals < 1:
        raise ValueError("windowIntervals must be positive")
    if eps <= 0.0 or not math.isfinite(eps):
        raise ValueError("eps must be positive and finite")
    mask, mode = None, 0
    if excludeMask is not None:
        mask = np.ascontiguousarray(excludeMask, dtype=np.uint8)
        if mask.ndim == 1:
            if mask.shape[0] != n:
                raise ValueError("excludeMask length must match interval count")
            mode = 1
        elif mask.ndim == 2:
            if mask.shape[0] != m or mask.shape[1] != n:
                raise ValueError("excludeMask shape must match localEvidence shape")
            mode = 2
        else:
            raise ValueError("excludeMask must be one- or two-dimensional")
    out = np.empty((m, n), np.float32)
    last_smooth_fallback_rows = 0
    if m == 0 or n == 0:
        return out
    L.require_gpu()
    fb = C.c_int64(0)
    L.check_value(L.lib().csr_munc_smooth_local(m, n, L.fp(localEvidence), windowIntervals, _u8p(mask), mode, eps, L.fp(out),
                                                C.byref(fb)))
    last_smooth_fallback_rows = int(fb.value)
    return out
