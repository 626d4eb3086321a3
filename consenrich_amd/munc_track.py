"""From the seed loop to a finished observation-variance matrix: the per-cell work of the reference between the dense seed loop
and `matrixMunc`, on the device (csrc/csr_munc_track.h), and the host work on the compact block records.

Drop-ins on host arrays, with the reference's signatures, defaults, coercions and `ValueError` texts in its order:
  cEvalPSplineLogVarianceTrend   pyx:5821-5894 (the de Boor evaluation of the pooled log-variance trend)
  cFinalizeMuncEBTrack           pyx:5445-5544 (floor / cap, shrinkage toward the prior, count floor, counters)
  eval_pspline_log_variance_trend  core.py:6628-6655
  get_munc_track                 core.py:8390-8880, the branch the CLI takes: a pooled trend, a prior mean track (or a prior
                                 variance track), a pooled Nu_0 and an effective Nu_L, and the `EB_use=False` branch
  apply_blacklist_munc_floor     core.py:7183-7222 with a non-negative minR
They move whole arrays over the bus and pin the kernels; the product is the resident form (`DeviceBatch.munc_block_sums`,
`munc_prior_track`, `munc_track_finish`, `driver.munc_track_batch`).  No CPU fallback.

Everything is bit for bit the reference's except what passes through the device's exp (the prior track: within one float32 ulp)
and log1p (the sum of q * predictor of a block).  The constant fallback of the trend is evaluated with the C library's exp.

`pooled_block_rows` is host work on the block records (consenrich.py:8041-8111).  Its `trigamma` defaults to SciPy's
polygamma(1, .); the reference takes it from the `itrigamma` package, and agreement with that package is unverified."""
from __future__ import annotations

import ctypes as C
import math
import operator

import numpy as np

from . import _lib as L

F32_MAX = 3.4028234663852886e38
NUMERIC_VARIANCE_FLOOR = 1.0e-12        # consenrich.py:453


def _f32(x) -> float:
    """A Cython `float` argument: the Python float rounded to float32 (infinite beyond its range)."""
    with np.errstate(over="ignore"):
        return float(np.float32(x))


def trend_fields(trend):
    """(knots, beta, degree, xMin, xMax) of a trend given as that tuple or as an object with those attributes."""
    if isinstance(trend, (tuple, list)):
        knots, beta, degree, x_min, x_max = trend
    else:
        knots, beta, degree, x_min, x_max = trend.knots, trend.beta, trend.degree, trend.xMin, trend.xMax
    return (np.asarray(knots, dtype=np.float64), np.asarray(beta, dtype=np.float64), int(degree), float(x_min), float(x_max))


def log_bounds(eps, max_variance):
    """(logFloor, logCap) of core.py:6634-6644."""
    floor = float(max(eps, 1.0e-12))
    if max_variance is None or not np.isfinite(float(max_variance)) or max_variance <= floor:
        cap = float(np.finfo(np.float32).max)
    else:
        cap = float(max_variance)
    return float(np.log(floor)), float(np.log(cap))


def munc_trend_predictor(values) -> np.ndarray:
    """core.py:6309-6315 on the host (NumPy's log1p), as the reference's callers of the native do."""
    arr = np.asarray(values, dtype=np.float64)
    with np.errstate(all="ignore"):
        out = np.sign(arr) * np.log1p(np.abs(arr))
    out[~np.isfinite(out)] = np.nan
    return out


def check_trend_limits(knots, beta, degree):
    """What the device can evaluate: the constant fallback, or degree <= 5, at most 512 basis functions and arrays long enough for
    every index the reference's loops form (it reads past them otherwise)."""
    if degree < 0 or knots.shape[0] == 0 or beta.shape[0] == 0:
        return
    if degree > L.MUNC_TRACK_MAX_DEGREE:
        raise ValueError(f"degree {degree}: the device evaluates B-splines up to degree {L.MUNC_TRACK_MAX_DEGREE}")
    if beta.shape[0] > L.MUNC_TRACK_MAX_BASIS:
        raise ValueError(f"{beta.shape[0]} basis functions: the device evaluates up to {L.MUNC_TRACK_MAX_BASIS}")
    if beta.shape[0] < degree + 1 or knots.shape[0] < beta.shape[0] + degree + 1:
        raise ValueError(f"knots and beta do not describe a B-spline of degree {degree}: need len(beta) >= degree + 1 and "
                         "len(knots) >= len(beta) + degree + 1")


def cEvalPSplineLogVarianceTrend(predictorTrack, knots, beta, degree, xMin, xMax, logFloor, logCap):
    """pyx:5821-5894: float32 exp of the clamped trend at every predictor value."""
    degree = operator.index(degree)
    if not -(1 << 31) <= degree < (1 << 31):
        raise OverflowError("value too large to convert to int")
    xMin, xMax, logFloor, logCap = float(xMin), float(xMax), float(logFloor), float(logCap)
    pred = np.ascontiguousarray(predictorTrack, dtype=np.float64).ravel()
    knots = np.ascontiguousarray(knots, dtype=np.float64).ravel()
    beta = np.ascontiguousarray(beta, dtype=np.float64).ravel()
    out = np.empty(pred.shape[0], dtype=np.float32)
    if pred.shape[0] == 0:
        return out
    check_trend_limits(knots, beta, degree)
    L.require_gpu()
    L.check_value(L.lib().csr_munc_eval_pspline(pred.shape[0], L.dp(pred), L.dp(knots), knots.shape[0], L.dp(beta), beta.shape[0],
                                                degree, xMin, xMax, logFloor, logCap, L.fp(out)))
    return out


def finalize_errors(res):
    """The error of the sequential loop of pyx:5393-5442 from the lowest invalid index of each kind: the lowest index raises, and
    at one index the local value is looked at first, then the prior, then the count floor."""
    kinds = (("localVarianceTrack must contain finite positive values at index {}", res["invalid_local"]),
             ("priorVarianceTrack must contain finite positive values at index {}", res["invalid_prior"]),
             ("countFloor must be nonnegative where finite at index {}", res["invalid_count_floor"]))
    hit = [(idx, order, text) for order, (text, idx) in enumerate(kinds) if idx >= 0]
    if hit:
        idx, _, text = min(hit)
        raise ValueError(text.format(idx))


def track_diagnostics(res, n, use_eb):
    """The native's diagnostics dict (pyx:5531-5544)."""
    return {"supportCount": int(res["support"]), "supportFraction": (float(res["support"]) / float(n)) if n > 0 else 0.0,
            "countFloorFiniteCount": int(res["floor_finite"]), "countFloorAddedCount": int(res["floor_added"]),
            "countFloorMissingCount": int(res["floor_missing"]), "finalShrinkagePairCount": int(n) if use_eb else 0,
            "finalShrinkagePairFraction": 1.0 if use_eb and n > 0 else 0.0}


def _out_dict(o):
    return {k: getattr(o, k) for k, _ in L.MuncTrackOut._fields_}


def cFinalizeMuncEBTrack(localVarianceTrack, priorVarianceTrack=None, countFloor=None, nuLocal=0.0, nuPrior=0.0,
                         varianceFloor=1.0e-12, varianceCap=F32_MAX, useEB=True):
    """pyx:5445-5544: (float32 track, diagnostics dict)."""
    nuLocal, nuPrior, varianceFloor, varianceCap = _f32(nuLocal), _f32(nuPrior), _f32(varianceFloor), _f32(varianceCap)
    useEB = bool(useEB)
    posterior = nuLocal + nuPrior
    local = np.ascontiguousarray(localVarianceTrack, dtype=np.float32).reshape(-1)
    n = local.shape[0]
    if varianceFloor <= 0.0 or not math.isfinite(varianceFloor):
        raise ValueError("varianceFloor must be positive and finite")
    if varianceCap < varianceFloor or not math.isfinite(varianceCap):
        raise ValueError("varianceCap must be finite and at least varianceFloor")
    prior = floor = None
    if useEB:
        if priorVarianceTrack is None:
            raise ValueError("priorVarianceTrack is required for MUNC EB finalization")
        if not math.isfinite(nuLocal) or nuLocal <= 0.0:
            raise ValueError("nuLocal must be positive and finite")
        if not math.isfinite(nuPrior) or nuPrior <= 0.0:
            raise ValueError("nuPrior must be positive and finite")
        if not math.isfinite(posterior) or posterior <= 0.0:
            raise ValueError("posterior sample size must be positive and finite")
        prior = np.ascontiguousarray(priorVarianceTrack, dtype=np.float32).reshape(-1)
        if prior.shape[0] != n:
            raise ValueError("priorVarianceTrack length must match localVarianceTrack length")
    if countFloor is not None:
        floor = np.ascontiguousarray(countFloor, dtype=np.float32).reshape(-1)
        if floor.shape[0] != n:
            raise ValueError("countFloor length must match localVarianceTrack length")
    out = np.empty(n, dtype=np.float32)
    res = L.MuncTrackOut(-1, -1, -1, 0, 0, 0, 0, 0.0)
    if n > 0:
        L.require_gpu()
        prm = L.MuncTrackPrm(nuLocal, nuPrior, posterior, 1.0, 0, 0)
        L.check_value(L.lib().csr_munc_finalize_track(n, L.fp(local), L.fp(prior), L.fp(floor), C.byref(prm), varianceFloor,
                                                      varianceCap, int(useEB), L.fp(out), C.byref(res)))
    res = _out_dict(res)
    finalize_errors(res)
    return out, track_diagnostics(res, n, useEB)


def eval_pspline_log_variance_trend(trend, meanTrack, eps=1.0e-2, maxVariance=None):
    """core.py:6628-6655: the prior variance track of a mean track."""
    log_floor, log_cap = log_bounds(eps, maxVariance)
    knots, beta, degree, x_min, x_max = trend_fields(trend)
    return cEvalPSplineLogVarianceTrend(munc_trend_predictor(meanTrack), knots, beta, degree, x_min, x_max, log_floor, log_cap)


def coerce_count_floor(countModelVarianceFloor, interval_count):
    """core.py:7388-7408: float64, NaN where not finite; None without a finite entry."""
    if countModelVarianceFloor is None:
        return None
    track = np.asarray(countModelVarianceFloor, dtype=np.float64).reshape(-1)
    if track.size != int(interval_count):
        raise ValueError("countModelVarianceFloor must be a one-dimensional track matching the MUNC interval count")
    finite = np.isfinite(track)
    if np.any(finite & (track < 0.0)):
        raise ValueError("countModelVarianceFloor must be nonnegative where finite")
    if not np.any(finite):
        return None
    out = np.full(track.shape, np.nan, dtype=np.float64)
    out[finite] = track[finite]
    return out


def variance_bounds(eps, varianceFloor, varianceCap):
    """(floor, cap or None, cap for the kernel) of core.py:8475-8487."""
    floor = float(max(eps, varianceFloor or eps, 1.0e-12))
    cap = None if varianceCap is None or not np.isfinite(float(varianceCap)) or float(varianceCap) <= floor else float(varianceCap)
    return floor, cap, (float(cap) if cap is not None else float(np.finfo(np.float32).max))


def _prior_strength(value):
    """core.py:8381-8387."""
    if value is None:
        return None
    nu0 = float(value)
    return None if not np.isfinite(nu0) or nu0 < 4.0 else nu0


def resolve_nu(EB_setNuL, EB_effectiveNuL, EB_setNu0, EB_pooledNu0):
    """(Nu_L, Nu_0) of core.py:8738-8804 where the caller gives both; the branches that estimate them are not built."""
    if EB_setNuL is not None and EB_setNuL > 3:
        nu_l = float(EB_setNuL)
    elif EB_effectiveNuL is not None:
        nu_l = float(EB_effectiveNuL)
        if not np.isfinite(nu_l) or nu_l < 4.0:
            raise ValueError("EB_effectiveNuL must be finite and at least 4.0")
    else:
        raise NotImplementedError("Nu_L from the local window is not built: pass EB_effectiveNuL or EB_setNuL")
    nu_0 = _prior_strength(EB_setNu0)
    if nu_0 is None:
        nu_0 = _prior_strength(EB_pooledNu0)
    if nu_0 is None:
        raise NotImplementedError("EB_computePriorStrength is not built: pass EB_pooledNu0 or EB_setNu0 (at least 4)")
    cap = 50.0 * float(nu_l)
    if np.isfinite(cap) and nu_0 > cap:
        nu_0 = float(cap)
    return nu_l, nu_0


def get_munc_track(chromosome, intervals, values, intervalSizeBP, muncTrendBlockSizeBP=None, muncLocalWindowSizeBP=None,
                   dependenceSpanIntervals=None, muncTrendBlockDependenceMultiplier=2.0,
                   muncLocalWindowDependenceMultiplier=2.0, muncVarianceModel="kalman", samplingIters=25_000, randomSeed=42,
                   excludeMask=None, useEMA=True, excludeFitCoefs=None, EB_use=True, EB_setNu0=None, EB_setNuL=None,
                   trendNumBasis=60, trendMinObsPerBasis=25.0, trendMinEdf=3.0, trendMaxEdf=30.0, trendLambdaMin=1.0e-6,
                   trendLambdaMax=1.0e6, trendLambdaGridSize=41, sparseIntervalIndices=None, sparseRegionMask=None, numNearest=0,
                   sparseSupportScaleBP=None, sparseSupportPrior=1.0, restrictLocalVarianceToSparseBed=False, EB_localQuantile=0.0,
                   verbose=False, eps=1.0e-6, varianceFloor=None, varianceCap=None, intervalsArr=None, excludeMaskArr=None,
                   pooledTrend=None, priorMeanTrack=None, replicateVarianceFactor=1.0, EB_pooledNu0=None, covariateTrack=None,
                   additiveCovariateModel=None, replicateIndex=None, sampleFile=None, countModelVarianceFloor=None,
                   localVarianceTrack=None, priorVarianceTrack=None, EB_effectiveNuL=None):
    """core.py:8390-8880 where the caller supplies the pooled trend, the prior mean (or prior variance) track, Nu_0 and Nu_L:
    (float32 track, support fraction).  The sparse-nearest, sparse-restricted and no-pooled-trend branches raise the
    reference's errors; the additive covariate model, the EMA of the mean track and the estimated Nu_0 / Nu_L raise
    NotImplementedError.  The sizing arguments only feed those unbuilt branches and the log lines and are not resolved."""
    floor_, cap_, cap_kernel = variance_bounds(eps, varianceFloor, varianceCap)
    if not (muncVarianceModel is None or (isinstance(muncVarianceModel, (int, np.integer)) and int(muncVarianceModel) == 0)
            or str(muncVarianceModel).strip().lower().replace("-", "").replace("_", "") in {"kalman", "smoother", "kf"}):
        raise ValueError(f"unsupported MUNC variance model {muncVarianceModel!r}; expected kalman")     # core.py:7948-7961
    factor = float(replicateVarianceFactor)
    if not np.isfinite(factor) or factor <= 0.0:
        raise ValueError("replicateVarianceFactor must be positive and finite")
    if intervalsArr is None:
        intervalsArr = np.ascontiguousarray(intervals, dtype=np.uint32).reshape(-1)
    else:
        intervalsArr = np.ascontiguousarray(intervalsArr, dtype=np.uint32).reshape(-1)
    valuesArr = np.ascontiguousarray(values, dtype=np.float32)
    if intervalsArr.shape[0] != valuesArr.size:
        raise ValueError("intervalsArr must match values length")
    if sampleFile is not None and str(sampleFile)[:7] == "":
        raise ValueError("sampleFile must be non-empty when provided")
    count_floor = coerce_count_floor(countModelVarianceFloor, valuesArr.size)
    if localVarianceTrack is None:
        raise ValueError("kalman MUNC requires localVarianceTrack")
    obs = np.ascontiguousarray(localVarianceTrack, dtype=np.float32).reshape(-1)
    if obs.shape[0] != valuesArr.size:
        raise ValueError("localVarianceTrack must match values length")
    obs, _ = cFinalizeMuncEBTrack(obs, useEB=False, varianceFloor=float(floor_), varianceCap=float(cap_kernel))
    if excludeMask is None:
        mask = (np.zeros_like(intervalsArr, dtype=np.uint8) if excludeMaskArr is None
                else np.ascontiguousarray(excludeMaskArr, dtype=np.uint8).reshape(-1))
    else:
        mask = np.ascontiguousarray(excludeMask, dtype=np.uint8).reshape(-1)
    if mask.shape != intervalsArr.shape:
        raise ValueError("excludeMaskArr must match intervals/values length")
    if int(numNearest) > 0 or sparseIntervalIndices is not None:
        raise ValueError("sparse-nearest MUNC is not supported by kalman MUNC")
    if bool(restrictLocalVarianceToSparseBed):
        raise ValueError("restrictLocalVarianceToSparseBed is not supported by kalman MUNC")
    if pooledTrend is None and EB_use:
        raise ValueError("kalman MUNC EB requires a pooled MUNC trend")
    if priorMeanTrack is None:
        mean = np.ascontiguousarray(valuesArr, dtype=np.float32)
    else:
        mean = np.ascontiguousarray(priorMeanTrack, dtype=np.float32).reshape(-1)
        if mean.shape[0] != valuesArr.size:
            raise ValueError("priorMeanTrack must match values length")
    if useEMA and priorMeanTrack is None:
        raise NotImplementedError("cEMA of the mean track is not built: pass priorMeanTrack")
    if not EB_use:
        out, diag = cFinalizeMuncEBTrack(obs, countFloor=count_floor, useEB=False, varianceFloor=float(floor_),
                                         varianceCap=float(cap_kernel))
        return out.astype(np.float32, copy=False), float(diag["supportFraction"])
    if priorVarianceTrack is None:
        prior = eval_pspline_log_variance_trend(pooledTrend, mean, eps=floor_, maxVariance=cap_)
    else:
        prior = np.ascontiguousarray(priorVarianceTrack, dtype=np.float32).reshape(-1)
        if prior.shape[0] != valuesArr.size:
            raise ValueError("priorVarianceTrack must match values length")
    if additiveCovariateModel is not None and covariateTrack is not None:
        raise NotImplementedError("the additive covariate model is not built")
    if abs(factor - 1.0) > 1.0e-8:
        prior = np.asarray(prior, dtype=np.float64).reshape(-1) * factor
    prior, _ = cFinalizeMuncEBTrack(prior, useEB=False, varianceFloor=float(floor_), varianceCap=float(cap_kernel))
    nu_l, nu_0 = resolve_nu(EB_setNuL, EB_effectiveNuL, EB_setNu0, EB_pooledNu0)
    posterior = nu_l + nu_0
    if not np.isfinite(posterior) or posterior <= 0.0:
        raise ValueError(f"MUNC EB posterior sample size is invalid on {chromosome}: {posterior}")
    out, diag = cFinalizeMuncEBTrack(obs, priorVarianceTrack=prior, countFloor=count_floor, nuLocal=float(nu_l),
                                     nuPrior=float(nu_0), useEB=True, varianceFloor=float(floor_), varianceCap=float(cap_kernel))
    return out.astype(np.float32, copy=False), float(diag["supportFraction"])


def apply_blacklist_munc_floor(muncMatrix, blacklistMask, minR, quantile=0.05):
    """core.py:7183-7222 with a non-negative minR, IN PLACE on a C-contiguous float32 track or matrix: the masked cells are
    raised to the row's floor (the `quantile` of its finite unmasked cells as np.quantile takes it on a float32 row, not below
    minR).  Returns the float64 floors.  A negative minR (the floor resolved from the matrix) is NotImplementedError."""
    arr = np.asarray(muncMatrix)
    if arr.ndim == 1:
        arr2 = arr.reshape(1, -1)
    elif arr.ndim == 2:
        arr2 = arr
    else:
        raise ValueError("muncMatrix must be one- or two-dimensional")
    mask = np.asarray(blacklistMask, dtype=bool).ravel()
    if mask.size != arr2.shape[1]:
        raise ValueError("blacklistMask length must match MUNC track length")
    requested = float(minR)
    if not np.isfinite(requested):
        raise ValueError("minR must be finite")
    if requested < 0.0:
        raise NotImplementedError("a negative minR (the floor resolved from the matrix quantile) is not built")
    floors = np.full(arr2.shape[0], requested, dtype=np.float64)
    if not np.any(mask):
        return floors
    if arr2.dtype != np.float32 or not arr2.flags.c_contiguous or not arr2.flags.writeable:
        raise TypeError("apply_blacklist_munc_floor works in place on a writeable C-contiguous float32 array")
    q = float(np.clip(float(quantile), 0.0, 1.0))
    if q != q:
        raise ValueError("Quantiles must be in the range [0, 1]")
    if arr2.shape[0] == 0:
        return floors
    L.require_gpu()
    mask8 = np.ascontiguousarray(mask, dtype=np.uint8)
    L.check_value(L.lib().csr_munc_blacklist_floor(arr2.shape[0], arr2.shape[1], L.fp(arr2), mask8.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                   requested, q, L.dp(floors)))
    return floors


# -- block records on the host ---------------------------------------------------------------------------------------------------
def block_layout(n, block_intervals):
    """(starts, ends) of the deterministic blocks of consenrich.py:7364-7373: max(2, block_intervals) intervals each, a last block
    shorter than 2 dropped."""
    size = max(2, int(block_intervals))
    starts = np.arange(0, int(n), size, dtype=np.int64)
    ends = np.minimum(starts + size, int(n))
    keep = (ends - starts) >= 2
    return starts[keep], ends[keep]


def block_sums(evidence, weight, exclude, mean, block_intervals):
    """The block-sum kernel on host arrays (the pinning device of `DeviceBatch.munc_block_sums`, with its record): evidence and
    weight (m, n) float32, exclude (n) bytes or None, mean (n) float64."""
    evidence = np.ascontiguousarray(evidence, dtype=np.float32)
    weight = np.ascontiguousarray(weight, dtype=np.float32)
    mean = np.ascontiguousarray(mean, dtype=np.float64).reshape(-1)
    if evidence.ndim != 2 or weight.shape != evidence.shape or mean.shape[0] != evidence.shape[1]:
        raise ValueError("evidence and weight must be (m, n), mean (n)")
    m, n = evidence.shape
    mask = None
    if exclude is not None:
        mask = np.ascontiguousarray(exclude, dtype=np.uint8).reshape(-1)
        if mask.shape[0] != n:
            raise ValueError("exclude length must match interval count")
    if max(2, int(block_intervals)) > L.MUNC_BLOCK_MAX:
        raise ValueError(f"block_intervals {int(block_intervals)}: the device stages blocks of up to {L.MUNC_BLOCK_MAX} intervals")
    starts, ends = block_layout(n, block_intervals)
    recs = np.zeros((m, starts.size), dtype=L.MUNC_BLOCK_REC)
    included = np.zeros(starts.size, dtype=np.int64)
    if m > 0 and starts.size > 0:
        L.require_gpu()
        L.check_value(L.lib().csr_munc_block_sums(m, n, L.fp(evidence), L.fp(weight),
                                                  None if mask is None else mask.ctypes.data_as(C.POINTER(C.c_uint8)), L.dp(mean),
                                                  int(block_intervals), recs.ctypes.data_as(C.c_void_p), L._i64p(included)))
    out = {k: np.ascontiguousarray(recs[k]) for k in ("valid", "q", "qp", "qe", "qq")}
    out.update(included=included, starts=starts, ends=ends)
    return out


def default_trigamma(x):
    from scipy.special import polygamma      # lazily: SciPy is needed by this default only

    return polygamma(1, x)


def inverse_trend_predictor(predictor):
    """consenrich.py:6362-6364."""
    arr = np.asarray(predictor, dtype=np.float64)
    with np.errstate(all="ignore"):
        return np.sign(arr) * np.expm1(np.abs(arr))


def pooled_block_rows(sums, chain_index=None, dependence_multiplier=1.0, trigamma=None):
    """consenrich.py:8020-8111 from the block records alone.  sums: what `DeviceBatch.munc_block_sums` returns (one dict per
    chain, None for a chain not taken: "valid", "q", "qp", "qe", "qq" of shape (m, blocks), "included" and "starts" per block).
    chain_index[chain]: the chromosome index recorded with the chain's rows (default: the chain's position).

    Returns the pooled rows in the reference's order (chains in order, sample-major within a chain): "means" (the inverse
    predictor of the block mean), "variances", "log_variance_noise" (trigamma(max(nEff, 4) / 2)), "sample_index",
    "chrom_index", "block_starts", "trend_weights", and "row_counts" per chain; "chains" holds the per-chain (m, blocks)
    matrices "predictor", "evidence", "weight", "support" and "valid"."""
    tri = default_trigamma if trigamma is None else trigamma
    divisor = float(max(1.0, float(dependence_multiplier)))
    parts = {k: [] for k in ("means", "variances", "log_variance_noise", "sample_index", "chrom_index", "block_starts",
                             "trend_weights")}
    row_counts, per_chain = [], []
    for c, rec in enumerate(sums):
        if rec is None:
            row_counts.append(0)
            per_chain.append(None)
            continue
        chrom = c if chain_index is None else int(chain_index[c])
        valid, q, qp, qe, qq = (np.asarray(rec[k]) for k in ("valid", "q", "qp", "qe", "qq"))
        m, blocks = q.shape
        predictor = np.full((m, blocks), np.nan, dtype=np.float64)
        evidence = np.full((m, blocks), np.nan, dtype=np.float64)
        weight = np.zeros((m, blocks), dtype=np.float64)
        support = np.zeros((m, blocks), dtype=np.float64)
        take = (valid > 0) & (q > 0.0)                  # consenrich.py:8020-8027
        with np.errstate(all="ignore"):
            predictor[take] = qp[take] / q[take]
            evidence[take] = qe[take] / q[take]
            weight[take] = q[take]
            eff = take & (qq > 0.0)
            support[eff] = np.maximum(1.0, (q[eff] * q[eff] / qq[eff]) / divisor)
        means = inverse_trend_predictor(predictor)
        starts = np.asarray(rec["starts"], dtype=np.int64)
        rows = 0
        keep = np.zeros((m, blocks), dtype=bool)
        for j in range(m):
            noise = np.asarray(tri(np.maximum(support[j], 4.0) / 2.0), dtype=np.float64)
            with np.errstate(all="ignore"):
                trend_w = 1.0 / noise
            ok = (np.isfinite(means[j]) & np.isfinite(evidence[j]) & np.isfinite(support[j]) & np.isfinite(weight[j])
                  & (evidence[j] >= NUMERIC_VARIANCE_FLOOR) & (support[j] > 0.0) & (weight[j] > 0.0))
            keep[j] = ok
            if not np.any(ok):
                continue
            count = int(np.count_nonzero(ok))
            rows += count
            parts["means"].append(means[j][ok])
            parts["variances"].append(evidence[j][ok])
            parts["log_variance_noise"].append(noise[ok])
            parts["sample_index"].append(np.full(count, j, dtype=np.int64))
            parts["chrom_index"].append(np.full(count, chrom, dtype=np.int64))
            parts["block_starts"].append(starts[ok])
            parts["trend_weights"].append(trend_w[ok])
        row_counts.append(rows)
        per_chain.append(dict(predictor=predictor, evidence=evidence, weight=weight, support=support, valid=keep, means=means))
    ints = ("sample_index", "chrom_index", "block_starts")
    out = {k: (np.concatenate(v) if v else np.empty(0, np.int64 if k in ints else np.float64)) for k, v in parts.items()}
    out["row_counts"] = row_counts
    out["chains"] = per_chain
    return out
