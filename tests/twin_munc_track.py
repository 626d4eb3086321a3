"""NumPy / Python twin of the reference's steps between the dense seed loop and a finished `matrixMunc` -- TEST INFRASTRUCTURE.

  cEvalPSplineLogVarianceTrend, cFinalizeMuncEBTrack   the two natives (pyx:5761-5894, 5364-5544), element by element
  eval_pspline_log_variance_trend, get_munc_track      core.py:6628-6655 and the branch of core.py:8390-8880 the CLI takes
  apply_blacklist_munc_floor, final_clamp              core.py:7183-7222, consenrich.py:9100-9113
  block_loop, pooled_rows                              the block loop of consenrich.py:7981-8111 as the reference runs it: a
                                                       Python loop over every (block, sample) with masked np.sum
  finished_matrix                                      all of it for one chain: what `driver.munc_track_batch` must leave

Python floats are IEEE doubles and math.exp / np.log1p are the C library's, as in the compiled reference:
tests/golden/make_munc_track_golden.py writes the fixtures only if this twin equals the reference bit for bit."""
import math

import numpy as np

F32_MAX = 3.4028234663852886e38
FLOOR = 1.0e-12


def _f32(x):
    with np.errstate(over="ignore"):
        return float(np.float32(x))


def predictor(values):
    arr = np.asarray(values, dtype=np.float64)
    with np.errstate(all="ignore"):
        out = np.sign(arr) * np.log1p(np.abs(arr))
    out[~np.isfinite(out)] = np.nan
    return out


def inverse_predictor(p):
    arr = np.asarray(p, dtype=np.float64)
    with np.errstate(all="ignore"):
        return np.sign(arr) * np.expm1(np.abs(arr))


# -- the two natives -------------------------------------------------------------------------------------------------------------
def _span(knots, n_basis, degree, x):
    if x <= knots[degree]:
        return degree
    if x >= knots[n_basis]:
        return n_basis - 1
    low, high = degree, n_basis
    while low < high:
        mid = low + ((high - low) >> 1)
        if x < knots[mid]:
            high = mid
        elif x >= knots[mid + 1]:
            low = mid + 1
        else:
            return mid
    return n_basis - 1


def _de_boor(knots, beta, n_basis, degree, x):
    span = _span(knots, n_basis, degree, x)
    work = [beta[min(max(span - degree + j, 0), n_basis - 1)] for j in range(degree + 1)]
    for r in range(1, degree + 1):
        for j in range(degree, r - 1, -1):
            idx = span - degree + j
            denom = knots[idx + degree - r + 1] - knots[idx]
            alpha = 0.0 if denom == 0.0 else (x - knots[idx]) / denom
            work[j] = ((1.0 - alpha) * work[j - 1]) + (alpha * work[j])
    return work[degree]


def _exp32(v):
    try:
        return np.float32(math.exp(v))
    except OverflowError:
        return np.float32(np.inf)


def cEvalPSplineLogVarianceTrend(predictorTrack, knots, beta, degree, xMin, xMax, logFloor, logCap):
    pred = np.ascontiguousarray(predictorTrack, dtype=np.float64).ravel()
    knots = [float(v) for v in np.ascontiguousarray(knots, dtype=np.float64).ravel()]
    beta = [float(v) for v in np.ascontiguousarray(beta, dtype=np.float64).ravel()]
    degree, n_basis = int(degree), len(beta)
    out = np.empty(pred.shape[0], dtype=np.float32)
    if pred.shape[0] == 0:
        return out

    def settle(v):
        if not math.isfinite(v):
            v = logCap if v > 0.0 else logFloor
        return logFloor if v < logFloor else (logCap if v > logCap else v)

    if degree < 0 or len(knots) == 0 or n_basis == 0:
        v = beta[0] if n_basis > 0 else logFloor
        out[:] = _exp32(settle(v))
        return out
    for i, x in enumerate(pred.tolist()):
        if not math.isfinite(x):
            v = logFloor
        else:
            x = xMin if x < xMin else (xMax if x > xMax else x)
            v = settle(_de_boor(knots, beta, n_basis, degree, x))
        v = logFloor if v < logFloor else (logCap if v > logCap else v)
        out[i] = _exp32(v)
    return out


def _first(mask):
    hit = np.flatnonzero(mask)
    return int(hit[0]) if hit.size else -1


def finalize_loop(local, prior, floor, nu_l, nu_0, vfloor, vcap, use_eb):
    """The loop of pyx:5393-5442 on float32 arrays, vectorised: (out, the lowest invalid index of each kind, the four counters
    over the whole track).  `floor` keeps the native's rule: NaN = missing."""
    n = local.shape[0]
    lv = local.astype(np.float64)
    bad_local = _first(~np.isfinite(lv) | (lv <= 0.0))
    support = int(np.count_nonzero(lv > vfloor))
    lv = np.clip(lv, vfloor, vcap)
    bad_prior = -1
    with np.errstate(all="ignore"):
        if use_eb:
            pv = prior.astype(np.float64)
            bad_prior = _first(~np.isfinite(pv) | (pv <= 0.0))
            pv = np.clip(pv, vfloor, vcap)
            out = ((nu_l * lv) + (nu_0 * pv)) / (nu_l + nu_0)
        else:
            out = lv.copy()
        out = np.where(out < vfloor, vfloor, np.where(out > vcap, vcap, out))
        bad_floor, finite, added, missing = -1, 0, 0, 0
        if floor is not None:
            cf = floor.astype(np.float64)
            there = ~np.isnan(cf)
            bad_floor = _first(there & (~np.isfinite(cf) | (cf < 0.0)))
            finite, missing = int(np.count_nonzero(there)), int(n - np.count_nonzero(there))
            added = int(np.count_nonzero(there & (cf > 0.0)))
            summed = out + np.where(there, cf, 0.0)
            summed = np.where(summed < vfloor, vfloor, np.where(summed > vcap, vcap, summed))
            out = np.where(there, summed, out)
        return out.astype(np.float32), (bad_local, bad_prior, bad_floor), (support, finite, added, missing)


def cFinalizeMuncEBTrack(localVarianceTrack, priorVarianceTrack=None, countFloor=None, nuLocal=0.0, nuPrior=0.0,
                         varianceFloor=1.0e-12, varianceCap=F32_MAX, useEB=True):
    nu_l, nu_0, vfloor, vcap = _f32(nuLocal), _f32(nuPrior), _f32(varianceFloor), _f32(varianceCap)
    useEB = bool(useEB)
    local = np.ascontiguousarray(localVarianceTrack, dtype=np.float32).reshape(-1)
    n = local.shape[0]
    if vfloor <= 0.0 or not math.isfinite(vfloor):
        raise ValueError("varianceFloor must be positive and finite")
    if vcap < vfloor or not math.isfinite(vcap):
        raise ValueError("varianceCap must be finite and at least varianceFloor")
    prior = floor = None
    if useEB:
        if priorVarianceTrack is None:
            raise ValueError("priorVarianceTrack is required for MUNC EB finalization")
        if not math.isfinite(nu_l) or nu_l <= 0.0:
            raise ValueError("nuLocal must be positive and finite")
        if not math.isfinite(nu_0) or nu_0 <= 0.0:
            raise ValueError("nuPrior must be positive and finite")
        if not math.isfinite(nu_l + nu_0) or nu_l + nu_0 <= 0.0:
            raise ValueError("posterior sample size must be positive and finite")
        prior = np.ascontiguousarray(priorVarianceTrack, dtype=np.float32).reshape(-1)
        if prior.shape[0] != n:
            raise ValueError("priorVarianceTrack length must match localVarianceTrack length")
    if countFloor is not None:
        floor = np.ascontiguousarray(countFloor, dtype=np.float32).reshape(-1)
        if floor.shape[0] != n:
            raise ValueError("countFloor length must match localVarianceTrack length")
    out, bad, counts = finalize_loop(local, prior, floor, nu_l, nu_0, vfloor, vcap, useEB)
    texts = ("localVarianceTrack must contain finite positive values at index {}",
             "priorVarianceTrack must contain finite positive values at index {}",
             "countFloor must be nonnegative where finite at index {}")
    hit = [(idx, k) for k, idx in enumerate(bad) if idx >= 0]
    if hit:
        idx, k = min(hit)           # the sequential loop: the lowest index; at one index local, then prior, then the floor
        raise ValueError(texts[k].format(idx))
    # counters: the loop got through every interval
    return out, {"supportCount": counts[0], "supportFraction": (float(counts[0]) / float(n)) if n > 0 else 0.0,
                 "countFloorFiniteCount": counts[1], "countFloorAddedCount": counts[2], "countFloorMissingCount": counts[3],
                 "finalShrinkagePairCount": n if useEB else 0, "finalShrinkagePairFraction": 1.0 if useEB and n > 0 else 0.0}


# -- the Python layer ------------------------------------------------------------------------------------------------------------
def log_bounds(eps, max_variance):
    floor = float(max(eps, 1.0e-12))
    cap = F32_MAX if max_variance is None or not np.isfinite(float(max_variance)) or max_variance <= floor else float(max_variance)
    return float(np.log(floor)), float(np.log(cap))


def eval_pspline_log_variance_trend(trend, meanTrack, eps=1.0e-2, maxVariance=None, native=None):
    knots, beta, degree, x_min, x_max = trend
    lo, hi = log_bounds(eps, maxVariance)
    fn = cEvalPSplineLogVarianceTrend if native is None else native
    return fn(predictor(meanTrack), np.asarray(knots, np.float64), np.asarray(beta, np.float64), int(degree), float(x_min),
              float(x_max), lo, hi)


def coerce_floor(count_floor, n):
    if count_floor is None:
        return None
    track = np.asarray(count_floor, dtype=np.float64).reshape(-1)
    if track.size != int(n):
        raise ValueError("countModelVarianceFloor must be a one-dimensional track matching the MUNC interval count")
    finite = np.isfinite(track)
    if np.any(finite & (track < 0.0)):
        raise ValueError("countModelVarianceFloor must be nonnegative where finite")
    if not np.any(finite):
        return None
    return np.where(finite, track, np.nan)


def get_munc_track(local, *, floor, cap, use_eb=True, trend=None, prior_mean=None, prior_variance=None, factor=1.0, nu0=None,
                   nuL=None, count_floor=None, natives=None):
    """`getMuncTrack` with localVarianceTrack, pooledTrend, priorMeanTrack / priorVarianceTrack, replicateVarianceFactor,
    EB_pooledNu0, EB_effectiveNuL, countModelVarianceFloor and eps = varianceFloor = floor, varianceCap = cap: (track,
    support fraction, diagnostics of the last native call).  natives: (cEval, cFinalize) to use instead of the twin's."""
    ev, fin = (cEvalPSplineLogVarianceTrend, cFinalizeMuncEBTrack) if natives is None else natives
    vfloor = float(max(floor, floor or floor, 1.0e-12))
    vcap = None if cap is None or not np.isfinite(float(cap)) or float(cap) <= vfloor else float(cap)
    kcap = float(vcap) if vcap is not None else F32_MAX
    factor = float(factor)
    if not np.isfinite(factor) or factor <= 0.0:
        raise ValueError("replicateVarianceFactor must be positive and finite")
    obs = np.ascontiguousarray(local, dtype=np.float32).reshape(-1)
    cf = coerce_floor(count_floor, obs.size)
    obs, _ = fin(obs, useEB=False, varianceFloor=vfloor, varianceCap=kcap)
    if trend is None and use_eb:
        raise ValueError("kalman MUNC EB requires a pooled MUNC trend")
    if not use_eb:
        out, diag = fin(obs, countFloor=cf, useEB=False, varianceFloor=vfloor, varianceCap=kcap)
        return out, float(diag["supportFraction"]), diag
    if prior_variance is None:
        mean = np.ascontiguousarray(prior_mean, dtype=np.float32).reshape(-1)
        prior = eval_pspline_log_variance_trend(trend, mean, eps=vfloor, maxVariance=vcap, native=ev)
    else:
        prior = np.ascontiguousarray(prior_variance, dtype=np.float32).reshape(-1)
    if abs(factor - 1.0) > 1.0e-8:
        prior = np.asarray(prior, dtype=np.float64).reshape(-1) * factor
    prior, _ = fin(prior, useEB=False, varianceFloor=vfloor, varianceCap=kcap)
    nu_l = float(nuL)
    if not np.isfinite(nu_l) or nu_l < 4.0:
        raise ValueError("EB_effectiveNuL must be finite and at least 4.0")
    nu_0 = min(float(nu0), 50.0 * nu_l)
    out, diag = fin(obs, priorVarianceTrack=prior, countFloor=cf, nuLocal=nu_l, nuPrior=nu_0, useEB=True, varianceFloor=vfloor,
                    varianceCap=kcap)
    return out, float(diag["supportFraction"]), diag


def apply_blacklist_munc_floor(matrix, mask, min_r, quantile=0.05):
    """In place on a float32 (m, n) matrix; returns the floors."""
    mask = np.asarray(mask, dtype=bool).ravel()
    floors = np.full(matrix.shape[0], float(min_r), dtype=np.float64)
    if not np.any(mask):
        return floors
    q = float(np.clip(float(quantile), 0.0, 1.0))
    for j in range(matrix.shape[0]):
        row = matrix[j, :]
        ref = row[~mask & np.isfinite(row)]
        fl = max(float(min_r), float(np.quantile(ref, q))) if ref.size else float(min_r)
        floors[j] = fl
        black = row[mask]
        row[mask] = np.where(np.isfinite(black), np.maximum(black, fl), fl)
    return floors


def final_clamp(matrix, cap):
    """consenrich.py:9092-9113 in place; raises its RuntimeError."""
    if not np.all(np.isfinite(matrix)):
        raise RuntimeError(f"MUNC matrix has {int(matrix.size - np.count_nonzero(np.isfinite(matrix)))} non-finite entries")
    np.maximum(matrix, np.float32(FLOOR), out=matrix)
    if cap is not None and np.isfinite(float(cap)) and float(cap) > FLOOR:
        np.minimum(matrix, np.float32(float(cap)), out=matrix)
    return matrix


# -- the block loop ----------------------------------------------------------------------------------------------------------------
def blocks(n, block_intervals):
    size = max(2, int(block_intervals))
    starts = np.arange(0, n, size, dtype=np.intp)
    ends = np.minimum(starts + size, n).astype(np.intp)
    keep = (ends - starts) >= 2
    return starts[keep], ends[keep]


def block_loop(evidence, weight, exclude, mean, block_intervals, multiplier=2.0, pred=None):
    """consenrich.py:7981-8040 for one chromosome: evidence / weight (m, n) float32, exclude (n) bytes, mean (n) float64.
    Returns the raw sums too (what the device hands back): valid, q, qp, qe, qq, included.  pred: a predictor track to use
    instead of predictor(mean) (the device's own log1p, when the rest is to be compared bit for bit)."""
    m, n = evidence.shape
    starts, ends = blocks(n, block_intervals)
    nb = starts.size
    pmat, emat = np.full((m, nb), np.nan), np.full((m, nb), np.nan)
    wmat, smat = np.zeros((m, nb)), np.zeros((m, nb))
    raw = {k: np.zeros((m, nb), np.int64 if k == "valid" else np.float64) for k in ("valid", "q", "qp", "qe", "qq")}
    included = np.zeros(nb, dtype=np.int64)
    ptrack = predictor(mean) if pred is None else np.asarray(pred, dtype=np.float64)
    q_all = np.ascontiguousarray(weight, dtype=np.float64)
    q_all[:, exclude != 0] = 0.0
    divisor = float(max(1.0, float(multiplier)))
    for b, (s, e) in enumerate(zip(starts, ends)):
        allowed = np.asarray(exclude[s:e]) == 0
        included[b] = int(np.count_nonzero(allowed))
        pb = np.asarray(ptrack[s:e], dtype=np.float64)
        for j in range(m):
            eb = np.asarray(evidence[j, s:e], dtype=np.float64)
            qb = np.asarray(q_all[j, s:e], dtype=np.float64)
            ok = allowed & np.isfinite(pb) & np.isfinite(eb) & (eb > 0.0) & np.isfinite(qb) & (qb > 0.0)
            raw["valid"][j, b] = int(np.count_nonzero(ok))
            qv, ev, pv = qb[ok], eb[ok], pb[ok]
            raw["q"][j, b] = float(np.sum(qv, dtype=np.float64))
            raw["qp"][j, b] = float(np.sum(qv * pv, dtype=np.float64))
            raw["qe"][j, b] = float(np.sum(qv * ev, dtype=np.float64))
            raw["qq"][j, b] = float(np.sum(qv * qv, dtype=np.float64))
            if not np.any(ok):
                continue
            q_sum = raw["q"][j, b]
            if q_sum <= 0.0:
                continue
            pmat[j, b] = raw["qp"][j, b] / q_sum
            emat[j, b] = raw["qe"][j, b] / q_sum
            wmat[j, b] = q_sum
            if raw["qq"][j, b] > 0.0:
                smat[j, b] = max(1.0, (q_sum * q_sum / raw["qq"][j, b]) / divisor)
    raw.update(included=included, starts=starts.astype(np.int64), ends=ends.astype(np.int64))
    return dict(predictor=pmat, evidence=emat, weight=wmat, support=smat, raw=raw)


def pooled_rows(loops, trigamma, chain_index=None):
    """consenrich.py:8041-8111 over the chromosomes' block_loop results (None: not taken), in the reference's order."""
    parts = {k: [] for k in ("means", "variances", "log_variance_noise", "sample_index", "chrom_index", "block_starts",
                             "trend_weights")}
    counts = []
    for c, lp in enumerate(loops):
        if lp is None:
            counts.append(0)
            continue
        means = inverse_predictor(lp["predictor"])
        rows = 0
        for j in range(means.shape[0]):
            mj, vj, kj, sj = means[j, :], lp["evidence"][j, :], lp["weight"][j, :], lp["support"][j, :]
            noise = np.asarray(trigamma(np.maximum(sj, 4.0) / 2.0), dtype=np.float64)
            tw = 1.0 / noise
            ok = np.isfinite(mj) & np.isfinite(vj) & np.isfinite(sj) & np.isfinite(kj) & (vj >= FLOOR) & (sj > 0.0) & (kj > 0.0)
            if not np.any(ok):
                continue
            cnt = int(np.count_nonzero(ok))
            rows += cnt
            parts["means"].append(mj[ok])
            parts["variances"].append(vj[ok])
            parts["log_variance_noise"].append(noise[ok])
            parts["sample_index"].append(np.full(cnt, j, np.int64))
            parts["chrom_index"].append(np.full(cnt, c if chain_index is None else int(chain_index[c]), np.int64))
            parts["block_starts"].append(lp["raw"]["starts"][ok])
            parts["trend_weights"].append(tw[ok])
        counts.append(rows)
    ints = ("sample_index", "chrom_index", "block_starts")
    out = {k: (np.concatenate(v) if v else np.empty(0, np.int64 if k in ints else np.float64)) for k, v in parts.items()}
    out["row_counts"] = counts
    return out


def finished_matrix(smooth, mean32, exclude, raw_floor, trend, factors, nu0, nuL, floor, cap, use_eb=True, quantile=0.05, prior=None):
    """What the reference leaves as one chromosome's matrixMunc: per sample `get_munc_track`, then the blacklist floor (with a
    mask) and the clamp.  prior: a prior variance track to use instead of the trend's (the device's own, for the bit-for-bit
    part of the composed check).  Returns (matrix, diagnostics per sample, floors)."""
    m, n = smooth.shape
    out, diags = np.empty((m, n), np.float32), []
    nu0 = np.broadcast_to(np.asarray(nu0, np.float64), (m,))
    nuL = np.broadcast_to(np.asarray(nuL, np.float64), (m,))
    for j in range(m):
        track, _, diag = get_munc_track(smooth[j], floor=floor, cap=cap if cap is not None and cap > 0.0 else None, use_eb=use_eb,
                                        trend=trend, prior_mean=mean32, prior_variance=prior, factor=factors[j], nu0=nu0[j],
                                        nuL=nuL[j], count_floor=None if raw_floor is None else raw_floor[j])
        out[j] = track
        diags.append(diag)
    floors = (apply_blacklist_munc_floor(out, exclude, FLOOR, quantile) if exclude is not None
              else np.full(m, FLOOR, dtype=np.float64))
    final_clamp(out, cap)
    return out, diags, floors
