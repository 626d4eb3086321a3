"""The dependence span on the device: a drop-in for the reference's `cchooseDependenceSpan` (pyx:3360-4120, helpers pyx:2645-3357)
and the same estimate from the matrices a `DeviceBatch` holds resident (`DeviceBatch.dependence_span`,
`driver.dependence_span_batch`).

The device does the three stages that touch the data (csrc/csr_depspan.h): which rows are byte-identical, the ranking score of
every full window of every eligible autosome (bit for bit: ties decide `positiveSignalRank`), and, for the sampled windows, the
clipped and centred rows (bit for bit), the masked lag sums, the pooled ACF and the crossing decision.  The host keeps what is
scalar bookkeeping in the reference too: names and eligibility, the candidate sort, the exponential keys of
`SeedSequence(randSeed).spawn(2)`, the walk over the candidates, the Kaplan-Meier quantiles, the bootstrap geometry, the
hierarchical bootstrap, the band inversion and every string.  Same signature, defaults, validations, error texts and return tuple
as the original; `period_diagnostics` is the one added keyword.  No CPU fallback: the entry points need the GPU.

Lag sums.  The reference takes the lag sums of a window from `np.fft`; the device adds the products directly, in index order, as
compensated dot products about an ulp from the exact sums.  The two routes differ by the FFT's rounding error, so a decision that
hangs on less than that is not the device's to take: a window whose smoothed |ACF| comes within MARGIN of the threshold at a lag
the persistence scan examined (the device returns that margin), or with a lag-zero covariance in the underflow range, is decided
on the host by NumPy's FFT route on the window's downloaded rows alone.  `decided_on_host` in the diagnostics counts them.  The
other decisions of a window (admissibility, quorum, the support cap) rest on integer pair counts and on the same double
divisions as the reference's, and the sign test of lagZero on a sum of squares that is zero in both routes or in neither: they
are exact on the device.

Not protected by a margin: `dominantACFPeriodBP` is the arg-max of a spectrum of the pooled ACF, and the device's pooled ACF
differs from the FFT route's by that route's rounding (some 1e-16).  Two frequency bins whose powers tie to that precision could
name another period than the reference; no window is sent to the host for it.  Signed zeros: the device orders -0.0 in front of
+0.0 where NumPy holds them equal, so a clip bound that falls among zeros of both signs may carry the other sign; no value and no
sum changes.  Up to 4096 rows.

Candidates are evaluated on the device in key-ordered groups (the first `windowCount` and some more; more if too few were valid);
`evaluatedCandidateWindowCount` is the reference's count: how far its walk goes.
"""
from __future__ import annotations

import ctypes as C
import math
import numbers

import numpy as np

from . import _lib as L

# The largest |pooled ACF (FFT route) - pooled ACF (exact lag sums)| that tests/golden/make_depspan_golden.py records over its
# cases is 5.6e-16 (E_ref; 64- to 8448-bin windows).  MARGIN is more than 100 times that (5.6e-14), with room for longer windows.
MARGIN = 1.0e-12

_NONSTANDARD = ("chrY", "chrM", "chrMT", "M", "MT", "_")        # constants.py `NONSTANDARD_CHROMOSOME_NAMES`


# ---------------------------------------------------------------------------------------------------------------
# scalars and names (pyx:2645-2706)
# ---------------------------------------------------------------------------------------------------------------
def _int_arg(value, name) -> int:
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, numbers.Integral):
        raise ValueError("%s must be an integer" % str(name))
    v = int(value)
    if v < -2147483648 or v > 2147483647:
        raise ValueError("%s is outside the supported integer range" % str(name))
    return v


def _real_arg(value, name) -> float:
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, numbers.Real):
        raise ValueError("%s must be a real scalar" % str(name))
    v = float(value)
    if not math.isfinite(v):
        raise ValueError("%s must be finite" % str(name))
    return v


def is_standard_autosome(chromosome) -> bool:
    """misc_util.py:70-79 `isStandardAutosomalChromosome`."""
    name = str(chromosome).strip()
    if name in _NONSTANDARD:
        return False
    if name.lower().startswith("chr"):
        name = name[3:]
    return name.isdigit() and 1 <= int(name) <= 22


def autosome_ordinal(chromosome) -> int:
    name = str(chromosome).strip()
    if name.lower().startswith("chr"):
        name = name[3:]
    return int(name)


def nearest_odd_bins(target_bp: int, interval_bp: int) -> int:
    """pyx:2693-2706 `_dependenceNearestOddBins`: the odd bin count whose length is nearest target_bp (ties go up)."""
    lower = max(1, int(math.floor(float(target_bp) / float(interval_bp))))
    if lower % 2 == 0:
        lower -= 1
    lower = max(1, lower)
    upper = lower + 2
    if abs(float(upper) * interval_bp - target_bp) <= abs(float(lower) * interval_bp - target_bp):
        return upper
    return lower


class Settings:
    """The validated arguments (pyx:3514-3620), in the reference's order of checks."""

    def __init__(self, n_names, n_matrices, intervalSizeBP, windowBP, windowCount, maxLagBP, workingQuantile, bootstrapDraws,
                 randSeed, minWindowCount, acfThreshold, acfSmoothingBP, crossingPersistenceBP, minFinitePairs,
                 minFinitePairCoverage):
        if n_names <= 0 or n_names != n_matrices:
            raise ValueError("chromosome inputs must be nonempty and have equal lengths")
        self.interval = _int_arg(intervalSizeBP, "intervalSizeBP")
        self.window_bp = _int_arg(windowBP, "windowBP")
        self.window_count = _int_arg(windowCount, "windowCount")
        self.max_lag_bp = _int_arg(maxLagBP, "maxLagBP")
        self.draws = _int_arg(bootstrapDraws, "bootstrapDraws")
        self.seed = _int_arg(randSeed, "randSeed")
        self.min_windows = _int_arg(minWindowCount, "minWindowCount")
        self.smoothing_bp = _int_arg(acfSmoothingBP, "acfSmoothingBP")
        self.persistence_bp = _int_arg(crossingPersistenceBP, "crossingPersistenceBP")
        self.min_pairs = _int_arg(minFinitePairs, "minFinitePairs")
        self.quantile = _real_arg(workingQuantile, "workingQuantile")
        self.threshold = _real_arg(acfThreshold, "acfThreshold")
        self.min_coverage = _real_arg(minFinitePairCoverage, "minFinitePairCoverage")
        if self.interval <= 0:
            raise ValueError("intervalSizeBP must be positive")
        if self.window_bp <= 0:
            raise ValueError("windowBP must be positive")
        if self.max_lag_bp <= 0 or self.max_lag_bp > self.window_bp // 2:
            raise ValueError("maxLagBP must satisfy 0 < maxLagBP <= windowBP / 2")
        if self.window_count <= 0 or self.draws <= 0:
            raise ValueError("windowCount and bootstrapDraws must be positive")
        if self.seed < 0:
            raise ValueError("randSeed must be nonnegative")
        if self.min_windows <= 0 or self.min_windows > self.window_count:
            raise ValueError("minWindowCount must satisfy 0 < minWindowCount <= windowCount")
        if self.quantile <= 0.0 or self.quantile >= 1.0:
            raise ValueError("workingQuantile must satisfy 0 < q < 1")
        if self.threshold <= 0.0 or self.threshold >= 1.0:
            raise ValueError("acfThreshold must satisfy 0 < x < 1")
        if self.smoothing_bp <= 0 or self.persistence_bp <= 0:
            raise ValueError("ACF smoothing and crossing persistence must be positive")
        if self.smoothing_bp > self.max_lag_bp or self.persistence_bp > self.max_lag_bp:
            raise ValueError("ACF smoothing and crossing persistence cannot exceed maxLagBP")
        if self.min_pairs <= 0:
            raise ValueError("minFinitePairs must be positive")
        if self.min_coverage <= 0.0 or self.min_coverage > 1.0:
            raise ValueError("minFinitePairCoverage must satisfy 0 < x <= 1")
        if self.window_bp % self.interval != 0 or self.max_lag_bp % self.interval != 0:
            raise ValueError("windowBP and maxLagBP must be integer multiples of intervalSizeBP")
        self.window_bins = self.window_bp // self.interval
        self.max_lag = self.max_lag_bp // self.interval
        self.smoothing = nearest_odd_bins(self.smoothing_bp, self.interval)
        self.persistence = max(1, int(math.ceil(float(self.persistence_bp) / float(self.interval))))
        if self.min_pairs > self.window_bins:
            raise ValueError("minFinitePairs cannot exceed the window bin count")
        if self.window_bins < 2 or self.max_lag < self.persistence or self.max_lag < self.smoothing:
            raise ValueError("physical window and lag settings are too short for the bin width")
        if self.max_lag > self.window_bins // 2:
            raise ValueError("binned maxLagBP must not exceed half of the binned windowBP")
        self.radius_correction = 3.0 / (2.0 * math.sqrt(-math.log(self.threshold)))     # pyx:2689-2690
        self.rank_coverage_min = math.sqrt(self.min_coverage)

    def c_cfg(self) -> L.DepspanCfg:
        return L.DepspanCfg(self.window_bins, self.max_lag, self.smoothing, self.persistence, self.min_pairs, self.threshold,
                            self.min_coverage)


def check_shapes(shapes, kinds) -> int:
    """pyx:3622-3632 on (ndim, shape, dtype kind) of every matrix; returns the shared row count."""
    rows = -1
    for shape, kind in zip(shapes, kinds):
        if len(shape) != 2 or shape[0] <= 0 or shape[1] < 2:
            raise ValueError("each chromosome matrix must be two-dimensional and nonempty")
        if kind not in "biuf":
            raise ValueError("chromosome matrices must contain real numeric values")
        if rows < 0:
            rows = int(shape[0])
        elif int(shape[0]) != rows:
            raise ValueError("chromosome matrices must have one shared row count")
    return rows


def eligible_autosomes(names, lengths, window_bins):
    """pyx:3634-3656: [(ordinal, "chrN", position in the input)] sorted, and the excluded names."""
    seen, records, excluded = set(), [], []
    for i, name in enumerate(names):
        if is_standard_autosome(name):
            ordinal = autosome_ordinal(name)
            if ordinal in seen:
                raise ValueError("duplicate canonical autosome chr%d" % ordinal)
            seen.add(ordinal)
            if int(lengths[i]) >= window_bins:
                records.append((ordinal, "chr%d" % ordinal, i))
            else:
                excluded.append("chr%d" % ordinal)
        else:
            excluded.append(str(name))
    records.sort(key=lambda r: (r[0], r[1]))        # (ordinals are unique: the matrices never enter the comparison)
    if not records:
        raise ValueError("dependence estimator found no eligible autosomes")
    return records, excluded


# ---------------------------------------------------------------------------------------------------------------
# one window on the host: the reference's steps with the lag sums from a given route (pyx:2916-3148)
# ---------------------------------------------------------------------------------------------------------------
def lag_sums_fft(centred, mask, max_lag):
    """The reference's route: power spectra of the centred values and of the mask, back-transformed (pyx:2957, 3000-3016)."""
    n = int(centred.size)
    size = 1 if 2 * n - 1 <= 1 else 1 << int(math.ceil(math.log2(float(2 * n - 1))))
    vf = np.fft.rfft(centred, n=size)
    mf = np.fft.rfft(np.asarray(mask, dtype=np.float64), n=size)
    sums = np.asarray(np.fft.irfft(vf * np.conjugate(vf), n=size)[:max_lag + 1], dtype=np.float64)
    pairs = np.asarray(np.rint(np.fft.irfft(mf * np.conjugate(mf), n=size)[:max_lag + 1]), dtype=np.float64)
    return sums, pairs


def centred_row(values32):
    """(centred float64 row with 0 where not finite, finite mask) or None for fewer than two finite values (pyx:2987-2999)."""
    values = np.asarray(values32, dtype=np.float64)
    mask = np.isfinite(values)
    if int(np.count_nonzero(mask)) < 2:
        return None
    finite = np.asarray(values[mask], dtype=np.float64)
    lower, upper = np.quantile(finite, [0.005, 0.995])
    out = np.zeros(values.size, dtype=np.float64)
    out[mask] = np.clip(finite, float(lower), float(upper))
    out[mask] -= float(np.mean(out[mask]))
    return out, mask


def window_on_host(window_rows, st: Settings, lag_sums=lag_sums_fft):
    """The window's record as the device leaves it (a dict with the fields of csr_depspan_window, plus "pooled").  lag_sums:
    (centred, mask, max_lag) -> (sums, pair counts) of lags 0..max_lag."""
    wb, ml = int(window_rows.shape[1]), st.max_lag
    acfs, pair_rows, cov_rows = [], [], []
    for row in window_rows:
        cm = centred_row(row)
        if cm is None:
            continue
        sums, pairs = lag_sums(cm[0], cm[1], ml)
        coverage = pairs / np.arange(wb, wb - ml - 1, -1, dtype=np.float64)
        cov = np.full(ml + 1, np.nan, dtype=np.float64)
        ok = (pairs >= st.min_pairs) & (coverage >= st.min_coverage)
        with np.errstate(all="ignore"):
            cov[ok] = sums[ok] / pairs[ok]
        zero = float(cov[0])
        if not math.isfinite(zero) or zero <= 0.0:
            continue
        with np.errstate(all="ignore"):
            acfs.append(np.asarray(cov[1:] / zero, dtype=np.float64))
        pair_rows.append(pairs[1:])
        cov_rows.append(coverage[1:])
    rec = dict(status=0, crossing_lag=-1, support_cap_lag=0, last_crossing_start=0, valid_rows=len(acfs), valid_rows_at_crossing=0,
               flags=0, finite_pair_min=math.nan, finite_pair_coverage_min=math.nan, revival=math.nan, margin=math.inf,
               pooled=np.full(ml, np.nan, dtype=np.float64))
    if not acfs:
        return rec
    valid = len(acfs)
    quorum = max(1, int(math.ceil(valid / 2.0)))
    acf = np.asarray(acfs, dtype=np.float64)
    contributing = np.isfinite(acf)
    counts = np.sum(contributing, axis=0)
    short = np.flatnonzero(counts < quorum)
    cap = int(short[0]) if short.size > 0 else ml
    rec["support_cap_lag"] = cap
    if cap <= 0:
        return rec
    pooled = rec["pooled"]
    if valid == 1:
        pooled[:cap] = acf[0, :cap]
    else:
        pooled[:cap] = np.nanmedian(acf[:, :cap], axis=0)
    half = (st.smoothing - 1) // 2
    prefix = np.concatenate((np.zeros(1, dtype=np.float64), np.cumsum(np.abs(pooled[:cap]))))
    last_start = cap - half - st.persistence + 1
    rec["last_crossing_start"] = last_start
    if last_start < 1 + half:
        return rec

    def smoothed(lag):
        return float(prefix[lag + half] - prefix[lag - half - 1]) / float(st.smoothing)

    crossing = -1
    for start in range(1 + half, last_start + 1):
        found = True
        for k in range(st.persistence):
            value = smoothed(start + k)
            if not math.isfinite(value):
                rec["margin"] = 0.0
                found = False
                break
            rec["margin"] = min(rec["margin"], abs(value - st.threshold))
            if value >= st.threshold:
                found = False
                break
        if found:
            crossing = start
            break
    rec["crossing_lag"] = crossing
    if crossing > 0:
        use_end = crossing + st.persistence - 1 + half
        s0, s1 = crossing - half, use_end
    else:
        use_end = cap
        s0, s1 = last_start - half, cap
    used = contributing[:, :use_end]
    used_pairs = np.asarray(pair_rows)[:, :use_end][used]
    used_cov = np.asarray(cov_rows)[:, :use_end][used]
    if used_pairs.size <= 0 or used_cov.size <= 0:
        return rec
    rec["finite_pair_min"] = float(np.min(used_pairs))
    rec["finite_pair_coverage_min"] = float(np.min(used_cov))
    rec["valid_rows_at_crossing"] = int(np.min(counts[s0 - 1:s1]))
    if crossing > 0:
        r0 = crossing + st.persistence - 1
        if r0 < cap:
            rec["revival"] = float(np.max(np.abs(pooled[r0:cap])))
    rec["status"] = 1
    return rec


_DPSS = {}


def period_diagnostics(acf, interval_bp: int):
    """pyx:2852-2902 `_dependencePeriodDiagnostics` without the revival: (dominant period in bp, oscillation strength) of the
    pooled ACF up to the support cap, or (None, None).  Needs SciPy."""
    try:
        from scipy import signal
    except ImportError as exc:
        raise ImportError("period_diagnostics=True needs SciPy (savgol_filter, dpss)") from exc
    n = int(acf.size)
    low_bp, high_bp = max(2.0 * interval_bp, 150.0), 500.0
    if n < 3 or low_bp > high_bp:
        return None, None
    envelope_bins = nearest_odd_bins(2000, interval_bp)
    if envelope_bins > n:
        envelope_bins = n if n % 2 == 1 else n - 1
    if envelope_bins < 3:
        return None, None
    acf = np.asarray(acf, dtype=np.float64)
    residual = acf - signal.savgol_filter(acf, envelope_bins, 2, mode="interp")
    tapers = _DPSS.get(n)
    if tapers is None:
        tapers = np.asarray(signal.windows.dpss(n, 2.5, Kmax=3, sym=False, norm=2), dtype=np.float64)
        _DPSS[n] = tapers
    power = np.mean(np.square(np.abs(np.fft.rfft(tapers * residual[np.newaxis, :], axis=1))), axis=0)
    freq = np.fft.rfftfreq(n, d=interval_bp)
    periods = np.full(freq.size, np.inf, dtype=np.float64)
    periods[freq > 0.0] = 1.0 / freq[freq > 0.0]
    band = np.flatnonzero((periods >= low_bp) & (periods <= high_bp) & ((n * interval_bp) >= (4.0 * periods)))
    if band.size <= 0:
        return None, None
    top = int(band[int(np.argmax(power[band]))])
    total = float(np.sum(power[band]))
    if total <= 0.0:
        return None, None
    return float(periods[top]), float(power[top]) / total


def window_result(rec, pooled, st: Settings, want_period: bool):
    """The reference's per-window dict (pyx:3113-3148) from a window record and its pooled ACF; None where it answers None."""
    if int(rec["status"]) == 0:
        return None
    crossing, cap = int(rec["crossing_lag"]), int(rec["support_cap_lag"])
    if crossing > 0:
        raw, censor_lag, reason = float(crossing) * float(st.interval), math.nan, "none"
    else:
        raw, censor_lag = math.nan, float(int(rec["last_crossing_start"])) * float(st.interval)
        reason = "maxLag" if cap >= st.max_lag else "support"
    radius = (raw if crossing > 0 else censor_lag) * st.radius_correction
    period, strength = period_diagnostics(np.ascontiguousarray(pooled[:cap]), st.interval) if want_period else (None, None)
    revival = float(rec["revival"])
    return {
        "rawCrossingLagBP": None if crossing < 0 else float(raw),
        "censorLagBP": None if crossing > 0 else float(censor_lag),
        "gaussianEquivalentRadiusBP": float(radius),
        "rightCensored": bool(crossing < 0),
        "censorReason": reason,
        "supportCapLagBP": int(cap * st.interval),
        "finitePairMinimumUsed": float(rec["finite_pair_min"]),
        "finitePairCoverageMinimumUsed": float(rec["finite_pair_coverage_min"]),
        "validRowCount": int(rec["valid_rows"]),
        "validRowsAtCrossing": int(rec["valid_rows_at_crossing"]),
        "dominantACFPeriodBP": period,
        "oscillationStrength": strength,
        "postCrossingRevival": None if math.isnan(revival) else revival,
    }


# ---------------------------------------------------------------------------------------------------------------
# Kaplan-Meier, bootstrap geometry (pyx:2750-2829, 3151-3357)
# ---------------------------------------------------------------------------------------------------------------
def km_quantile(values, censored, quantile: float):
    """The first event time at which the Kaplan-Meier estimate of the distribution reaches `quantile`, or None."""
    v = np.ascontiguousarray(np.asarray(values, dtype=np.float64).ravel(), dtype=np.float64)
    cen = np.asarray(censored, dtype=np.bool_).ravel()
    n = int(v.size)
    if n <= 0 or cen.size != n:
        return None
    order = np.argsort(v, kind="mergesort")
    sv, sc = v[order], cen[order]
    start, at_risk, survival = 0, n, 1.0
    for t in np.unique(sv):
        stop = int(np.searchsorted(sv, t, side="right"))
        events = int(np.count_nonzero(~sc[start:stop]))
        if events > 0:
            survival *= 1.0 - (float(events) / float(at_risk))
            if (1.0 - survival) + 1.0e-15 >= quantile:
                return float(t)
        at_risk -= stop - start
        start = stop
    return None


def km_survival_at(values, censored, grid):
    """The Kaplan-Meier survival estimate read at every time of `grid` (1 in front of the first time)."""
    v = np.asarray(values, dtype=np.float64).ravel()
    cen = np.asarray(censored, dtype=np.bool_).ravel()
    g = np.asarray(grid, dtype=np.float64).ravel()
    if v.size <= 0 or cen.size != v.size:
        raise ValueError("Kaplan-Meier inputs must have equal positive lengths")
    order = np.argsort(v, kind="mergesort")
    sv, sc = v[order], cen[order]
    times = np.unique(sv)
    steps = np.ones(times.size, dtype=np.float64)
    start, at_risk, survival = 0, int(v.size), 1.0
    for k in range(int(times.size)):
        stop = int(np.searchsorted(sv, float(times[k]), side="right"))
        events = int(np.count_nonzero(~sc[start:stop]))
        if events > 0:
            survival *= 1.0 - (float(events) / float(at_risk))
        steps[k] = survival
        at_risk -= stop - start
        start = stop
    pos = np.searchsorted(times, g, side="right") - 1
    out = np.ones(g.size, dtype=np.float64)
    ok = pos >= 0
    out[ok] = steps[pos[ok]]
    return out


def coordinate_runs(windows, by_chrom):
    """Runs of selected windows that touch end to start, per chromosome in ordinal order: (runs, adjacencies, longest run)."""
    runs, adjacent, longest = [], 0, 1
    for _, chrom in sorted((autosome_ordinal(c), str(c)) for c in by_chrom):
        idx = [i for _, i in sorted((int(windows[int(i)]["startBP"]), int(i)) for i in by_chrom[chrom])]
        if not idx:
            continue
        run, left = [idx[0]], idx[0]
        for i in idx[1:]:
            if int(windows[i]["startBP"]) == int(windows[left]["endBP"]):
                run.append(i)
                adjacent += 1
            else:
                runs.append(run)
                longest = max(longest, len(run))
                run = [i]
            left = i
        runs.append(run)
        longest = max(longest, len(run))
    return runs, int(adjacent), int(longest)


def politis_white_block(component, runs, longest: int) -> float:
    """pyx:3202-3305: the Politis-White block length of one component along the coordinate runs, clamped to [1, longest run]."""
    values = np.asarray(component, dtype=np.float64).ravel()
    n = int(values.size)
    if n <= 1 or longest <= 1:
        return 1.0
    sd = float(np.std(values))
    if not math.isfinite(sd) or sd <= 1.0e-12:
        return 1.0
    z = (values - float(np.mean(values))) / sd
    k_n = max(5, int(math.ceil(math.log10(float(n)))))
    max_lag = min(longest - 1, int(math.ceil(math.sqrt(float(n)))) + k_n)
    if max_lag <= 0:
        return 1.0
    acov = np.zeros(max_lag + 1, dtype=np.float64)
    acov[0] = float(np.mean(np.square(z)))
    if float(acov[0]) <= 0.0:
        return 1.0
    for lag in range(1, max_lag + 1):
        total, pairs = 0.0, 0
        for run in runs:
            if len(run) <= lag:
                continue
            rv = z[np.asarray(run, dtype=np.int64)]
            total += float(np.dot(rv[:-lag], rv[lag:]))
            pairs += len(run) - lag
        if pairs > 0:
            acov[lag] = total / float(pairs)
    critical = 2.0 * math.sqrt(math.log10(float(n)) / float(n))
    m_hat, cutoff = 0, min(k_n, max_lag)
    for lag in range(cutoff, max_lag + 1):
        first = lag - cutoff + 1
        if bool(np.all(np.abs(acov[first:lag + 1] / float(acov[0])) < critical)):
            m_hat = first
            break
    if m_hat <= 0:
        for lag in range(max_lag, 0, -1):
            if abs(float(acov[lag]) / float(acov[0])) > critical:
                m_hat = lag
                break
        if m_hat <= 0:
            m_hat = 1
    m = min(max_lag, 2 * m_hat)
    g_value, long_run = 0.0, float(acov[0])
    for lag in range(1, m + 1):
        weight = 1.0 if (float(lag) / float(m)) <= 0.5 else 2.0 * (1.0 - (float(lag) / float(m)))
        g_value += 2.0 * weight * lag * float(acov[lag])
        long_run += 2.0 * weight * float(acov[lag])
    denominator = 2.0 * long_run * long_run
    if denominator <= 0.0 or not math.isfinite(denominator):
        return 1.0
    block = math.pow((2.0 * g_value * g_value) / denominator, 1.0 / 3.0) * math.pow(float(n), 1.0 / 3.0)
    block_max = max(1.0, min(3.0 * math.sqrt(float(n)), float(n) / 3.0))
    if not math.isfinite(block):
        return 1.0
    return max(1.0, min(block, block_max, float(longest)))


def bootstrap_geometry(windows, by_chrom, radii, censored):
    """pyx:3308-3357: (block length in windows, adjacencies, longest run)."""
    runs, adjacent, longest = coordinate_runs(windows, by_chrom)
    parts = (np.log(np.asarray(radii, dtype=np.float64)), (~np.asarray(censored, dtype=np.bool_)).astype(np.float64),
             np.asarray([float(w["score"]) for w in windows], dtype=np.float64))
    blocks = [politis_white_block(p, runs, longest) for p in parts]
    return max(1, min(longest, int(math.ceil(max(blocks))))), adjacent, longest


# ---------------------------------------------------------------------------------------------------------------
# the estimate, over a backend that answers the three device stages
# ---------------------------------------------------------------------------------------------------------------
def rank_candidates(st: Settings, eligible, lengths, scores, counts):
    """pyx:3664-3740: the candidate windows in key order, as (key, ordinal, startBP, eligible index, startBin, endBin, score,
    positiveSignalRank), and the bootstrap's generator.  scores / counts: per full window, eligible chromosomes in order."""
    cand, at = [], 0
    for k, (ordinal, _, pos) in enumerate(eligible):
        for w in range(int(lengths[pos]) // st.window_bins):
            if int(counts[at + w]) > 0:
                s = float(scores[at + w])
                b0 = w * st.window_bins
                cand.append((-s, int(ordinal), int(b0 * st.interval), k, b0, b0 + st.window_bins, s))
        at += int(lengths[pos]) // st.window_bins
    cand.sort()
    n = len(cand)
    selection_seed, bootstrap_seed = np.random.SeedSequence(st.seed).spawn(2)
    keys = np.ascontiguousarray(np.random.default_rng(selection_seed).exponential(size=n), dtype=np.float64)
    start = 0
    while start < n:
        end = start + 1
        while end < n and cand[end][0] == cand[start][0]:
            end += 1
        rank = 0.5 * (float(start + 1) + float(end))
        weight = float(n) - rank + 1.0
        for i in range(start, end):
            c = cand[i]
            cand[i] = (float(float(keys[i]) / weight), c[1], c[2], c[3], c[4], c[5], float(c[6]), float(rank))
        start = end
    cand.sort()
    return cand, np.random.default_rng(bootstrap_seed)


def choose(names, lengths, row_count, backend, st: Settings, *, want_period=True, margin=None):
    """pyx:3634-4120 over a backend with unique_rows(), window_scores(rows), window_acf(rows, windows) and window_rows(k, start,
    rows) for the eligible chromosomes it was opened with (`backend.open(positions)`)."""
    margin = MARGIN if margin is None else float(margin)
    eligible, excluded = eligible_autosomes(names, lengths, st.window_bins)
    if backend.needs_gpu:
        L.require_gpu()
    backend.open([pos for _, _, pos in eligible])
    rows = backend.unique_rows()
    if len(rows) <= 0:
        raise RuntimeError("dependence estimator found no unique rows")
    scores, counts = backend.window_scores(rows)
    cand, boot_rng = rank_candidates(st, eligible, lengths, scores, counts)

    selected, radii, censored = [], [], []
    pair_minima, cov_minima, rows_at_crossing, censor_times = [], [], [], []
    periods, strengths, revivals = [], [], []
    by_chrom = {}
    evaluated, on_host, at = 0, 0, 0
    group = st.window_count + max(8, st.window_count // 8)
    while at < len(cand) and len(selected) < st.window_count:
        part = cand[at:at + group]
        recs, pooled = backend.window_acf(rows, [(c[3], c[4]) for c in part])
        for k, c in enumerate(part):
            evaluated += 1
            rec, acf = recs[k], pooled[k]
            if backend.needs_gpu and ((int(rec["status"]) != 0 and not float(rec["margin"]) >= margin) or int(rec["flags"]) != 0):
                rec = window_on_host(backend.window_rows(c[3], c[4], rows), st)
                acf = rec["pooled"]
                on_host += 1
            result = window_result(rec, acf, st, want_period)
            if result is None:
                continue
            chrom = eligible[c[3]][1]
            window = {"chromosome": str(chrom), "startBP": int(c[4] * st.interval), "endBP": int(c[5] * st.interval),
                      "score": float(c[6]), "positiveSignalRank": float(c[7])}
            window.update(result)
            selected.append(window)
            radii.append(float(result["gaussianEquivalentRadiusBP"]))
            censored.append(bool(result["rightCensored"]))
            pair_minima.append(float(result["finitePairMinimumUsed"]))
            cov_minima.append(float(result["finitePairCoverageMinimumUsed"]))
            rows_at_crossing.append(int(result["validRowsAtCrossing"]))
            if result["rightCensored"]:
                censor_times.append(float(result["gaussianEquivalentRadiusBP"]))
            if result["dominantACFPeriodBP"] is not None:
                periods.append(float(result["dominantACFPeriodBP"]))
            if result["oscillationStrength"] is not None:
                strengths.append(float(result["oscillationStrength"]))
            if result["postCrossingRevival"] is not None:
                revivals.append(float(result["postCrossingRevival"]))
            by_chrom.setdefault(str(chrom), []).append(len(selected) - 1)
            if len(selected) >= st.window_count:
                break
        at += len(part)
        group *= 2

    used = ["chr%d" % o for o in sorted(autosome_ordinal(c) for c in by_chrom)]
    n_sel, n_used = len(selected), len(used)
    n_censored = int(np.count_nonzero(censored))
    n_support = sum(1 for w in selected if w["censorReason"] == "support")
    n_cap = sum(1 for w in selected if w["censorReason"] == "maxLag")
    counts_by_chrom = {c: int(len(by_chrom[c])) for c in used}
    censor_fraction = float(n_censored) / float(n_sel) if n_sel > 0 else 0.0
    if n_sel < st.min_windows:
        raise RuntimeError("dependence estimator has %d valid windows from %d autosomes, needs at least %d windows, "
                           "censor fraction %.6f" % (n_sel, n_used, st.min_windows, censor_fraction))
    full_median = km_quantile(radii, censored, 0.5)
    full_span = km_quantile(radii, censored, st.quantile)
    if full_median is None or full_span is None:
        raise RuntimeError("dependence estimator Kaplan-Meier quantiles are unresolved for %d valid windows from %d autosomes; "
                           "censor fraction %.6f" % (n_sel, n_used, censor_fraction))
    block, adjacent, longest = bootstrap_geometry(selected, by_chrom, radii, censored)

    grid = np.unique(np.asarray(radii, dtype=np.float64))
    survival = km_survival_at(radii, censored, grid)
    eps = 1.0 / (2.0 * float(n_sel))
    transformed = np.log(-np.log(np.clip(survival, eps, 1.0 - eps)))
    domain = (survival >= 0.25) & (survival <= 0.75)
    if int(np.count_nonzero(domain)) <= 0:
        domain[int(np.argmin(np.abs(survival - 0.5)))] = True
    restart = 1.0 / float(block)
    ordered = {c: [i for _, i in sorted((int(selected[int(i)]["startBP"]), int(i)) for i in by_chrom[c])] for c in used}
    boot_median, boot_span, distances = [], [], []
    ok_median = ok_span = ok_joint = 0
    for _ in range(st.draws):
        dv, dc = [], []
        for s in boot_rng.integers(0, n_used, size=n_used):
            chain = ordered[used[int(s)]]
            pos = int(boot_rng.integers(0, len(chain)))
            for _ in range(len(chain)):
                i = chain[pos]
                dv.append(float(radii[i]))
                dc.append(bool(censored[i]))
                nxt = pos + 1
                if (float(boot_rng.random()) < restart or nxt >= len(chain)
                        or int(selected[chain[nxt]]["startBP"]) != int(selected[i]["endBP"])):
                    pos = int(boot_rng.integers(0, len(chain)))
                else:
                    pos = nxt
        dm = km_quantile(dv, dc, 0.5)
        ds = km_quantile(dv, dc, st.quantile)
        if dm is not None:
            ok_median += 1
            boot_median.append(float(dm))
        if ds is not None:
            ok_span += 1
            boot_span.append(float(ds))
        if dm is not None and ds is not None:
            ok_joint += 1
        d_transformed = np.log(-np.log(np.clip(km_survival_at(dv, dc, grid), eps, 1.0 - eps)))
        distances.append(float(np.max(np.abs(d_transformed - transformed)[domain])))
    required = int(math.ceil(0.95 * float(st.draws)))
    if ok_joint < required or ok_median < required or ok_span < required:
        raise RuntimeError("dependence estimator resolved %d of %d joint bootstrap draws; needs %d"
                           % (ok_joint, st.draws, required))

    estimate, span = float(full_median), float(full_span)
    critical = float(np.quantile(np.asarray(distances, dtype=np.float64), 0.95))
    lower_s = np.exp(-np.exp(transformed + critical))
    upper_s = np.exp(-np.exp(transformed - critical))
    inside = (lower_s <= 0.5) & (upper_s >= 0.5)
    closure = False
    if int(np.count_nonzero(inside)) <= 0:
        left = math.log(-math.log(1.0 - eps))
        left_lower, left_upper = math.exp(-math.exp(left + critical)), math.exp(-math.exp(left - critical))
        jumps = []
        for k in range(int(grid.size)):
            if left_lower > 0.5 and left_upper > 0.5 and float(lower_s[k]) < 0.5 and float(upper_s[k]) < 0.5:
                jumps.append(k)
            left_lower, left_upper = float(lower_s[k]), float(upper_s[k])
        if len(jumps) != 1:
            raise RuntimeError("dependence estimator could not invert its simultaneous survival band")
        lower_bp = upper_bp = float(grid[jumps[0]])
        closure = True
    else:
        lower_bp, upper_bp = float(np.min(grid[inside])), float(np.max(grid[inside]))
    if not math.isfinite(lower_bp) or not math.isfinite(upper_bp):
        raise RuntimeError("dependence estimator produced nonfinite survival-band endpoints")
    lower_bp, upper_bp = min(lower_bp, estimate), max(upper_bp, estimate)

    def med(x):
        return float(np.median(np.asarray(x, dtype=np.float64))) if len(x) > 0 else None

    diagnostics = {
        "status": "estimated",
        "method": "rankWeightedFinitePairWindowACF",
        "randomSeed": int(st.seed),
        "estimateBP": float(estimate),
        "lowerBP": float(lower_bp),
        "upperBP": float(upper_bp),
        "fullSampleMedianRadiusBP": float(full_median),
        "fullSampleWorkingSpanBP": float(full_span),
        "workingSpanBP": float(span),
        "bootstrapMedianRadiusBP": boot_median,
        "bootstrapWorkingSpanBP": boot_span,
        "workingQuantile": float(st.quantile),
        "inferenceScope": "conditionalOnInputTracksAndSelectedWindows",
        "confidenceIntervalMethod": "centralInterquartileSimultaneousLogLogKMSurvivalBand",
        "survivalBandRegionLower": 0.25,
        "survivalBandRegionUpper": 0.75,
        "survivalBandJumpClosureUsed": bool(closure),
        "survivalBandJumpClosureCount": int(1 if closure else 0),
        "confidenceLevel": 0.95,
        "intervalSizeBP": int(st.interval),
        "windowBP": int(st.window_bp),
        "windowCountRequested": int(st.window_count),
        "candidateWindowCount": int(len(cand)),
        "evaluatedCandidateWindowCount": int(evaluated),
        "selectedWindowCount": int(n_sel),
        "minWindowCount": int(st.min_windows),
        "selectedAutosomeCount": int(n_used),
        "chromosomesUsed": [str(c) for c in used],
        "chromosomesExcluded": sorted(set(excluded)),
        "selectedWindows": selected,
        "inputRowCount": int(row_count),
        "uniqueRowCount": int(len(rows)),
        "duplicateRowCount": int(row_count - len(rows)),
        "rowDeduplication": "exactBytes",
        "acfThreshold": float(st.threshold),
        "acfSmoothingBP": int(st.smoothing_bp),
        "acfSmoothingBins": int(st.smoothing),
        "crossingPersistenceBP": int(st.persistence_bp),
        "crossingPersistenceBins": int(st.persistence),
        "minFinitePairs": int(st.min_pairs),
        "minFinitePairCoverage": float(st.min_coverage),
        "maxLagBP": int(st.max_lag * st.interval),
        "gaussianRadiusCorrection": float(st.radius_correction),
        "censorFraction": float(censor_fraction),
        "crossedWindowCount": int(n_sel - n_censored),
        "rightCensoredWindowCount": int(n_censored),
        "supportCensoredWindowCount": int(n_support),
        "capCensoredWindowCount": int(n_cap),
        "censorTimeBPMinimum": None if not censor_times else float(np.min(censor_times)),
        "censorTimeBPMedian": None if not censor_times else float(np.median(censor_times)),
        "censorTimeBPMaximum": None if not censor_times else float(np.max(censor_times)),
        "finitePairMinimumUsed": float(np.min(np.asarray(pair_minima, dtype=np.float64))),
        "finitePairCoverageMinimumUsed": float(np.min(np.asarray(cov_minima, dtype=np.float64))),
        "validRowsAtCrossingMinimum": int(np.min(np.asarray(rows_at_crossing, dtype=np.int64))),
        "selectedCountsByChromosome": counts_by_chrom,
        "selectedAdjacencyCount": int(adjacent),
        "selectedLongestRun": int(longest),
        "radiusDistributionBP": [float(v) for v in radii],
        "radiusCensored": [bool(v) for v in censored],
        "dominantACFPeriodBPMedian": med(periods),
        "oscillationStrength": med(strengths),
        "postCrossingRevival": med(revivals),
        "unresolvedPeriodFraction": float(1.0 - (float(len(periods)) / float(n_sel))),
        "periodicitySearchMinBP": int(max(2 * st.interval, 150)),
        "periodicitySearchMaxBP": 500,
        "bootstrapMethod": "hierarchicalAutosomeStationaryWindow",
        "bootstrapBlockLengthWindows": int(block),
        "bootstrapRestartProbability": float(restart),
        "bootstrapDrawsRequested": int(st.draws),
        "bootstrapResolvedMedianDraws": int(ok_median),
        "bootstrapResolvedWorkingDraws": int(ok_span),
        "bootstrapResolvedJointDraws": int(ok_joint),
        "decided_on_host": int(on_host),
    }
    return (int(math.ceil(estimate / float(st.interval))), int(math.ceil(lower_bp / float(st.interval))),
            int(math.ceil(upper_bp / float(st.interval))), diagnostics)


# ---------------------------------------------------------------------------------------------------------------
# the two device backends
# ---------------------------------------------------------------------------------------------------------------
def _i32(values):
    return np.ascontiguousarray(values, dtype=np.int32)


class _DeviceBackend:
    needs_gpu = True

    def __init__(self, st: Settings):
        self.st = st

    def _windows(self, windows):
        n = len(windows)
        which = _i32([w[0] for w in windows])
        start = np.ascontiguousarray([w[1] for w in windows], dtype=np.int64)
        recs = np.zeros(n, dtype=L.DEPSPAN_WINDOW)
        pooled = np.full((n, self.st.max_lag), np.nan, dtype=np.float64)
        return n, which, start, recs, pooled


class HostArrayBackend(_DeviceBackend):
    """The host-array entry of the C ABI: float32 matrices, staged one chromosome or one window set at a time."""

    def __init__(self, matrices, st: Settings):
        super().__init__(st)
        self.all = matrices

    def open(self, positions):
        self.mats = [self.all[p] for p in positions]
        self.n_bins = np.ascontiguousarray([m.shape[1] for m in self.mats], dtype=np.int64)
        self.ptrs = (C.c_void_p * len(self.mats))(*[m.ctypes.data for m in self.mats])
        self.rows_total = int(self.mats[0].shape[0])

    def unique_rows(self):
        kept, n = np.zeros(self.rows_total, dtype=np.int32), C.c_int32(0)
        L.check(L.lib().csr_depspan_unique_rows(len(self.mats), self.n_bins.ctypes.data_as(L.I64P), self.ptrs, self.rows_total,
                                                kept.ctypes.data_as(L.I32P), C.byref(n)))
        return [int(r) for r in kept[:n.value]]

    def window_scores(self, rows):
        total = int(np.sum(self.n_bins // self.st.window_bins))
        score, count = np.full(total, np.nan, dtype=np.float64), np.zeros(total, dtype=np.int64)
        r = _i32(rows)
        L.check(L.lib().csr_depspan_window_scores(len(self.mats), self.n_bins.ctypes.data_as(L.I64P), self.ptrs, self.rows_total,
                                                  r.size, r.ctypes.data_as(L.I32P), self.st.window_bins,
                                                  self.st.rank_coverage_min, L.dp(score), count.ctypes.data_as(L.I64P)))
        return score, count

    def window_acf(self, rows, windows):
        n, which, start, recs, pooled = self._windows(windows)
        r, cfg = _i32(rows), self.st.c_cfg()
        L.check(L.lib().csr_depspan_window_acf(len(self.mats), self.n_bins.ctypes.data_as(L.I64P), self.ptrs, self.rows_total,
                                               r.size, r.ctypes.data_as(L.I32P), C.byref(cfg), n, which.ctypes.data_as(L.I32P),
                                               start.ctypes.data_as(L.I64P), recs.ctypes.data, L.dp(pooled)))
        return recs, pooled

    def window_rows(self, k, start, rows):
        return np.asarray(self.mats[k][rows, start:start + self.st.window_bins])


class BatchBackend(_DeviceBackend):
    """The batch entry: the resident data of the listed chains of a DeviceBatch; nothing resident changes."""

    def __init__(self, batch, chains, st: Settings):
        super().__init__(st)
        self.batch, self.listed = batch, [int(c) for c in chains]

    def open(self, positions):
        self.chains = _i32([self.listed[p] for p in positions])
        self.n_bins = np.asarray([self.batch.chain_lens[int(c)] for c in self.chains], dtype=np.int64)
        self._rows_cache = {}

    def _call(self, fn, *args):
        L.check(fn(self.batch._ctx, self.chains.size, self.chains.ctypes.data_as(L.I32P), *args))

    def unique_rows(self):
        kept, n = np.zeros(self.batch.m, dtype=np.int32), C.c_int32(0)
        self._call(L.lib().csr_batch_depspan_unique_rows, kept.ctypes.data_as(L.I32P), C.byref(n))
        return [int(r) for r in kept[:n.value]]

    def window_scores(self, rows):
        total = int(np.sum(self.n_bins // self.st.window_bins))
        score, count = np.full(total, np.nan, dtype=np.float64), np.zeros(total, dtype=np.int64)
        r = _i32(rows)
        self._call(L.lib().csr_batch_depspan_window_scores, r.size, r.ctypes.data_as(L.I32P), self.st.window_bins,
                   self.st.rank_coverage_min, L.dp(score), count.ctypes.data_as(L.I64P))
        return score, count

    def window_acf(self, rows, windows):
        n, which, start, recs, pooled = self._windows(windows)
        r, cfg = _i32(rows), self.st.c_cfg()
        self._call(L.lib().csr_batch_depspan_window_acf, r.size, r.ctypes.data_as(L.I32P), C.byref(cfg), n,
                   which.ctypes.data_as(L.I32P), start.ctypes.data_as(L.I64P), recs.ctypes.data, L.dp(pooled))
        return recs, pooled

    def window_rows(self, k, start, rows):
        chain = int(self.chains[k])
        if chain not in self._rows_cache:
            self._rows_cache = {chain: self.batch.download_inputs(chain)[0]}
        return np.asarray(self._rows_cache[chain][rows, start:start + self.st.window_bins])


def _as_float32(matrix):
    """The matrix as C-ordered float32 if that changes no value; TypeError otherwise."""
    if matrix.dtype == np.float32:
        return np.ascontiguousarray(matrix)
    out = np.ascontiguousarray(matrix, dtype=np.float32)
    if not np.array_equal(out.astype(np.float64), np.asarray(matrix, dtype=np.float64), equal_nan=True):
        raise TypeError("chromosome matrices must be float32 or convert to float32 without change: the device stages read "
                        "float32 rows")
    return out


def cchooseDependenceSpan(chromosomeNames, chromosomeMatrices, intervalSizeBP, windowBP=100000, windowCount=256, maxLagBP=50000,
                          workingQuantile=0.75, bootstrapDraws=500, randSeed=1729, minWindowCount=20, acfThreshold=0.1,
                          acfSmoothingBP=250, crossingPersistenceBP=250, minFinitePairs=200, minFinitePairCoverage=0.5, *,
                          period_diagnostics=True, _margin=None):
    """pyx:3360-4120: (point, lower, upper, diagnostics) of the dependence span in intervals.  With period_diagnostics=False the
    SciPy part (`dominantACFPeriodBP`, `oscillationStrength`) is None for every window; `decided_on_host` is the one added key."""
    try:
        names, matrices = list(chromosomeNames), list(chromosomeMatrices)
    except Exception as exc:
        raise ValueError("chromosome inputs must be finite sequences") from exc
    st = Settings(len(names), len(matrices), intervalSizeBP, windowBP, windowCount, maxLagBP, workingQuantile, bootstrapDraws,
                  randSeed, minWindowCount, acfThreshold, acfSmoothingBP, crossingPersistenceBP, minFinitePairs,
                  minFinitePairCoverage)
    matrices = [np.asarray(m) for m in matrices]
    row_count = check_shapes([m.shape for m in matrices], [m.dtype.kind for m in matrices])
    lengths = [int(m.shape[1]) for m in matrices]
    eligible_autosomes(names, lengths, st.window_bins)         # (its ValueErrors come before the dtype's TypeError)
    matrices = [_as_float32(m) for m in matrices]
    return choose(names, lengths, row_count, HostArrayBackend(matrices, st), st, want_period=bool(period_diagnostics),
                  margin=_margin)


def batch_dependence_span(batch, names, interval_bp, *, chains=None, windowBP=100000, windowCount=256, maxLagBP=50000,
                          workingQuantile=0.75, bootstrapDraws=500, randSeed=1729, minWindowCount=20, acfThreshold=0.1,
                          acfSmoothingBP=250, crossingPersistenceBP=250, minFinitePairs=200, minFinitePairCoverage=0.5,
                          period_diagnostics=True, _margin=None):
    """`cchooseDependenceSpan` of the resident matrices of `chains` (default: every chain) named `names`."""
    listed = list(range(len(batch.chain_lens))) if chains is None else [int(c) for c in chains]
    names = list(names)
    st = Settings(len(names), len(listed), interval_bp, windowBP, windowCount, maxLagBP, workingQuantile, bootstrapDraws, randSeed,
                  minWindowCount, acfThreshold, acfSmoothingBP, crossingPersistenceBP, minFinitePairs, minFinitePairCoverage)
    for c in listed:
        if not 0 <= c < len(batch.chain_lens):
            raise ValueError("chain index out of range")
    lengths = [int(batch.chain_lens[c]) for c in listed]
    row_count = check_shapes([(batch.m, n) for n in lengths], ["f"] * len(lengths))
    return choose(names, lengths, row_count, BatchBackend(batch, listed, st), st, want_period=bool(period_diagnostics),
                  margin=_margin)
