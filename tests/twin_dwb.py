"""Pure-Python / NumPy twin of the stationary-null dependent wild bootstrap (DWB) natives and of the panel built from them
(reference: pyx:9283-9424 `cGenerateDWBMultipliersFromNoise`, `cApplyStationaryNullDWB`, `cStationaryNullDWBDraw`;
peaks.py:559-830 `_calibrateStationaryNullDWB`).  TEST INFRASTRUCTURE: explicit ordered loops, no device, no product code.

The natives are pinned to the compiled reference's recordings (tests/golden/dwb/dwb_*.npz, tests/test_dwb_twin.py).  The panel
composition cannot be run through the reference where the fixtures are made (its `consenrich.core` does not import there), so
`panel()` is this project's restatement of peaks.py:593-805 from plain `np.quantile` / `np.mean` on whole draws; `panel(fast=True)`
is the same composition from order statistics and `np_order_sum`, the way the device path is put together."""
from __future__ import annotations

import ctypes
import ctypes.util
import math

import numpy as np

TINY = float(np.finfo(np.float64).tiny)
QMETHOD = "interpolated_inverted_cdf"


# ---------------------------------------------------------------------------------------------------------------
# the three natives
# ---------------------------------------------------------------------------------------------------------------
def kernel_code(kernel) -> int:
    name = str(kernel).strip().lower().replace("-", "_")
    if name in ("bartlett", "triangle", "triangular"):
        return 0
    if name == "parzen":
        return 1
    if name in ("qs", "quadratic_spectral", "quadraticspectral"):
        return 2
    raise ValueError(f"Unknown DWB kernel: {kernel}")


def _c_int(v) -> int:
    v = int(v)
    if not -(1 << 31) <= v < (1 << 31):
        raise OverflowError("value too large to convert to int")
    return v


def max_lag(bandwidth: int, code: int) -> int:
    bw = bandwidth if bandwidth >= 2 else 2
    return max(8 * bw, 32) if code == 2 else bw


_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.sincos.argtypes = [ctypes.c_double, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]
_libm.sincos.restype = None


def _sincos(y: float):
    """The C library's sincos: the reference, built with -fno-math-errno, gets sin(y) and cos(y) of the quadratic-spectral kernel
    from ONE sincos call, whose sine differs from sin()'s by an ulp at isolated arguments (bandwidth 64, lag 88)."""
    s, c = ctypes.c_double(), ctypes.c_double()
    _libm.sincos(float(y), ctypes.byref(s), ctypes.byref(c))
    return s.value, c.value


def kernel_value(code: int, lag: int, bandwidth: int) -> float:
    bw = float(bandwidth if bandwidth >= 1 else 1)
    ax = math.fabs(float(lag)) / bw
    if code == 0:
        return 1.0 - ax if ax <= 1.0 else 0.0
    if code == 1:
        if ax <= 0.5:
            return 1.0 - 6.0 * ax * ax + 6.0 * ax * ax * ax
        if ax <= 1.0:
            return 2.0 * (1.0 - ax) * (1.0 - ax) * (1.0 - ax)
        return 0.0
    if ax < 1.0e-12:
        return 1.0
    y = (6.0 * math.pi * ax) / 5.0
    sin_y, cos_y = _sincos(y)
    return (25.0 / (12.0 * math.pi * math.pi * ax * ax)) * ((sin_y / max(y, 1.0e-12)) - cos_y)


def weights(bandwidth: int, code: int) -> np.ndarray:
    bw = bandwidth if bandwidth >= 2 else 2
    lagmax = max_lag(bw, code)
    w = [kernel_value(code, j - lagmax, bw) for j in range(2 * lagmax + 1)]
    norm_sq = 0.0
    for v in w:
        norm_sq += v * v
    norm = math.sqrt(max(norm_sq, TINY))
    return np.array([v / norm for v in w], np.float64)


def _f64(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(-1), dtype=np.float64)


def cGenerateDWBMultipliersFromNoise(noise, bandwidth, kernel="bartlett"):
    bandwidth = _c_int(bandwidth)
    bw = bandwidth if bandwidth >= 2 else 2
    code = kernel_code(kernel)
    lagmax = max_lag(bw, code)
    z = _f64(noise)
    n = z.shape[0] - 2 * lagmax
    if n <= 0:
        raise ValueError("noise length is too short for the requested DWB bandwidth")
    w = weights(bw, code).tolist()
    zl = z.tolist()
    u = [0.0] * n
    mean = 0.0
    for i in range(n):
        v = 0.0
        for j, wj in enumerate(w):
            v += zl[i + j] * wj
        u[i] = v
        mean += v
    mean = mean / float(n)
    if n >= 2:
        var = 0.0
        for i in range(n):
            d = u[i] - mean
            var += d * d
        sd = math.sqrt(var / float(n - 1)) if var == var and var >= 0.0 else float("nan")
    else:
        sd = 0.0
    if (not math.isfinite(sd)) or sd <= TINY:
        return np.ones(n, np.float64)
    return np.array([(u[i] - mean) / sd for i in range(n)], np.float64)


def cApplyStationaryNullDWB(template, multipliers):
    t, m = _f64(template), _f64(multipliers)
    n = t.shape[0]
    if m.shape[0] != n:
        raise ValueError("template and multipliers must have the same length")
    tl, ml = t.tolist(), m.tolist()
    out = [0.0] * n
    mean = 0.0
    for i in range(n):
        out[i] = tl[i] * ml[i]
        mean += out[i]
    if n > 0:
        mean = mean / float(n)
        for i in range(n):
            out[i] = out[i] - mean
    return np.array(out, np.float64)


def cStationaryNullDWBDraw(template, bandwidth, rng, kernel="bartlett"):
    t = _f64(template)
    bandwidth = _c_int(bandwidth)
    bw = bandwidth if bandwidth >= 2 else 2
    lagmax = max_lag(bw, kernel_code(kernel))
    noise = rng.standard_normal(int(t.shape[0] + 2 * lagmax))
    return cApplyStationaryNullDWB(t, cGenerateDWBMultipliersFromNoise(noise, bw, kernel))


def draw_fast(template, bandwidth, noise, kernel="bartlett"):
    """The same draw with the stencil as a vectorised accumulation over the taps (ascending j, separate multiply and add) and the
    three sums as strictly sequential folds (np.cumsum is one): for the panel tests' longer chains."""
    t = _f64(template)
    n = t.shape[0]
    bw = bandwidth if bandwidth >= 2 else 2
    code = kernel_code(kernel)
    w = weights(bw, code)
    z = _f64(noise)
    assert z.shape[0] == n + 2 * max_lag(bw, code)
    u = np.zeros(n, np.float64)
    for j in range(w.shape[0]):
        u = u + z[j:j + n] * w[j]
    mean = float(np.cumsum(np.concatenate(([0.0], u)))[-1]) / float(n)
    if n >= 2:
        d = u - mean
        sd = float(np.sqrt(np.cumsum(np.concatenate(([0.0], d * d)))[-1] / float(n - 1)))
    else:
        sd = 0.0
    mult = np.ones(n, np.float64) if (not math.isfinite(sd)) or sd <= TINY else (u - mean) / sd
    prod = t * mult
    m2 = float(np.cumsum(np.concatenate(([0.0], prod)))[-1]) / float(n)
    return prod - m2


# ---------------------------------------------------------------------------------------------------------------
# NumPy's summation order (np.sum / np.mean of a contiguous float64 vector) and its inverted-CDF quantile
# ---------------------------------------------------------------------------------------------------------------
CHUNK = 8192


def _pairwise(a, lo, n):
    if n < 8:
        res = 0.0
        for i in range(n):
            res += a[lo + i]
        return res
    if n <= 128:
        r = [a[lo + k] for k in range(8)]
        i = 8
        while i < n - (n % 8):
            for k in range(8):
                r[k] += a[lo + i + k]
            i += 8
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
        while i < n:
            res += a[lo + i]
            i += 1
        return res
    n2 = n // 2
    n2 -= n2 % 8
    return _pairwise(a, lo, n2) + _pairwise(a, lo + n2, n - n2)


def np_order_sum(x) -> float:
    """np.sum(x) of a contiguous float64 vector, in NumPy's order: the ascending fold of the pairwise-tree sums of chunks of
    8192 elements."""
    a = np.asarray(x, np.float64).tolist()
    n = len(a)
    if n == 0:
        return 0.0
    total = None
    for lo in range(0, n, CHUNK):
        s = _pairwise(a, lo, min(CHUNK, n - lo))
        total = s if total is None else total + s
    return float(total)


def quantile_ranks(n: int, q: float):
    """(lo, hi, g) of np.quantile(x, q, method="interpolated_inverted_cdf") on n values."""
    v = n * q - 1.0
    lo = math.floor(v)
    g = v - lo
    hi = lo + 1
    lo_i = int(min(max(lo, 0), n - 1))
    hi_i = int(min(max(hi, 0), n - 1))
    return lo_i, hi_i, float(g)


def lerp(a: float, b: float, g: float) -> float:
    d = b - a
    return float(b - d * (1.0 - g)) if g >= 0.5 else float(a + d * g)


def quantile_from_sorted(xs, q: float) -> float:
    lo, hi, g = quantile_ranks(len(xs), q)
    return lerp(float(xs[lo]), float(xs[hi]), g)


def small_quantile(x, q: float) -> float:
    return quantile_from_sorted(np.sort(np.asarray(x, np.float64)), q)


# ---------------------------------------------------------------------------------------------------------------
# the panel (peaks.py:593-805), one chain
# ---------------------------------------------------------------------------------------------------------------
def tail_quantile(z: float) -> float:
    """peaks.py:609-610: 1 - norm.sf(max(z, 0)) for z > 0, else 0.5 (norm.sf(z) = erfc(z / sqrt 2) / 2)."""
    from scipy import stats

    return 1.0 - float(stats.norm.sf(float(max(z, 0.0)))) if float(z) > 0.0 else 0.5


def stream(seed: int, count: int) -> np.ndarray:
    return np.random.default_rng(int(seed)).standard_normal(int(count))


def _sd1(x) -> float:
    return float(np.std(x, ddof=1)) if len(x) > 1 else 0.0


def thresholds(upper, z, null_center, null_scale, cal_q, floor):
    """peaks.py:632-658 for one z: (empirical upper, threshold offset, empirical scale, threshold, null scale)."""
    emp = float(np.quantile(upper, cal_q, method=QMETHOD))
    f_off, f_scale = (0.0, 0.0) if floor is None else (float(max(floor[0], 0.0)), float(max(floor[1], 0.0)))
    off = float(max(emp, f_off, 0.0))
    if float(z) > 0.0:
        emp_scale = float(max(float(null_scale), off / float(z), 1.0e-6))
    else:
        emp_scale = float(max(float(null_scale), off, 1.0e-6))
    thr = float(null_center + off)
    scale = float(max(emp_scale, f_scale, 1.0e-6))
    return emp, off, emp_scale, thr, scale, f_off, f_scale


def finish(metrics, null_occ, null_soft, cal_q):
    """peaks.py:764-805 for one z."""
    occ_cal = float(np.quantile(null_occ, cal_q, method=QMETHOD))
    soft_cal = float(np.quantile(null_soft, cal_q, method=QMETHOD))
    raw = metrics["observed_tail_occupancy"] - occ_cal
    if not np.isfinite(raw):
        raw = 0.0
    metrics.update(
        null_tail_occupancy=float(np.mean(null_occ)), null_tail_occupancy_calibrated=occ_cal,
        null_tail_occupancy_sd=_sd1(null_occ), null_soft_tail=float(np.mean(null_soft)),
        null_soft_tail_calibrated=soft_cal, null_soft_tail_sd=_sd1(null_soft),
        budget_occupancy_raw=float(max(raw, 0.0)),
        budget_soft_raw=float(np.clip(metrics["observed_soft_tail"] - soft_cal, 0.0, 1.0)))


def panel(score, template, null_center, null_scale, *, z_grid, bandwidth, num_bootstrap=128, kernel="bartlett", seed=0,
          cal_q=0.9, floors=None, tail_quantiles=None, noise=None, fast=False, draw=draw_fast):
    """One chain's panel: {z index: dict of the numeric fields}.  noise: the seed's stream (a longer one serves: draw b uses
    noise[b * stride : (b + 1) * stride]); fast=True composes from order statistics and np_order_sum."""
    score, template = _f64(score), _f64(template)
    n = template.shape[0]
    B = max(int(num_bootstrap), 8)
    cal_q = float(np.clip(cal_q, 0.50, 0.999))
    bw = bandwidth if bandwidth >= 2 else 2
    stride = n + 2 * max_lag(bw, kernel_code(kernel))
    if noise is None:
        noise = stream(seed, B * stride)
    tq = [tail_quantile(z) for z in z_grid] if tail_quantiles is None else [float(q) for q in tail_quantiles]
    draws = [draw(template, bw, noise[b * stride:(b + 1) * stride], kernel) for b in range(B)]
    out = []
    for k, z in enumerate(z_grid):
        if fast:
            upper = np.array([small_quantile(d, tq[k]) for d in draws], np.float64)
        else:
            upper = np.array([float(np.quantile(d, tq[k], method=QMETHOD)) for d in draws], np.float64)
        emp, off, emp_scale, thr, scale, f_off, f_scale = thresholds(upper, z, null_center, null_scale, cal_q,
                                                                     None if floors is None else floors[k])
        s = max(scale, TINY)
        off2 = float(thr) - float(null_center)      # peaks.py:751: the offset the second loop compares against
        if fast:
            obs_occ = float(np.count_nonzero(score > thr)) / score.shape[0]
            obs_soft = np_order_sum(np.clip((score - thr) / s, 0.0, None)) / score.shape[0]
            occ = np.array([float(np.count_nonzero(d > off2)) / n for d in draws], np.float64)
            soft = np.array([np_order_sum(np.clip((d - off2) / s, 0.0, None)) / n for d in draws], np.float64)
        else:
            obs_occ = float(np.mean(score > thr))
            obs_soft = float(np.mean(np.clip((score - thr) / s, 0.0, None)))
            occ = np.array([float(np.mean(d > off2)) for d in draws], np.float64)
            soft = np.array([float(np.mean(np.clip((d - off2) / s, 0.0, None))) for d in draws], np.float64)
        m = dict(threshold_z=float(max(z, 0.0)), tail_quantile=tq[k], upper_tail_offsets=upper,
                 bootstrap_upper_tail_offset=emp, upper_tail_offset_mean=float(np.mean(upper)),
                 upper_tail_offset_sd=_sd1(upper), threshold_offset_floor=f_off, null_scale_floor=f_scale,
                 threshold_offset=off, empirical_null_scale=emp_scale, null_center=float(null_center), null_scale=scale,
                 threshold=thr, pooled_floor_applied=bool((f_off > emp + 1.0e-12) or (f_scale > emp_scale + 1.0e-12)),
                 observed_tail_occupancy=obs_occ, observed_soft_tail=obs_soft, null_occupancies=occ, null_soft_tails=soft,
                 num_bootstrap=B, null_quantile=cal_q)
        finish(m, occ, soft, cal_q)
        out.append(m)
    return out


def same_panel(a, b):
    """Names of the fields of two panels' results (lists over z) that differ: floats by their 64-bit patterns."""
    bad = []
    for k, (ma, mb) in enumerate(zip(a, b)):
        if sorted(ma) != sorted(mb):
            bad.append((k, "keys"))
            continue
        for key, va in ma.items():
            vb = mb[key]
            if isinstance(va, (bool, int)) or isinstance(vb, (bool, int)):
                ok = va == vb and type(va) is type(vb)
            else:
                xa, xb = np.atleast_1d(np.asarray(va, np.float64)), np.atleast_1d(np.asarray(vb, np.float64))
                ok = xa.shape == xb.shape and np.array_equal(xa.view(np.uint64), xb.view(np.uint64))
            if not ok:
                bad.append((k, key))
    return bad
