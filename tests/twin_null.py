"""CPU twins of the robust null of a ROCCO score track (reference: peaks.py:312-339 `_halfSampleMode`, 418-496
`_selectRobustNullSupport`, 499-540 `estimateROCCONull`, 543-556 `_estimateTemplateScale`, 1077-1122
`_prepareNullResidualTemplate`), written in this project's words and reviewed against those lines.

Two restatements of the same computation:
  plain_*        the reference's steps with np.sort, np.quantile, np.median, scipy.stats.iqr, np.std, np.clip;
  structured_*   the device's decomposition: every order statistic is a rank (+ lerp) of ONE sorted copy of the track, the
                 half-sample mode is a level-by-level first arg-min, every sum is the ascending fold of pairwise-tree sums of
                 chunks of 8192 values, the support is a compaction in track order.
tests/test_null_twin.py holds them equal bit for bit; tests/test_gpu_null.py compares the device with the plain one.
"""
from __future__ import annotations

import math

import numpy as np

from twin_dwb import lerp, np_order_sum, quantile_ranks

try:
    from scipy import stats as _stats

    def _iqr(x):
        return float(_stats.iqr(x, rng=(25, 75)))
except ImportError:        # scipy.stats.iqr(x, rng=(25, 75)) is this difference of two NumPy percentiles
    def _iqr(x):
        p = np.percentile(x, [25, 75])
        return float(np.subtract(p[1], p[0]))

TINY = float(np.finfo(np.float64).tiny)
QM = "interpolated_inverted_cdf"
CENTRAL, NEAREST = "mode_centered_central_support", "mode_centered_nearest_support"


def as_vector(name, values):
    a = np.asarray(values, dtype=np.float64)
    if a.ndim != 1:
        raise ValueError(f"`{name}` must be one-dimensional")
    if a.size == 0:
        raise ValueError(f"`{name}` must be non-empty")
    if not np.all(np.isfinite(a)):
        raise ValueError(f"`{name}` contains non-finite values")
    return a


def min_support(n: int) -> int:
    return max(16, int(math.ceil(0.05 * n)))


# ---------------------------------------------------------------------------------------------------------------
# plain
# ---------------------------------------------------------------------------------------------------------------
def plain_half_sample_mode(v) -> float:
    """Recursive shortest half: the FIRST start with the smallest v[start + window - 1] - v[start], strict '<'."""
    v = np.asarray(v, np.float64)
    n = int(v.size)
    if n == 0:
        return 0.0
    if n == 1:
        return float(v[0])
    if n == 2:
        return float(np.mean(v))
    if n == 3:
        return float(np.mean(v[:2])) if float(v[1] - v[0]) <= float(v[2] - v[1]) else float(np.mean(v[1:]))
    w = int(math.ceil(n / 2))
    best, width = 0, float(v[w - 1] - v[0])
    for s in range(1, n - w + 1):
        cand = float(v[s + w - 1] - v[s])
        if cand < width:
            best, width = s, cand
    return plain_half_sample_mode(v[best:best + w])


def plain_triple(x):
    """(MAD * 1.4826, IQR / 1.349, std with ddof 1) with the reference's size guards."""
    x = np.asarray(x, np.float64)
    mad = 1.4826 * float(np.median(np.abs(x - np.median(x))))
    iqr = _iqr(x) / 1.349 if x.size >= 4 else 0.0
    sd = float(np.std(x, ddof=1)) if x.size >= 2 else 0.0
    return mad, iqr, sd


def plain_support(values, q=0.60):
    z = as_vector("values", values)
    n = int(z.size)
    q = float(np.clip(q, 0.05, 0.95))
    need = min_support(n)
    cutoff = float(np.quantile(z, q, method=QM))
    bulk, source = z[z <= cutoff], "lower_bulk"
    if bulk.size < need:
        bulk, source = z, "full_track"
    bulk = np.sort(bulk)
    if bulk.size >= 4:
        center, how = float(plain_half_sample_mode(bulk)), f"{source}_half_sample_mode"
    else:
        center, how = float(np.median(bulk)), f"{source}_median"
    r = bulk - center
    scale = float(max(*plain_triple(r), 1.0e-6))
    half = float(np.quantile(np.abs(r), 0.50, method=QM)) if r.size >= 4 else scale
    radius = float(max(2.5 * scale, half, 1.0e-6))
    support, method = z[np.abs(z - center) <= radius], CENTRAL
    if support.size < need:
        support, method = z[np.argsort(np.abs(z - center))[:need]], NEAREST
    return support, dict(null_method=method, support_size=int(support.size), lower_bulk_size=int(bulk.size), bulk_quantile=q,
                         bulk_cutoff=cutoff, provisional_center=center, center_method=how, support_radius=radius,
                         support_scale=scale)


def details_of(meta, center, scale, n):
    d = dict(meta)
    d.update(scale_method="central_support_mad", null_center=float(center), null_scale=float(scale),
             null_center_shift_from_zero=float(center), support_fraction=float(meta["support_size"] / max(int(n), 1)))
    return d


def plain_null(score, q=0.60):
    z = as_vector("scoreTrack", score)
    support, meta = plain_support(z, q)
    center = float(meta["provisional_center"])
    scale = float(max(*plain_triple(support - center), 1.0e-6))
    return center, scale, details_of(meta, center, scale, z.size)


def plain_template(score, center, scale, q=0.60):
    z = np.asarray(score, np.float64)
    centered = z - float(center)
    support, meta = plain_support(z, q)
    vals = support - float(center)
    if vals.size < 4:
        vals = centered
    clip_abs = float(max(np.quantile(np.abs(vals), 0.95, method=QM) if vals.size > 0 else 0.0, scale, 1.0e-6))
    t = np.clip(centered, -clip_abs, clip_abs)
    t = t - float(np.mean(t))
    sd = float(np.std(t, ddof=1)) if t.size >= 2 else 0.0
    t = t * (float(scale) / sd) if np.isfinite(sd) and sd > TINY else np.zeros_like(t)
    return t, dict(clip_abs=clip_abs, template_std=float(np.std(t, ddof=1)) if t.size >= 2 else 0.0,
                   template_mean=float(np.mean(t)), template_support_radius=float(meta["support_radius"]),
                   template_support_size=float(meta["support_size"]))


def plain_scale(template) -> float:
    return float(max(*plain_triple(as_vector("template", template)), 1.0e-6))


def plain_all(score, q=0.60):
    """What DeviceBatch.rocco_null returns for a chain, plus the template."""
    center, scale, details = plain_null(score, q)
    template, meta = plain_template(score, center, scale, q)
    return dict(null_center=center, null_scale=scale, details=details, template_meta=meta, template=template,
                decided_on_host=details["null_method"] == NEAREST)


# ---------------------------------------------------------------------------------------------------------------
# structured
# ---------------------------------------------------------------------------------------------------------------
def sorted_quantile(s, q):
    lo, hi, g = quantile_ranks(len(s), q)
    return lerp(float(s[lo]), float(s[hi]), g)


def sorted_percentile(s, q):
    """np.percentile(.., method="linear") at q in [0, 1): virtual index (n - 1) q."""
    v = (len(s) - 1) * q
    lo = math.floor(v)
    return lerp(float(s[lo]), float(s[min(lo + 1, len(s) - 1)]), v - lo)


def sorted_median(s):
    n = len(s)
    return float(s[n // 2]) if n % 2 else (float(s[n // 2 - 1]) + float(s[n // 2])) / 2.0


def order_std(x):
    """np.std(x, ddof=1): both sums in NumPy's order."""
    x = np.asarray(x, np.float64)
    mean = np_order_sum(x) / x.size
    d = x - mean
    return math.sqrt(np_order_sum(d * d) / (x.size - 1))


def level_half_sample_mode(v) -> float:
    """One first arg-min per level over the window starts, until <= 3 values are left."""
    v = np.asarray(v, np.float64)
    lo, n = 0, int(v.size)
    while n > 3:
        w = (n + 1) // 2
        widths = v[lo + w - 1:lo + n] - v[lo:lo + n - w + 1]
        lo, n = lo + int(np.argmin(widths)), w          # np.argmin: the lowest index among equal widths
    if n == 1:
        return float(v[lo])
    if n == 2 or float(v[lo + 1] - v[lo]) <= float(v[lo + 2] - v[lo + 1]):
        return (float(v[lo]) + float(v[lo + 1])) / 2.0
    return (float(v[lo + 1]) + float(v[lo + 2])) / 2.0


def structured_triple(sorted_x, abs_dev_sorted, in_order):
    """The triple from a sorted copy of x, the sorted |x - median(x)| and x in summation order."""
    n = len(sorted_x)
    mad = 1.4826 * sorted_median(abs_dev_sorted)
    iqr = (sorted_percentile(sorted_x, 0.75) - sorted_percentile(sorted_x, 0.25)) / 1.349 if n >= 4 else 0.0
    sd = order_std(in_order) if n >= 2 else 0.0
    return mad, iqr, sd


def structured_all(score, q=0.60, given=None):
    z = as_vector("scoreTrack", score)
    n = int(z.size)
    q = float(np.clip(q, 0.05, 0.95))
    need = min_support(n)
    s = np.sort(z)                                      # the ONE sort
    cutoff = sorted_quantile(s, q)
    m, source = int(np.searchsorted(s, cutoff, side="right")), "lower_bulk"
    if m < need:
        m, source = n, "full_track"
    bulk = s[:m]
    if m >= 4:
        center, how = level_half_sample_mode(bulk), f"{source}_half_sample_mode"
    else:
        center, how = sorted_median(bulk), f"{source}_median"
    r = bulk - center                                   # sorted, because the bulk is
    scale = float(max(*structured_triple(r, np.sort(np.abs(r - sorted_median(r))), r), 1.0e-6))
    half = sorted_quantile(np.sort(np.abs(r)), 0.50) if m >= 4 else scale
    radius = float(max(2.5 * scale, half, 1.0e-6))
    flags = np.abs(z - center) <= radius
    pos = np.cumsum(flags) - flags                      # exclusive prefix sum: where each member lands
    support = np.empty(int(flags.sum()), np.float64)
    support[pos[flags]] = z[flags]                      # the scatter, in track order
    method = CENTRAL
    first = int(np.searchsorted(s - center, -radius, side="left"))     # the support is s[first : first + size] as a set
    if support.size < need:
        support, method = z[np.argsort(np.abs(z - center))[:need]], NEAREST
        sup_sorted = np.sort(support)
    else:
        sup_sorted = s[first:first + support.size]
    meta = dict(null_method=method, support_size=int(support.size), lower_bulk_size=m, bulk_quantile=q, bulk_cutoff=cutoff,
                provisional_center=center, center_method=how, support_radius=radius, support_scale=scale)
    cs_sorted, cs = sup_sorted - center, support - center
    null_scale = float(max(*structured_triple(cs_sorted, np.sort(np.abs(cs - sorted_median(cs_sorted))), cs), 1.0e-6))
    t_center, t_scale = (center, null_scale) if given is None else (float(given[0]), float(given[1]))
    centered = z - t_center
    vals = support - t_center
    if vals.size < 4:
        vals = centered
    clip_abs = float(max(sorted_quantile(np.sort(np.abs(vals)), 0.95), t_scale, 1.0e-6))
    t = np.minimum(np.maximum(centered, -clip_abs), clip_abs)
    t = t - np_order_sum(t) / n
    sd = order_std(t) if n >= 2 else 0.0
    t = t * (t_scale / sd) if np.isfinite(sd) and sd > TINY else np.zeros_like(t)
    tmeta = dict(clip_abs=clip_abs, template_std=order_std(t) if n >= 2 else 0.0, template_mean=np_order_sum(t) / n,
                 template_support_radius=float(radius), template_support_size=float(support.size))
    return dict(null_center=center, null_scale=null_scale, details=details_of(meta, center, null_scale, n), template_meta=tmeta,
                template=t, decided_on_host=method == NEAREST)


def structured_scale(template) -> float:
    x = as_vector("template", template)
    s = np.sort(x)
    return float(max(*structured_triple(s, np.sort(np.abs(s - sorted_median(s))), x), 1.0e-6))


# ---------------------------------------------------------------------------------------------------------------
# the case table shared by the CPU and the GPU tests
# ---------------------------------------------------------------------------------------------------------------
SIZES = (1, 2, 3, 4, 5, 15, 16, 17, 26, 27, 64, 129, 8191, 8192, 8193, 16385, 20000)
KINDS = ("gauss", "rounded", "constant")


def track(kind: str, n: int, seed: int = 7) -> np.ndarray:
    """gauss: a Gaussian bulk plus a shifted tenth; rounded: the same at two decimals (many ties); constant."""
    if kind == "constant":
        return np.full(n, 0.75)
    rng = np.random.default_rng(seed * 1000003 + n)
    z = rng.standard_normal(n)
    hot = rng.random(n) < 0.10
    z[hot] = z[hot] + 4.0
    z = z + 0.0                                         # (no -0.0: see consenrich_amd.null)
    return np.round(z, 2) + 0.0 if kind == "rounded" else z


def short_support_track() -> np.ndarray:
    """n = 1000 at bulk quantile 0.05: the lowest twentieth is an evenly spaced cluster (exact binary steps, so every window of
    a level is equally wide and the first one wins: the centre sits at the cluster's low edge), the rest lies far away.  The
    central support then misses the cluster's top values and falls short of minSupport = 50: the nearest-support branch."""
    z = np.concatenate([np.arange(50) * 0.015625, 100.0 + np.arange(950) * 0.25])
    return np.random.default_rng(11).permutation(z)


def same(a, b) -> bool:
    """Two results of *_all agree bit for bit: every number, every string, every template value."""
    if a["decided_on_host"] != b["decided_on_host"]:
        return False
    for k in ("null_center", "null_scale"):
        if np.float64(a[k]).tobytes() != np.float64(b[k]).tobytes():
            return False
    for part in ("details", "template_meta"):
        if set(a[part]) != set(b[part]):
            return False
        for k, v in a[part].items():
            w = b[part][k]
            if isinstance(v, str) or isinstance(w, str):
                if v != w:
                    return False
            elif np.float64(v).tobytes() != np.float64(w).tobytes():
                return False
    return np.asarray(a["template"], np.float64).tobytes() == np.asarray(b["template"], np.float64).tobytes()


def first_difference(a, b) -> str:
    for k in ("decided_on_host", "null_center", "null_scale"):
        if a[k] != b[k]:
            return f"{k}: {a[k]!r} != {b[k]!r}"
    for part in ("details", "template_meta"):
        for k in sorted(set(a[part]) | set(b[part])):
            if a[part].get(k) != b[part].get(k):
                return f"{part}[{k}]: {a[part].get(k)!r} != {b[part].get(k)!r}"
    ta, tb = np.asarray(a["template"]), np.asarray(b["template"])
    if ta.shape != tb.shape:
        return f"template shapes {ta.shape} != {tb.shape}"
    bad = np.flatnonzero(ta != tb)
    return f"template differs at {bad[:5].tolist()} ({bad.size} values)" if bad.size else "only the sign of a zero differs"
