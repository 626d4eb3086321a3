"""The robust null of a ROCCO score track on the device: drop-ins for the reference's `estimateROCCONull` (peaks.py:499-540),
`_prepareNullResidualTemplate` (1077-1122) and `_estimateTemplateScale` (543-556), all built on `_selectRobustNullSupport`
(418-496) and `_halfSampleMode` (312-339).

Same argument names, coercions, detail keys / strings and `ValueError` texts as the originals; every check runs before any GPU
call.  The track is sorted on the device (csrc/csr_null.h); the cutoff, the half-sample mode, the order statistics of the
residuals, the stable compaction of the support, NumPy-order sums and the template are device work, the scalars between them are
composed by the C ABI (`csr_null_*`, `csr_batch_null_*`).  Every number equals the reference's bit for bit.  No CPU fallback --
with ONE exception the reference forces:

Host-decided tracks.  When the central support holds fewer than max(16, ceil(0.05 n)) values (always so below 16 values) the
reference takes `np.argsort(|z - centre|)[:minSupport]`, an unstable sort whose tie order -- and with it the order in which the
support's standard deviation is summed -- the values do not determine.  Such a track is decided by the same NumPy calls on the
host (`_host_null`), as `segments` does for its undetermined views, and the result says so (`decided_on_host: True`).

Negative zeros.  `np.sort` does not order -0.0 against +0.0; the device key does (-0.0 first).  With -0.0 in a track the results
can therefore differ from the reference's in the SIGN OF A ZERO, and in nothing else (they compare equal with `==`).
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib as L

TINY = float(np.finfo(np.float64).tiny)
_QMETHOD = "interpolated_inverted_cdf"
_BULK = ("lower_bulk", "full_track")
_CENTER = ("half_sample_mode", "median")
_METHOD = ("mode_centered_central_support", "mode_centered_nearest_support")


def _as_float_vector(name: str, values) -> np.ndarray:
    """peaks.py:126-134."""
    arr = np.asarray(values, dtype=np.float64)
    if arr.ndim != 1:
        raise ValueError(f"`{name}` must be one-dimensional")
    if arr.size == 0:
        raise ValueError(f"`{name}` must be non-empty")
    if not np.all(np.isfinite(arr)):
        raise ValueError(f"`{name}` contains non-finite values")
    return np.ascontiguousarray(arr)


# ---------------------------------------------------------------------------------------------------------------
# host-decided tracks: the reference's steps in NumPy
# ---------------------------------------------------------------------------------------------------------------
def _half_sample_mode(v: np.ndarray) -> float:
    while v.size > 3:
        w = (v.size + 1) // 2
        start = int(np.argmin(v[w - 1:] - v[: v.size - w + 1]))      # the first minimum
        v = v[start:start + w]
    if v.size == 1:
        return float(v[0])
    if v.size == 2 or float(v[1] - v[0]) <= float(v[2] - v[1]):
        return float(np.mean(v[:2]))
    return float(np.mean(v[1:]))


def _scale_parts(x: np.ndarray):
    mad = 1.4826 * float(np.median(np.abs(x - np.median(x))))
    pct = np.percentile(x, [25, 75]) if x.size >= 4 else None       # what scipy.stats.iqr(x, rng=(25, 75)) subtracts
    iqr = float(pct[1] - pct[0]) / 1.349 if x.size >= 4 else 0.0
    sd = float(np.std(x, ddof=1)) if x.size >= 2 else 0.0
    return mad, iqr, sd


def _host_support(z: np.ndarray, bulk_quantile: float):
    n = int(z.size)
    q = float(np.clip(bulk_quantile, 0.05, 0.95))
    min_support = max(16, int(math.ceil(0.05 * n)))
    cutoff = float(np.quantile(z, q, method=_QMETHOD))
    bulk, source = z[z <= cutoff], _BULK[0]
    if bulk.size < min_support:
        bulk, source = z, _BULK[1]
    bulk = np.sort(np.asarray(bulk, dtype=np.float64))
    mode = bulk.size >= 4
    center = float(_half_sample_mode(bulk) if mode else np.median(bulk))
    resid = bulk - center
    mad, iqr, sd = _scale_parts(resid)
    scale = float(max(mad, iqr, sd, 1.0e-6))
    half = float(np.quantile(np.abs(resid), 0.50, method=_QMETHOD)) if resid.size >= 4 else scale
    radius = float(max(2.5 * scale, half, 1.0e-6))
    support, method = z[np.abs(z - center) <= radius], _METHOD[0]
    if support.size < min_support:
        order = np.argsort(np.abs(z - center))
        support, method = z[np.asarray(order[:min_support], dtype=np.int64)], _METHOD[1]
    meta = {"null_method": method, "support_size": int(support.size), "lower_bulk_size": int(bulk.size), "bulk_quantile": q,
            "bulk_cutoff": cutoff, "provisional_center": center, "center_method": f"{source}_{_CENTER[0] if mode else _CENTER[1]}",
            "support_radius": radius, "support_scale": scale}
    return np.asarray(support, dtype=np.float64), meta


def _details(meta: dict, center: float, scale: float, n: int) -> dict:
    return {"null_method": str(meta["null_method"]), "scale_method": "central_support_mad", "support_size": int(meta["support_size"]),
            "lower_bulk_size": int(meta["lower_bulk_size"]), "bulk_quantile": float(meta["bulk_quantile"]),
            "bulk_cutoff": float(meta["bulk_cutoff"]), "provisional_center": float(meta["provisional_center"]),
            "center_method": str(meta["center_method"]), "support_radius": float(meta["support_radius"]),
            "support_scale": float(meta["support_scale"]), "null_center": float(center), "null_scale": float(scale),
            "null_center_shift_from_zero": float(center), "support_fraction": float(meta["support_size"] / max(int(n), 1))}


def _host_null(z: np.ndarray, bulk_quantile: float):
    support, meta = _host_support(z, bulk_quantile)
    center = float(meta["provisional_center"])
    scale = float(max(*_scale_parts(support - center), 1.0e-6))
    return center, scale, _details(meta, center, scale, z.size)


def _host_template(z: np.ndarray, center: float, scale: float, bulk_quantile: float):
    centered = z - float(center)
    support, meta = _host_support(z, bulk_quantile)
    vals = support - float(center)
    if vals.size < 4:
        vals = centered
    clip_abs = float(max(np.quantile(np.abs(vals), 0.95, method=_QMETHOD) if vals.size > 0 else 0.0, scale, 1.0e-6))
    t = np.clip(centered, -clip_abs, clip_abs).astype(np.float64, copy=False)
    t = t - float(np.mean(t))
    sd = float(np.std(t, ddof=1)) if t.size >= 2 else 0.0
    t = t * (float(scale) / sd) if np.isfinite(sd) and sd > TINY else np.full_like(t, 0.0, dtype=np.float64)
    return t, {"clip_abs": clip_abs, "template_std": float(np.std(t, ddof=1)) if t.size >= 2 else 0.0,
               "template_mean": float(np.mean(t)), "template_support_radius": float(meta["support_radius"]),
               "template_support_size": float(meta["support_size"])}


# ---------------------------------------------------------------------------------------------------------------
# the device's answer as the reference's dicts
# ---------------------------------------------------------------------------------------------------------------
def _meta_of(o) -> dict:
    return {"null_method": _METHOD[o.null_method], "support_size": int(o.support_size), "lower_bulk_size": int(o.lower_bulk_size),
            "bulk_quantile": float(o.bulk_quantile), "bulk_cutoff": float(o.bulk_cutoff),
            "provisional_center": float(o.provisional_center),
            "center_method": f"{_BULK[o.bulk_source]}_{_CENTER[o.center_method]}", "support_radius": float(o.support_radius),
            "support_scale": float(o.support_scale)}


def _template_meta_of(o) -> dict:
    return {"clip_abs": float(o.clip_abs), "template_std": float(o.template_std), "template_mean": float(o.template_mean),
            "template_support_radius": float(o.support_radius), "template_support_size": float(o.support_size)}


def chain_result(o, n: int) -> dict:
    """One record of csr_batch_null_prepare / csr_null_prepare (not host-decided) as rocco_null returns it."""
    center, scale = float(o.null_center), float(o.null_scale)
    return {"null_center": center, "null_scale": scale, "details": _details(_meta_of(o), center, scale, n),
            "template_meta": _template_meta_of(o), "decided_on_host": False}


def host_result(z: np.ndarray, bulk_quantile: float):
    """A host-decided track: (record as chain_result gives it, template)."""
    center, scale, details = _host_null(z, bulk_quantile)
    template, meta = _host_template(z, center, scale, bulk_quantile)
    return {"null_center": center, "null_scale": scale, "details": details, "template_meta": meta, "decided_on_host": True}, template


def _device_prepare(z: np.ndarray, bulk_quantile: float, given=None):
    L.require_gpu()
    out = L.NullOut()
    template = np.empty(z.shape[0], np.float64)
    g = None if given is None else np.asarray(given, np.float64)
    L.check_value(L.lib().csr_null_prepare(L.dp(z), z.shape[0], float(bulk_quantile), L.dp(g), C.byref(out), L.dp(template)))
    return out, template


# ---------------------------------------------------------------------------------------------------------------
# drop-ins on host arrays
# ---------------------------------------------------------------------------------------------------------------
def null_and_template(scoreTrack, bulkQuantile: float = 0.60) -> dict:
    """Both reference calls of peaks.py:1153-1162 in one device run: chain_result's record plus `template`."""
    z = _as_float_vector("scoreTrack", scoreTrack)
    out, template = _device_prepare(z, bulkQuantile)
    if out.host_fallback:
        res, template = host_result(z, bulkQuantile)
    else:
        res = chain_result(out, z.shape[0])
    res["template"] = template
    return res


def estimateROCCONull(scoreTrack, bulkQuantile: float = 0.60):
    """peaks.py:499-540: (nullCenter, nullScale, details)."""
    res = null_and_template(scoreTrack, bulkQuantile)
    return res["null_center"], res["null_scale"], res["details"]


def prepare_null_residual_template(scoreTrack, nullCenter, nullScale, bulkQuantile: float = 0.60):
    """peaks.py:1077-1122 `_prepareNullResidualTemplate`: (template, meta) around the given centre and scale."""
    z = np.ascontiguousarray(np.asarray(scoreTrack, dtype=np.float64))
    _as_float_vector("values", z)
    out, template = _device_prepare(z, bulkQuantile, given=[float(nullCenter), float(nullScale)])
    if out.host_fallback:
        return _host_template(z, float(nullCenter), float(nullScale), bulkQuantile)
    return template, _template_meta_of(out)


def estimate_template_scale(template) -> float:
    """peaks.py:543-556 `_estimateTemplateScale`."""
    t = _as_float_vector("template", template)
    L.require_gpu()
    out = np.empty(4, np.float64)
    L.check_value(L.lib().csr_null_scale(L.dp(t), t.shape[0], L.dp(out)))
    return float(out[0])


def sort_values(values) -> np.ndarray:
    """The device's ascending sort of a finite float64 vector (what every order statistic above is read from)."""
    v = _as_float_vector("values", values)
    L.require_gpu()
    out = np.empty(v.shape[0], np.float64)
    L.check_value(L.lib().csr_null_sort(L.dp(v), v.shape[0], L.dp(out)))
    return out
