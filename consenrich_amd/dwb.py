"""Stationary-null dependent wild bootstrap (DWB) on the device: drop-ins for the reference natives
`cGenerateDWBMultipliersFromNoise`, `cApplyStationaryNullDWB`, `cStationaryNullDWBDraw` (pyx:9283-9424) and the bootstrap panel
of `_calibrateStationaryNullDWB` (peaks.py:559-805) for every chain of one seed in one call.

Same argument names, coercions and `ValueError` texts as the originals; every check runs before any GPU call.  The draws, their
order statistics and their tail statistics come from the C ABI (`csr_dwb_*`, csrc/csr_dwb.h) and equal the reference's values
bit for bit; what is left on the host is the noise stream (NumPy's generator, one stream per seed), the lerp between two order
statistics, and the reductions over the B draws.  No CPU fallback.

What stays with the caller: the dependence span (bandwidth) and the policy that turns the returned metrics into a budget.  The
null centre / scale / template come from `consenrich_amd.null` (host arrays) or `DeviceBatch.rocco_null` (resident: a batch's panel
and replays then take `templates=None`).
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib as L
from ._lib import _c_int, _f64

TINY = float(np.finfo(np.float64).tiny)
_QMETHOD = "interpolated_inverted_cdf"
MAX_Z = 8       # two ranks per z, 16 ranks per draw on the device


def kernel_code(kernel) -> int:
    """pyx:9283-9291."""
    name = str(kernel).strip().lower().replace("-", "_")
    if name in ("bartlett", "triangle", "triangular"):
        return 0
    if name == "parzen":
        return 1
    if name in ("qs", "quadratic_spectral", "quadraticspectral"):
        return 2
    raise ValueError(f"Unknown DWB kernel: {kernel}")


def max_lag(bandwidth: int, kernel="bartlett") -> int:
    """pyx:9294-9302 (a bandwidth below 2 counts as 2)."""
    bw = bandwidth if bandwidth >= 2 else 2
    return max(8 * bw, 32) if kernel_code(kernel) == 2 else bw


def _kname(kernel) -> bytes:
    return str(kernel).encode("utf-8")


def cGenerateDWBMultipliersFromNoise(noise, bandwidth, kernel="bartlett"):
    """pyx:9325-9380: standardised multipliers from supplied Gaussian noise (len(noise) - 2 maxLag values)."""
    bandwidth = _c_int(bandwidth)
    lag = max_lag(bandwidth, kernel)
    z = _f64(noise)
    n = z.shape[0] - 2 * lag
    if n <= 0:
        raise ValueError("noise length is too short for the requested DWB bandwidth")
    L.require_gpu()
    out = np.empty(n, np.float64)
    L.check_value(L.lib().csr_dwb_multipliers(L.dp(z), z.shape[0], bandwidth, _kname(kernel), L.dp(out)))
    return out


def cApplyStationaryNullDWB(template, multipliers):
    """pyx:9383-9412: template * multipliers minus the mean of the products."""
    t, m = _f64(template), _f64(multipliers)
    if m.shape[0] != t.shape[0]:
        raise ValueError("template and multipliers must have the same length")
    out = np.empty(t.shape[0], np.float64)
    if t.shape[0] == 0:
        return out
    L.require_gpu()
    L.check_value(L.lib().csr_dwb_apply(L.dp(t), t.shape[0], L.dp(m), m.shape[0], L.dp(out)))
    return out


def cStationaryNullDWBDraw(template, bandwidth, rng, kernel="bartlett"):
    """pyx:9415-9424: one draw; consumes exactly len(template) + 2 maxLag normals from `rng`."""
    t = _f64(template)
    bandwidth = _c_int(bandwidth)
    lag = max_lag(bandwidth, kernel)
    noise = _f64(rng.standard_normal(int(t.shape[0] + 2 * lag)))
    if t.shape[0] == 0:
        raise ValueError("noise length is too short for the requested DWB bandwidth")
    L.require_gpu()
    out = np.empty(t.shape[0], np.float64)
    L.check_value(L.lib().csr_dwb_draw(L.dp(t), t.shape[0], bandwidth, _kname(kernel), L.dp(noise), noise.shape[0], L.dp(out)))
    return out


# ---------------------------------------------------------------------------------------------------------------
# the panel
# ---------------------------------------------------------------------------------------------------------------
def tail_quantile(z: float) -> float:
    """peaks.py:609-610: the quantile of a draw that is its upper-tail offset at z."""
    if not float(z) > 0.0:
        return 0.5
    from scipy import stats      # the reference's own source of norm.sf; pass tail_quantiles to do without

    return 1.0 - float(stats.norm.sf(float(max(z, 0.0))))


def quantile_ranks(n: int, q: float):
    """np.quantile(x, q, method="interpolated_inverted_cdf") on n values = lerp(sorted[lo], sorted[hi], g)."""
    v = n * q - 1.0
    lo = math.floor(v)
    g = v - lo
    return int(min(max(lo, 0), n - 1)), int(min(max(lo + 1, 0), n - 1)), float(g)


def _lerp(a, b, g):
    d = b - a
    return b - d * (1.0 - g) if g >= 0.5 else a + d * g


def _sd1(x) -> float:
    return float(np.std(x, ddof=1)) if len(x) > 1 else 0.0


def noise_stream(random_seed: int, count: int) -> np.ndarray:
    """The seed's noise: successive `standard_normal` calls of the reference's loop are consecutive slices of this one call."""
    return np.random.default_rng(int(random_seed)).standard_normal(int(count))


def _tail_of_vector(x, thresholds, scales):
    """(counts, soft means) of one host vector at len(thresholds) (threshold, scale) pairs, on the device."""
    x = _f64(x)
    nz = len(thresholds)
    off, sc = np.asarray(thresholds, np.float64), np.asarray(scales, np.float64)
    cnt, soft = np.zeros(nz, np.int64), np.zeros(nz, np.float64)
    L.check_value(L.lib().csr_dwb_tail_stats(None, L.dp(x), x.shape[0], nz, L.dp(off), L.dp(sc), cnt.ctypes.data_as(L.I64P), L.dp(soft)))
    return cnt, soft


def _checked_templates(templates, lens):
    """The chains' templates as float64 vectors; None = the batch's resident ones (DeviceBatch.rocco_null), checked by the library."""
    if templates is None:
        return None
    tmpl = [_f64(t) for t in templates]
    for c in range(len(lens)):
        if tmpl[c].shape[0] != lens[c] or lens[c] <= 0:
            raise ValueError("a template must be as long as its chain's score track and not empty")
        if not np.all(np.isfinite(tmpl[c])):
            raise ValueError("`template` contains non-finite values")
    return tmpl


def _begin_panel(lib, ctx, n_arr, bw_arr, kernel, tmpl, z_stream, n_draws, draws_per_group):
    bw_p = bw_arr.ctypes.data_as(C.POINTER(C.c_int32))
    if tmpl is None:        # the resident templates of the batch context: nothing is uploaded but the noise
        L.check_value(lib.csr_batch_dwb_panel_begin(ctx, bw_p, _kname(kernel), L.dp(z_stream), z_stream.shape[0], n_draws, draws_per_group))
        return
    t_all = np.ascontiguousarray(np.concatenate(tmpl))
    L.check_value(lib.csr_dwb_panel_begin(ctx, len(n_arr), n_arr.ctypes.data_as(L.I64P), bw_p, _kname(kernel), L.dp(t_all), L.dp(z_stream),
                                          z_stream.shape[0], n_draws, draws_per_group))


def _run_panel(ctx, observed, lens, templates, null_centers, null_scales, *, threshold_z_grid, tail_quantiles, bandwidths,
               num_bootstrap, kernel, random_seed, calibration_quantile, pooled_floors, draws_per_group, noise):
    nc = len(lens)
    zs = [float(z) for z in threshold_z_grid]
    nz = len(zs)
    if not 1 <= nz <= MAX_Z:
        raise ValueError(f"threshold_z_grid must hold 1..{MAX_Z} values")
    kernel_code(kernel)     # ValueError before anything else
    B = max(int(num_bootstrap), 8)
    cal_q = float(np.clip(calibration_quantile, 0.50, 0.999))
    tq = [tail_quantile(z) for z in zs] if tail_quantiles is None else [float(q) for q in tail_quantiles]
    if len(tq) != nz:
        raise ValueError("one tail quantile per threshold z")
    bws = [_c_int(b) for b in (bandwidths if np.ndim(bandwidths) else [bandwidths] * nc)]
    centers = [float(v) for v in (null_centers if np.ndim(null_centers) else [null_centers] * nc)]
    scales0 = [float(v) for v in (null_scales if np.ndim(null_scales) else [null_scales] * nc)]
    if not (len(bws) == len(centers) == len(scales0) == nc) or (templates is not None and len(templates) != nc):
        raise ValueError("one bandwidth, null centre, null scale and template per chain")
    tmpl = _checked_templates(templates, lens)
    floors = None
    if pooled_floors is not None:
        floors = np.asarray(pooled_floors, np.float64)
        if floors.shape != (nc, nz, 2):
            raise ValueError("pooled_floors must have shape (chains, z, 2): threshold-offset floor, null-scale floor")
    strides = [lens[c] + 2 * max_lag(bws[c], kernel) for c in range(nc)]
    need = B * max(strides)
    z_stream = noise_stream(random_seed, need) if noise is None else _f64(noise)
    if z_stream.shape[0] < need:
        raise ValueError("noise length is too short for the requested DWB bandwidth")
    L.require_gpu()
    lib = L.lib()
    ranks = np.empty((nc, 2 * nz), np.int64)
    gam = np.empty((nc, nz), np.float64)
    for c in range(nc):
        for k in range(nz):
            ranks[c, 2 * k], ranks[c, 2 * k + 1], gam[c, k] = quantile_ranks(lens[c], tq[k])
    n_arr = np.asarray(lens, np.int64)
    bw_arr = np.asarray(bws, np.int32)
    _begin_panel(lib, ctx, n_arr, bw_arr, kernel, tmpl, z_stream, B, int(draws_per_group))
    try:
        # phase A: two order statistics per (draw, z); the lerp and the reductions over the draws on the host
        os_ = np.empty((nc, B, 2 * nz), np.float64)
        L.check_value(lib.csr_dwb_panel_order_stats(ctx, 2 * nz, ranks.ctypes.data_as(L.I64P), L.dp(os_)))
        out = [[None] * nz for _ in range(nc)]
        off2 = np.empty((nc, nz), np.float64)
        sc = np.empty((nc, nz), np.float64)
        thr = np.empty((nc, nz), np.float64)
        for c in range(nc):
            for k, z in enumerate(zs):
                g = float(gam[c, k])
                upper = np.array([_lerp(float(os_[c, b, 2 * k]), float(os_[c, b, 2 * k + 1]), g) for b in range(B)], np.float64)
                emp = float(np.quantile(upper, cal_q, method=_QMETHOD))
                f_off = float(max(floors[c, k, 0], 0.0)) if floors is not None else 0.0
                f_scale = float(max(floors[c, k, 1], 0.0)) if floors is not None else 0.0
                t_off = float(max(emp, f_off, 0.0))
                if z > 0.0:
                    emp_scale = float(max(scales0[c], t_off / z, 1.0e-6))
                else:
                    emp_scale = float(max(scales0[c], t_off, 1.0e-6))
                thr[c, k] = float(centers[c] + t_off)
                sc[c, k] = float(max(emp_scale, f_scale, 1.0e-6))
                off2[c, k] = float(thr[c, k]) - centers[c]      # peaks.py:751: what the second loop compares the draws with
                out[c][k] = dict(
                    threshold_z=float(max(z, 0.0)), tail_quantile=tq[k], upper_tail_offsets=upper,
                    bootstrap_upper_tail_offset=emp, upper_tail_offset_mean=float(np.mean(upper)),
                    upper_tail_offset_sd=_sd1(upper), threshold_offset_floor=f_off, null_scale_floor=f_scale,
                    threshold_offset=t_off, empirical_null_scale=emp_scale, null_center=centers[c], null_scale=float(sc[c, k]),
                    threshold=float(thr[c, k]),
                    pooled_floor_applied=bool((f_off > emp + 1.0e-12) or (f_scale > emp_scale + 1.0e-12)),
                    num_bootstrap=B, null_quantile=cal_q)
        # phase B: tail occupancy and soft tail of every draw at the thresholds phase A gave
        cnt = np.empty((nc, B, nz), np.int64)
        soft = np.empty((nc, B, nz), np.float64)
        L.check_value(lib.csr_dwb_panel_tail_stats(ctx, nz, L.dp(off2), L.dp(sc), cnt.ctypes.data_as(L.I64P), L.dp(soft)))
    finally:
        L.check(lib.csr_dwb_panel_end(ctx))
    for c in range(nc):
        o_cnt, o_soft = observed(c, thr[c], sc[c])
        for k in range(nz):
            m = out[c][k]
            occ = np.array([int(cnt[c, b, k]) / lens[c] for b in range(B)], np.float64)
            sft = np.ascontiguousarray(soft[c, :, k])
            m["observed_tail_occupancy"] = int(o_cnt[k]) / observed.length(c)
            m["observed_soft_tail"] = float(o_soft[k])
            m["null_occupancies"], m["null_soft_tails"] = occ, sft
            occ_cal = float(np.quantile(occ, cal_q, method=_QMETHOD))
            soft_cal = float(np.quantile(sft, cal_q, method=_QMETHOD))
            raw = m["observed_tail_occupancy"] - occ_cal
            if not np.isfinite(raw):
                raw = 0.0
            m.update(null_tail_occupancy=float(np.mean(occ)), null_tail_occupancy_calibrated=occ_cal,
                     null_tail_occupancy_sd=_sd1(occ), null_soft_tail=float(np.mean(sft)), null_soft_tail_calibrated=soft_cal,
                     null_soft_tail_sd=_sd1(sft), budget_occupancy_raw=float(max(raw, 0.0)),
                     budget_soft_raw=float(np.clip(m["observed_soft_tail"] - soft_cal, 0.0, 1.0)))
    return out


class _HostObserved:
    def __init__(self, tracks):
        self.tracks = tracks

    def length(self, c):
        return self.tracks[c].shape[0]

    def __call__(self, c, thresholds, scales):
        return _tail_of_vector(self.tracks[c], thresholds, scales)


def stationary_null_panel(score_tracks, templates, null_centers, null_scales, *, threshold_z_grid, tail_quantiles=None,
                          bandwidths, num_bootstrap=128, kernel="bartlett", random_seed=0, calibration_quantile=0.9,
                          pooled_floors=None, draws_per_group=0, noise=None):
    """The bootstrap panel of `_calibrateStationaryNullDWB` (peaks.py:593-805) for every chain of one seed.

    score_tracks / templates: one float64 vector per chain (equal lengths per chain); null_centers / null_scales / bandwidths:
    one value per chain (or one for all); threshold_z_grid: up to 8 values; tail_quantiles: the quantile of a draw taken at
    each z (default: the reference's 1 - norm.sf(z), 0.5 for z <= 0); pooled_floors: (chains, z, 2) threshold-offset and
    null-scale floors.  num_bootstrap is raised to 8 and calibration_quantile clipped to [0.5, 0.999] as in the reference.
    draws_per_group bounds the device working set (0 = default) and changes no result; noise: the seed's stream when the caller
    already has it (at least num_bootstrap * max(n + 2 maxLag) values).

    Returns, per chain, one dict per z with the numeric fields of the reference's threshold views / metrics: the per-draw
    upper_tail_offsets, bootstrap_upper_tail_offset (their calibration quantile), upper_tail_offset_mean / _sd, threshold_offset,
    empirical_null_scale, null_scale, threshold, observed_tail_occupancy, observed_soft_tail, the per-draw null_occupancies /
    null_soft_tails, null_tail_occupancy / _calibrated / _sd, null_soft_tail / _calibrated / _sd, budget_occupancy_raw and
    budget_soft_raw."""
    tracks = [_f64(s) for s in score_tracks]
    for s in tracks:
        if s.shape[0] == 0 or not np.all(np.isfinite(s)):
            raise ValueError("`scoreTrack` must be a non-empty finite vector")
    return _run_panel(None, _HostObserved(tracks), [s.shape[0] for s in tracks], templates, null_centers, null_scales,
                      threshold_z_grid=threshold_z_grid, tail_quantiles=tail_quantiles, bandwidths=bandwidths,
                      num_bootstrap=num_bootstrap, kernel=kernel, random_seed=random_seed,
                      calibration_quantile=calibration_quantile, pooled_floors=pooled_floors, draws_per_group=draws_per_group,
                      noise=noise)


# ---------------------------------------------------------------------------------------------------------------
# null replays scored as candidate segments (peaks.py:2858-2922): a third phase of the panel
# ---------------------------------------------------------------------------------------------------------------
SEGMENT_GROUP_BYTES = 16 << 30      # device memory a group of replay draws may take (rows + segment work space)
SEGMENT_MAX_JOBS = 65535            # (draw, scale, view) jobs per chain of one device run (include/consenrich_amd.h)


def _replay_group(lens, n_scales, n_views, num_replay, draws_per_group):
    """Draws per group: the caller's, or what fits SEGMENT_GROUP_BYTES by the bound of include/consenrich_amd.h."""
    s, v = max(max(n_scales), 1), max(max(n_views), 1)
    most = min(num_replay, SEGMENT_MAX_JOBS // (s * v))     # draws x scales x views per chain: one grid dimension
    if draws_per_group and int(draws_per_group) > 0:
        return min(int(draws_per_group), most)
    per_draw = sum(lens) * (16.0 + 16.0 * v + 24.5 * s * v)
    return int(min(max(SEGMENT_GROUP_BYTES // max(per_draw, 1.0), 1), most))


def _run_replays(ctx, observed, lens, templates, threshold_views, *, bandwidths, num_replay, kernel, random_seed, scale_bins,
                 min_run_bins, max_gap_bins, max_segments, max_segments_per_view, draws_per_group, noise):
    from . import segments as S

    nc = len(lens)
    kernel_code(kernel)
    R = int(num_replay)
    if R <= 0:
        raise ValueError("num_replay must be positive")
    total_cap, view_cap = S._caps(max_segments, max_segments_per_view)
    if view_cap is None:
        raise ValueError("null replays on the device need max_segments_per_view > 0")
    bws = [_c_int(b) for b in (bandwidths if np.ndim(bandwidths) else [bandwidths] * nc)]
    if not (len(bws) == len(threshold_views) == nc) or (templates is not None and len(templates) != nc):
        raise ValueError("one bandwidth, template and set of threshold views per chain")
    tmpl = _checked_templates(templates, lens)
    views = [S.Views(v) for v in threshold_views]
    replay_views = [v.for_replay() for v in views]
    per_chain_bins = scale_bins is not None and len(scale_bins) > 0 and np.ndim(scale_bins[0]) > 0
    scales = [S.resolve_scales(lens[c], scale_bins[c] if per_chain_bins else scale_bins, bws[c]) for c in range(nc)]
    min_run, gap = max(int(min_run_bins), 1), max(int(max_gap_bins), 0)
    strides = [lens[c] + 2 * max_lag(bws[c], kernel) for c in range(nc)]
    need = R * max(strides)
    z_stream = noise_stream(random_seed, need) if noise is None else _f64(noise)
    if z_stream.shape[0] < need:
        raise ValueError("noise length is too short for the requested DWB bandwidth")
    L.require_gpu()
    lib = L.lib()
    group = _replay_group(lens, [len(s) for s in scales], [len(v.keys) for v in views], R, draws_per_group)
    n_arr, bw_arr = np.asarray(lens, np.int64), np.asarray(bws, np.int32)
    n_s, sc_all, n_v, thr_all, ns_all = S.pack(scales, [v.threshold for v in replay_views], [v.null_scale for v in replay_views])
    replays = [[None] * R for _ in range(nc)]
    capped = fallback = 0
    _begin_panel(lib, ctx, n_arr, bw_arr, kernel, tmpl, z_stream, R, group)
    try:
        for d0 in range(0, R, group):
            g = min(group, R - d0)
            rows, counters, flagged = np.zeros(nc * g, np.int64), np.zeros(nc * g * 3, np.int64), C.c_int32(0)
            L.check_value(lib.csr_dwb_panel_segments(ctx, d0, g, n_s.ctypes.data_as(L.I32P), sc_all.ctypes.data_as(L.I64P),
                                                     n_v.ctypes.data_as(L.I32P), L.dp(thr_all), L.dp(ns_all), min_run, gap, view_cap,
                                                     rows.ctypes.data_as(L.I64P), counters.ctypes.data_as(L.I64P), C.byref(flagged)))
            # the flagged views of this group are resolved before the next group overwrites its rows
            tracks = S.collect(ctx, rows, counters, flagged.value, view_cap)
            capped += S.last_run_stats()["capped_views"]
            fallback += S.last_run_stats()["fallback_views"]
            for c in range(nc):
                for b in range(g):
                    cands, diag = S.compose(tracks[c * g + b], replay_views[c], total_cap, view_cap)
                    replays[c][d0 + b] = dict(
                        candidate_count=len(cands), diagnostics=diag,
                        score=np.asarray([k["score"] for k in cands], np.float64),
                        integrated_excess=np.asarray([k["integrated_excess"] for k in cands], np.float64),
                        max_excess=np.asarray([k["max_excess"] for k in cands], np.float64))
    finally:
        L.check(lib.csr_dwb_panel_end(ctx))
    obs = observed(views, scales, min_run, gap, total_cap, view_cap)
    return [dict(observed=obs[c], replays=replays[c], scale_bins=scales[c], draws_per_group=group, capped_views=capped,
                 fallback_views=fallback) for c in range(nc)]


def null_replay_candidates(score_tracks, templates, threshold_views, *, bandwidths, num_replay=64, kernel="bartlett", random_seed=0,
                           scale_bins=None, min_run_bins=1, max_gap_bins=0, max_segments=20000, max_segments_per_view=1000,
                           draws_per_group=0, noise=None):
    """The candidate side of the reference's DWB peak scoring (peaks.py:2685, 2858-2922) for every chain of one seed.

    threshold_views: per chain, a mapping key -> view or a sequence of views -- dicts with threshold_z, threshold, null_scale and
    null_center, e.g. what `stationary_null_panel` returns for the chain.  scale_bins: explicit scales for all chains, one list
    per chain, or None for the reference's five scales at dependence span = the chain's bandwidth.  The replays are draws
    0 .. num_replay - 1 of the seed's noise stream, exactly the panel's, scored against the views shifted by their null centre
    (`_thresholdViewsForNullReplay`); draws_per_group (0 = what fits 16 GiB) bounds the device working set and changes no result.

    Returns, per chain, a dict: observed = (candidates, diagnostics) of the score track as `segments.multiscale_candidates`
    gives them; replays = per draw a dict with candidate_count, the metric arrays score / integrated_excess / max_excess of its
    candidates and the cap diagnostics; scale_bins; capped_views / fallback_views of all replays (views over the per-view cap,
    and those of them NumPy decided on the host)."""
    from . import segments as S

    tracks = [_f64(s) for s in score_tracks]

    def observed(views, scales, min_run, gap, total_cap, view_cap):
        return [S.compose(S.cMultiscaleCandidateSegmentStats(tracks[c], np.asarray(scales[c], np.int64),
                                                             np.asarray(views[c].threshold, np.float64),
                                                             np.asarray(views[c].null_scale, np.float64), min_run, gap, view_cap),
                          views[c], total_cap, view_cap) for c in range(len(tracks))]

    return _run_replays(None, observed, [s.shape[0] for s in tracks], templates, threshold_views, bandwidths=bandwidths,
                        num_replay=num_replay, kernel=kernel, random_seed=random_seed, scale_bins=scale_bins,
                        min_run_bins=min_run_bins, max_gap_bins=max_gap_bins, max_segments=max_segments,
                        max_segments_per_view=max_segments_per_view, draws_per_group=draws_per_group, noise=noise)
