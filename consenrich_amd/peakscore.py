"""The numeric side of the reference's DWB peak scoring on the device (`_addDWBPeakScoringToPeakMeta`, peaks.py:2605-3157):

  best_segment_scores                 `_bestSegmentScoreAcrossThresholdViews` (peaks.py:2295-2356) of many segments at once,
  empirical_replay_segment_pvalues    `_empiricalReplaySegmentPValues` (2182-2203),
  replay_fdr_qvalues                  `_replayFDRQValues` (2206-2257),
  replay_pq                           both, and max(q, p), for up to three metrics in one device run,
  merge_candidate_regions             the `candidateBySpan` merge (2694-2825): host bookkeeping around the device's scores,
  score_candidate_regions             the numeric content of the whole scorer from candidates, replays and peaks
                                      (`DeviceBatch.dwb_peak_scoring` and `driver.score_peaks_batch` feed it from a batch).

Same coercions, empty-input results and `ValueError` texts as the originals; every returned number equals the reference's bit for
bit.  The excess sums (NumPy's summation order), maxima, sorts, counts, p and q values come from the C ABI (`csr_peakscore_*`,
csrc/csr_peakscore.h); no CPU fallback.  The drop-ins pool the replay draws before they go to the device: both functions read the
draws only through the counts #(draw >= x), and `_replayFDRQValues` through their mean over the draws, which is the pooled count
divided by the number of draws -- exact in float64.

  ReplayPool                          the replays' three metric columns in a pool on the device (csr_dwb_panel_pool_*).

What stays on the host: every string field but the view key, the merge's bookkeeping, the two quantiles over the draws, views
over the per-view cap and draws over the total cap whose order the values do not decide (a tie at the view cap, a NaN score).
"""
from __future__ import annotations

from collections.abc import Mapping

import numpy as np

from . import _lib as L
from ._lib import _f64, _i32p, _i64p
from .segments import Views

MAX_VIEWS = 16
METRICS = ("score", "integrated_excess", "max_excess")      # the reference's width_adjusted_mass, integrated_excess, max_excess
_ZERO = dict(score=0.0, integrated_excess=0.0, mean_excess=0.0, max_excess=0.0, threshold_key="", threshold_z=0.0, threshold=0.0,
             null_scale=1.0)


# ---------------------------------------------------------------------------------------------------------------
# segment scores
# ---------------------------------------------------------------------------------------------------------------
def _clamp_i64(values) -> np.ndarray:
    """Python ints of any size as int64 (the reference clamps them to the track anyway)."""
    lo, hi = -(1 << 62), 1 << 62
    if isinstance(values, np.ndarray) and values.dtype.kind in "iu" and values.dtype != np.uint64:
        return np.ascontiguousarray(np.clip(np.asarray(values, np.int64).reshape(-1), lo, hi), np.int64)
    return np.ascontiguousarray([min(max(int(v), lo), hi) for v in np.asarray(values, dtype=object).reshape(-1)], np.int64)


def segment_score_arrays(ctx, chain, scores, starts, ends, views: Views):
    """(score, integrated, mean, max, view index) arrays of the segments: of the host vector `scores` (ctx None), or of the
    resident score track of `chain` of the batch context `ctx`.  Needs at least one view."""
    st, en = _clamp_i64(starts), _clamp_i64(ends)
    if st.shape[0] != en.shape[0]:
        raise ValueError("starts and ends must have the same length")
    nv = len(views.keys)
    if not 1 <= nv <= MAX_VIEWS:
        raise ValueError(f"1 to {MAX_VIEWS} threshold views per call")
    thr, ns = np.asarray(views.threshold, np.float64), np.asarray(views.null_scale, np.float64)
    k = st.shape[0]
    flt = [np.zeros(k, np.float64) for _ in range(4)]
    view = np.zeros(k, np.int32)
    if k == 0:
        return (*flt, view)
    L.require_gpu()
    if ctx is None:
        x = _f64(scores)
        L.check_value(L.lib().csr_peakscore_segments(L.dp(x), x.shape[0], k, _i64p(st), _i64p(en), nv, L.dp(thr), L.dp(ns),
                                                     *[L.dp(a) for a in flt], _i32p(view)))
    else:
        L.check_value(L.lib().csr_batch_peakscore_segments(ctx, int(chain), k, _i64p(st), _i64p(en), nv, L.dp(thr), L.dp(ns),
                                                           *[L.dp(a) for a in flt], _i32p(view)))
    return (*flt, view)


def score_details(arrays, views: Views) -> list:
    """segment_score_arrays' result as the reference's dicts (one per segment)."""
    score, integ, mean, mx, view = arrays
    out = []
    for q in range(score.shape[0]):
        v = int(view[q])
        out.append(dict(score=float(score[q]), integrated_excess=float(integ[q]), mean_excess=float(mean[q]), max_excess=float(mx[q]),
                        threshold_key=views.keys[v], threshold_z=views.z[v], threshold=views.threshold[v],
                        null_scale=getattr(views, "raw_null_scale", views.null_scale)[v]))
    return out


class _Views(Views):
    """Views that also keep `null_scale` as the reference's score dict reports it (before it is raised to DBL_MIN)."""

    def __init__(self, threshold_views):
        super().__init__(threshold_views)
        items = threshold_views.items() if isinstance(threshold_views, Mapping) else enumerate(threshold_views)
        self.raw_null_scale = [float(v.get("null_scale", 1.0)) for _, v in items if isinstance(v, Mapping)]   # Views' own filter
        assert len(self.raw_null_scale) == len(self.keys)


def best_segment_scores(scores, starts, ends, threshold_views) -> list:
    """`_bestSegmentScoreAcrossThresholdViews(scores, start, end, thresholdViews)` for every (start, end): a list of its dicts
    (score, integrated_excess, mean_excess, max_excess, threshold_key, threshold_z, threshold, null_scale).  Without a view every
    segment gets the reference's all-zero record."""
    views = _Views(threshold_views)
    if not views.keys:
        return [dict(_ZERO) for _ in range(len(_clamp_i64(starts)))]
    x = np.asarray(scores, dtype=np.float64)
    return score_details(segment_score_arrays(None, 0, x, starts, ends, views), views)


# ---------------------------------------------------------------------------------------------------------------
# empirical p and q values
# ---------------------------------------------------------------------------------------------------------------
def _pool(null_by_draw):
    draws = [np.asarray(d, dtype=np.float64).ravel() for d in null_by_draw]
    pool = np.ascontiguousarray(np.concatenate(draws) if draws else np.zeros(0, np.float64), np.float64)
    return pool, len(draws)


def replay_pq(observed, pool, n_draws, what=L.PEAK_P | L.PEAK_Q | L.PEAK_Q_MAX_P):
    """observed: (metrics, K), pool: (metrics, N) -- the statistics of all `n_draws` replay draws of a metric, in any order.
    Returns dict(p, q, exceedances) of (metrics, K) arrays (those asked for by `what`: L.PEAK_P, L.PEAK_Q, L.PEAK_Q_MAX_P for
    q = max(q, p)).  Raises the reference's ValueErrors on non-finite statistics."""
    obs = np.ascontiguousarray(np.atleast_2d(np.asarray(observed, np.float64)), np.float64)
    pl = np.ascontiguousarray(np.atleast_2d(np.asarray(pool, np.float64)), np.float64)
    m, k = obs.shape
    if pl.shape[0] != m:
        raise ValueError("observed and pool must have the same number of metrics")
    n = pl.shape[1]
    want_p, want_q = bool(what & L.PEAK_P), bool(what & (L.PEAK_Q | L.PEAK_Q_MAX_P))
    p = np.ones((m, k), np.float64) if want_p else None
    q = np.ones((m, k), np.float64) if want_q else None
    exc = np.zeros((m, k), np.int64)
    if k > 0:
        L.require_gpu()
        L.check_value(L.lib().csr_peakscore_pq(L.dp(obs), k, L.dp(pl) if n > 0 else None, n, int(n_draws), m, int(what), L.dp(p), L.dp(q),
                                               _i64p(exc), None))
    return dict(p=p, q=q, exceedances=exc)


def empirical_replay_segment_pvalues(observed, null_by_draw) -> np.ndarray:
    """`_empiricalReplaySegmentPValues(observedStats, nullStatsByDraw)`."""
    obs = np.ascontiguousarray(np.asarray(observed, dtype=np.float64).ravel())
    pool, n_draws = _pool(null_by_draw)
    if obs.size == 0:
        return np.asarray([], dtype=np.float64)
    if pool.size == 0:
        return np.ones(obs.size, dtype=np.float64)
    return replay_pq(obs[None, :], pool[None, :], n_draws, L.PEAK_P)["p"][0]


def replay_fdr_qvalues(observed, null_by_draw) -> np.ndarray:
    """`_replayFDRQValues(observedStats, nullStatsByDraw)`."""
    obs = np.ascontiguousarray(np.asarray(observed, dtype=np.float64).ravel())
    if obs.size == 0:
        return np.asarray([], dtype=np.float64)
    pool, n_draws = _pool(null_by_draw)
    return replay_pq(obs[None, :], pool[None, :], n_draws, L.PEAK_Q)["q"][0]


# ---------------------------------------------------------------------------------------------------------------
# the candidateBySpan merge (host bookkeeping)
# ---------------------------------------------------------------------------------------------------------------
def merge_candidate_regions(observed_candidates, peaks, peak_scores, n, intervals=None, ends=None) -> list:
    """peaks.py:2694-2825 without its strings' meaning: `candidateDetails` before the p / q fields are added.

    observed_candidates: the dicts of `segments.multiscale_candidates`; peaks: (start_idx, end_idx) per exported peak, in peak
    order; peak_scores: best_segment_scores of those peaks; n: the track's length; intervals / ends: the bins' coordinates (None:
    start = start_idx, end = end_idx + 1).

    Numerically: per distinct (start_idx, end_idx) the metrics of the LAST element whose score is >= everything before it,
    starting from an all-zero record with score 0.0; observed candidates first in their order, then the peaks in theirs.  The
    overlap counts come from two searchsorted calls on the sorted candidate starts and ends (candidates that overlap a peak =
    all - those ending before it - those starting after it), the overlapping scales from the candidates between those bounds."""
    n = int(n)
    by_span: dict = {}

    def coords(a, b):
        if intervals is not None and ends is not None:
            return int(intervals[a]), int(ends[b])
        return int(a), int(b + 1)

    def merge(start_idx, end_idx, detail, source, scale=None, overlap=None):
        a = int(max(int(start_idx), 0))
        b = int(min(max(int(end_idx), a), n - 1))
        rec = by_span.get((a, b))
        if rec is None:
            cs, ce = coords(a, b)
            rec = dict(candidate_id="", start_idx=a, end_idx=b, start=cs, end=ce, exported=False, candidate_sources=[],
                       candidate_scale_bins=[], candidate_threshold_keys=[], score=0.0, integrated_excess=0.0, mean_excess=0.0,
                       max_excess=0.0, threshold_key="", threshold_z=0.0, threshold=0.0, null_scale=1.0)
            by_span[(a, b)] = rec
        if source not in rec["candidate_sources"]:
            rec["candidate_sources"] = rec["candidate_sources"] + [str(source)]
        if scale is not None and int(scale) not in rec["candidate_scale_bins"]:
            rec["candidate_scale_bins"] = sorted(rec["candidate_scale_bins"] + [int(scale)])
        key = str(detail.get("threshold_key", ""))
        if key and key not in rec["candidate_threshold_keys"]:
            rec["candidate_threshold_keys"] = rec["candidate_threshold_keys"] + [key]
        if overlap is not None:
            rec["overlapping_multiscale_candidate_count"] = max(int(rec.get("overlapping_multiscale_candidate_count", 0)), int(overlap))
        if float(detail.get("score", 0.0)) >= float(rec["score"]):
            rec.update(score=float(detail.get("score", 0.0)), integrated_excess=float(detail.get("integrated_excess", 0.0)),
                       mean_excess=float(detail.get("mean_excess", 0.0)), max_excess=float(detail.get("max_excess", 0.0)),
                       threshold_key=key, threshold_z=float(detail.get("threshold_z", 0.0)), threshold=float(detail.get("threshold", 0.0)),
                       null_scale=float(detail.get("null_scale", 1.0)))

    for cand in observed_candidates:
        merge(cand["start_idx"], cand["end_idx"], cand, "multiscale_threshold_run", scale=int(cand.get("scale_bins", 1)))
    o_start = np.asarray([int(c["start_idx"]) for c in observed_candidates], np.int64)
    o_end = np.asarray([int(c["end_idx"]) for c in observed_candidates], np.int64)
    o_scale = np.asarray([int(c.get("scale_bins", 1)) for c in observed_candidates], np.int64)
    by_start, by_end = np.argsort(o_start, kind="mergesort"), np.argsort(o_end, kind="mergesort")
    s_sorted, e_sorted = o_start[by_start], o_end[by_end]
    for (a, b), detail in zip(peaks, peak_scores):
        a, b = int(a), int(b)
        merge(a, b, detail, "exported_peak")
        if o_start.size > 0:
            ended = int(np.searchsorted(e_sorted, a, side="left"))              # end < a
            begun = int(np.searchsorted(s_sorted, b, side="right"))             # start <= b
            late = np.zeros(o_start.size, bool)
            late[by_end[:ended]] = True
            hit = by_start[:begun][~late[by_start[:begun]]]
            # (with start <= end for every candidate and a <= b, a candidate that ended before the peak also began before its end:
            # hit.size == begun - ended)
            count = int(hit.size)
            if count > 0:
                scales = np.unique(o_scale[hit])
                for s in scales:
                    merge(a, b, detail, "multiscale_threshold_overlap", scale=int(s), overlap=count)
        by_span[(a, b)]["exported"] = True      # (KeyError for a peak outside the track, as in the reference)
    out = sorted((dict(r) for r in by_span.values()), key=lambda r: (int(r["start_idx"]), int(r["end_idx"])))
    for i, r in enumerate(out, start=1):
        r["candidate_id"] = f"dwb_candidate_{i}"
    return out


# ---------------------------------------------------------------------------------------------------------------
# the scorer: candidates and replays in, p / q values per candidate region and per exported peak out
# ---------------------------------------------------------------------------------------------------------------
METRIC_SOURCES = {"summit_excess": "max_excess", "integrated_excess": "integrated_excess", "width_adjusted_mass": "score"}
PRIMARY = "width_adjusted_mass"
_QMETHOD = "interpolated_inverted_cdf"
_PEAK_KEYS = ("candidate_id", "candidate_sources", "candidate_scale_bins", "candidate_threshold_keys",
              "overlapping_multiscale_candidate_count", "dwb_peak_score", "dwb_peak_empirical_p", "dwb_peak_empirical_q",
              "dwb_empirical_null_replays", "dwb_empirical_p", "dwb_empirical_q", "dwb_empirical_statistic", "dwb_peak_null_exceedances",
              "dwb_peak_scoring_threshold_key", "dwb_peak_scoring_threshold_z", "dwb_peak_integrated_excess", "dwb_peak_mean_excess",
              "dwb_peak_max_excess", "dwb_null_replay_num_draws", "dwb_null_replay_max_score_mean", "dwb_null_replay_max_score_q95",
              "dwb_null_replay_candidate_count_mean", "dwb_null_replay_candidate_count_q95")


def disabled(reason: str, num_peaks: int) -> dict:
    """The reference's early exits (peaks.py:2616-2676)."""
    return dict(enabled=False, reason=str(reason), num_peaks=int(num_peaks))


def score_candidate_regions(observed, replays, peaks, peak_scores, n, *, num_bootstrap=None, scale_bins=(), min_run_bins=1,
                            dependence_span=0, random_seed=0, intervals=None, ends=None, pool=None) -> dict:
    """The numeric content of peaks.py:2694-3157 from its three inputs: observed = (candidates, diagnostics) of the score track,
    replays = per draw a dict with candidate_count, diagnostics and the metric arrays score / integrated_excess / max_excess (what
    `dwb.null_replay_candidates` and `DeviceBatch.dwb_replay` return per chain), peaks = (start_idx, end_idx) per exported peak
    with their best_segment_scores.  The merge is host bookkeeping; the p values, max(q, p) and the exceedance counts of the three
    metrics come from ONE device run over the pooled replay statistics; the two quantiles over the draws are NumPy's.
    pool: instead of `replays`, a chain of an open device pool (`ReplayPool.chain(c)`: num_draws, pq, counts, maxima, diagnostics).

    Returns dict(enabled=True, candidate_details, peaks, summary): candidate_details as `merge_candidate_regions` gives them plus
    the reference's numeric dwb_* fields and the three metrics with _p and _q; peaks: the same fields per exported peak, in peak
    order; summary: the numeric fields of the reference's summary and false_segment_diagnostics."""
    cands, diag = observed
    if len(peaks) == 0:
        return disabled("no_peaks", 0)
    r = len(replays) if pool is None else int(pool["num_draws"])
    if r <= 0:
        return disabled("no_bootstrap_draws", len(peaks))
    details = merge_candidate_regions(cands, peaks, peak_scores, n, intervals, ends)
    metrics = list(METRIC_SOURCES)
    obs = np.asarray([[float(d[METRIC_SOURCES[m]]) for d in details] for m in metrics], np.float64)
    if pool is None:
        pooled = np.asarray([np.concatenate([np.asarray(rep[METRIC_SOURCES[m]], np.float64).ravel() for rep in replays])
                             for m in metrics], np.float64)
        res = replay_pq(obs, pooled, r)
        counts = np.asarray([int(rep["candidate_count"]) for rep in replays], np.int64)
        maxima = np.asarray([float(np.max(rep["score"])) if len(rep["score"]) else 0.0 for rep in replays], np.float64)
        diags = [rep["diagnostics"] for rep in replays]
    else:
        res = pool["pq"]({METRIC_SOURCES[m]: obs[k] for k, m in enumerate(metrics)})
        res = {key: np.asarray([val[METRIC_SOURCES[m]] for m in metrics]) for key, val in res.items()}
        counts, maxima, diags = np.asarray(pool["counts"], np.int64), np.asarray(pool["maxima"], np.float64), pool["diagnostics"]
    primary = metrics.index(PRIMARY)
    p, q = res["p"][primary], res["q"][primary]
    max_q95 = float(np.quantile(maxima, 0.95, method=_QMETHOD))
    max_mean = float(np.mean(maxima))
    count_mean = float(np.mean(counts))
    count_q95 = float(max(float(np.quantile(counts, 0.95, method=_QMETHOD)), count_mean))
    cap_draws = sum(bool(d["cap_hit"]) for d in diags)
    false_segments = dict(
        num_replays=r, budget_num_bootstrap=int(r if num_bootstrap is None else num_bootstrap), observed_segment_count=len(peaks),
        observed_candidate_count=len(details), false_segment_count_mean=count_mean, false_segment_count_q95=count_q95,
        false_segment_fdr_estimate=float(np.clip(count_mean / float(max(len(peaks), 1)), 0.0, 1.0)),
        candidate_fdr_estimate=float(np.clip(count_mean / float(max(len(details), 1)), 0.0, 1.0)),
        dependence_span=int(dependence_span), scale_bins=[int(s) for s in scale_bins], candidate_cap_hit=bool(cap_draws > 0),
        candidate_cap_hit_draws=int(cap_draws),
        candidate_per_view_cap_hit_draws=sum(int(d["per_view_cap_hit_count"]) > 0 for d in diags),
        candidate_total_cap_hit_draws=sum(bool(d["total_cap_hit"]) for d in diags),
        candidate_discarded_by_per_view_cap=sum(int(d["discarded_by_per_view_cap"]) for d in diags),
        candidate_discarded_by_total_cap=sum(int(d["discarded_by_total_cap"]) for d in diags),
        max_segments=diag.get("max_segments"), max_segments_per_scale_threshold=diag.get("max_segments_per_view"))
    for i, d in enumerate(details):
        stat = float(obs[primary][i])
        d.update(dwb_peak_score=stat, dwb_peak_empirical_p=float(p[i]), dwb_peak_empirical_q=float(q[i]), dwb_empirical_null_replays=r,
                 dwb_empirical_p=float(p[i]), dwb_empirical_q=float(q[i]), dwb_empirical_statistic=stat)
        for k, m in enumerate(metrics):
            d[m] = float(obs[k][i])
            d[f"{m}_p"] = float(res["p"][k][i])
            d[f"{m}_q"] = float(res["q"][k][i])
        d.update(dwb_peak_null_exceedances=int(res["exceedances"][primary][i]), dwb_peak_scoring_threshold_key=str(d["threshold_key"]),
                 dwb_peak_scoring_threshold_z=float(d["threshold_z"]), dwb_peak_integrated_excess=float(d["integrated_excess"]),
                 dwb_peak_mean_excess=float(d["mean_excess"]), dwb_peak_max_excess=float(d["max_excess"]), dwb_null_replay_num_draws=r,
                 dwb_null_replay_max_score_mean=max_mean, dwb_null_replay_max_score_q95=max_q95,
                 dwb_null_replay_candidate_count_mean=count_mean, dwb_null_replay_candidate_count_q95=count_q95)
    by_span = {(int(d["start_idx"]), int(d["end_idx"])): d for d in details}
    out_peaks = []
    for a, b in peaks:
        d = by_span[(int(a), int(b))]
        rec = {k: d.get(k, 0 if k == "overlapping_multiscale_candidate_count" else None) for k in _PEAK_KEYS}
        for m in metrics:
            rec.update({m: d[m], f"{m}_p": d[f"{m}_p"], f"{m}_q": d[f"{m}_q"]})
        out_peaks.append(rec)
    summary = dict(
        enabled=True, primary_metric=PRIMARY, metrics=sorted(metrics), num_peaks=len(peaks), num_candidate_regions=len(details),
        num_bootstrap=r, budget_num_bootstrap=false_segments["budget_num_bootstrap"], random_seed=int(random_seed),
        dependence_span=int(dependence_span), scale_bins=[int(s) for s in scale_bins], min_run_bins=int(max(int(min_run_bins), 1)),
        observed_candidate_count=len(details), raw_multiscale_candidate_count=len(cands),
        observed_candidate_cap_hit=bool(diag["cap_hit"]), null_replay_candidate_cap_hit=bool(cap_draws > 0),
        null_replay_candidate_cap_hit_draws=int(cap_draws), null_replay_candidate_count_mean=count_mean,
        null_replay_candidate_count_q95=count_q95, null_replay_max_score_mean=max_mean, null_replay_max_score_q95=max_q95,
        min_p=float(np.min(p)), min_q=float(np.min(q)), false_segment_diagnostics=false_segments)
    return dict(enabled=True, candidate_details=details, peaks=out_peaks, summary=summary)



# ---------------------------------------------------------------------------------------------------------------
# the replay pool on the device
# ---------------------------------------------------------------------------------------------------------------
POOL_COLUMNS = ("score", "integrated_excess", "max_excess")       # the pool's column order (csr_dwb_panel_pool_pq)
_last_pool = dict(fetched_replay_tracks=0, host_decided_draws=0, flagged_views=0)


def last_pool_stats() -> dict:
    """Of the last ReplayPool of this process: replay tracks whose rows left the device (= host-decided draws: over the total cap
    with a NaN score), and views over the per-view cap that NumPy decided from their scores and starts."""
    return dict(_last_pool)


def _resolve_flagged(lib, ctx, n_flagged, cap):
    """The views over the per-view cap that the values do not decide, as `segments.collect` resolves them (pyx:9634-9635)."""
    import ctypes as C

    for k in range(int(n_flagged)):
        track, si, view, nc = C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_int64(0)
        L.check_value(lib.csr_segments_flagged(ctx, k, C.byref(track), C.byref(si), C.byref(view), C.byref(nc)))
        score, start = np.empty(nc.value, np.float64), np.empty(nc.value, np.int64)
        L.check_value(lib.csr_segments_flagged_fetch(ctx, k, L.dp(score), _i64p(start)))
        selected = np.argpartition(-score, cap - 1)[:cap]
        selected = np.ascontiguousarray(selected[np.argsort(start[selected], kind="mergesort")], np.int64)
        L.check_value(lib.csr_segments_flagged_select(ctx, k, selected.shape[0], _i64p(selected)))


class ReplayPool:
    """The null replays of a panel scored as candidate segments, their three metric columns kept in a pool on the device (one per
    chain): csr_dwb_panel_begin, csr_dwb_panel_pool_begin, then per group of draws csr_dwb_panel_segments (rows stay on the
    device), the flagged views as `segments.collect` resolves them, csr_dwb_panel_pool_append.  A draw over the total cap with a
    NaN score is composed on the host from its fetched rows (`segments.compose`, as before) and uploaded.  Use as a context
    manager; `chain(c)` is what `score_candidate_regions(pool=...)` takes.  The draws, views, scales and caps are those of
    `dwb.null_replay_candidates`."""

    def __init__(self, ctx, lens, templates, threshold_views, *, bandwidths, num_replay, kernel="bartlett", random_seed=0,
                 scale_bins=None, min_run_bins=1, max_gap_bins=0, max_segments=20000, max_segments_per_view=1000, draws_per_group=0,
                 noise=None):
        from . import dwb as W
        from . import segments as S

        self.ctx, self.nc, self.R = ctx, len(lens), int(num_replay)
        W.kernel_code(kernel)
        if self.R <= 0:
            raise ValueError("num_replay must be positive")
        self.total_cap, self.view_cap = S._caps(max_segments, max_segments_per_view)
        if self.view_cap is None:
            raise ValueError("null replays on the device need max_segments_per_view > 0")
        nc = self.nc
        bws = [W._c_int(b) for b in (bandwidths if np.ndim(bandwidths) else [bandwidths] * nc)]
        if not (len(bws) == len(threshold_views) == nc) or (templates is not None and len(templates) != nc):
            raise ValueError("one bandwidth, template and set of threshold views per chain")
        self.views = [S.Views(v) for v in threshold_views]
        self.replay_views = [v.for_replay() for v in self.views]
        per_chain = scale_bins is not None and len(scale_bins) > 0 and np.ndim(scale_bins[0]) > 0
        self.scales = [S.resolve_scales(lens[c], scale_bins[c] if per_chain else scale_bins, bws[c]) for c in range(nc)]
        self.min_run, self.gap = max(int(min_run_bins), 1), max(int(max_gap_bins), 0)
        strides = [lens[c] + 2 * W.max_lag(bws[c], kernel) for c in range(nc)]
        need = self.R * max(strides)
        self.noise = W.noise_stream(random_seed, need) if noise is None else _f64(noise)
        if self.noise.shape[0] < need:
            raise ValueError("noise length is too short for the requested DWB bandwidth")
        self.tmpl = W._checked_templates(templates, lens)
        self.group = W._replay_group(lens, [len(s) for s in self.scales], [len(v.keys) for v in self.views], self.R, draws_per_group)
        self.lens, self.bws, self.kernel = list(lens), bws, kernel
        self.stats = None

    def __enter__(self):
        from . import dwb as W
        from . import segments as S
        import ctypes as C

        L.require_gpu()
        lib, ctx, nc = L.lib(), self.ctx, self.nc
        n_s, sc_all, n_v, thr_all, ns_all = S.pack(self.scales, [v.threshold for v in self.replay_views],
                                                   [v.null_scale for v in self.replay_views])
        W._begin_panel(lib, ctx, np.asarray(self.lens, np.int64), np.asarray(self.bws, np.int32), self.kernel, self.tmpl, self.noise,
                       self.R, self.group)
        try:
            L.check_value(lib.csr_dwb_panel_pool_begin(ctx, 0 if self.total_cap is None else self.total_cap))
            flagged_views = decided = 0
            for d0 in range(0, self.R, self.group):
                g = min(self.group, self.R - d0)
                rows, counters, flagged = np.zeros(nc * g, np.int64), np.zeros(nc * g * 3, np.int64), C.c_int32(0)
                L.check_value(lib.csr_dwb_panel_segments(ctx, d0, g, _i32p(n_s), _i64p(sc_all), _i32p(n_v), L.dp(thr_all), L.dp(ns_all),
                                                         self.min_run, self.gap, self.view_cap, _i64p(rows), _i64p(counters),
                                                         C.byref(flagged)))
                _resolve_flagged(lib, ctx, flagged.value, self.view_cap)
                flagged_views += int(flagged.value)
                undecided = C.c_int32(0)
                L.check_value(lib.csr_dwb_panel_pool_append(ctx, d0, C.byref(undecided)))
                for k in range(undecided.value):
                    self._decide_on_host(lib, k, g, d0, counters.reshape(-1, 3))
                decided += int(undecided.value)
            cd = nc * self.R
            count, before, cnt, mx = np.zeros(cd, np.int64), np.zeros(cd, np.int64), np.zeros(3 * cd, np.int64), np.zeros(cd, np.float64)
            fetched = C.c_int64(0)
            L.check_value(lib.csr_dwb_panel_pool_draw_stats(ctx, _i64p(count), _i64p(before), _i64p(cnt), L.dp(mx), C.byref(fetched)))
            self.stats = dict(count=count.reshape(nc, self.R), before=before.reshape(nc, self.R), counters=cnt.reshape(nc, self.R, 3),
                              max_score=mx.reshape(nc, self.R))
            _last_pool.update(fetched_replay_tracks=int(fetched.value), host_decided_draws=decided, flagged_views=flagged_views)
        except BaseException:
            L.check(lib.csr_dwb_panel_end(ctx))
            raise
        return self

    def __exit__(self, *exc):
        L.check(L.lib().csr_dwb_panel_end(self.ctx))

    def _decide_on_host(self, lib, k, g, d0, counters):
        import ctypes as C
        from . import segments as S

        chain, draw, n_rows = C.c_int32(0), C.c_int32(0), C.c_int64(0)
        L.check_value(lib.csr_dwb_panel_pool_flagged(self.ctx, k, C.byref(chain), C.byref(draw), C.byref(n_rows)))
        ints = [np.empty(n_rows.value, np.int64) for _ in range(4)]
        flts = [np.empty(n_rows.value, np.float64) for _ in range(4)]
        L.check_value(lib.csr_dwb_panel_pool_flagged_fetch(self.ctx, k, *[_i64p(a) for a in ints], *[L.dp(a) for a in flts]))
        cnt = counters[chain.value * g + (draw.value - d0)]
        cands, _ = S.compose((*ints, *flts, int(cnt[0]), int(cnt[1]), int(cnt[2])), self.replay_views[chain.value], self.total_cap,
                             self.view_cap)
        cols = [np.ascontiguousarray([c[key] for c in cands], np.float64) for key in POOL_COLUMNS]
        L.check_value(lib.csr_dwb_panel_pool_flagged_upload(self.ctx, k, cols[0].shape[0], *[L.dp(a) for a in cols]))

    def chain(self, c: int) -> dict:
        st = self.stats
        diags = []
        for b in range(self.R):
            before, count, (eligible, hits, dropped) = int(st["before"][c, b]), int(st["count"][c, b]), st["counters"][c, b]
            hit = before > count
            diags.append(dict(eligible_candidate_count=int(eligible), candidate_count_before_total_cap=before, candidate_count=count,
                              cap_hit=bool(int(hits) > 0 or hit), per_view_cap_hit_count=int(hits), total_cap_hit=bool(hit),
                              discarded_by_per_view_cap=int(dropped), discarded_by_total_cap=int(before - count),
                              max_segments=self.total_cap, max_segments_per_view=self.view_cap))
        return dict(num_draws=self.R, pq=lambda obs: self.pq(c, obs), counts=st["count"][c], maxima=st["max_score"][c], diagnostics=diags)

    def download(self, c: int) -> dict:
        """The chain's pool as it stands: column name -> values (draw after draw; a capped draw in descending order of score)."""
        import ctypes as C

        n = C.c_int64(0)
        L.check_value(L.lib().csr_dwb_panel_pool_download(self.ctx, int(c), C.byref(n), None, None, None))
        cols = [np.empty(n.value, np.float64) for _ in POOL_COLUMNS]
        L.check_value(L.lib().csr_dwb_panel_pool_download(self.ctx, int(c), C.byref(n), *[L.dp(a) for a in cols]))
        return dict(zip(POOL_COLUMNS, cols))

    def pq(self, c: int, observed: dict) -> dict:
        """observed: column name (POOL_COLUMNS) -> K statistics.  p, max(q, p) and exceedance counts per column."""
        obs = np.ascontiguousarray([np.asarray(observed[key], np.float64) for key in POOL_COLUMNS], np.float64)
        k = obs.shape[1]
        p, q, exc = np.ones((3, k), np.float64), np.ones((3, k), np.float64), np.zeros((3, k), np.int64)
        if k:
            L.check_value(L.lib().csr_dwb_panel_pool_pq(self.ctx, int(c), L.dp(obs), k, L.PEAK_P | L.PEAK_Q | L.PEAK_Q_MAX_P, L.dp(p),
                                                       L.dp(q), _i64p(exc), None))
        return {name: {key: arr[i] for i, key in enumerate(POOL_COLUMNS)} for name, arr in (("p", p), ("q", q), ("exceedances", exc))}
