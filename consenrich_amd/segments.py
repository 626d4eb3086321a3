"""Multiscale candidate segments on the device: the drop-in for the reference native `cMultiscaleCandidateSegmentStats`
(pyx:9460-9669) and the numeric part of `_multiscaleCandidateSegments` (peaks.py:2359-2481).

Same argument names, coercions, `ValueError` text and 11-tuple as the original; every returned value equals the reference's bit
for bit.  The prefixes, runs, statistics and the per-view cap come from the C ABI (`csr_segments_*`, csrc/csr_segments.h).  One
thing is left to NumPy on the host: a view over the cap whose chosen set the values alone do not determine (a non-finite
candidate score, or equal values at ranks cap and cap + 1) is answered with the reference's own two calls, np.argpartition and
a mergesort by start, on that view's candidate scores and starts -- the only arrays fetched for it.  No CPU fallback otherwise.

What follows: the empirical p and q values and the merge with exported peaks are `consenrich_amd/peakscore.py`; every
string-valued field but the view key stays with the caller.
"""
from __future__ import annotations

import ctypes as C
from collections.abc import Mapping

import numpy as np

from . import _lib as L
from ._lib import _c_int, _f64, _i32p, _i64, _i64p

TINY = float(np.finfo(np.float64).tiny)
MAX_SEGMENTS = 20000            # peaks.py:122-123
MAX_SEGMENTS_PER_VIEW = 1000
MAX_SCALES = MAX_VIEWS = 16     # per track on the device

_last = dict(capped_views=0, fallback_views=0)


def last_run_stats() -> dict:
    """Of the last device run of this process: views that hit the cap, and how many of them NumPy decided on the host."""
    return dict(_last)


def collect(ctx, rows_per_track, counters, n_flagged, cap):
    """After a phase-1 call on `ctx`: resolve the flagged views, fetch the rows, split them by track -> one 11-tuple per track."""
    lib = L.lib()
    for k in range(int(n_flagged)):
        track, si, view, nc = C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_int64(0)
        L.check_value(lib.csr_segments_flagged(ctx, k, C.byref(track), C.byref(si), C.byref(view), C.byref(nc)))
        score, start = np.empty(nc.value, np.float64), np.empty(nc.value, np.int64)
        L.check_value(lib.csr_segments_flagged_fetch(ctx, k, L.dp(score), _i64p(start)))
        selected = np.argpartition(-score, cap - 1)[:cap]                       # pyx:9634-9635
        selected = selected[np.argsort(start[selected], kind="mergesort")]
        selected = np.ascontiguousarray(selected, np.int64)
        L.check_value(lib.csr_segments_flagged_select(ctx, k, selected.shape[0], _i64p(selected)))
    rows = np.asarray(rows_per_track, np.int64).reshape(-1)
    counters = np.asarray(counters, np.int64).reshape(-1, 3)
    total = int(rows.sum())
    ints = [np.empty(total, np.int64) for _ in range(4)]
    flts = [np.empty(total, np.float64) for _ in range(4)]
    L.check_value(lib.csr_segments_fetch(ctx, *[_i64p(a) for a in ints], *[L.dp(a) for a in flts]))
    _last["capped_views"] = int(counters[:, 1].sum())
    _last["fallback_views"] = int(n_flagged)
    out, lo = [], 0
    for t in range(rows.shape[0]):
        hi = lo + int(rows[t])
        out.append((*[a[lo:hi].copy() for a in ints], *[a[lo:hi].copy() for a in flts], int(counters[t, 0]), int(counters[t, 1]),
                    int(counters[t, 2])))
        lo = hi
    return out


def pack(scales_per_chain, thresholds_per_chain, null_scales_per_chain):
    """Per-chain scales and views as the C ABI takes them: counts per chain, values one chain after the other."""
    sc = [_i64(s) for s in scales_per_chain]
    th = [_f64(t) for t in thresholds_per_chain]
    ns = [_f64(s) for s in null_scales_per_chain]
    for s, t, u in zip(sc, th, ns):
        if t.shape[0] != u.shape[0]:
            raise ValueError("thresholds and nullScales must have the same length")
        if s.shape[0] > MAX_SCALES or t.shape[0] > MAX_VIEWS:
            raise ValueError(f"at most {MAX_SCALES} scales and {MAX_VIEWS} views per track")
    cat = lambda xs, dt: np.ascontiguousarray(np.concatenate(xs) if xs else np.zeros(0, dt), dt)  # noqa: E731
    return (np.asarray([s.shape[0] for s in sc], np.int32), cat(sc, np.int64), np.asarray([t.shape[0] for t in th], np.int32),
            cat(th, np.float64), cat(ns, np.float64))


def cMultiscaleCandidateSegmentStats(scores, scales, thresholds, nullScales, minRunBins=1, maxGapBins=0, maxSegmentsPerView=0):
    """pyx:9460-9669.  Returns (start, end, scale, view, score, integrated, mean, max, eligibleCount, perViewCapHitCount,
    perViewDiscardedCount): rows ordered by scale, view, start; `scale` holds the width clamped to [1, n].

    Limits the reference native does not have: at most 16 scales and 16 views per call (the device keeps them in a fixed-size
    chain record; more raise ConsenrichAMDError), and a track shorter than 2^31 - 64 bins."""
    x, sc, thr, ns = _f64(scores), _i64(scales), _f64(thresholds), _f64(nullScales)
    min_run, gap, cap = _c_int(minRunBins), _c_int(maxGapBins), _c_int(maxSegmentsPerView)
    if thr.shape[0] != ns.shape[0]:
        raise ValueError("thresholds and nullScales must have the same length")
    if x.shape[0] <= 0 or sc.shape[0] <= 0 or thr.shape[0] <= 0:
        return (*[np.zeros(0, np.int64) for _ in range(4)], *[np.zeros(0, np.float64) for _ in range(4)], 0, 0, 0)
    L.require_gpu()
    rows, counters, flagged = np.zeros(1, np.int64), np.zeros(3, np.int64), C.c_int32(0)
    L.check_value(L.lib().csr_segments_run(None, L.dp(x), x.shape[0], sc.shape[0], _i64p(sc), thr.shape[0], L.dp(thr), ns.shape[0], L.dp(ns),
                                           min_run, gap, cap, _i64p(rows), _i64p(counters), C.byref(flagged)))
    return collect(None, rows, counters, flagged.value, max(cap, 0))[0]


# ---------------------------------------------------------------------------------------------------------------
# the numeric part of `_multiscaleCandidateSegments`
# ---------------------------------------------------------------------------------------------------------------
def resolve_scales(n, scale_bins=None, dependence_span=None, lower_span=None, upper_span=None):
    """`_resolveMultiscaleCandidateBins` (peaks.py:2260-2292): clamped to [1, max(n, 1)], repeats dropped, ascending."""
    n = max(int(n), 1)
    if scale_bins is not None:
        raw = [int(s) for s in scale_bins]
    else:
        span = 0 if dependence_span is None else int(dependence_span)
        lower = span if lower_span is None else int(lower_span)
        upper = span if upper_span is None else int(upper_span)
        raw = [1, max(2, int(round(max(lower, 1) / 2.0))), max(2, lower), max(2, span), max(2, upper)]
    out = []
    for s in raw:
        s = min(max(s, 1), n)
        if s not in out:
            out.append(s)
    return sorted(out)


class Views:
    """The threshold views of one track: a mapping key -> dict (entries that are no mapping are skipped, as in the reference), or
    a sequence of dicts (keys "0", "1", ...).  Each dict: threshold_z, threshold, null_scale (and null_center for replays)."""

    def __init__(self, threshold_views):
        items = threshold_views.items() if isinstance(threshold_views, Mapping) else ((str(i), v) for i, v in enumerate(threshold_views))
        items = [(str(k), v) for k, v in items if isinstance(v, Mapping)]
        self.keys = [k for k, _ in items]
        self.z = [float(v.get("threshold_z", 0.0)) for _, v in items]
        self.threshold = [float(v.get("threshold", 0.0)) for _, v in items]
        self.null_scale = [float(max(float(v.get("null_scale", 1.0)), TINY)) for _, v in items]
        self.null_center = [float(v.get("null_center", 0.0)) for _, v in items]

    def for_replay(self):
        """`_thresholdViewsForNullReplay` (peaks.py:2588-2602): thresholds relative to the null centre."""
        return Views({k: dict(threshold_z=z, threshold=float(t - c), null_scale=s) for k, z, t, c, s in
                      zip(self.keys, self.z, self.threshold, self.null_center,
                          [float(s) for s in self.null_scale])})


def _caps(max_segments, max_segments_per_view):
    total = None if max_segments is None or int(max_segments) <= 0 else int(max_segments)
    view = None if max_segments_per_view is None or int(max_segments_per_view) <= 0 else int(max_segments_per_view)
    return total, view


def compose(native_rows, views: Views, total_cap, view_cap):
    """From the native's 11-tuple to (candidates, diagnostics): dedupe on (start, end, scale, key), the total cap by a stable
    descending sort on score, then the re-sort on (start, end, scale, key)."""
    r = native_rows
    cands, seen = [], set()
    for q in range(r[0].shape[0]):
        v = int(r[3][q])
        ident = (int(r[0][q]), int(r[1][q]), int(r[2][q]), views.keys[v])
        if ident in seen:
            continue
        seen.add(ident)
        cands.append(dict(start_idx=ident[0], end_idx=ident[1], scale_bins=ident[2], threshold_key=views.keys[v],
                          threshold_z=views.z[v], threshold=views.threshold[v], null_scale=views.null_scale[v], score=float(r[4][q]),
                          integrated_excess=float(r[5][q]), mean_excess=float(r[6][q]), max_excess=float(r[7][q])))
    before = len(cands)
    hit = total_cap is not None and before > total_cap
    dropped = 0
    if hit:
        dropped = before - total_cap
        cands = sorted(cands, key=lambda c: float(c["score"]), reverse=True)[:total_cap]
        cands.sort(key=lambda c: (c["start_idx"], c["end_idx"], c["scale_bins"], c["threshold_key"]))
    diag = dict(eligible_candidate_count=int(r[8]), candidate_count_before_total_cap=before, candidate_count=len(cands),
                cap_hit=bool(int(r[9]) > 0 or hit), per_view_cap_hit_count=int(r[9]), total_cap_hit=bool(hit),
                discarded_by_per_view_cap=int(r[10]), discarded_by_total_cap=int(dropped), max_segments=total_cap,
                max_segments_per_view=view_cap)
    return cands, diag


def multiscale_candidates(scores, threshold_views, scale_bins=None, min_run_bins=1, max_gap_bins=0, max_segments=MAX_SEGMENTS,
                          max_segments_per_view=MAX_SEGMENTS_PER_VIEW, dependence_span=None):
    """The numeric part of `_multiscaleCandidateSegments`: (candidates, diagnostics).  candidates: dicts with start_idx, end_idx,
    scale_bins, threshold_key, threshold_z, threshold, null_scale, score, integrated_excess, mean_excess, max_excess."""
    x = _f64(scores)
    views = Views(threshold_views)
    total_cap, view_cap = _caps(max_segments, max_segments_per_view)
    scales = resolve_scales(x.shape[0], scale_bins, dependence_span)
    rows = cMultiscaleCandidateSegmentStats(x, np.asarray(scales, np.int64), np.asarray(views.threshold, np.float64),
                                            np.asarray(views.null_scale, np.float64), max(int(min_run_bins), 1),
                                            max(int(max_gap_bins), 0), 0 if view_cap is None else view_cap)
    return compose(rows, views, total_cap, view_cap)
