"""Pure-Python twin of the multiscale candidate-segment stage: `cMultiscaleCandidateSegmentStats` (pyx:9460-9669) and the numeric
part of `_multiscaleCandidateSegments` (peaks.py:2359-2481).  TEST INFRASTRUCTURE ONLY.

The native's two float64 prefixes are sums in index order; `np.add.accumulate` from a leading 0.0 is that fold.  Everything else
is elementwise IEEE arithmetic (one operation per rounding, no fused multiply-add), gathers and integer bookkeeping, written
with NumPy.  tests/golden/make_segments_golden.py writes fixtures only if this twin equals the compiled reference bit for bit on
every case of segments_cases.cases(); tests/test_segments_twin.py pins it to those fixtures."""
from __future__ import annotations

import numpy as np

TINY = float(np.finfo(np.float64).tiny)
MAX_SEGMENTS = 20000            # peaks.py:122-123
MAX_SEGMENTS_PER_VIEW = 1000


def _f64(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(-1), dtype=np.float64)


def _i64(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.int64).reshape(-1), dtype=np.int64)


def prefix(x):
    return np.add.accumulate(np.concatenate(([0.0], x)))


def smooth(x, pf, w):
    n = x.shape[0]
    if w <= 1 or n <= 1:
        return x
    left = (w - 1) // 2
    right = w - 1 - left
    i = np.arange(n, dtype=np.int64)
    return (pf[np.minimum(i + right + 1, n)] - pf[np.maximum(i - left, 0)]) / float(w)


def runs(flag, gap):
    """(starts, ends) of the runs of `flag` bridged over at most `gap` false bins."""
    idx = np.flatnonzero(flag)
    if idx.size == 0:
        return idx, idx
    brk = np.flatnonzero(np.diff(idx) > gap + 1)
    return idx[np.concatenate(([0], brk + 1))], idx[np.concatenate((brk, [idx.size - 1]))]


def cMultiscaleCandidateSegmentStats(scores, scales, thresholds, nullScales, minRunBins=1, maxGapBins=0, maxSegmentsPerView=0):
    x, sc, thr, ns = _f64(scores), _i64(scales), _f64(thresholds), _f64(nullScales)
    if thr.shape[0] != ns.shape[0]:
        raise ValueError("thresholds and nullScales must have the same length")
    n = x.shape[0]
    min_run = minRunBins if minRunBins > 1 else 1
    gap = maxGapBins if maxGapBins > 0 else 0
    cap = maxSegmentsPerView if maxSegmentsPerView > 0 else 0
    cols = [[] for _ in range(8)]
    eligible = cap_hit = discarded = 0
    if n > 0 and sc.shape[0] > 0 and thr.shape[0] > 0:
        pf = prefix(x)
        with np.errstate(all="ignore"):
            views = []
            for v in range(thr.shape[0]):
                s = float(ns[v])
                if s < TINY:
                    s = TINY
                e = (x - thr[v]) / s
                e = np.where(e < 0.0, 0.0, e)
                views.append((e, prefix(e)))
            for w0 in sc:
                w = int(min(max(int(w0), 1), n))
                sm = smooth(x, pf, w)
                for v in range(thr.shape[0]):
                    ex, ep = views[v]
                    st, en = runs(sm > thr[v], gap)
                    length = en - st + 1
                    keep = length >= min_run
                    st, en, length = st[keep], en[keep], length[keep]
                    k = st.shape[0]
                    if k == 0:
                        continue
                    eligible += k
                    integ = ep[en + 1] - ep[st]
                    lf = length.astype(np.float64)
                    mean = integ / lf
                    score = integ / np.sqrt(np.maximum(lf, 1.0))
                    bounds = np.empty(2 * k, np.int64)
                    bounds[0::2], bounds[1::2] = st, en + 1
                    mx = np.fmax.reduceat(np.concatenate((ex, [0.0])), bounds)[0::2]
                    mx = np.where(mx > 0.0, mx, 0.0)        # from 0.0 with `>`: a NaN never enters
                    sel = np.arange(k)
                    if cap > 0 and k > cap:
                        cap_hit += 1
                        discarded += k - cap
                        sel = np.argpartition(-score, cap - 1)[:cap]
                        sel = sel[np.argsort(st[sel], kind="mergesort")]
                    for col, val in zip(cols, (st[sel], en[sel], np.full(sel.shape[0], w, np.int64),
                                               np.full(sel.shape[0], v, np.int64), score[sel], integ[sel], mean[sel], mx[sel])):
                        col.append(val)
    out = []
    for q, col in enumerate(cols):
        dt = np.int64 if q < 4 else np.float64
        out.append(np.concatenate(col).astype(dt) if col else np.zeros(0, dt))
    return (*out, int(eligible), int(cap_hit), int(discarded))


def loop_native(scores, scales, thresholds, nullScales, minRunBins=1, maxGapBins=0, maxSegmentsPerView=0):
    """The same stage bin by bin with Python floats (small inputs): what the vectorised twin above is checked against."""
    x, sc, thr, ns = _f64(scores), _i64(scales), _f64(thresholds), _f64(nullScales)
    if thr.shape[0] != ns.shape[0]:
        raise ValueError("thresholds and nullScales must have the same length")
    n = x.shape[0]
    min_run, gap, cap = max(minRunBins, 1), max(maxGapBins, 0), max(maxSegmentsPerView, 0)
    rows, eligible, cap_hit, discarded = [], 0, 0, 0
    if n > 0 and sc.shape[0] > 0 and thr.shape[0] > 0:
        xs = [float(v) for v in x]
        pf = [0.0]
        for v in xs:
            pf.append(pf[-1] + v)
        for w0 in sc:
            w = int(min(max(int(w0), 1), n))
            left = (w - 1) // 2
            right = w - 1 - left
            sm = xs if (w <= 1 or n <= 1) else [(pf[min(i + right + 1, n)] - pf[max(i - left, 0)]) / float(w) for i in range(n)]
            for v in range(thr.shape[0]):
                t, s = float(thr[v]), float(ns[v])
                if s < TINY:
                    s = TINY
                with np.errstate(all="ignore"):
                    ex = [float(np.float64(a - t) / np.float64(s)) for a in xs]
                ex = [0.0 if e < 0.0 else e for e in ex]
                ep = [0.0]
                for e in ex:
                    ep.append(ep[-1] + e)
                found, start, last = [], -1, -1
                for i in range(n):
                    if sm[i] > t:
                        if start < 0:
                            start = i
                        elif i - last > gap + 1:
                            found.append((start, last))
                            start = i
                        last = i
                if start >= 0:
                    found.append((start, last))
                cand = []
                for a, b in found:
                    length = float(b - a + 1)
                    if length < float(min_run):
                        continue
                    integ = ep[b + 1] - ep[a]
                    m = 0.0
                    for j in range(a, b + 1):
                        if ex[j] > m:
                            m = ex[j]
                    with np.errstate(all="ignore"):
                        cand.append((a, b, w, v, float(np.float64(integ) / np.sqrt(np.float64(max(length, 1.0)))), integ,
                                     float(np.float64(integ) / np.float64(length)), m))
                if not cand:
                    continue
                eligible += len(cand)
                if cap > 0 and len(cand) > cap:
                    cap_hit += 1
                    discarded += len(cand) - cap
                    score = np.asarray([c[4] for c in cand], np.float64)
                    start_ = np.asarray([c[0] for c in cand], np.int64)
                    sel = np.argpartition(-score, cap - 1)[:cap]
                    sel = sel[np.argsort(start_[sel], kind="mergesort")]
                    cand = [cand[int(q)] for q in sel]
                rows.extend(cand)
    out = [np.asarray([r[q] for r in rows], np.int64 if q < 4 else np.float64) for q in range(8)]
    return (*out, int(eligible), int(cap_hit), int(discarded))


def same(a, b):
    """Two 11-tuples: integers with ==, floats by their 64-bit patterns."""
    if len(a) != 11 or len(b) != 11:
        return False
    for q in range(8):
        xa, xb = np.asarray(a[q]), np.asarray(b[q])
        if xa.dtype != xb.dtype or xa.shape != xb.shape:
            return False
        if not np.array_equal(xa.view(np.uint64), xb.view(np.uint64)):
            return False
    return all(int(a[q]) == int(b[q]) for q in (8, 9, 10))


# ---------------------------------------------------------------------------------------------------------------
# the numeric part of `_multiscaleCandidateSegments`
# ---------------------------------------------------------------------------------------------------------------
def resolve_scales(n, scale_bins=None, dependence_span=None, lower_span=None, upper_span=None):
    """peaks.py:2260-2292: clamp to [1, max(n, 1)], drop repeats, ascending."""
    n = max(int(n), 1)
    if scale_bins is not None:
        raw = [int(s) for s in scale_bins]
    else:
        span = 0 if dependence_span is None else int(dependence_span)
        lower = span if lower_span is None else int(lower_span)
        upper = span if upper_span is None else int(upper_span)
        raw = [1, max(2, int(round(max(lower, 1) / 2.0))), max(2, lower), max(2, span), max(2, upper)]
    return sorted({min(max(s, 1), n) for s in raw})


def multiscale_candidates(scores, threshold_views, scale_bins=None, min_run_bins=1, max_gap_bins=0, max_segments=MAX_SEGMENTS,
                          max_segments_per_view=MAX_SEGMENTS_PER_VIEW, native=None):
    """(candidates, diagnostics): threshold_views maps a key to a dict with threshold_z / threshold / null_scale."""
    native = native or cMultiscaleCandidateSegmentStats
    x = _f64(scores)
    scales = resolve_scales(x.shape[0], scale_bins)
    total_cap = None if max_segments is None or int(max_segments) <= 0 else int(max_segments)
    view_cap = None if max_segments_per_view is None or int(max_segments_per_view) <= 0 else int(max_segments_per_view)
    keys = [str(k) for k, v in threshold_views.items() if isinstance(v, dict)]
    views = [v for v in threshold_views.values() if isinstance(v, dict)]
    zs = [float(v.get("threshold_z", 0.0)) for v in views]
    thr = [float(v.get("threshold", 0.0)) for v in views]
    ns = [float(max(float(v.get("null_scale", 1.0)), TINY)) for v in views]
    r = native(x, np.asarray(scales, np.int64), np.asarray(thr, np.float64), np.asarray(ns, np.float64), max(int(min_run_bins), 1),
               max(int(max_gap_bins), 0), 0 if view_cap is None else view_cap)
    cands, seen = [], set()
    for q in range(r[0].shape[0]):
        v = int(r[3][q])
        ident = (int(r[0][q]), int(r[1][q]), int(r[2][q]), keys[v])
        if ident in seen:
            continue
        seen.add(ident)
        cands.append(dict(start_idx=ident[0], end_idx=ident[1], scale_bins=ident[2], threshold_key=keys[v], threshold_z=zs[v],
                          threshold=thr[v], null_scale=ns[v], score=float(r[4][q]), integrated_excess=float(r[5][q]),
                          mean_excess=float(r[6][q]), max_excess=float(r[7][q])))
    before = len(cands)
    hit = total_cap is not None and before > total_cap
    if hit:
        cands = sorted(cands, key=lambda c: c["score"], reverse=True)[:total_cap]
        cands.sort(key=lambda c: (c["start_idx"], c["end_idx"], c["scale_bins"], c["threshold_key"]))
    diag = dict(eligible_candidate_count=int(r[8]), candidate_count_before_total_cap=before, candidate_count=len(cands),
                cap_hit=bool(int(r[9]) > 0 or hit), per_view_cap_hit_count=int(r[9]), total_cap_hit=bool(hit),
                discarded_by_per_view_cap=int(r[10]), discarded_by_total_cap=before - len(cands) if hit else 0,
                max_segments=total_cap, max_segments_per_view=view_cap)
    return cands, diag


def same_candidates(a, b):
    """Two (candidates, diagnostics) pairs: floats by bit pattern, everything else with ==."""
    (ca, da), (cb, db) = a, b
    if da != db or len(ca) != len(cb):
        return False
    for x, y in zip(ca, cb):
        if sorted(x) != sorted(y):
            return False
        for k, v in x.items():
            if isinstance(v, float):
                if np.float64(v).view(np.uint64) != np.float64(y[k]).view(np.uint64):
                    return False
            elif v != y[k]:
                return False
    return True
