"""Pure-Python twin of the numeric side of the reference's DWB peak scoring, in two forms that the tests hold equal bit for bit:

  the reference's steps restated (`*_steps`): one view at a time with NumPy's own sum / max, one searchsorted per (observed
  statistic, draw) inside Python loops, the running minimum down the descending order, the dict merge by span;

  the device's decomposition (`*_device`): the leaf list of NumPy's pairwise tree and its fold (csrc/csr_peakscore.h
  k_peak_view_score), pooled counts from ONE sorted pool, the raw FDR as a function of the value alone with a prefix minimum along
  the ascending order, and the last arg-max by span for the merge.

Nothing here imports the product."""
import math

import numpy as np

TINY = float(np.finfo(np.float64).tiny)
CHUNK = 8192
ZERO = dict(score=0.0, integrated_excess=0.0, mean_excess=0.0, max_excess=0.0, threshold_key="", threshold_z=0.0, threshold=0.0,
            null_scale=1.0)
NUMERIC = ("score", "integrated_excess", "mean_excess", "max_excess")


def bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float64)).view(np.uint64)


# ---------------------------------------------------------------------------------------------------------------
# segment scores
# ---------------------------------------------------------------------------------------------------------------
def _clamped(n, start, end):
    return max(int(start), 0), min(int(end), int(n) - 1)


def view_score_steps(scores, start, end, view):
    x = np.asarray(scores, np.float64)
    a, b = _clamped(x.size, start, end)
    if b < a:
        return dict(score=0.0, integrated_excess=0.0, mean_excess=0.0, max_excess=0.0)
    thr = float(view.get("threshold", 0.0))
    scale = float(max(float(view.get("null_scale", 1.0)), TINY))
    e = np.clip((x[a:b + 1] - thr) / scale, 0.0, None)
    total = float(np.sum(e))
    return dict(score=float(total / math.sqrt(float(b - a + 1))), integrated_excess=total, mean_excess=float(np.mean(e)),
                max_excess=float(np.max(e)))


def best_score_steps(scores, start, end, views):
    best = None
    for key, view in views.items():
        if not isinstance(view, dict):
            continue
        cand = dict(view_score_steps(scores, start, end, view), threshold_key=str(key), threshold_z=float(view.get("threshold_z", 0.0)),
                    threshold=float(view.get("threshold", 0.0)), null_scale=float(view.get("null_scale", 1.0)))
        if best is None or cand["score"] > best["score"]:
            best = cand
    return dict(ZERO) if best is None else best


def tree_leaves(n):
    """(lo, len) of the leaves of NumPy's pairwise tree over n <= CHUNK values, left to right."""
    out, stack = [], [(0, int(n))]
    while stack:
        lo, m = stack.pop()
        if m <= 128:
            out.append((lo, m))
            continue
        n2 = m // 2
        n2 -= n2 % 8
        stack.append((lo + n2, m - n2))
        stack.append((lo, n2))
    return out


def leaf_sum(e):
    """NumPy's unrolled block sum of 8 <= n <= 128 values, or the plain loop below 8."""
    n = len(e)
    if n < 8:
        r = 0.0
        for v in e:
            r = r + float(v)
        return r
    acc = [float(e[k]) for k in range(8)]
    i = 8
    while i < n - n % 8:
        for k in range(8):
            acc[k] = acc[k] + float(e[i + k])
        i += 8
    r = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]))
    while i < n:
        r = r + float(e[i])
        i += 1
    return r


def _fold(n, sums):
    """The tree over n values folded from its leaf sums (taken in order)."""
    if n <= 128:
        return sums.pop(0)
    n2 = n // 2
    n2 -= n2 % 8
    left = _fold(n2, sums)
    return left + _fold(n - n2, sums)


def numpy_sum_device(e):
    """np.sum of a contiguous float64 vector as the device evaluates it: chunks of 8192 in ascending order, each the fold of its
    leaf sums."""
    total = 0.0
    for c0 in range(0, len(e), CHUNK):
        chunk = e[c0:c0 + CHUNK]
        with np.errstate(all="ignore"):
            sums = [leaf_sum(chunk[lo:lo + m]) for lo, m in tree_leaves(len(chunk))]
            part = _fold(len(chunk), sums)
            total = part if c0 == 0 else total + part
    return total


def _max_device(e):
    m = 0.0
    for v in e:
        v = float(v)
        m = m if m != m else (v if v != v else (v if v > m else m))
    return m


def segment_arrays_device(scores, starts, ends, thresholds, null_scales):
    """(score, integrated, mean, max, view index) per segment, the way the two kernels compute them."""
    x = np.asarray(scores, np.float64)
    k = len(starts)
    out = [np.zeros(k, np.float64) for _ in range(4)] + [np.zeros(k, np.int32)]
    for q in range(k):
        a, b = _clamped(x.size, starts[q], ends[q])
        if b < a:
            continue
        length = float(b - a + 1)
        root = math.sqrt(length)
        for v, (thr, s) in enumerate(zip(thresholds, null_scales)):
            with np.errstate(all="ignore"):
                d = (x[a:b + 1] - float(thr)) / float(max(float(s), TINY))
                e = np.where((d > 0.0) | (d != d), d, 0.0)
                total = numpy_sum_device(e)
                score = np.float64(total) / np.float64(root)
                mean = np.float64(total) / np.float64(length)
            if v == 0 or score > out[0][q]:
                out[0][q], out[1][q], out[2][q], out[3][q], out[4][q] = score, total, mean, _max_device(e), v
    return tuple(out)


def details_from_arrays(arrays, views):
    items = [(str(k), v) for k, v in views.items() if isinstance(v, dict)]
    out = []
    for q in range(arrays[0].shape[0]):
        key, view = items[int(arrays[4][q])]
        out.append(dict(score=float(arrays[0][q]), integrated_excess=float(arrays[1][q]), mean_excess=float(arrays[2][q]),
                        max_excess=float(arrays[3][q]), threshold_key=key, threshold_z=float(view.get("threshold_z", 0.0)),
                        threshold=float(view.get("threshold", 0.0)), null_scale=float(view.get("null_scale", 1.0))))
    return out


def same_details(a, b):
    if len(a) != len(b):
        return False
    for x, y in zip(a, b):
        if set(x) != set(y):
            return False
        for k in x:
            if isinstance(x[k], float) or isinstance(y[k], float):
                if bits(x[k]) != bits(y[k]):
                    return False
            elif x[k] != y[k]:
                return False
    return True


# ---------------------------------------------------------------------------------------------------------------
# empirical p and q values
# ---------------------------------------------------------------------------------------------------------------
P_TEXT = "replay segment statistics contain non-finite values"
Q_TEXT = "replay FDR statistics contain non-finite values"


def pvalues_steps(observed, null_by_draw):
    obs = np.asarray(observed, np.float64).ravel()
    parts = [np.asarray(d, np.float64).ravel() for d in null_by_draw]
    parts = [d for d in parts if d.size > 0]
    if obs.size == 0:
        return np.asarray([], np.float64)
    if not parts:
        return np.ones(obs.size, np.float64)
    null = np.concatenate(parts)
    if not (np.all(np.isfinite(obs)) and np.all(np.isfinite(null))):
        raise ValueError(P_TEXT)
    null.sort()
    tail = null.size - np.searchsorted(null, obs, side="left")
    return np.clip((1.0 + tail.astype(np.float64)) / float(null.size + 1), 0.0, 1.0)


def qvalues_steps(observed, null_by_draw):
    obs = np.asarray(observed, np.float64).ravel()
    if obs.size == 0:
        return np.asarray([], np.float64)
    draws = [np.sort(np.asarray(d, np.float64).ravel()) for d in null_by_draw]
    if not np.all(np.isfinite(obs)) or any(not np.all(np.isfinite(d)) for d in draws):
        raise ValueError(Q_TEXT)
    ascending = np.sort(obs)
    order = np.argsort(-obs, kind="mergesort")
    pseudo = 1.0 / float(len(draws) + 1) if draws else 1.0
    raw = np.ones(obs.size, np.float64)
    for rank, idx in enumerate(order):
        x = float(obs[idx])
        at = int(ascending.size - np.searchsorted(ascending, x, side="left"))
        expected = float(np.mean([d.size - np.searchsorted(d, x, side="left") for d in draws])) if draws else 0.0
        raw[rank] = float(np.clip((expected + pseudo) / float(max(at, 1)), 0.0, 1.0))
    q = np.ones(obs.size, np.float64)
    running = 1.0
    for rank in range(obs.size - 1, -1, -1):
        running = min(running, float(raw[rank]))
        q[int(order[rank])] = running
    return np.clip(q, 0.0, 1.0)


def pq_device(observed, pool, n_draws):
    """(p, q, exceedances) of one metric from the pooled draws: sorted pool, counts by bisection on `<`, the raw FDR per ascending
    observed value, its prefix minimum, and the way back through one more bisection.  q is `_replayFDRQValues`' (no max with p)."""
    obs = np.asarray(observed, np.float64).ravel()
    pool = np.sort(np.asarray(pool, np.float64).ravel())
    k, n, r = obs.size, pool.size, int(n_draws)
    count = lambda x: (n - np.searchsorted(pool, x, side="left")).astype(np.int64) if n else np.zeros(np.shape(x), np.int64)  # noqa: E731
    c = count(obs)
    p = np.clip((1.0 + c.astype(np.float64)) / float(n + 1), 0.0, 1.0) if n else np.ones(k, np.float64)
    asc = np.sort(obs)
    at = k - np.searchsorted(asc, asc, side="left")
    expected = count(asc).astype(np.float64) / float(r) if r > 0 else np.zeros(k, np.float64)
    pseudo = 1.0 / float(r + 1) if r > 0 else 1.0
    raw = np.clip((expected + pseudo) / np.maximum(at, 1).astype(np.float64), 0.0, 1.0)
    prefix = np.minimum.accumulate(raw) if k else raw
    q = prefix[np.searchsorted(asc, obs, side="left")] if k else np.asarray([], np.float64)
    return p, np.clip(q, 0.0, 1.0), c


# ---------------------------------------------------------------------------------------------------------------
# the merge by span
# ---------------------------------------------------------------------------------------------------------------
def merge_steps(observed_candidates, peaks, peak_scores, n, intervals=None, ends=None):
    """The dict merge, element by element, with the overlap test as the two comparisons over ALL candidates per peak."""
    spans = {}

    def put(start_idx, end_idx, detail, source, scale=None, overlap=None):
        a = max(int(start_idx), 0)
        b = min(max(int(end_idx), a), int(n) - 1)
        if (a, b) not in spans:
            lo, hi = (int(intervals[a]), int(ends[b])) if intervals is not None and ends is not None else (a, b + 1)
            spans[(a, b)] = dict(candidate_id="", start_idx=a, end_idx=b, start=lo, end=hi, exported=False, candidate_sources=[],
                                 candidate_scale_bins=[], candidate_threshold_keys=[], **{k: v for k, v in ZERO.items()})
        rec = spans[(a, b)]
        if source not in rec["candidate_sources"]:
            rec["candidate_sources"].append(source)
        if scale is not None and int(scale) not in rec["candidate_scale_bins"]:
            rec["candidate_scale_bins"] = sorted(rec["candidate_scale_bins"] + [int(scale)])
        key = str(detail.get("threshold_key", ""))
        if key and key not in rec["candidate_threshold_keys"]:
            rec["candidate_threshold_keys"].append(key)
        if overlap is not None:
            rec["overlapping_multiscale_candidate_count"] = max(rec.get("overlapping_multiscale_candidate_count", 0), int(overlap))
        if float(detail.get("score", 0.0)) >= float(rec["score"]):
            for k in NUMERIC + ("threshold_z", "threshold"):
                rec[k] = float(detail.get(k, 0.0))
            rec["null_scale"] = float(detail.get("null_scale", 1.0))
            rec["threshold_key"] = key

    for cand in observed_candidates:
        put(cand["start_idx"], cand["end_idx"], cand, "multiscale_threshold_run", scale=cand.get("scale_bins", 1))
    o_start = np.asarray([int(c["start_idx"]) for c in observed_candidates], np.int64)
    o_end = np.asarray([int(c["end_idx"]) for c in observed_candidates], np.int64)
    o_scale = np.asarray([int(c.get("scale_bins", 1)) for c in observed_candidates], np.int64)
    for (a, b), detail in zip(peaks, peak_scores):
        put(a, b, detail, "exported_peak")
        over = (o_end >= int(a)) & (o_start <= int(b))
        for s in np.unique(o_scale[over]):
            put(a, b, detail, "multiscale_threshold_overlap", scale=int(s), overlap=int(np.sum(over)))
        spans[(int(a), int(b))]["exported"] = True
    out = sorted(spans.values(), key=lambda r: (r["start_idx"], r["end_idx"]))
    for i, r in enumerate(out, start=1):
        r["candidate_id"] = f"dwb_candidate_{i}"
    return out


def merge_numeric_device(observed_candidates, peaks, peak_scores, n):
    """Per distinct span the numeric record: of the elements of the span in order (observed candidates, then peaks) the LAST one
    whose score is >= the running best, which starts at 0.0 -- (start_idx, end_idx) -> dict of the NUMERIC fields, threshold_key."""
    groups = {}
    elements = [(c["start_idx"], c["end_idx"], c) for c in observed_candidates] + [(a, b, d) for (a, b), d in zip(peaks, peak_scores)]
    for a, b, d in elements:
        a = max(int(a), 0)
        b = min(max(int(b), a), int(n) - 1)
        groups.setdefault((a, b), []).append(d)
    out = {}
    for span, ds in groups.items():
        best, pick = 0.0, None
        for d in ds:
            if float(d.get("score", 0.0)) >= best:
                best, pick = float(d.get("score", 0.0)), d
        src = ZERO if pick is None else pick
        out[span] = {k: src.get(k, ZERO[k]) for k in NUMERIC + ("threshold_key",)}
    return out


# ---------------------------------------------------------------------------------------------------------------
# the scorer, step by step: per-draw lists, the two drop-ins per metric, np.maximum, the per-candidate loop
# ---------------------------------------------------------------------------------------------------------------
SOURCES = (("summit_excess", "max_excess"), ("integrated_excess", "integrated_excess"), ("width_adjusted_mass", "score"))


def score_steps(scores, views, observed, replays, peaks, *, scale_bins, dependence_span, random_seed, min_run_bins=1,
                num_bootstrap=None):
    """observed = (candidates, diagnostics); replays = [(candidates, diagnostics)] per draw (tests/twin_segments.py);
    peaks = [(start_idx, end_idx)].  Returns what `DeviceBatch.dwb_peak_scoring` returns for one chain."""
    if not peaks:
        return dict(enabled=False, reason="no_peaks", num_peaks=0)
    if not replays:
        return dict(enabled=False, reason="no_bootstrap_draws", num_peaks=len(peaks))
    cands, diag = observed
    x = np.asarray(scores, np.float64)
    with np.errstate(all="ignore"):
        peak_scores = [best_score_steps(x, a, b, views) for a, b in peaks]
    details = merge_steps([dict(c) for c in cands], peaks, peak_scores, x.size)
    obs = {m: np.asarray([float(d[src]) for d in details], np.float64) for m, src in SOURCES}
    # (a draw's candidates: a list of dicts, or the metric arrays under their names)
    column = lambda rc, src: np.asarray(rc[src] if isinstance(rc, dict) else [float(c[src]) for c in rc], np.float64)  # noqa: E731
    null = {m: [column(rc, src) for rc, _ in replays] for m, src in SOURCES}
    p = {m: pvalues_steps(obs[m], null[m]) for m, _ in SOURCES}
    q = {m: np.maximum(qvalues_steps(obs[m], null[m]), p[m]) for m, _ in SOURCES}
    prim = "width_adjusted_mass"
    counts = np.asarray([d.size for d in null[prim]], np.int64)
    maxima = np.asarray([float(np.max(d)) if d.size else 0.0 for d in null[prim]], np.float64)
    max_q95 = float(np.quantile(maxima, 0.95, method="interpolated_inverted_cdf"))
    max_mean, count_mean = float(np.mean(maxima)), float(np.mean(counts))
    count_q95 = float(max(float(np.quantile(counts, 0.95, method="interpolated_inverted_cdf")), count_mean))
    r = len(replays)
    cap_draws = sum(1 for _, d in replays if d["cap_hit"])
    fsd = dict(num_replays=r, budget_num_bootstrap=r if num_bootstrap is None else int(num_bootstrap), observed_segment_count=len(peaks),
               observed_candidate_count=len(details), false_segment_count_mean=count_mean, false_segment_count_q95=count_q95,
               false_segment_fdr_estimate=float(np.clip(count_mean / float(max(len(peaks), 1)), 0.0, 1.0)),
               candidate_fdr_estimate=float(np.clip(count_mean / float(max(len(details), 1)), 0.0, 1.0)),
               dependence_span=int(dependence_span), scale_bins=[int(s) for s in scale_bins], candidate_cap_hit=cap_draws > 0,
               candidate_cap_hit_draws=cap_draws,
               candidate_per_view_cap_hit_draws=sum(1 for _, d in replays if d["per_view_cap_hit_count"] > 0),
               candidate_total_cap_hit_draws=sum(1 for _, d in replays if d["total_cap_hit"]),
               candidate_discarded_by_per_view_cap=sum(d["discarded_by_per_view_cap"] for _, d in replays),
               candidate_discarded_by_total_cap=sum(d["discarded_by_total_cap"] for _, d in replays),
               max_segments=diag["max_segments"], max_segments_per_scale_threshold=diag["max_segments_per_view"])
    pooled = np.concatenate(null[prim])
    for i, d in enumerate(details):
        stat = float(obs[prim][i])
        d["dwb_peak_score"] = d["dwb_empirical_statistic"] = stat
        d["dwb_peak_empirical_p"] = d["dwb_empirical_p"] = float(p[prim][i])
        d["dwb_peak_empirical_q"] = d["dwb_empirical_q"] = float(q[prim][i])
        d["dwb_empirical_null_replays"] = d["dwb_null_replay_num_draws"] = r
        for m, _ in SOURCES:
            d[m], d[f"{m}_p"], d[f"{m}_q"] = float(obs[m][i]), float(p[m][i]), float(q[m][i])
        d["dwb_peak_null_exceedances"] = int(np.sum(pooled >= stat)) if pooled.size else 0
        d["dwb_peak_scoring_threshold_key"], d["dwb_peak_scoring_threshold_z"] = str(d["threshold_key"]), float(d["threshold_z"])
        for k in ("integrated_excess", "mean_excess", "max_excess"):
            d[f"dwb_peak_{k}"] = float(d[k])
        d["dwb_null_replay_max_score_mean"], d["dwb_null_replay_max_score_q95"] = max_mean, max_q95
        d["dwb_null_replay_candidate_count_mean"], d["dwb_null_replay_candidate_count_q95"] = count_mean, count_q95
    by_span = {(d["start_idx"], d["end_idx"]): d for d in details}
    keys = ("candidate_id", "candidate_sources", "candidate_scale_bins", "candidate_threshold_keys",
            "overlapping_multiscale_candidate_count", "dwb_peak_score", "dwb_peak_empirical_p", "dwb_peak_empirical_q",
            "dwb_empirical_null_replays", "dwb_empirical_p", "dwb_empirical_q", "dwb_empirical_statistic", "dwb_peak_null_exceedances",
            "dwb_peak_scoring_threshold_key", "dwb_peak_scoring_threshold_z", "dwb_peak_integrated_excess", "dwb_peak_mean_excess",
            "dwb_peak_max_excess", "dwb_null_replay_num_draws", "dwb_null_replay_max_score_mean", "dwb_null_replay_max_score_q95",
            "dwb_null_replay_candidate_count_mean", "dwb_null_replay_candidate_count_q95")
    out_peaks = []
    for a, b in peaks:
        d = by_span[(int(a), int(b))]
        rec = {k: d.get(k, 0 if k == "overlapping_multiscale_candidate_count" else None) for k in keys}
        for m, _ in SOURCES:
            rec[m], rec[f"{m}_p"], rec[f"{m}_q"] = d[m], d[f"{m}_p"], d[f"{m}_q"]
        out_peaks.append(rec)
    summary = dict(enabled=True, primary_metric=prim, metrics=sorted(m for m, _ in SOURCES), num_peaks=len(peaks),
                   num_candidate_regions=len(details), num_bootstrap=r, budget_num_bootstrap=fsd["budget_num_bootstrap"],
                   random_seed=int(random_seed), dependence_span=int(dependence_span), scale_bins=[int(s) for s in scale_bins],
                   min_run_bins=max(int(min_run_bins), 1), observed_candidate_count=len(details), raw_multiscale_candidate_count=len(cands),
                   observed_candidate_cap_hit=bool(diag["cap_hit"]), null_replay_candidate_cap_hit=cap_draws > 0,
                   null_replay_candidate_cap_hit_draws=cap_draws, null_replay_candidate_count_mean=count_mean,
                   null_replay_candidate_count_q95=count_q95, null_replay_max_score_mean=max_mean, null_replay_max_score_q95=max_q95,
                   min_p=float(np.min(p[prim])), min_q=float(np.min(q[prim])), false_segment_diagnostics=fsd)
    return dict(enabled=True, candidate_details=details, peaks=out_peaks, summary=summary)


def differences(got, want, path=""):
    """Where two nested results differ: floats by their 64-bit pattern, everything else with == (bool is not int)."""
    if isinstance(want, dict):
        if not isinstance(got, dict) or set(got) != set(want):
            return [f"{path}: keys {sorted(set(got) ^ set(want)) if isinstance(got, dict) else type(got)}"]
        return [d for k in want for d in differences(got[k], want[k], f"{path}/{k}")]
    if isinstance(want, (list, tuple)):
        if not isinstance(got, (list, tuple)) or len(got) != len(want):
            return [f"{path}: length"]
        return [d for i, (g, w) in enumerate(zip(got, want)) for d in differences(g, w, f"{path}[{i}]")]
    if isinstance(want, float) or isinstance(got, float):
        return [] if isinstance(got, float) and isinstance(want, float) and bits(got) == bits(want) else [f"{path}: {got!r} != {want!r}"]
    return [] if type(got) is type(want) and got == want else [f"{path}: {got!r} != {want!r}"]
