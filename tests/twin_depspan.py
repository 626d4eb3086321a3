"""NumPy twins of the dependence span, for tests and for the golden maker (no GPU, no library).

The three device stages are answered on the CPU the way the reference computes them -- byte comparison of rows, its per-window
ranking loop, its per-window function -- and plugged into the estimate of consenrich_amd/depspan.py (`choose`), whose host
steps the goldens of the compiled reference check.  Two forms, which differ in the lag sums of a window only:
  route "fft"    the reference's route: np.fft power spectra of the centred values and of the mask;
  route "truth"  the same steps with every lag sum as a direct sum of products in long double (a 64-bit significand: the
                 products and the sums are rounded at about 5e-20 relative, four orders below the 1e-15 floor of the gates).
"""
import hashlib

import numpy as np

from consenrich_amd import depspan as D


def lag_sums_truth(centred, mask, max_lag):
    c = np.asarray(centred, dtype=np.longdouble)
    m = np.asarray(mask, dtype=np.bool_)
    n = int(c.size)
    sums = np.zeros(max_lag + 1, dtype=np.float64)
    pairs = np.zeros(max_lag + 1, dtype=np.float64)
    for lag in range(max_lag + 1):
        sums[lag] = float(np.sum(c[:n - lag] * c[lag:], dtype=np.longdouble))
        pairs[lag] = float(np.count_nonzero(m[:n - lag] & m[lag:]))
    return sums, pairs


ROUTES = {"fft": D.lag_sums_fft, "truth": lag_sums_truth}


class TwinBackend:
    needs_gpu = False

    def __init__(self, matrices, st, route="fft"):
        self.all, self.st, self.lag_sums = matrices, st, ROUTES[route]
        self.windows = {}       # (eligible index, start bin) -> the window's record, as evaluated

    def open(self, positions):
        self.mats = [self.all[p] for p in positions]

    def unique_rows(self):
        kept, buckets = [], {}
        for r in range(int(self.mats[0].shape[0])):
            h = hashlib.sha256()
            for m in self.mats:
                h.update(np.ascontiguousarray(m[r]).view(np.uint8))
            same = [k for k in buckets.get(h.digest(), [])
                    if all(np.array_equal(m[r].view(np.uint32), m[k].view(np.uint32)) for m in self.mats)]
            if not same:
                buckets.setdefault(h.digest(), []).append(r)
                kept.append(r)
        return kept

    def window_scores(self, rows):
        wb, scores, counts = self.st.window_bins, [], []
        for m in self.mats:
            for w in range(int(m.shape[1]) // wb):
                per_row = []
                for r in rows:
                    v = np.asarray(m[r, w * wb:(w + 1) * wb], dtype=np.float64)
                    fin = np.isfinite(v)
                    k = int(np.count_nonzero(fin))
                    if k > 0 and (float(k) / float(wb)) >= self.st.rank_coverage_min:
                        per_row.append(float(wb) / float(k) * float(np.sum(np.maximum(v[fin], 0.0))))
                counts.append(len(per_row))
                scores.append(float(np.median(np.asarray(per_row, dtype=np.float64))) if per_row else np.nan)
        return np.asarray(scores, dtype=np.float64), np.asarray(counts, dtype=np.int64)

    def window_rows(self, k, start, rows):
        return np.asarray(self.mats[k][rows, start:start + self.st.window_bins])

    def window_acf(self, rows, windows):
        recs = []
        for k, start in windows:
            rec = D.window_on_host(self.window_rows(k, start, rows), self.st, self.lag_sums)
            self.windows[(int(k), int(start))] = rec
            recs.append(rec)
        return recs, [r["pooled"] for r in recs]


def settings(n_names, n_matrices, interval, kw):
    d = dict(windowBP=100000, windowCount=256, maxLagBP=50000, workingQuantile=0.75, bootstrapDraws=500, randSeed=1729,
             minWindowCount=20, acfThreshold=0.1, acfSmoothingBP=250, crossingPersistenceBP=250, minFinitePairs=200,
             minFinitePairCoverage=0.5)
    d.update(kw)
    return D.Settings(n_names, n_matrices, interval, d["windowBP"], d["windowCount"], d["maxLagBP"], d["workingQuantile"],
                      d["bootstrapDraws"], d["randSeed"], d["minWindowCount"], d["acfThreshold"], d["acfSmoothingBP"],
                      d["crossingPersistenceBP"], d["minFinitePairs"], d["minFinitePairCoverage"])


def run(names, matrices, interval, *, route="fft", period_diagnostics=True, **kw):
    """(result tuple, backend) of the twin; the backend holds every evaluated window's record."""
    try:
        names, matrices = list(names), list(matrices)
    except Exception as exc:
        raise ValueError("chromosome inputs must be finite sequences") from exc
    st = settings(len(names), len(matrices), interval, kw)
    matrices = [np.asarray(m) for m in matrices]
    rows = D.check_shapes([m.shape for m in matrices], [m.dtype.kind for m in matrices])
    lengths = [int(m.shape[1]) for m in matrices]
    backend = TwinBackend(matrices, st, route)
    return D.choose(names, lengths, rows, backend, st, want_period=period_diagnostics), backend


def fft_twin(names, matrices, interval, **kw):
    return run(names, matrices, interval, route="fft", **kw)[0]


def truth_twin(names, matrices, interval, **kw):
    return run(names, matrices, interval, route="truth", **kw)[0]


# ---- comparisons shared by the golden maker and the tests --------------------------------------------------------------------
CONTINUOUS_WINDOW = ("oscillationStrength", "postCrossingRevival")
CONTINUOUS_TOP = ("oscillationStrength", "postCrossingRevival")
EXTRA_KEYS = ("decided_on_host",)


def strip(result):
    """The result without the keys this project adds, as plain JSON-able data."""
    point, lower, upper, diag = result
    diag = {k: v for k, v in diag.items() if k not in EXTRA_KEYS}
    return [int(point), int(lower), int(upper), diag]


def discrete_differences(want, got, skip_period=False):
    """Where two stripped results differ in anything but the continuous quantities: a list of texts (empty: equal).  Floats are
    compared exactly (scores, ranks, radii, bootstrap lists)."""
    out = []
    for i in range(3):
        if want[i] != got[i]:
            out.append(f"tuple[{i}]: {want[i]} != {got[i]}")
    dw, dg = want[3], got[3]
    if list(dw.keys()) != list(dg.keys()):
        out.append(f"keys: {list(dw.keys())} != {list(dg.keys())}")
        return out
    for key in dw:
        if key == "selectedWindows":
            if len(dw[key]) != len(dg[key]):
                out.append(f"selectedWindows: {len(dw[key])} != {len(dg[key])}")
                continue
            for n, (a, b) in enumerate(zip(dw[key], dg[key])):
                if list(a.keys()) != list(b.keys()):
                    out.append(f"selectedWindows[{n}] keys")
                    continue
                for f in a:
                    if f in CONTINUOUS_WINDOW or (skip_period and f == "dominantACFPeriodBP"):
                        if (a[f] is None) != (b[f] is None) and not (skip_period and f != "postCrossingRevival"):
                            out.append(f"selectedWindows[{n}].{f}: {a[f]} / {b[f]}")
                        continue
                    if a[f] != b[f] or type(a[f]) is not type(b[f]):
                        out.append(f"selectedWindows[{n}].{f}: {a[f]!r} != {b[f]!r}")
        elif key in CONTINUOUS_TOP or (skip_period and key in ("dominantACFPeriodBPMedian", "unresolvedPeriodFraction")):
            if (dw[key] is None) != (dg[key] is None) and not (skip_period and key != "postCrossingRevival"):
                out.append(f"{key}: {dw[key]} / {dg[key]}")
        elif dw[key] != dg[key] or type(dw[key]) is not type(dg[key]):
            out.append(f"{key}: {dw[key]!r} != {dg[key]!r}")
    return out


def continuous_error(want, got, field):
    """The largest |difference| of a continuous per-window field (and of its top-level median) between two stripped results."""
    worst = 0.0
    for a, b in zip(want[3]["selectedWindows"], got[3]["selectedWindows"]):
        if a[field] is not None and b[field] is not None:
            worst = max(worst, abs(float(a[field]) - float(b[field])))
    if want[3][field] is not None and got[3][field] is not None:
        worst = max(worst, abs(float(want[3][field]) - float(got[3][field])))
    return worst
