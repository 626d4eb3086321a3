"""Case table for the multiscale candidate-segment native `cMultiscaleCandidateSegmentStats` (pyx:9460-9669).  Inputs are
re-synthesised from the table; the committed segments/segments_*.npz fixtures hold the REAL reference's outputs
(tests/golden/make_segments_golden.py).  Every comparison is exact: integers with ==, float64 values by their 64-bit patterns.

A case with more than FULL_ROWS output rows is recorded as its row count, its three counters and the SHA-256 of its eight row
arrays (equal digests = equal bits); smaller cases are recorded in full."""
from __future__ import annotations

import hashlib

import numpy as np

FETCH = 64          # values of a row the device walk fetches at a time (one per lane)
TILE = 256          # values per LDS tile of the device walk (csrc/csr_segments.h SEG_WT)
SEED = 505
CENTER, SD = 0.25, 1.3
Z = (0.0, 1.5, 2.0, 2.5, 3.0)
THRESHOLDS = tuple(CENTER + SD * z for z in Z)
NULL_SCALES = (1.3, 1.3, 0.05, 1e-320, 2.0)     # the fourth clamps to DBL_MIN: its excesses overflow, inf and NaN propagate
LENGTHS = (1, 2, FETCH - 1, FETCH, FETCH + 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 8193, 16385)
RUN_GAP = ((1, 0), (3, 2), (0, -1))
GROUPS = ("table", "special", "cap")
FULL_ROWS = 1024
FIELDS = ("start", "end", "scale", "view", "score", "integrated", "mean", "max")
CAP_N, CAP = 8193, 16


def scores(n, seed=SEED):
    return np.random.default_rng(seed).normal(CENTER, SD, n)


def cases():
    cs = []
    for n in LENGTHS:
        for min_run, gap in RUN_GAP:
            cs.append(dict(group="table", name=f"table_n{n}_run{min_run}_gap{gap}", gen="gauss", n=n, scales=(1, 2, 5, 17, n),
                           min_run=min_run, gap=gap, cap=0))
    # a scale of 0 (counts as 1), a repeated scale, a scale beyond n (counts as n)
    cs.append(dict(group="special", name="scales_zero_dup_beyond", gen="gauss", n=TILE + 1, scales=(0, 5, 5, TILE + 11), min_run=1,
                   gap=0, cap=0))
    cs.append(dict(group="special", name="constant_at_threshold", gen="const", n=TILE + 44, scales=(1, 2, 5, 17), min_run=1, gap=0, cap=0))
    cs.append(dict(group="special", name="all_below", gen="below", n=TILE + 44, scales=(1, 2, 5, 17), min_run=1, gap=0, cap=0))
    cs.append(dict(group="special", name="last_bin_ends_a_run", gen="tail", n=TILE + 1, scales=(1, 2, 5), min_run=1, gap=1, cap=0))
    cs.append(dict(group="special", name="a_wide_gap", gen="gauss", n=2 * TILE + 1, scales=(1, 5), min_run=2, gap=2 * TILE, cap=0))
    cs.append(dict(group="special", name="empty_track", gen="gauss", n=0, scales=(1, 2), min_run=1, gap=0, cap=0))
    cs.append(dict(group="special", name="no_views", gen="gauss", n=70, scales=(1, 2), min_run=1, gap=0, cap=0, views=0))
    cs.append(dict(group="special", name="no_scales", gen="gauss", n=70, scales=(), min_run=1, gap=0, cap=0))
    # the per-view cap (the inputs of the table at n = 8193)
    cs.append(dict(group="cap", name="cap16_n8193", gen="gauss", n=CAP_N, scales=(1, 2, 5, 17, CAP_N), min_run=1, gap=0, cap=CAP))
    cs.append(dict(group="cap", name="cap16_n8193_run3_gap2", gen="gauss", n=CAP_N, scales=(1, 2, 5, 17, CAP_N), min_run=3, gap=2,
                   cap=CAP))
    cs.append(dict(group="cap", name="cap1_n513", gen="gauss", n=2 * TILE + 1, scales=(1, 2, 5, 17), min_run=1, gap=0, cap=1))
    return cs


def inputs(case):
    """(scores, scales, thresholds, nullScales) of a case."""
    n = case["n"]
    x = scores(n)
    if case["gen"] == "const":
        x = np.full(n, THRESHOLDS[1])
    elif case["gen"] == "below":
        x = np.full(n, -10.0) + 0.001 * np.arange(n)
    elif case["gen"] == "tail":
        x = x.copy()
        x[-3:] = 9.0
        x[-7:-5] = 9.0
    nv = case.get("views", len(Z))
    return (x, np.asarray(case["scales"], np.int64), np.asarray(THRESHOLDS[:nv], np.float64),
            np.asarray(NULL_SCALES[:nv], np.float64))


def run_case(mod, case):
    """The native of `mod` on the case's inputs -> its 11-tuple."""
    x, sc, thr, ns = inputs(case)
    out = mod.cMultiscaleCandidateSegmentStats(x, sc, thr, ns, case["min_run"], case["gap"], case["cap"])
    assert len(out) == 11
    for q in range(8):
        a = np.asarray(out[q])
        assert a.dtype == (np.int64 if q < 4 else np.float64) and a.ndim == 1 and a.shape == np.asarray(out[0]).shape
    return out


def digest(result):
    h = hashlib.sha256()
    for q in range(8):
        h.update(np.ascontiguousarray(result[q]).tobytes())
    return np.frombuffer(h.digest(), np.uint8).copy()


def record(result):
    """What a fixture holds of one case."""
    rec = dict(rows=np.asarray([np.asarray(result[0]).shape[0]], np.int64),
               counters=np.asarray([int(result[8]), int(result[9]), int(result[10])], np.int64), sha256=digest(result))
    if rec["rows"][0] <= FULL_ROWS:
        for q, f in enumerate(FIELDS):
            rec[f] = np.asarray(result[q])
    return rec


def differences(result, rec):
    """Names of what differs between a native's 11-tuple and a case's record."""
    bad = []
    if np.asarray(result[0]).shape[0] != int(rec["rows"][0]):
        bad.append("rows")
    if [int(result[8]), int(result[9]), int(result[10])] != [int(v) for v in rec["counters"]]:
        bad.append("counters")
    for q, f in enumerate(FIELDS):
        if f in rec:
            a, b = np.asarray(result[q]), np.asarray(rec[f])
            if a.dtype != b.dtype or a.shape != b.shape or not np.array_equal(a.view(np.uint64), b.view(np.uint64)):
                bad.append(f)
    if not np.array_equal(digest(result), rec["sha256"]):
        bad.append("sha256")
    return bad


def load_group(path):
    """{case name: record} of one segments_<group>.npz."""
    out = {}
    with np.load(path) as z:
        for key in z.files:
            name, field = key.rsplit("/", 1)
            out.setdefault(name, {})[field] = z[key]
    return out


def cap_probe(x, scales, thr, ns, min_run, gap, cap):
    """A NumPy restatement of which views exceed the cap: {(scale index, view): (candidates, all finite, tie at the cap)}."""
    import twin_segments as T

    n = x.shape[0]
    pf = T.prefix(x)
    out = {}
    with np.errstate(all="ignore"):
        for si, w0 in enumerate(scales):
            w = int(min(max(int(w0), 1), n))
            sm = T.smooth(x, pf, w)
            for v in range(len(thr)):
                e = (x - thr[v]) / max(ns[v], T.TINY)
                ep = T.prefix(np.where(e < 0.0, 0.0, e))
                st, en = T.runs(sm > thr[v], max(gap, 0))
                keep = en - st + 1 >= max(min_run, 1)
                st, en = st[keep], en[keep]
                if st.shape[0] <= cap:
                    continue
                score = (ep[en + 1] - ep[st]) / np.sqrt((en - st + 1).astype(np.float64))
                finite = bool(np.all(np.isfinite(score)))
                srt = np.sort(score)[::-1]
                out[(si, v)] = (int(st.shape[0]), finite, bool(finite and srt[cap - 1] == srt[cap]))
    return out
