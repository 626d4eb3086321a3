"""The case table of the DWB peak-scoring tests: inputs are re-synthesised from here, tests/golden/peakscore/peakscore_*.npz hold
the REAL reference's outputs on them (tests/golden/make_peakscore_golden.py).  Shared by the CPU twin test and the GPU tests."""
import numpy as np

TINY = float(np.finfo(np.float64).tiny)
SORT_TILE = 2048        # keys per bitonic tile of the device sort (csrc/csr_null.h NULL_TILE)
N_TRACK = 20001

# ---------------------------------------------------------------------------------------------------------------
# segment scores
# ---------------------------------------------------------------------------------------------------------------
LENGTHS = (1, 7, 8, 9, 127, 128, 129, 8191, 8192, 8193, N_TRACK)


def track(n=N_TRACK, seed=5):
    rng = np.random.default_rng(seed)
    x = rng.normal(0.3, 1.2, n)
    x[::97] = 0.5           # exactly at a threshold: an excess of +0.0
    x[11::389] = -0.0
    x[min(n - 1, 150)] = 60.0     # over the DBL_MIN view's threshold: (60 - 4) / DBL_MIN is inf
    return x


def segments(n=N_TRACK):
    """(starts, ends): every length of LENGTHS that fits at two offsets, one segment clamped at each end, empty ones."""
    st, en = [], []
    for length in LENGTHS:
        if length > n:
            continue
        for off in (min(100, n - length), n - length):
            st.append(off)
            en.append(off + length - 1)
    st += [-5, n - 4, 50, n + 3, -9, 0]
    en += [10, n + 7, 49, n + 9, -2, -1]
    return np.asarray(st, np.int64), np.asarray(en, np.int64)


def view_sets():
    """views4: the second view ties the first exactly (the first must win); the third is all NaN after a finite one (it never
    replaces); the fourth clamps to DBL_MIN (inf where a value exceeds its threshold: it replaces there).  nan_first: a NaN score
    in front is never replaced.  one: a single plain view.  skipped: an entry that is no mapping in between."""
    a = dict(threshold_z=2.0, threshold=0.5, null_scale=1.3)
    b = dict(threshold_z=2.5, threshold=0.5, null_scale=1.3)
    nan = dict(threshold_z=3.0, threshold=float("nan"), null_scale=0.7)
    tiny = dict(threshold_z=3.5, threshold=4.0, null_scale=0.0)
    return {"views4": {"a": a, "b": b, "nan": nan, "tiny": tiny},
            "nan_first": {"nan": nan, "a": a},
            "one": {"z2": dict(threshold_z=2.0, threshold=-0.25, null_scale=0.05)},
            "skipped": {"a": a, "not a view": 3.0, "hi": dict(threshold_z=1.0, threshold=0.1, null_scale=0.9)}}


def segment_cases():
    out = [dict(name=f"seg_n{N_TRACK}_{k}", n=N_TRACK, views=k) for k in view_sets()]
    out += [dict(name=f"seg_n{n}_views4", n=n, views="views4") for n in (1, 9, 300)]
    return out


# ---------------------------------------------------------------------------------------------------------------
# p and q values
# ---------------------------------------------------------------------------------------------------------------
K_LIST = (0, 1, 33, 4097)
DRAW_SIZES = {"r0": (), "r1": (1,), "r1_empty": (0,), "r5": (1000, 0, 600, 400, SORT_TILE + 1 - 2000)}


def draws(sizes, seed=17):
    """Values on a grid of tenths (many ties), both zeros, per draw."""
    rng = np.random.default_rng(seed)
    out = []
    for s in sizes:
        d = np.round(rng.normal(1.0, 2.0, s), 1)
        d[::7] = 0.0
        d[3::11] = -0.0
        out.append(d)
    return out


def observed(k, null_draws, seed=23):
    """Copies of pooled values (side="left" matters), repeats, both zeros, one value above and one below the whole pool."""
    rng = np.random.default_rng(seed + k)
    pool = np.concatenate(null_draws) if null_draws else np.zeros(0)
    base = np.round(rng.normal(1.5, 2.5, k), 1)
    if pool.size:
        take = rng.integers(0, pool.size, k)
        base = np.where(rng.random(k) < 0.6, pool[take], base)
    special = [0.0, -0.0, 1.0e3, -1.0e3, 0.0, 1.0e3]
    for i, v in enumerate(special[:k]):
        base[(i * 5) % k] = v
    if k > 8:
        base[k // 2] = base[k // 3]
    return np.ascontiguousarray(base, np.float64)


def pq_cases():
    return [dict(name=f"pq_k{k}_{r}", k=k, draws=r) for k in K_LIST for r in DRAW_SIZES]


def pq_inputs(case):
    d = draws(DRAW_SIZES[case["draws"]])
    return observed(case["k"], d), d


# ---------------------------------------------------------------------------------------------------------------
# the merge
# ---------------------------------------------------------------------------------------------------------------
def merge_inputs(seed=3, n=400, k=60, peaks=12):
    """Observed candidates with repeated spans, repeated scores inside a span and a NaN score; peaks of which some coincide with
    a candidate's span and some overlap none."""
    rng = np.random.default_rng(seed)
    cands = []
    for i in range(k):
        a = int(rng.integers(0, n - 40))
        b = a + int(rng.integers(0, 12))
        if i % 5 == 1:
            a, b = cands[-1]["start_idx"], cands[-1]["end_idx"]
        score = float(np.round(rng.gamma(2.0, 1.0), 1))
        if i == 7:
            score = float("nan")
        cands.append(dict(start_idx=a, end_idx=b, scale_bins=int((1, 2, 5)[i % 3]), threshold_key=f"z{i % 4}", threshold_z=float(i % 4),
                          threshold=0.1 * (i % 4), null_scale=1.0 + (i % 4), score=score, integrated_excess=score * 2.0,
                          mean_excess=score / 3.0, max_excess=score / 2.0))
    spans, details = [], []
    for j in range(peaks):
        if j % 3 == 0:
            a, b = cands[j]["start_idx"], cands[j]["end_idx"]
        elif j % 3 == 1:
            a = int(rng.integers(0, n - 40))
            b = a + int(rng.integers(0, 30))
        else:
            a, b = n - 30 + j, n - 30 + j       # beyond every candidate
        s = float(np.round(rng.gamma(2.0, 1.0), 1))
        spans.append((a, b))
        details.append(dict(score=s, integrated_excess=s * 1.5, mean_excess=s / 4.0, max_excess=s / 5.0, threshold_key=f"z{j % 4}",
                            threshold_z=float(j % 4), threshold=0.1 * (j % 4), null_scale=1.0 + (j % 4)))
    return cands, spans, details, n


# ---------------------------------------------------------------------------------------------------------------
# the scorer: two chains, their views, templates and peaks
# ---------------------------------------------------------------------------------------------------------------
SCORER_LENS = (4097, 1031)
SCORER_BWS = (5, 3)
SCORER_SCALES = (1, 2, 5)
SCORER_Z = (1.5, 2.0, 2.5)
SCORER_SEED, SCORER_REPLAYS, SCORER_GROUP = 11, 4, 3        # a group boundary inside the replays
SCORER_VIEW_CAP, SCORER_TOTAL_CAP = 16, 40
SCORER_CENTERS, SCORER_NULL_SCALES = (0.2, -0.1), (1.0, 0.8)
SCORER_TEMPLATE_SD = (1.0, 0.35)        # chain 0: every draw exceeds the total cap; chain 1: a handful of candidates per draw


def scorer_inputs():
    """(scores, templates, views) per chain: score tracks with planted bumps of several widths."""
    rng = np.random.default_rng(808)
    scores, tmpls, views = [], [], []
    for c, n in enumerate(SCORER_LENS):
        x = rng.normal(SCORER_CENTERS[c], 0.6, n)
        for k, (at, width, height) in enumerate(((n // 7, 1, 4.0), (n // 3, 6, 3.0), (n // 2, 25, 2.5), (n - 40, 12, 3.5))):
            x[at:at + width] += height + 0.01 * k
        scores.append(x)
        tmpls.append(rng.normal(0.0, SCORER_TEMPLATE_SD[c], n))
        views.append([dict(threshold_z=z, threshold=SCORER_CENTERS[c] + z * SCORER_NULL_SCALES[c], null_scale=SCORER_NULL_SCALES[c],
                           null_center=SCORER_CENTERS[c]) for z in SCORER_Z])
    return scores, tmpls, views


def scorer_twin(scores, tmpls, views, bws=SCORER_BWS, scales=SCORER_SCALES, replays=SCORER_REPLAYS, seed=SCORER_SEED,
                total_cap=SCORER_TOTAL_CAP, view_cap=SCORER_VIEW_CAP):
    """Per chain what the twins of the replay loop compute: observed (candidates, diagnostics), replays [(candidates,
    diagnostics)] draw by draw on tests/twin_dwb.py's draws, and the scales (scales None: the five of the chain's bandwidth)."""
    import twin_dwb
    import twin_segments as TS

    r = replays
    strides = [t.shape[0] + 2 * twin_dwb.max_lag(max(bw, 2), 0) for t, bw in zip(tmpls, bws)]
    noise = twin_dwb.stream(seed, r * max(strides))
    out = []
    for c, t in enumerate(tmpls):
        vw = {str(i): v for i, v in enumerate(views[c])}
        rv = {k: dict(threshold_z=v["threshold_z"], threshold=float(v["threshold"] - v["null_center"]), null_scale=v["null_scale"])
              for k, v in vw.items()}
        sc = TS.resolve_scales(t.shape[0], scales, bws[c])
        kw = dict(scale_bins=sc, min_run_bins=1, max_gap_bins=0, max_segments=total_cap, max_segments_per_view=view_cap)
        reps = [TS.multiscale_candidates(twin_dwb.draw_fast(t, max(bws[c], 2), noise[b * strides[c]:(b + 1) * strides[c]],
                                                            "bartlett"), rv, **kw) for b in range(r)]
        # every draw's candidate scores before the total cap, descending: what the cut falls into
        before = [sorted((k["score"] for k in TS.multiscale_candidates(
            twin_dwb.draw_fast(t, max(bws[c], 2), noise[b * strides[c]:(b + 1) * strides[c]], "bartlett"), rv,
            **dict(kw, max_segments=None))[0]), reverse=True) for b in range(r)]
        out.append(dict(observed=TS.multiscale_candidates(scores[c], vw, **kw), replays=reps, scale_bins=sc, views=vw,
                        scores_before_total_cap=before))
    return out


def scorer_case_facts(twin, peaks):
    """What the scorer case is there for, as found on the twin: a replay draw over the total cap whose scores at ranks cap and
    cap + 1 are equal (the stable order decides the cut), a draw under the cap, an exported peak on an observed candidate's span."""
    cap = SCORER_TOTAL_CAP
    before = [s for ch in twin for s in ch["scores_before_total_cap"]]
    spans = [{(k["start_idx"], k["end_idx"]) for k in ch["observed"][0]} for ch in twin]
    return dict(draw_over_the_total_cap_with_a_tie_across_the_cut=any(len(s) > cap and s[cap - 1] == s[cap] for s in before),
                draw_under_the_total_cap=any(0 < len(s) < cap for s in before),
                peak_on_an_observed_candidate=any(p in spans[c] for c in range(len(twin)) for p in peaks[c]))


def scorer_peaks(twin):
    """Per chain (start_idx, end_idx) of the exported peaks: one that coincides with an observed candidate, one that overlaps
    several, one that overlaps none, one twice."""
    out = []
    for c, n in enumerate(SCORER_LENS):
        cands = twin[c]["observed"][0]
        hit = cands[len(cands) // 2]
        spans = [(int(hit["start_idx"]), int(hit["end_idx"])), (n // 2 - 3, n // 2 + 30), (5, 9), (n // 3, n // 3 + 5)]
        out.append(sorted(set(spans)))
    return out
