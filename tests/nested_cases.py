"""Case table of the nested ROCCO refinement (tests/test_nested_twin.py, tests/test_gpu_nested.py and the fixture maker
tests/golden/make_nested_golden.py).  Inputs are re-synthesised from seeds; the fixtures hold outputs only.

TILE is the unit at which the device's walk changes path: the 32 bins of a back-pointer word (csrc/csr_nested.h NESTED_WORD).
WIDE_MIN_RUN is the first `minRun` served by the states-as-lanes kernel (NESTED_REG_STATES + 1)."""
import numpy as np

TILE = 32
WIDE_MIN_RUN = 9
CHUNK = 8192


def _hann(w):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * (np.arange(w) + 0.5) / w)


def parent(rng, length, humps, noise=0.15, height=2.0):
    """One parent region: `humps` Hann humps side by side over `length` bins, plus noise"""
    x = np.zeros(length)
    edges = np.linspace(0, length, humps + 1).astype(int)
    for a, b in zip(edges[:-1], edges[1:]):
        if b > a:
            x[a:b] = height * rng.uniform(0.5, 1.5) * _hann(b - a)
    return x + noise * rng.standard_normal(length)


def planted(seed, lengths, humps=None, valley=None, dyadic=False, lead=3, noise=0.15):
    """(scores, solution): parents of the given lengths joined by flat negative valleys of 1..40 bins"""
    rng = np.random.default_rng(seed)
    parts, mask = [np.full(lead, -1.0)], [np.zeros(lead, bool)]
    for k, L in enumerate(lengths):
        h = int(rng.integers(1, 5)) if humps is None else humps[k % len(humps)]
        parts.append(parent(rng, int(L), min(h, max(int(L) // 4, 1)), noise))
        mask.append(np.ones(int(L), bool))
        v = int(rng.integers(1, 41)) if valley is None else valley
        parts.append(np.full(v, -1.0))
        mask.append(np.zeros(v, bool))
    x = np.concatenate(parts)
    if dyadic:
        x = np.round(x * 4.0) / 4.0
    return np.ascontiguousarray(x, np.float64), np.concatenate(mask).astype(np.uint8)


def _mixed_lengths(seed, count, lo=1, hi=260):
    rng = np.random.default_rng(seed)
    return [int(v) for v in np.exp(rng.uniform(np.log(lo), np.log(hi), count)).astype(int)]


# ---- `_refineNestedROCCOSolution` ------------------------------------------------------------------------------------------
# geometry: None (bin mode), ("uniform", 25), or ("mixed",): widths 25 and 50 bp in alternating stretches
REFINE = [
    dict(name="planted40", seed=11, lengths=_mixed_lengths(1, 40, 8, 120), gamma=1.0, penalty=0.3),
    dict(name="planted40_bp25", seed=11, lengths=_mixed_lengths(1, 40, 8, 120), gamma=1.0, penalty=0.3, geometry=("uniform", 25),
         min_bp=125),
    dict(name="mixed_widths", seed=12, lengths=_mixed_lengths(2, 24, 4, 90), gamma=1.0, penalty=0.3, geometry=("mixed",), min_bp=125),
    dict(name="scale0", seed=13, lengths=_mixed_lengths(3, 12, 6, 80), gamma=1.0, penalty=0.3, scale=0.0),
    dict(name="scale1", seed=13, lengths=_mixed_lengths(3, 12, 6, 80), gamma=1.0, penalty=0.3, scale=1.0),
    dict(name="iters0", seed=14, lengths=[20, 30, 7], gamma=1.0, penalty=0.3, iters=0),
    dict(name="iters1", seed=14, lengths=[20, 30, 7, 60], gamma=1.0, penalty=0.3, iters=1),
    dict(name="jaccard04", seed=15, lengths=_mixed_lengths(4, 12, 20, 90), gamma=1.0, penalty=0.3, jaccard=0.4),
    dict(name="mask_equal", seed=16, lengths=[6, 7, 9], humps=[1], gamma=8.0, penalty=-5.0, scale=1.0, noise=0.0),
    dict(name="short_regions", seed=17, lengths=[1, 2, 4, 5, 6, 1, 5, 6], gamma=0.5, penalty=0.2),
    dict(name="min_run1", seed=18, lengths=[1, 2, 3, 9, 17], gamma=0.5, penalty=0.4, min_bins=1),
    dict(name="min_run2", seed=18, lengths=[2, 3, 4, 9, 33], gamma=0.5, penalty=0.4, min_bins=2),
    dict(name="min_run_wide", seed=19, lengths=[WIDE_MIN_RUN - 1, WIDE_MIN_RUN, WIDE_MIN_RUN + 1, 31, 64, 200], humps=[4], gamma=0.2,
         penalty=0.3, min_bins=WIDE_MIN_RUN),
    dict(name="min_run_wide40", seed=19, lengths=[40, 41, 95, 300], humps=[4], gamma=0.2, penalty=0.3, min_bins=40),
    dict(name="dyadic", seed=20, lengths=_mixed_lengths(5, 30, 5, 70), gamma=0.5, penalty=0.25, dyadic=True),
    dict(name="dyadic_scale1", seed=21, lengths=_mixed_lengths(6, 30, 5, 70), gamma=1.0, penalty=0.5, dyadic=True, scale=1.0),
    dict(name="all_negative", seed=22, lengths=[5, 6, 12, 40], gamma=0.5, penalty=0.3, shift=-5.0),
    dict(name="tile_edges", seed=23, lengths=[TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1], humps=[3], gamma=0.5,
         penalty=0.3),
    dict(name="chunk_edges", seed=24, lengths=[CHUNK - 1, CHUNK, CHUNK + 1], humps=[4], gamma=1.0, penalty=0.3, noise=0.3),
    dict(name="ragged", seed=25, lengths=_mixed_lengths(7, 150, 1, 700), gamma=1.0, penalty=0.3),
    dict(name="selected_over_8192", seed=26, lengths=_mixed_lengths(8, 90, 60, 220), gamma=1.0, penalty=0.3),
    dict(name="empty_mask", seed=27, lengths=[], gamma=1.0, penalty=0.3, lead=50),
    dict(name="required_ends", seed=28, lengths=[12, 12, 12], gamma=0.5, penalty=0.3, plant="required"),
    # children of one and of two bins that reach layer 2 (the quantile of one value, of two values), and processed regions with exactly
    # one and exactly two strictly positive scores
    dict(name="tiny_children", seed=30, lengths=[3, 4, 6, 2, 1], gamma=0.5, penalty=0.4, min_bins=1, plant="spikes", valley=3),
    # the largest minimum run the states-as-lanes kernel serves, in a region one bin longer, as long, and longer
    dict(name="min_run_255", seed=31, lengths=[256, 255, 300], humps=[2], gamma=0.2, penalty=0.3, min_bins=255, valley=2),
    dict(name="raw_scores", seed=29, lengths=_mixed_lengths(9, 10, 8, 60), gamma=1.0, penalty=0.3, raw=True),
]


def refine_inputs(case):
    """keyword arguments of the refinement for one case"""
    x, sol = planted(case["seed"], case["lengths"], humps=case.get("humps"), valley=case.get("valley"), dyadic=case.get("dyadic", False),
                     lead=case.get("lead", 3), noise=case.get("noise", 0.15))
    if "shift" in case:
        x = np.where(sol > 0, x + case["shift"], x - 10.0)
    if case.get("plant") == "required":
        # the largest raw score first, last, and tied (the leftmost of two equal maxima is required)
        runs = np.flatnonzero(np.diff(np.concatenate(([0], sol, [0]))) == 1)
        x[runs[0]] = 9.0
        x[runs[1] + 11] = 9.0
        x[runs[2] + 3] = x[runs[2] + 8] = 9.0
    if case.get("plant") == "spikes":
        # every parent is -3 but for one bin (two neighbours in the second parent) of 5
        runs = np.flatnonzero(np.diff(np.concatenate(([0], sol, [0]))) == 1)
        x[sol > 0] = -3.0
        for k, (a, at) in enumerate(zip(runs, (1, 1, 2, 0, 0))):
            x[a + at] = 5.0
            if k == 1:
                x[a + at + 1] = 5.0
    kw = dict(scores=x, solution=sol, gamma=case["gamma"], selectionPenalty=case["penalty"], nestedRoccoIters=case.get("iters", 3),
              nestedRoccoBudgetScale=case.get("scale", 0.75), jaccardThreshold=case.get("jaccard", 0.999),
              minRegionBP=case.get("min_bp"), minRegionBins=case.get("min_bins", 5))
    geo = case.get("geometry")
    if geo:
        w = np.full(x.size, 25, np.int64)
        if geo[0] == "mixed":
            w[(np.arange(x.size) // 37) % 2 == 1] = 50
        ends = np.cumsum(w)
        kw.update(intervals=ends - w + 1000, ends=ends + 1000)
    if case.get("raw"):
        rng = np.random.default_rng(case["seed"] + 1000)
        kw["rawScores"] = x + 0.5 * rng.standard_normal(x.size)
    return kw


# ---- `_solveParentConditionedSubpeaks` -------------------------------------------------------------------------------------
def _near_ties():
    """Two ways to the same place whose values differ by 5e-13 (inside the tolerance: the count decides) and by 2e-12 (outside)"""
    x = np.array([1.0, -0.5, 0.5 + 5e-13, 1.0, -0.5, 0.5 + 2e-12, 1.0, -0.5, 0.5 - 5e-13, 1.0, -0.5, 0.5 - 2e-12, 1.0])
    return x


SOLVE = [
    dict(name="len1", x=[0.7], M=5, req=0, penalty=0.1, costs="edges"),
    dict(name="len_eq_min_run", seed=1, n=5, M=5, req="argmax", penalty=0.2, costs="edges"),
    dict(name="len_min_run_plus1", seed=2, n=6, M=5, req="argmax", penalty=0.2, costs="edges"),
    dict(name="min_run1", seed=3, n=40, M=1, req="argmax", penalty=0.3, costs="edges"),
    dict(name="min_run2", seed=4, n=40, M=2, req="argmax", penalty=0.3, costs="edges"),
    dict(name="min_run5", seed=5, n=90, M=5, req="argmax", penalty=0.3, costs="edges"),
    dict(name="min_run_wide", seed=6, n=150, M=WIDE_MIN_RUN, req="argmax", penalty=0.3, costs="edges"),
    dict(name="min_run_wide64", seed=6, n=300, M=64, req="argmax", penalty=0.3, costs="edges"),
    dict(name="min_run_255", seed=15, n=600, M=255, req="argmax", penalty=0.3, costs="edges"),
    dict(name="min_run_255_len256", seed=16, n=256, M=255, req="argmax", penalty=0.3, costs="edges"),
    dict(name="required_first", seed=7, n=30, M=3, req=0, penalty=0.5, costs="edges"),
    dict(name="required_last", seed=7, n=30, M=3, req=29, penalty=0.5, costs="edges"),
    dict(name="no_required", seed=8, n=50, M=4, req=None, penalty=0.4, costs="edges"),
    dict(name="no_required_all_negative", seed=8, n=50, M=4, req=None, penalty=9.0, costs="edges"),
    dict(name="all_negative", seed=9, n=25, M=5, req="argmax", penalty=0.0, costs="edges", shift=-9.0),
    dict(name="scalar_cost", seed=10, n=60, M=3, req="argmax", penalty=0.2, costs=0.3, run_penalty=0.0),
    dict(name="random_costs", seed=11, n=80, M=4, req="argmax", penalty=0.2, costs="random", run_penalty=0.05),
    dict(name="dyadic", seed=14, n=120, M=3, req="argmax", penalty=0.25, costs=0.25, run_penalty=0.25, dyadic=True),
    dict(name="dyadic_min_run1", seed=13, n=120, M=1, req="argmax", penalty=0.25, costs=0.25, run_penalty=0.0, dyadic=True),
    dict(name="near_ties", x=_near_ties().tolist(), M=1, req=0, penalty=0.0, costs=0.5, run_penalty=0.0),
    dict(name="near_ties_m2", x=np.repeat(_near_ties(), 2).tolist(), M=2, req=0, penalty=0.0, costs=0.5, run_penalty=0.5),
    dict(name="word_minus1", seed=14, n=TILE - 1, M=5, req="argmax", penalty=0.3, costs="edges"),
    dict(name="word", seed=14, n=TILE, M=5, req="argmax", penalty=0.3, costs="edges"),
    dict(name="word_plus1", seed=14, n=TILE + 1, M=5, req="argmax", penalty=0.3, costs="edges"),
]


def solve_inputs(case):
    if "x" in case:
        x = np.asarray(case["x"], np.float64)
    else:
        rng = np.random.default_rng(case["seed"])
        x = parent(rng, case["n"], max(case["n"] // 25, 1), 0.3, 1.5) - 0.3
        if case.get("dyadic"):
            x = np.round(x * 4.0) / 4.0
        x = x + case.get("shift", 0.0)
    n = x.size
    internal = 0.25
    if case["costs"] == "edges":
        costs = np.full(n + 1, internal)
        costs[0] = costs[-1] = 1e-12
        rp = internal
    elif case["costs"] == "random":
        costs = np.random.default_rng(case["seed"] + 500).uniform(0.0, 0.6, n + 1)
        rp = case["run_penalty"]
    else:
        costs = float(case["costs"])
        rp = case["run_penalty"]
    req = case["req"]
    if req == "argmax":
        req = int(np.argmax(x))
    return dict(scores=x, boundaryCosts=costs, selectionPenalty=case["penalty"], minRunBins=case["M"], requiredIndex=req, runPenalty=rp)


# ---- the argument checks: (keyword overrides, the reference's message) --------------------------------------------------------
def refine_errors():
    x, sol = planted(1, [10, 12])
    good = dict(scores=x, solution=sol, gamma=1.0, selectionPenalty=0.3)
    bad = x.copy()
    bad[3] = np.nan
    return good, [
        (dict(scores=bad), "`scores` contains non-finite values"),
        (dict(scores=np.zeros(0)), "`scores` must be non-empty"),
        (dict(scores=x.reshape(1, -1)), "`scores` must be one-dimensional"),
        (dict(rawScores=x[:-1]), "`rawScores` must match `scores` length"),
        (dict(rawScores=bad), "`rawScores` contains non-finite values"),
        (dict(solution=sol[:-1]), "`solution` must match `scores` length"),
        (dict(intervals=np.arange(x.size)), "`intervals` and `ends` must be supplied together"),
        (dict(intervals=np.arange(3), ends=np.arange(3)), "`intervals` and `ends` must match `scores` length"),
        (dict(gamma=-1.0), "`gamma` must be finite and non-negative"),
        (dict(gamma=float("inf")), "`gamma` must be finite and non-negative"),
        (dict(selectionPenalty=float("nan")), "`selectionPenalty` must be finite"),
        (dict(nestedRoccoBudgetScale=float("nan")), "`nestedRoccoBudgetScale` must be finite"),
    ]


def solve_errors():
    x = np.linspace(-1.0, 1.0, 12)
    good = dict(scores=x, boundaryCosts=0.1, selectionPenalty=0.2, minRunBins=3, requiredIndex=4, runPenalty=0.1)
    bad = x.copy()
    bad[0] = np.inf
    return good, [
        (dict(scores=np.zeros(0)), "`scores` must be a non-empty one-dimensional array"),
        (dict(scores=bad), "`scores` contains non-finite values"),
        (dict(boundaryCosts=np.ones(5)), "`boundaryCosts` must be scalar or have length len(scores) + 1"),
        (dict(boundaryCosts=-0.1), "`boundaryCosts` must be finite and non-negative"),
        (dict(selectionPenalty=float("inf")), "`selectionPenalty` must be finite"),
        (dict(runPenalty=-1.0), "`runPenalty` must be finite and non-negative"),
        (dict(requiredIndex=12), "`requiredIndex` is outside `scores`"),
        (dict(requiredIndex=-1), "`requiredIndex` is outside `scores`"),
    ]
