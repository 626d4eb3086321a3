"""The case table of the massive sub-peak clean-up: small synthetic children (bins of 25, 50 or 100 bp, hand-made policies with
thresholds of 700-3000 bp, so candidates are 29-200 bins; three cases sit on the edges of the device's sort tile) and small sets
of peak widths for the policy.  The fixtures (tests/golden/cleanup) hold OUTPUTS only; every input is re-synthesised from here.

FORCE     kwargs of `_forceMassiveSubpeakSegments`, one call per child of a case;
SPLITS    kwargs of `_bestMassiveSubpeakSplit`;
CONTRACTS kwargs of `_contractMassiveSubpeakSegment`;
POLICIES  kwargs of `_learnMassiveSubpeakWidthPolicy` (the widths also go through the width scores and the width p value)."""
import math
import zlib

import numpy as np

SORT_TILE = 2048


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def profile(name, chunks, grid=None):
    """scores: chunks of (bins, level, noise) one after the other; `grid` rounds to multiples of it (ties become exact)"""
    rng = _rng(name)
    out = np.concatenate([level + noise * rng.standard_normal(bins) for bins, level, noise in chunks])
    if grid:
        out = np.round(out / grid) * grid
    return np.ascontiguousarray(out, np.float64)


def coords(widths, origin=1000):
    edges = origin + np.concatenate(([0], np.cumsum(np.asarray(widths, np.int64))))
    return edges[:-1].astype(np.int64), edges[1:].astype(np.int64)


def signal(name, n):
    x = np.round(_rng(name + "/state").standard_normal(n) * 4.0) / 4.0     # (a coarse grid: equal maxima occur)
    return np.ascontiguousarray(x, np.float64)


def policy(threshold, contract=None, min_bp=None):
    p = {"width_threshold_bp": threshold}
    if contract is not None:
        p["contract_width_bp"] = contract
    if min_bp is not None:
        p["min_bp"] = min_bp
    return p


def _force(name, scores, widths, pol, children=None, cost=0.5, min_run=1, q=0.25, min_z=2.0, max_depth=8, own=False):
    n = int(scores.size)
    widths = [widths] * n if isinstance(widths, int) else list(widths)
    assert len(widths) == n, (name, len(widths), n)
    return dict(name=name, scores=scores, widths=widths, policy=pol, children=children or [(0, n - 1)], cost=cost, min_run=min_run, q=q,
                min_z=min_z, max_depth=max_depth, own=own)


TWO = [(30, 5.0, 0.3), (20, 0.0, 0.3), (30, 5.0, 0.3)]
THREE = [(30, 5.0, 0.3), (16, 0.0, 0.2), (30, 6.0, 0.3), (10, 2.0, 0.2), (30, 5.0, 0.3)]
COMB = [c for k in range(9) for c in ((12, 6.0, 0.2), (8, 0.4 * k, 0.1))] + [(12, 6.0, 0.2)]
CORE = [(30, 1.0, 0.1), (8, 10.0, 0.5), (30, 1.0, 0.1)]
TWIN_PEAKS = [(20, 1.0, 0.0), (1, 9.0, 0.0), (18, 1.0, 0.0), (1, 9.0, 0.0), (20, 1.0, 0.0)]
ADJACENT_PEAKS = [(20, 1.0, 0.0), (2, 9.0, 0.0), (20, 1.0, 0.0)]
BROAD = [(6, 0.0, 0.1), (50, 5.0, 0.4), (6, 0.0, 0.1)]
MOSTLY_ZERO = [(40, 0.0, 0.0), (26, 3.0, 1.0)]


def _tile(name, n):
    a = n // 3
    return _force(name, profile(name, [(a, 4.0, 0.5), (n - 2 * a, 0.0, 0.5), (a, 4.0, 0.5)]), 25, policy(2000, 1500), cost=1.0)


def force_cases():
    out = [
        _force("two_plateaus", profile("two_plateaus", TWO), 100, policy(2000, 1500)),
        _force("three_plateaus", profile("three_plateaus", THREE), 100, policy(2000, 1500)),
        _force("three_depth0", profile("three_plateaus", THREE), 100, policy(2000, 1500), max_depth=0),
        _force("three_depth1", profile("three_plateaus", THREE), 100, policy(2000, 1500), max_depth=1),
        _force("three_depth2", profile("three_plateaus", THREE), 100, policy(2000, 1500), max_depth=2),
        _force("three_negative_depth", profile("three_plateaus", THREE), 100, policy(2000, 1500), max_depth=-3),
        _force("comb", profile("comb", COMB), 100, policy(2000, 1500), cost=0.1),
        _force("child_contract", profile("child_contract", TWO), 100, policy(3500, 1000)),
        _force("flat", np.full(60, 2.5), 50, policy(1000, 800), cost=0.0),
        _force("flat_zero_cost_one", np.zeros(48), 25, policy(700, 600), cost=1.0),
        _force("short", profile("short", [(29, 1.0, 0.5)]), 25, policy(700, 500)),
        _force("core", profile("core", CORE), 100, policy(2000, 1500), cost=50.0),
        _force("twin_peaks", profile("twin_peaks", TWIN_PEAKS), 50, policy(1500, 1000), cost=50.0),
        _force("adjacent_peaks", profile("adjacent_peaks", ADJACENT_PEAKS), 50, policy(1500, 1000), cost=50.0),
        _force("broad", profile("broad", BROAD), 100, policy(2000, 1500), cost=50.0),
        _force("broad_grid", profile("broad_grid", BROAD, grid=0.5), 100, policy(2000, 1500), cost=50.0),
        _force("dome", np.concatenate((np.zeros(6), 5.0 - ((np.arange(50) - 25.0) / 25.0) ** 2, np.zeros(6))), 100, policy(2000, 1500), cost=50.0),
        _force("mostly_zero", profile("mostly_zero", MOSTLY_ZERO), 50, policy(1500, 1000), cost=0.2),
        _force("refused_bins", profile("refused_bins", BROAD), 100, policy(2000, 1500), cost=50.0, min_run=16),
        _force("uneven", profile("uneven", TWO), [25, 75, 50, 100] * 20, policy(2000, 1500)),
        _force("uneven_zero_width", profile("uneven_zero", TWO), ([0, 100, 50] * 27)[:80], policy(1500, 1000)),
        _force("min_bp_used", profile("two_plateaus", TWO), 100, policy(2000, None, 1200)),
        _force("neither_given", profile("two_plateaus", TWO), 100, policy(2000)),
        _force("contract_above_threshold", profile("two_plateaus", TWO), 100, policy(2000, 5000)),
        _force("contract_not_positive", profile("two_plateaus", TWO), 100, policy(9000, -1.0)),
        _force("quantile_high", profile("quantile_high", TWO), 100, policy(2000, 1500), q=0.4),
        _force("quantile_clipped", profile("quantile_clipped", TWO), 100, policy(2000, 1500), q=1.5),
        _force("min_run_wins", profile("min_run_wins", TWO), 100, policy(2000, 1500), min_run=7),
        _force("ends", profile("ends", [(40, 4.0, 0.4), (10, 0.0, 0.2), (30, 1.0, 0.2), (40, 4.0, 0.4)]), 50, policy(1500, 1000),
               children=[(0, 39), (50, 64), (80, 119)], own=True),
        _force("no_candidate", profile("no_candidate", [(30, 2.0, 0.5)]), 50, policy(2000, 1500), children=[(0, 9), (12, 29)]),
        _force("nan_threshold", profile("no_candidate", [(30, 2.0, 0.5)]), 50, policy(float("nan"), 1500)),
        _force("zero_threshold", profile("zero_threshold", [(40, 2.0, 0.5)]), 50, policy(0.0, 1500)),
        _tile("tile_minus_1", SORT_TILE - 1), _tile("tile", SORT_TILE), _tile("tile_plus_1", SORT_TILE + 1),
        _tile("beyond_tile", 3 * SORT_TILE + 300),      # (the nodes below the first split are longer than the tile as well)
    ]
    # z just below and at the minimum: the minimum is the split's own z (accepted: z < z is false) and the next double above it
    for name, bump in (("z_at_minimum", False), ("z_just_below", True)):
        out.append(dict(_force(name, profile("two_plateaus", TWO), 100, policy(2000, 1500)), z_from_split=True, z_bump=bump))
    return out


def force_inputs(case):
    """One kwargs dict of `_forceMassiveSubpeakSegments` per child of the case."""
    iv, en = coords(case["widths"])
    x = signal(case["name"], case["scores"].size)
    min_z = case["min_z"]
    if case.get("z_from_split"):
        import twin_cleanup as T

        n = int(case["scores"].size)
        z = T.best_split(case["scores"], case["cost"], max(case["min_run"], math.ceil(250 / case["widths"][0]), math.ceil(0.05 * n)), case["q"])["z"]
        min_z = math.nextafter(z, math.inf) if case["z_bump"] else z
    calls = []
    for a, b in case["children"]:
        child = {"start_idx": a, "end_idx": b, "subpeak_objective": 1.25 + a, "subpeak_boundary_penalty": 0.5}
        if case["own"]:
            child["split_from_parent"] = True
        calls.append(dict(child=child, scores=case["scores"], state=x, intervals=iv, ends=en, widthPolicy=case["policy"],
                          boundaryCost=case["cost"], minRunBins=case["min_run"], splitQuantile=case["q"], minSplitZ=min_z,
                          maxDepth=case["max_depth"]))
    return calls


def split_cases():
    flat = np.full(40, 1.5)
    return [
        dict(name="split_two", scores=profile("two_plateaus", TWO), boundaryCost=0.5, minRunBins=4),
        dict(name="split_short", scores=profile("two_plateaus", TWO)[:11], boundaryCost=0.5, minRunBins=4),
        dict(name="split_exact_3m", scores=profile("two_plateaus", TWO)[20:32], boundaryCost=0.0, minRunBins=4),
        dict(name="split_flat", scores=flat, boundaryCost=0.0, minRunBins=3),
        dict(name="split_negative_cost", scores=profile("three_plateaus", THREE), boundaryCost=-2.0, minRunBins=0, splitQuantile=0.1),
        dict(name="split_mostly_zero", scores=profile("mostly_zero", MOSTLY_ZERO), boundaryCost=0.2, minRunBins=5),
        dict(name="split_q0", scores=profile("three_plateaus", THREE), boundaryCost=0.2, minRunBins=5, splitQuantile=0.0),
        dict(name="split_q1", scores=profile("three_plateaus", THREE), boundaryCost=0.2, minRunBins=5, splitQuantile=1.0),
    ] + [dict(name=f"split_len_{n}", scores=profile("comb", COMB)[:n], boundaryCost=0.1, minRunBins=3, splitQuantile=q)
         for n, q in ((33, 0.25), (34, 0.25), (35, 0.25), (36, 0.25), (37, 0.3), (38, 0.7))]


def contract_cases():
    def c(name, scores, widths, thr, min_run, a=None, b=None, q=0.25):
        n = int(scores.size)
        iv, en = coords([widths] * n if isinstance(widths, int) else widths)
        return dict(name=name, startIdx=0 if a is None else a, endIdx=n - 1 if b is None else b, scores=scores, intervals=iv, ends=en,
                    thresholdBP=thr, minRunBins=min_run, splitQuantile=q)
    core, broad = profile("core", CORE), profile("broad", BROAD)
    return [
        c("contract_core", core, 100, 1500, 3),
        c("contract_core_inner", core, 100, 1500, 3, 10, 60),
        c("contract_broad", broad, 100, 1500, 3),
        c("contract_wider_than_all", broad, 100, 1.0e6, 3),
        c("contract_too_few_bins", broad, 100, 1500, 40),
        c("contract_flat", np.full(31, 2.0), 50, 600, 2),
        c("contract_flat_even", np.full(30, 2.0), 50, 600, 2),
        c("contract_twin_peaks", profile("twin_peaks", TWIN_PEAKS), 50, 1000, 3),
        c("contract_bad_range", core, 100, 1500, 3, 5, 200),
        c("contract_bad_threshold", core, 100, float("inf"), 3),
        c("contract_zero_threshold", core, 100, 0.0, 3),
        c("contract_one_bin", core, 100, 1500, 1, 33, 33),
        c("contract_uneven", core, [25, 75, 50, 100] * 17, 1500, 3),
    ]


def _bulk(center, scale, n):
    """n widths whose logs sit on an even grid of normal quantiles around `center` (deterministic, no random stream)"""
    u = (np.arange(n) + 0.5) / n
    # a rational approximation of the normal quantile is enough here: the reference decides from the widths it is given
    t = np.sqrt(-2.0 * np.log(np.minimum(u, 1.0 - u)))
    zq = t - (2.515517 + 0.802853 * t + 0.010328 * t * t) / (1.0 + 1.432788 * t + 0.189269 * t * t + 0.001308 * t ** 3)
    zq = np.where(u < 0.5, -zq, zq)
    return np.round(np.exp(center + scale * zq))


def policy_cases():
    narrow, wide = _bulk(math.log(1000.0), 0.3, 30), _bulk(8.0, 0.5, 30)
    return [
        dict(name="few_widths", widthsBP=narrow[:24]),
        dict(name="disabled", widthsBP=np.concatenate((narrow, [20000.0])), enabled=False),
        dict(name="no_tail", widthsBP=_bulk(math.log(1000.0), 0.3, 40)),
        dict(name="cluster_too_large", widthsBP=np.concatenate((narrow, [20000.0, 20000.0]))),
        dict(name="log_gap_too_small", widthsBP=np.concatenate((narrow, [7000.0, 7600.0]))),
        # (the cluster of two opens with a wide enough gap, but its narrower member is not significant at this alpha; the gap below the
        # widest one is too small)
        dict(name="cluster_q_above_alpha", widthsBP=np.concatenate((_bulk(8.0, 0.3, 398), [8200.0, 8900.0])), alpha=0.02),
        dict(name="active_gap", widthsBP=np.concatenate((wide[:29], [10500.0]))),
        dict(name="active_cap", widthsBP=np.concatenate((wide[:29], [40000.0]))),
        dict(name="active_min_bp", widthsBP=np.concatenate((narrow, [9000.0]))),
        dict(name="active_own_min_bp", widthsBP=np.concatenate((narrow, [3500.0])), minBP=2500),
        dict(name="mad_zero", widthsBP=np.concatenate(([1000.0] * 24, [2000.0] * 14, [30000.0]))),
        dict(name="mad_and_iqr_zero", widthsBP=np.concatenate(([1000.0] * 38, [30000.0]))),
        dict(name="small_bulk", widthsBP=np.asarray([500.0, 700.0, 900.0, 9000.0]), minPeaks=3, maxFraction=0.5),
        dict(name="invalid_widths", widthsBP=np.concatenate((narrow, [np.nan, -5.0, 0.0, np.inf, 9000.0]))),
        dict(name="empty", widthsBP=np.asarray([], np.float64)),
        dict(name="alpha_out_of_range", widthsBP=np.concatenate((narrow, [9000.0])), alpha=1.5, minLogGap=0.0),
    ]


FORCE, SPLITS, CONTRACTS, POLICIES = force_cases(), split_cases(), contract_cases(), policy_cases()
# the one case that holds a non-finite score inside a candidate: the reference raises, the device call refuses before any launch
NONFINITE = "nonfinite_candidate"


def nonfinite_inputs():
    s = profile("broad", BROAD).copy()
    s[20] = np.nan
    return force_inputs(_force(NONFINITE, s, 100, policy(2000, 1500)))[0]


# ---------------------------------------------------------------------------------------------------------------
# `_solutionToChromNarrowPeakRows` under a width policy
# ---------------------------------------------------------------------------------------------------------------
FULL_POLICY = {"active": True, "width_threshold_bp": 2000, "contract_width_bp": 1500, "min_bp": 1500, "null_center": 6.5, "null_scale": 0.4}


def _row_track(name, gap_at=()):
    """a chain of 100 bp bins: selected runs (two plateaus, a short hump, a broad plateau, a core, one that ends in the last bin)
    between unselected stretches; `gap_at`: coordinate gaps after these bins"""
    rng = _rng(name)
    runs = [profile(name + "/a", TWO), profile(name + "/b", [(12, 3.0, 0.3)]), profile(name + "/c", BROAD), profile(name + "/d", CORE),
            profile(name + "/e", THREE)]
    parts, mask = [], []
    for k, r in enumerate(runs):
        if k:
            parts.append(-1.0 + 0.1 * rng.standard_normal(6))
            mask.append(np.zeros(6, np.uint8))
        parts.append(r)
        mask.append(np.ones(r.size, np.uint8))
    s = np.concatenate(parts)
    n = int(s.size)
    widths = np.full(n, 100, np.int64)
    edges = 5000 + np.concatenate(([0], np.cumsum(widths)))
    iv, en = edges[:-1].copy(), edges[1:].copy()
    for g in gap_at:
        iv[g + 1:] += 300
        en[g + 1:] += 300
    x = np.round((s + rng.standard_normal(n)) * 4.0) / 4.0
    u = np.abs(rng.standard_normal(n)) + 0.2
    u[::17] = np.nan
    return dict(intervals=iv, ends=en, state=x, scores=s, solution=np.concatenate(mask), uncertainty=u)


def row_cases():
    base = dict(chromosome="chrT", prefix="twin", nullScale=0.5, trimScoreFloor=0.0, subpeakSelectionPenalty=0.3, subpeakBoundaryCost=0.25,
                minSubpeakBins=3, returnExportDetails=True, massiveSubpeakCleanup=True)
    inactive = dict(FULL_POLICY, active=False)
    return [
        dict(name="rows_active", track=("rows", ()), **base, massiveSubpeakWidthPolicy=dict(FULL_POLICY)),
        dict(name="rows_gap_in_front", track=("rows", (24, 140)), **base, massiveSubpeakWidthPolicy=dict(FULL_POLICY)),
        dict(name="rows_no_split", track=("rows", ()), **{**base, "splitSubpeaks": False}, massiveSubpeakWidthPolicy=dict(FULL_POLICY)),
        dict(name="rows_no_filter", track=("rows", ()), **base, massiveSubpeakWidthPolicy=dict(FULL_POLICY), dropMedianSignalBelowNegativeLocalP=False),
        dict(name="rows_inactive_policy", track=("rows", ()), **base, massiveSubpeakWidthPolicy=inactive),
        dict(name="rows_cleanup_off", track=("rows", ()), **{**base, "massiveSubpeakCleanup": False}, massiveSubpeakWidthPolicy=dict(FULL_POLICY)),
        dict(name="rows_no_null", track=("rows", ()), **base, massiveSubpeakWidthPolicy={"active": True, "width_threshold_bp": 2500}),
        dict(name="rows_no_threshold", track=("rows", ()), **base, massiveSubpeakWidthPolicy={"active": True, "width_threshold_bp": None,
                                                                                                "null_center": 6.5, "null_scale": 0.4}),
        dict(name="rows_no_candidate", track=("rows", ()), **base, massiveSubpeakWidthPolicy=dict(FULL_POLICY, width_threshold_bp=50000)),
        dict(name="rows_own_quantile", track=("rows2", ()), **{**base, "trimScoreFloor": None}, massiveSubpeakWidthPolicy=dict(FULL_POLICY),
             massiveSubpeakSplitQuantile=0.4, massiveSubpeakSplitZ=0.5),
        dict(name="rows_empty_mask", track=("rows", ()), empty=True, **base, massiveSubpeakWidthPolicy=dict(FULL_POLICY)),
    ]


def row_inputs(case):
    kw = {k: v for k, v in case.items() if k not in ("name", "track", "empty")}
    kw.update(_row_track(*case["track"]))
    if case.get("empty"):
        kw["solution"] = np.zeros_like(kw["solution"])
    return kw


ROWS = row_cases()
