"""Case table of the broad-mode tests: the smallest shapes at which the lanes and wavefronts of csrc/csr_broad.h and the host half
of consenrich_amd/broad.py can go wrong.  A MERGE case is a set of keyword arguments of `_mergeBroadRunsByObjective`, a ROWS case
one of `_solutionToChromBroadPeakRows`; both are synthesised here from seeds.  The fixtures under tests/golden/broad hold the
reference's OUTPUTS only (tests/golden/make_broad_golden.py), in the canonical form of `canon`: every value with its Python type,
floats by bit pattern, dicts with their keys in order."""
import json
import struct

import numpy as np

from narrowpeak_cases import coords, layout, runs_mask, wave

GAP_LENGTHS = (1, 7, 8, 9, 127, 128, 129, 8192, 8193)      # the leaf, the eight accumulators, the first split, the chunk fold
PARENT_LENGTHS = (1, 2, 3, 4, 63, 64, 65, 128, 129, 2047, 2048, 2049, 8192, 8193)


# ---------------------------------------------------------------------------------------------------------------
# the canonical form of a result
# ---------------------------------------------------------------------------------------------------------------
def canon(v):
    """A JSON-able form that keeps what the tests compare: the exact type of every value, floats bit for bit, the order of keys"""
    t = type(v).__name__
    if v is None or isinstance(v, (bool, str)):
        return [t, v]
    if type(v) is int:
        return [t, str(v)]
    if type(v) is float:
        return [t, struct.pack("<d", v).hex()]
    if isinstance(v, (list, tuple)):
        return [t, [canon(x) for x in v]]
    if isinstance(v, dict):
        return [t, [[canon(k), canon(x)] for k, x in v.items()]]
    return [t, repr(v)]     # (a NumPy scalar or array where a Python value belongs: never equal to a fixture)


def pack(v):
    return np.frombuffer(json.dumps(canon(v)).encode(), np.uint8)


def unpack(a):
    return json.loads(bytes(np.asarray(a, np.uint8)).decode())


def differences(got, want, path="", out=None, limit=8):
    """Where two canonical forms differ (paths, at most `limit`)"""
    out = [] if out is None else out
    if len(out) >= limit:
        return out
    if got[0] != want[0]:
        out.append(f"{path}: type {got[0]} != {want[0]}")
    elif isinstance(got[1], list) and isinstance(want[1], list):
        if len(got[1]) != len(want[1]):
            out.append(f"{path}: length {len(got[1])} != {len(want[1])}")
        for k, (g, w) in enumerate(zip(got[1], want[1])):
            if got[0] == "dict":
                if g[0] != w[0]:
                    out.append(f"{path}: key {g[0][1]} != {w[0][1]}")
                differences(g[1], w[1], f"{path}.{g[0][1]}", out, limit)
            else:
                differences(g, w, f"{path}[{k}]", out, limit)
    elif got[1] != want[1]:
        out.append(f"{path}: {got[1]} != {want[1]}")
    return out


# ---------------------------------------------------------------------------------------------------------------
# bridging
# ---------------------------------------------------------------------------------------------------------------
def merge_base(name, n, runs, scores, step=25, gaps=(), **kw):
    iv, en = coords(n, step, gaps)
    out = dict(runs=[(int(a), int(b)) for a, b in runs], scores=np.asarray(scores, np.float64), intervals=iv, ends=en, chromosome="chrT",
               selectionPenalty=0.5, boundaryCost=0.75, maxGapBP=10 ** 9, blacklistByChrom={}, runPenalty=0.0, dipPenaltyFraction=0.5)
    out.update(kw)
    return dict(name=name, kw=out)


def _gap_runs(lengths, run=3, lead=0):
    runs, pos = [], lead
    for k in list(lengths) + [0]:
        runs.append((pos, pos + run - 1))
        pos += run + k
    return pos, runs


def _merge_gap_lengths(name, fraction, seed, **kw):
    # runs of 3 bins with every gap length of GAP_LENGTHS between them, the first run at bin 0 and the last at bin n - 1; two more
    # runs follow a coordinate break with NO bin between them (a gap of 0 bins and 75 bp).  The scores wave about the penalty; every
    # second gap lies far below it and does not merge.  (The merged runs show a gap's DECISION; the sums themselves are compared
    # with NumPy's bit for bit in the tests)
    n, runs = _gap_runs(GAP_LENGTHS)
    brk = n - 1
    runs = runs + [(n, n + 2)]
    n += 3
    rng = np.random.default_rng(seed)
    s = 0.5 + 0.02 * rng.standard_normal(n) + 0.4 * np.sin(np.arange(n) * 0.37)
    for k in range(1, len(GAP_LENGTHS), 2):
        s[runs[k][1] + 1:runs[k + 1][0]] -= 4.5
    return merge_base(name, n, runs, s, gaps=(brk,), dipPenaltyFraction=fraction, **kw)


def _merge_gain_zero():
    # dyadic values: two gap bins of penalty - 1 with f = 0.5 sum to -1, and 2 * 0.5 brings the gain to exactly 0: no merge (strict
    # >); the next gap's bins of penalty - 0.5 leave a gain of 0.5: merged; the third is exactly 0 only with the run penalty
    n, runs = layout([4, 4, 4, 4], gap=2, lead=1, tail=1)
    s = np.full(n, 2.0)
    s[5:7], s[11:13], s[17:19] = 0.5 - 1.0, 0.5 - 0.5, 0.5 - 1.0
    return merge_base("gain_zero", n, runs, s, boundaryCost=0.5)


def _merge_run_penalty():
    c = _merge_gain_zero()
    c["name"] = "run_penalty"
    c["kw"]["runPenalty"] = 0.25
    return c


def _merge_distance_blacklist():
    # 25 bp bins.  gaps (bins): 4 = 100 bp == maxGapBP (allowed), 5 = 125 bp (distance), 6 = 150 bp and blacklisted (both fail:
    # counts as distance), 2 with a blacklist interval inside (blacklist), 3 with blacklist intervals that only touch its two ends
    # (allowed), 1 clear
    lengths = [4, 5, 6, 2, 3, 1]
    n, runs = _gap_runs(lengths, run=4, lead=2)
    n += 2
    gap_bp = [(25 * (runs[k][1] + 1), 25 * runs[k + 1][0]) for k in range(len(lengths))]
    bl = np.asarray([[gap_bp[2][0] + 10, gap_bp[2][0] + 20], [gap_bp[3][0] + 5, gap_bp[3][0] + 6], [gap_bp[4][0] - 30, gap_bp[4][0]],
                     [gap_bp[4][1], gap_bp[4][1] + 30]], np.int64)
    s = np.full(n, 0.75)        # every open gap gains
    return merge_base("distance_blacklist", n, runs, s, maxGapBP=100, blacklistByChrom={"chrT": bl, "chrU": bl[:1] * 0})


def _merge_misc():
    # scores not finite inside a gap (a NaN gain does not merge; +inf does), a negative selection penalty and boundary cost (floored
    # at 0), a maxGapBP below 0 (0: only the touching runs across no coordinates merge), runs given as lists
    n, runs = layout([2, 2, 2, 2], gap=3, lead=0, tail=0)
    s = np.full(n, -0.25)
    s[3], s[8] = np.nan, np.inf
    return merge_base("nonfinite_gap", n, [list(r) for r in runs], s, selectionPenalty=-1.0, boundaryCost=-2.0)


def merge_cases():
    return [
        _merge_gap_lengths("gap_lengths_soft", 0.5, 11),
        _merge_gap_lengths("gap_lengths_hard", 1.0, 12),
        _merge_gap_lengths("gap_lengths_above_one", 1.75, 13, boundaryCost=0.01),
        _merge_gap_lengths("gap_lengths_below_zero", -0.5, 14, boundaryCost=0.0, selectionPenalty=0.55),
        _merge_gain_zero(),
        _merge_run_penalty(),
        _merge_distance_blacklist(),
        _merge_misc(),
        merge_base("max_gap_zero", 12, [(0, 2), (3, 5), (8, 11)], np.ones(12), maxGapBP=-5),
        merge_base("one_run", 9, [(2, 5)], np.ones(9)),
        merge_base("empty_soft", 9, [], np.ones(9), runPenalty=-1.0, maxGapBP=-3),
        merge_base("empty_hard", 9, [], np.ones(9), dipPenaltyFraction=3.0, runPenalty=0.5),
    ]


# ---------------------------------------------------------------------------------------------------------------
# rows
# ---------------------------------------------------------------------------------------------------------------
def rows_base(name, n, parents, children, scores, state, step=25, gaps=(), **kw):
    iv, en = coords(n, step, gaps)
    out = dict(chromosome="chrT", intervals=iv, ends=en, state=np.asarray(state, np.float64), scores=np.asarray(scores, np.float64),
               parentSolution=runs_mask(n, parents), childSolution=runs_mask(n, children), prefix="bp", returnExportDetails=True)
    out.update(kw)
    return dict(name=name, kw=out)


def _rows_lengths(name, lengths, seed, **kw):
    # parents of the given lengths, the first at bin 0 and the last at bin n - 1; a child in the middle third of every parent of 3
    # bins or more
    n, parents = layout(list(lengths), gap=2)
    children = [(a + (b - a + 1) // 3, b - (b - a + 1) // 3) for a, b in parents if b - a >= 2]
    x = wave(n, seed, 0.013, 0.4, 0.5)
    s = np.abs(wave(n, seed + 1, 0.021, 0.2, 0.3))
    u = 0.3 + 0.2 * np.abs(wave(n, seed + 2, 0.05))
    return rows_base(name, n, parents, children, s, x, **{"uncertainty": u, **kw})


def _rows_filters():
    # 100 bp bins, parents of 12 bins unless noted.  In order: median == threshold (kept: the comparison is strict); median below it
    # (dropped by the median filter); 6 bins = 600 bp (passes the median filter, dropped by width); uncertainty partly non-finite;
    # uncertainty with no finite value (no filter, local_median_p None); an arg-max tie; an even median of two different values
    n, parents = layout([12, 12, 6, 12, 12, 12, 12], gap=3, lead=2, tail=2)
    x = wave(n, 21, 0.9, 1.0, 0.3)
    u = np.full(n, 0.5)
    (a0, b0), (a1, b1), _, (a3, b3), (a4, b4), (a5, b5), (a6, b6) = parents
    x[a0:b0 + 1] = -1.0
    x[a1:b1 + 1] = -1.0
    x[a1 + 2] = -1.5
    x[a1 + 7] = -1.25
    x[a1 + 3:a1 + 7] = -1.0625       # (the median of 12 lies between the sixth and seventh values)
    u[a3:b3 + 1:2] = np.nan
    u[a3 + 1] = np.inf
    u[a3 + 3] = -np.inf
    u[a4:b4 + 1] = np.nan
    x[a5 + 4] = x[a5 + 9] = 7.5
    x[a6:b6 + 1] = [0.25, 4.0, 1.0, 3.0, 2.0, 2.5, 0.5, 3.5, 1.5, 0.75, 5.0, 0.125]
    s = np.abs(wave(n, 22, 0.7)) + 0.1
    children = [(a0 + 3, a0 + 5), (a3, a3 + 2), (a6 + 9, b6)]
    return rows_base("filters", n, parents, children, s, x, step=100, uncertainty=u)


def _rows_blocks():
    # 250 bp bins; a coordinate break inside the first parent's run (cut there) and inside a child.  Children: overhanging the
    # parent's left and right edge, none, one in the middle (both 1 bp sentinels), one at the start only, two adjacent runs of the child
    # mask that a coordinate break separates, a child that is the whole parent
    n = 96
    parents = [(4, 19), (24, 31), (36, 47), (52, 63), (68, 79), (84, 91)]
    children = [(2, 6), (17, 21), (40, 42), (52, 54), (70, 77), (84, 91)]
    gaps = (11, 73)
    x = wave(n, 31, 0.5, 1.5, 0.2)
    s = np.abs(wave(n, 32, 0.3)) + 0.2
    return rows_base("blocks", n, parents, children, s, x, step=250, gaps=gaps)


def _rows_scores(name, values):
    # constant scores per parent: the mean is the value itself.  250 bp bins, 8 bins per parent
    n, parents = layout([8] * len(values), gap=2, lead=1, tail=1)
    s = np.zeros(n)
    for (a, b), v in zip(parents, values):
        s[a:b + 1] = v
    return rows_base(name, n, parents, [], s, wave(n, 41, 0.6, 1.0), step=250)


def _rows_nan():
    # a NaN in the signal inside the second of three parents: the chain is decided on the host
    n, parents = layout([70, 90, 66], gap=4, lead=3, tail=3)
    x = wave(n, 51, 0.2, 0.8)
    x[parents[1][0] + 17] = np.nan
    return rows_base("nan_signal", n, parents, [(parents[0][0] + 5, parents[0][0] + 9)], np.abs(wave(n, 52, 0.4)), x,
                     uncertainty=np.full(n, 0.2))


def rows_cases():
    small = [k for k in PARENT_LENGTHS if k <= 2049]
    return [
        _rows_lengths("lengths", small, 1, minPeakBP=1),
        _rows_lengths("lengths_chunk", [8192, 8193, 129], 4, minPeakBP=0, returnExportDetails=False),
        _rows_lengths("lengths_no_uncertainty", [1, 40, 41, 65, 200], 7, uncertainty=None),
        _rows_filters(),
        _rows_blocks(),
        _rows_scores("one_score", [0.375] * 4),
        _rows_scores("half_way", [0.0, 0.75, 1.0, 0.25]),
        _rows_nan(),
        rows_base("empty_masks", 40, [], [], np.ones(40), np.ones(40)),
        rows_base("empty_masks_pair", 40, [], [(3, 9)], np.ones(40), np.ones(40), returnExportDetails=False, uncertainty=np.ones(40)),
        rows_base("all_dropped", 40, [(2, 9)], [], np.ones(40), np.ones(40)),       # 200 bp < 1000 bp
    ]


# ---------------------------------------------------------------------------------------------------------------
# envelope and support runs (peaks.py:6884-6932): a PARENTS case is a set of keyword arguments of twin_broad.parents
# ---------------------------------------------------------------------------------------------------------------
SUPPORT_THRESHOLD = 0.5


def support_chain(name, n, seed, domains, strong, weak, breaks=(), **kw):
    """noise about -0.5 with planted domains (first bin, last bin, height); the masks as lists of runs"""
    rng = np.random.default_rng(seed)
    s = -0.5 + 0.3 * rng.standard_normal(n)
    for a, b, h in domains:
        s[a:b + 1] = h + 0.2 * rng.standard_normal(b - a + 1)
    s = np.where(np.abs(s - SUPPORT_THRESHOLD) < 0.02, SUPPORT_THRESHOLD + 0.05, s)     # (no score within rounding of the threshold)
    iv, en = coords(n, 25, breaks)
    out = dict(scores=s, strong=runs_mask(n, strong), weak=runs_mask(n, weak), threshold=SUPPORT_THRESHOLD, intervals=iv, ends=en,
               chromosome=name, selection_penalty=0.2, boundary_cost=1.0, max_gap_bp=2000, blacklist=None, dip_penalty_fraction=0.5,
               run_penalty=0.0)
    out.update(kw)
    return dict(name=name, kw=out)


def parents_cases():
    """The first six are the chains of the resident batch test, in its order"""
    return [
        # plain: domains that touch the strong mask, the weak mask, both and neither; a blacklisted gap; gaps beyond the bound
        support_chain("chr1", 3001, 1, [(40, 130, 1.4), (134, 260, 1.1), (300, 380, 0.9), (600, 700, 1.2), (712, 790, 1.3), (2950, 3000, 1.5)],
                      [(60, 80), (620, 640), (2960, 2990)], [(50, 100), (200, 210), (720, 730)],
                      blacklist={"chr1": np.asarray([[25 * 705, 25 * 708]], np.int64)}),
        # masked out in the batch
        support_chain("chr2", 700, 2, [(100, 200, 1.2)], [(120, 130)], [(110, 150)]),
        # both masks empty: no run touches, and the envelope has none either
        support_chain("chr3", 520, 3, [(100, 160, 1.2), (300, 380, 1.0)], [], [], selection_penalty=0.3, boundary_cost=0.5),
        # coordinate breaks: one exactly on a 1024-bin block edge inside a support run (one piece touches, one does not), one
        # inside a support run whose two pieces both touch (a gap of 0 bins and 75 bp)
        support_chain("chr4", 2600, 4, [(1000, 1100, 1.3), (1480, 1530, 1.2), (2000, 2100, 1.1)], [(1050, 1060), (1490, 1495)],
                      [(1510, 1512), (2050, 2051)], breaks=(1023, 1500), selection_penalty=0.25, boundary_cost=1.5, max_gap_bp=5000),
        # the envelope fallback: the masks lie where no score reaches the threshold
        support_chain("chr5", 1500, 5, [], [(100, 120)], [(115, 140), (400, 410)], boundary_cost=2.0, max_gap_bp=10 ** 7),
        # long: a run from bin 0, one to bin n - 1, one across a block edge, a gap of more than 8192 bins over a run that does not touch
        support_chain("chr6", 21000, 6, [(0, 60, 1.5), (3000, 3050, 1.0), (9000, 9100, 1.2), (9104, 9300, 1.3), (10200, 10300, 1.1),
                                         (20900, 20999, 1.4)],
                      [(10, 20), (9200, 9210), (20950, 20960)], [(9050, 9060), (10230, 10250)], max_gap_bp=10 ** 7),
        # many breaks (the bisection): one inside every 7 bins of a touching domain, the first and the last of the list on a run's edge
        support_chain("chr7", 400, 7, [(100, 169, 1.3), (200, 230, 1.2)], [(120, 125)], [(150, 160), (210, 212)],
                      breaks=tuple(range(99, 171, 7)), max_gap_bp=100),
        # the fallback with a break inside an envelope run, and gaps that bridge under a run penalty
        support_chain("chr8", 300, 8, [], [(40, 60), (64, 70)], [(55, 66), (200, 205)], breaks=(50,), boundary_cost=0.0, run_penalty=3.0,
                      max_gap_bp=300, dip_penalty_fraction=1.0),
    ]


HOST_DECIDED = ("nan_signal",)
NEEDED_PARENTS = ("break_on_block_edge", "piece_not_touching", "piece_touching", "support_not_touching", "envelope_fallback",
                  "empty_envelope", "run_from_bin_0", "run_to_last_bin", "run_across_block_edge", "kept_gap_over_chunk",
                  "kept_gap_without_bin", "gap_beyond_bound", "break_bisected", "fallback_run_cut_at_break")
# what the case table must still do (BRANCHES of the twin's device form, summed over the cases)
NEEDED = tuple(f"gap_len_{k}" for k in GAP_LENGTHS) + tuple(f"parent_len_{k}" for k in PARENT_LENGTHS) + (
    "gap_without_bin", "no_runs", "gain_zero", "gap_at_max", "distance", "both_fail", "argmax_tie", "uncertainty_some_nonfinite",
    "uncertainty_none_finite", "median_equal_threshold", "dropped_median", "dropped_width", "no_child", "sentinel_left", "sentinel_right",
    "decided_on_host", "span_floor", "half_way")


def case(table, name):
    return next(c for c in table if c["name"] == name)


def rows_errors():
    """A good call and the overrides that make the reference raise ValueError, with its text"""
    good = dict(rows_base("good", 40, [(2, 30)], [(5, 8)], np.ones(40), np.ones(40), step=100, uncertainty=np.ones(40))["kw"])
    msg = "`intervals`, `ends`, `state`, `scores`, and solutions must match length"
    return good, [
        (dict(scores=np.ones(39)), msg), (dict(parentSolution=np.ones(41, np.uint8)), msg), (dict(childSolution=np.ones(3, np.uint8)), msg),
        (dict(ends=np.arange(39)), msg), (dict(uncertainty=np.ones(39)), "`uncertainty` must match `state` length"),
        (dict(exportFilterUncertaintyMultiplier=-1.0), "`exportFilterUncertaintyMultiplier` must be finite and non-negative"),
        (dict(exportFilterUncertaintyMultiplier=float("nan")), "`exportFilterUncertaintyMultiplier` must be finite and non-negative"),
    ]


def merge_errors():
    good = dict(merge_base("good", 12, [(0, 2), (5, 7)], np.ones(12))["kw"])
    return good, [(dict(scores=np.ones(11)), "`scores`, `intervals`, and `ends` must match length"),
                  (dict(ends=np.arange(13)), "`scores`, `intervals`, and `ends` must match length")]
