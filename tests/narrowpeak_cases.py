"""Case table of the narrowPeak export tests: the smallest shapes at which the kernels of csrc/csr_export.h can go wrong.  Every
case is a set of keyword arguments of `_solutionToChromNarrowPeakRows`, synthesised here; the fixtures under
tests/golden/narrowpeak hold the reference's OUTPUTS only (tests/golden/make_narrowpeak_golden.py)."""
import numpy as np

TILE = 32           # bins per back-pointer word (NESTED_WORD)
WIDE_MIN_RUN = 9    # the smallest minimum run of the states-as-lanes kernel


def coords(n, step, gaps=()):
    """bins of `step` bp; after each bin of `gaps` the coordinates jump by 3 * step"""
    iv = np.arange(n, dtype=np.int64) * step
    for g in gaps:
        iv[g + 1:] += 3 * step
    return iv, iv + step


def runs_mask(n, runs):
    m = np.zeros(n, np.uint8)
    for a, b in runs:
        m[a:b + 1] = 1
    return m


def layout(lengths, gap=3, lead=0, tail=0):
    """runs of the given lengths, `gap` unselected bins between two, `lead` in front and `tail` behind: (n, runs)"""
    runs, pos = [], lead
    for k in lengths:
        runs.append((pos, pos + k - 1))
        pos += k + gap
    return pos - gap + tail, runs


def wave(n, seed, period=0.45, lift=0.3, noise=0.2):
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    return 2.0 * np.sin(i * period) + lift + noise * rng.standard_normal(n)


def base(name, n, runs, scores, state, step=25, gaps=(), **kw):
    iv, en = coords(n, step, gaps)
    out = dict(chromosome="chrT", intervals=iv, ends=en, state=np.asarray(state, np.float64), scores=np.asarray(scores, np.float64),
               solution=runs_mask(n, runs), prefix="np", nullScale=0.5, subpeakSelectionPenalty=0.3, subpeakBoundaryCost=0.25,
               minSubpeakBins=5, returnExportDetails=True)
    out.update(kw)
    return dict(name=name, kw=out)


def _lengths_min5():
    # parents of 1, 4, 5 and 6 bins at min run 5, the first touching bin 0 and the last bin n - 1; 100 bp bins: the one-bin child is
    # under 200 bp
    n, runs = layout([1, 4, 5, 6, 7])
    s = np.abs(wave(n, 1)) + 0.5
    x = wave(n, 2, 0.8)
    return base("lengths_min5", n, runs, s, x, step=100, uncertainty=0.1 + 0.05 * np.abs(wave(n, 3)))


def _word_edges(min_run, name):
    n, runs = layout([31, 32, 33, 64, 65], lead=2, tail=2)
    return base(name, n, runs, wave(n, 4), wave(n, 5, 0.31) + 1.0, step=50, minSubpeakBins=min_run, uncertainty=0.2 + 0.1 * np.abs(wave(n, 6)))


def _gaps():
    # a coordinate gap inside the first run (after bin 9: it is cut there) and one between two runs (after bin 22: no cut)
    n = 60
    runs = [(4, 19), (25, 40), (50, 59)]
    return base("gaps", n, runs, np.abs(wave(n, 7)) + 0.4, wave(n, 8, 0.6), gaps=(9, 22), uncertainty=np.full(n, 0.05))


def _splits():
    # three bumps in one parent (three children), one bump with poor tails (one child shorter than its parent), a parent kept whole
    bump, valley = [2.0, 2.5, 3.0, 2.5, 2.0, 1.5, 2.0, 2.2], [-3.0] * 6
    three = bump + valley + bump + valley + bump
    single = [-2.0] * 4 + bump + [-2.0] * 5
    whole = [1.5, 1.75, 2.0, 2.5, 2.25, 2.0, 1.5, 1.25, 1.5]
    n, runs = layout([len(three), len(single), len(whole)], lead=1, tail=1)
    s = np.full(n, -1.0)
    for (a, b), v in zip(runs, (three, single, whole)):
        s[a:b + 1] = v
    return base("splits", n, runs, s, s + 0.25 * wave(n, 9, 1.1), trimScoreFloor=None)


def _ties():
    # dyadic values: tied maxima of the scores and of the signal, bins whose adjusted score is exactly zero (equal values, the
    # smaller count wins), boundaries of cost 0.25
    pattern = np.asarray([1.0, 1.0, 2.0, 2.0, 1.0, 1.0, 0.5, 1.0, 1.0, 2.0, 1.0, 1.0, 0.75, 1.0, 2.0, 2.0, 1.0, 1.0, 1.25, 1.0])
    n, runs = layout([20, 20, 12], lead=1, tail=1)
    s = np.zeros(n)
    s[runs[0][0]:runs[0][1] + 1] = pattern
    s[runs[1][0]:runs[1][1] + 1] = pattern[::-1]
    s[runs[2][0]:runs[2][1] + 1] = pattern[:12]
    x = np.round(np.abs(wave(n, 10, 0.9)) * 2.0) / 2.0
    return base("ties", n, runs, s, x, subpeakSelectionPenalty=1.0, subpeakBoundaryCost=0.25, trimScoreFloor=None)


def _near_ties():
    # the same with scores a few 1e-13 off: differences inside the 1e-12 comparison
    c = _ties()
    s = c["kw"]["scores"].copy()
    s[2::3] += 3.0e-13
    s[1::5] -= 2.0e-13
    c["kw"]["scores"] = s
    c["name"] = "near_ties"
    return c


def _trims():
    # the DP keeps every parent whole (a negative penalty); the trim at floor 0 then cuts left only, right only, both, nothing, and
    # not at all where the summit's own score is not above the floor
    left = [-0.2, -0.1, 0.5, 1.0, 2.0, 1.0, 0.5, 0.25]
    right = left[::-1]
    both = [-0.2, 0.0, 0.5, 1.0, 2.0, 1.0, 0.0, -0.1]
    none = [0.5, 1.0, 2.0, 1.0, 0.5, 0.25, 0.5, 0.75]
    below = [0.5, 1.0, -0.1, 1.0, 0.5, 0.25, 0.5, 0.75]
    island = [0.5, 0.0, 0.5, 2.0, 0.5, -0.5, 3.0, 0.75]     # a better stretch beyond a bin at the floor stays outside
    parts = (left, right, both, none, below, island)
    n, runs = layout([8] * len(parts), lead=1, tail=1)
    s, x = np.full(n, -1.0), np.zeros(n)
    for (a, b), v in zip(runs, parts):
        s[a:b + 1] = v
        x[a:b + 1] = v
    x[runs[4][0] + 2] = 9.0         # `below`: the signal peaks where the score is negative
    x[runs[5][0] + 3] = 9.0
    return base("trims", n, runs, s, x, step=200, subpeakSelectionPenalty=-5.0, subpeakBoundaryCost=0.0)


def _medians():
    # children of 1, 2, 3 and 4 bins after the trim (200 bp bins: none is too narrow); uncertainty with some and with no finite
    # value in a child; a child dropped by the median test, one kept at equality
    widths = (1, 2, 3, 4, 3, 2, 4, 3)
    n, runs = layout([8] * len(widths), lead=1, tail=1)
    s, x, u = np.full(n, -1.0), np.zeros(n), np.full(n, 0.125)
    rng = np.random.default_rng(11)
    for k, ((a, b), w) in enumerate(zip(runs, widths)):
        s[a:b + 1] = -0.5
        s[a + 2:a + 2 + w] = 1.0 + np.arange(w) * 0.25
        x[a:b + 1] = np.round(rng.standard_normal(8) * 8.0) / 8.0
        x[a + 2] = 4.0
    a = runs[4][0]
    u[a + 2:a + 5] = [np.nan, 0.5, np.inf]                  # one finite value left
    a = runs[5][0]
    u[a + 2:a + 4] = [np.nan, -np.inf]                      # none finite: no filter for this child
    x[a:a + 8] = -9.0                                       # (the summit stays inside the window: everything else is lower)
    x[a + 2:a + 4] = [-7.0, -8.0]
    a = runs[6][0]
    x[a:a + 8] = -9.0
    x[a + 2:a + 6] = [-1.0, -3.0, -2.0, -4.0]               # median -2.5 < -2 * 0.125: dropped
    a = runs[7][0]
    x[a:a + 8] = -9.0
    x[a + 2:a + 5] = [-0.25, -0.5, -0.125]                  # median -0.25 = -2 * 0.125: kept
    return base("medians", n, runs, s, x, step=200, subpeakSelectionPenalty=-5.0, subpeakBoundaryCost=0.0, uncertainty=u)


def _no_uncertainty():
    c = _medians()
    c["kw"]["uncertainty"] = None
    c["name"] = "no_uncertainty"
    return c


def _filter_off():
    c = _medians()
    c["kw"]["dropMedianSignalBelowNegativeLocalP"] = False
    c["kw"]["exportFilterUncertaintyMultiplier"] = 0.5
    c["name"] = "filter_off"
    return c


def _one_score():
    # every kept peak has the same raw score: the span floor, every score 250
    n, runs = layout([9, 9, 9], lead=1, tail=1)
    s, x = np.full(n, -1.0), wave(n, 12)
    for a, b in runs:
        s[a:b + 1] = [0.5, 1.0, 1.5, 2.0, 3.0, 2.0, 1.5, 1.0, 0.5]
    return base("one_score", n, runs, s, x, subpeakSelectionPenalty=-5.0, subpeakBoundaryCost=0.0)


def _half_way():
    # raw scores 0, 4 and 3: 250 + 750 * 0.75 = 812.5 exactly, which rounds to the even 812; and 1, for 437.5 -> 438
    n, runs = layout([9, 9, 9, 9], lead=1, tail=1)
    s, x = np.full(n, -1.0), wave(n, 13)
    for (a, b), top in zip(runs, (0.0, 4.0, 3.0, 1.0)):
        s[a:b + 1] = top - np.abs(np.arange(9) - 4) * 0.25
    return base("half_way", n, runs, s, x, subpeakSelectionPenalty=-9.0, subpeakBoundaryCost=0.0, trimScoreFloor=None)


def _empty():
    n = 40
    return base("empty_mask", n, [], wave(n, 14), wave(n, 15))


def _empty_pair():
    c = _empty()
    c["kw"]["returnExportDetails"] = False
    c["name"] = "empty_mask_pair"
    return c


def _pair():
    c = _word_edges(5, "pair_form")
    c["kw"]["returnExportDetails"] = False
    return c


def _no_split():
    c = _word_edges(5, "no_split")
    c["kw"]["splitSubpeaks"] = False
    return c


def _null_scale():
    # no penalty and no cost given: both fall back on max(nullScale, 0)
    c = _word_edges(5, "null_scale")
    c["kw"].update(subpeakSelectionPenalty=None, subpeakBoundaryCost=None, nullScale=0.4, trimScoreFloor=float("inf"))
    return c


def _nan_signal():
    # a NaN of the signal inside a selected run: the chain the host decides
    c = _word_edges(5, "nan_signal")
    x = c["kw"]["state"].copy()
    x[36 + int(np.argmax(c["kw"]["scores"][36:68]))] = np.nan       # the second run's required bin: inside a child whatever the split
    c["kw"]["state"] = x
    return c


CASES = [_lengths_min5(), _word_edges(5, "word_edges"), _word_edges(WIDE_MIN_RUN, "min_run_wide"), _gaps(), _splits(), _ties(),
         _near_ties(), _trims(), _medians(), _no_uncertainty(), _filter_off(), _one_score(), _half_way(), _empty(), _empty_pair(),
         _pair(), _no_split(), _null_scale(), _nan_signal()]
HOST_DECIDED = ("nan_signal",)


def inputs(case):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in case["kw"].items()}


def case(name):
    return next(c for c in CASES if c["name"] == name)


def errors():
    """(good keyword arguments, [(override, the reference's message)])"""
    good = inputs(case("word_edges"))
    n = good["scores"].size
    return good, [
        (dict(scores=good["scores"][:-1]), "`intervals`, `ends`, `state`, `scores`, and `solution` must match length"),
        (dict(solution=good["solution"][1:]), "`intervals`, `ends`, `state`, `scores`, and `solution` must match length"),
        (dict(uncertainty=np.ones(n + 1)), "`uncertainty` must match `state` length"),
        (dict(exportFilterUncertaintyMultiplier=-1.0), "`exportFilterUncertaintyMultiplier` must be finite and non-negative"),
        (dict(scores=np.where(np.arange(n) == 10, np.inf, good["scores"])), "`scores` contains non-finite values"),
        (dict(subpeakSelectionPenalty=float("nan")), "`selectionPenalty` must be finite"),
        (dict(subpeakBoundaryCost=float("inf")), "`boundaryCosts` must be finite and non-negative"),
    ]
