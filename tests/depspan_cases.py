"""The case table of the dependence-span tests and the synthesis of their inputs.

Inputs come from NumPy's generator (uniform doubles: integer arithmetic and one multiplication) and +, -, x, cumulative sums and
casts only -- no exp / log, so the bytes do not depend on the C library of the box.  Every golden fixture stores the SHA-256 of
its input bytes and the tests assert it before anything else.

A chromosome is a row of windows; window w of a chromosome is a moving average of width q[w] of uniform noise (so its ACF falls
linearly and reaches zero at lag q[w]) on a level that differs from window to window (so the ranking scores differ).  `edits`
then plant the edges a case is about."""
import hashlib

import numpy as np


def moving_average(rng, n, q):
    e = rng.random(n + q) - 0.5
    c = np.cumsum(e)
    return c[q:] - c[:-q]


def build(case):
    """names, matrices (float32) of a case."""
    rng = np.random.default_rng(case["seed"])
    wb, rows = case["window_bins"], case["rows"]
    mats = []
    for ci, n in enumerate(case["lens"]):
        mat = np.zeros((rows, n), dtype=np.float64)
        nw = -(-n // wb)
        for w in range(nw):
            q = case.get("q", {}).get((ci, w), int(rng.integers(case["q_range"][0], case["q_range"][1])))
            level = 0.25 * float(rng.integers(0, 16)) + 0.015625 * w
            a, b = w * wb, min(n, (w + 1) * wb)
            for r in range(rows):
                mat[r, a:b] = level + (0.5 + 0.25 * r) * moving_average(rng, b - a, q)
        mats.append(mat.astype(np.float32))
    nan = np.float32(np.nan)
    for ed in case.get("edits", ()):
        kind = ed[0]
        if kind == "nan":               # ("nan", chrom, row, start, stop)
            mats[ed[1]][ed[2], ed[3]:ed[4]] = nan
        elif kind == "nan_all":         # ("nan_all", chrom, start, stop): every row
            mats[ed[1]][:, ed[2]:ed[3]] = nan
        elif kind == "dup_row":         # ("dup_row", src, dst): in every chromosome
            for m in mats:
                m[ed[2]] = m[ed[1]]
        elif kind == "const":           # ("const", chrom, window, value): every row
            mats[ed[1]][:, ed[2] * wb:(ed[2] + 1) * wb] = np.float32(ed[3])
        elif kind == "copy_window":     # ("copy_window", chrom, from window, to window)
            mats[ed[1]][:, ed[3] * wb:(ed[3] + 1) * wb] = mats[ed[1]][:, ed[2] * wb:(ed[2] + 1) * wb]
        elif kind == "ramp":            # ("ramp", chrom, window, slope): every row gains slope * (bin within the window)
            mats[ed[1]][:, ed[2] * wb:(ed[2] + 1) * wb] += (ed[3] * np.arange(wb, dtype=np.float64)).astype(np.float32)
        elif kind == "square":          # ("square", chrom, window, period, amplitude): every row gains a square wave
            wave = ((np.arange(wb) // (ed[3] // 2)) % 2).astype(np.float32) * np.float32(ed[4])
            mats[ed[1]][:, ed[2] * wb:(ed[2] + 1) * wb] += wave
        elif kind == "inf":             # ("inf", chrom, row, bin)
            mats[ed[1]][ed[2], ed[3]] = np.float32(np.inf)
        else:
            raise ValueError(kind)
    return list(case["names"]), mats


def input_sha(mats):
    h = hashlib.sha256()
    for m in mats:
        h.update(np.asarray(m.shape, dtype=np.int64).tobytes())
        h.update(np.ascontiguousarray(m).tobytes())
    return h.hexdigest()


def _case(name, *, names, lens, rows, window_bins, interval, max_lag_bins, smooth_bp, persist_bp, seed, q_range=(3, 40), q=None,
          edits=(), window_count=24, min_windows=8, draws=30, min_pairs=100, min_cov=0.5, threshold=0.1, quantile=0.75,
          rand_seed=1729):
    return dict(name=name, names=names, lens=lens, rows=rows, window_bins=window_bins, seed=seed, q_range=q_range, q=q or {},
                edits=tuple(edits), interval=interval,
                kw=dict(windowBP=window_bins * interval, windowCount=window_count, maxLagBP=max_lag_bins * interval,
                        workingQuantile=quantile, bootstrapDraws=draws, randSeed=rand_seed, minWindowCount=min_windows,
                        acfThreshold=threshold, acfSmoothingBP=smooth_bp, crossingPersistenceBP=persist_bp,
                        minFinitePairs=min_pairs, minFinitePairCoverage=min_cov))


def cases():
    out = []
    # base: 256-bin windows, 96 lags; two autosomes out of ordinal order, chrX, an autosome shorter than a window, a trailing
    # partial window, a duplicated row, NaN stretches
    out.append(_case("base", names=["chr2", "chr1", "chrX", "chr3"], lens=[14 * 256 + 100, 16 * 256, 6 * 256, 200], rows=5,
                     window_bins=256, interval=5, max_lag_bins=96, smooth_bp=25, persist_bp=15, seed=11,
                     edits=[("nan", 0, 0, 300, 420), ("nan", 0, 2, 1000, 1100), ("nan", 1, 4, 2000, 2300), ("nan", 1, 1, 50, 60),
                            ("inf", 1, 0, 700), ("dup_row", 1, 3)]))
    # tile edges: window_bins no multiple of the 512-value LDS tile and longer than one; max_lag_bins + 1 no multiple of 64;
    # max_lag_bins = window_bins // 2; long enough in bp for the period diagnostics to find a band
    out.append(_case("tile_edges", names=["chr1", "chr2"], lens=[9 * 700 + 3, 8 * 700], rows=3, window_bins=700, interval=5,
                     max_lag_bins=350, smooth_bp=35, persist_bp=20, seed=12, q_range=(5, 60), window_count=14, min_windows=6,
                     min_pairs=200, edits=[("nan", 0, 1, 800, 1000)]))
    # long window: more than 8192 bins at interval 1, two rows: pins the summation order of one long contiguous float64 array
    out.append(_case("long_window", names=["chr1", "chr2"], lens=[3 * 8448, 3 * 8448 + 17], rows=2, window_bins=8448, interval=1,
                     max_lag_bins=130, smooth_bp=5, persist_bp=4, seed=13, q_range=(10, 90), window_count=6, min_windows=3,
                     draws=20, min_pairs=500, edits=[("nan", 0, 0, 100, 1900), ("nan", 1, 1, 9000, 9300)]))
    # row rules: m = 1
    out.append(_case("single_row", names=["chr1", "chr2"], lens=[10 * 256, 9 * 256 + 9], rows=1, window_bins=256, interval=1,
                     max_lag_bins=96, smooth_bp=3, persist_bp=2, seed=14, window_count=16, min_windows=6,
                     edits=[("nan", 0, 0, 300, 330)]))
    # row rules: two rows (np.nanmedian of two); a row with fewer than two finite values in a window; a row below the ranking
    # coverage in a window; a window no row covers (no candidate)
    out.append(_case("row_rules", names=["chr1", "chr2"], lens=[10 * 256, 10 * 256], rows=2, window_bins=256, interval=1,
                     max_lag_bins=96, smooth_bp=5, persist_bp=3, seed=15, window_count=18, min_windows=6,
                     edits=[("nan", 0, 0, 256, 511), ("nan", 0, 1, 512 + 60, 768), ("nan_all", 1, 768, 1024),
                            ("nan", 1, 0, 1024, 1280)]))
    # outcomes: a constant window (None), windows censored by maxLag (a strong square wave of period 32: the smoothed |ACF| never
    # falls below the threshold) and by support (a ramp with finite values in its first 150 bins only: the pairs of the lags
    # beyond 50 fall below minFinitePairs), smoothing and persistence of several bins
    out.append(_case("outcomes", names=["chr1", "chr2"], lens=[10 * 256, 10 * 256], rows=3, window_bins=256, interval=5,
                     max_lag_bins=96, smooth_bp=35, persist_bp=25, seed=16, window_count=20, min_windows=6, min_cov=0.05,
                     edits=[("const", 0, 3, 2.0), ("square", 0, 2, 32, 16.0), ("ramp", 1, 4, 0.125),
                            ("nan_all", 1, 4 * 256 + 150, 5 * 256)]))
    # outcomes: smoothing and persistence of one bin
    out.append(_case("one_bin", names=["chr1", "chr2"], lens=[10 * 256, 10 * 256], rows=3, window_bins=256, interval=1,
                     max_lag_bins=96, smooth_bp=1, persist_bp=1, seed=17, window_count=20, min_windows=6,
                     edits=[("ramp", 0, 1, 0.125), ("nan", 1, 2, 100, 180)]))
    # ties: two byte-identical windows share a rank
    out.append(_case("ties", names=["chr1", "chr2"], lens=[10 * 256, 10 * 256], rows=3, window_bins=256, interval=1,
                     max_lag_bins=96, smooth_bp=5, persist_bp=3, seed=18, window_count=20, min_windows=6,
                     edits=[("copy_window", 0, 2, 6), ("copy_window", 1, 0, 9)]))
    # the shortened run of the reference's rank-weighted sampling test: 64-bin windows at interval 1, the first one constant, the
    # others one shape on offsets that tie in pairs (the shape is a moving average here, where the reference's test smooths
    # normal noise with a Gaussian filter: no libm in the input)
    out.append(contract_case("contract_shortened", 12, window_count=20, min_windows=10))
    return out


def contract_case(name, n_windows, *, window_count, min_windows):
    case = _case(name, names=["chr11"], lens=[n_windows * 64], rows=1, window_bins=64, interval=1, max_lag_bins=24, smooth_bp=1,
                 persist_bp=1, seed=9, window_count=window_count, min_windows=min_windows, draws=20, rand_seed=21, threshold=0.15,
                 min_pairs=8)
    case["contract"] = n_windows
    return case


def build_any(case):
    if "contract" not in case:
        return build(case)
    rng = np.random.default_rng(case["seed"])
    shape = moving_average(rng, 64, 4)
    shape = shape - np.min(shape) + 1.0
    blocks = [np.full(64, 400.0, dtype=np.float32)]
    total = 300
    for i in range(1, case["contract"]):
        blocks.append(np.asarray(shape + (2.0 + float((total - i) // 2)), dtype=np.float32))
    return list(case["names"]), [np.concatenate(blocks)[None, :]]


def runtime_error_cases():
    """(case, the text the RuntimeError must contain)."""
    return [(contract_case("contract_too_few", 20, window_count=20, min_windows=20), "needs at least 20 windows")]


def value_error_cases():
    """(name, names, matrices, interval, keywords, text): every ValueError of the reference, in its order of checks."""
    good = np.zeros((2, 600), dtype=np.float32)
    base = dict(windowBP=100, maxLagBP=50, acfSmoothingBP=5, crossingPersistenceBP=5, minFinitePairs=10, windowCount=4,
                minWindowCount=2, bootstrapDraws=5)
    out = []

    def add(name, text, names=("chr1",), mats=None, interval=1, **kw):
        out.append((name, list(names) if names is not None else None, [good] if mats is None else mats, interval, {**base, **kw}, text))

    add("not_sequences", "chromosome inputs must be finite sequences", names=None)
    add("empty", "chromosome inputs must be nonempty and have equal lengths", names=(), mats=[])
    add("unequal", "chromosome inputs must be nonempty and have equal lengths", names=("chr1", "chr2"))
    add("interval_bool", "intervalSizeBP must be an integer", interval=True)
    add("interval_float", "intervalSizeBP must be an integer", interval=1.0)
    add("window_range", "windowBP is outside the supported integer range", windowBP=1 << 40)
    add("quantile_str", "workingQuantile must be a real scalar", workingQuantile="0.5")
    add("threshold_nan", "acfThreshold must be finite", acfThreshold=float("nan"))
    add("interval_zero", "intervalSizeBP must be positive", interval=0)
    add("window_zero", "windowBP must be positive", windowBP=0)
    add("lag_large", "maxLagBP must satisfy 0 < maxLagBP <= windowBP / 2", maxLagBP=51)
    add("count_zero", "windowCount and bootstrapDraws must be positive", windowCount=0)
    add("draws_zero", "windowCount and bootstrapDraws must be positive", bootstrapDraws=0)
    add("seed_negative", "randSeed must be nonnegative", randSeed=-1)
    add("min_windows", "minWindowCount must satisfy 0 < minWindowCount <= windowCount", minWindowCount=5)
    add("quantile_one", "workingQuantile must satisfy 0 < q < 1", workingQuantile=1.0)
    add("threshold_one", "acfThreshold must satisfy 0 < x < 1", acfThreshold=1.0)
    add("smoothing_zero", "ACF smoothing and crossing persistence must be positive", acfSmoothingBP=0)
    add("persistence_large", "ACF smoothing and crossing persistence cannot exceed maxLagBP", crossingPersistenceBP=51)
    add("pairs_zero", "minFinitePairs must be positive", minFinitePairs=0)
    add("coverage_large", "minFinitePairCoverage must satisfy 0 < x <= 1", minFinitePairCoverage=1.5)
    add("multiples", "windowBP and maxLagBP must be integer multiples of intervalSizeBP", interval=3)
    add("pairs_window", "minFinitePairs cannot exceed the window bin count", minFinitePairs=101)
    add("too_short", "physical window and lag settings are too short for the bin width", interval=10, windowBP=100, maxLagBP=20,
        acfSmoothingBP=20, crossingPersistenceBP=10, minFinitePairs=1)
    # ("binned maxLagBP must not exceed half of the binned windowBP" cannot be reached: maxLagBP <= windowBP // 2 with both
    # multiples of the interval already bounds the binned lag by half the binned window)
    add("ndim", "each chromosome matrix must be two-dimensional and nonempty", mats=[np.zeros(600, dtype=np.float32)])
    add("kind", "chromosome matrices must contain real numeric values", mats=[np.zeros((2, 600), dtype=np.complex64)])
    add("row_count", "chromosome matrices must have one shared row count", names=("chr1", "chr2"),
        mats=[good, np.zeros((3, 600), dtype=np.float32)])
    add("duplicate", "duplicate canonical autosome chr1", names=("chr1", "1"), mats=[good, good])
    add("no_eligible", "dependence estimator found no eligible autosomes", names=("chrX", "chr2"),
        mats=[good, np.zeros((2, 50), dtype=np.float32)])
    return out


def call(fn, case, **extra):
    names, mats = build_any(case)
    return fn(names, mats, case["interval"], **case["kw"], **extra)
