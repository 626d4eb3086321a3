"""Case table for the effective sample size scan `cEstimateEffectiveSampleSize` (pyx:9160-9279).  Inputs are re-synthesised from
(series, n, seed); the committed ess/ess_*.npz fixtures hold the REAL reference's outputs (tests/golden/make_ess_golden.py).
Every comparison is exact: floats by their 64-bit patterns.

Sizes are the edges of the device path, not workload sizes: the 64 lags of a wavefront, the 512-value LDS tile and its 64-value
pad, and the rounds of lags -- 256 lags, then 512, 1024, ...; a call whose scans all end within 512 lags runs them in one round
(csrc/csr_ess.h, csr_host_ess.inl)."""
from __future__ import annotations

import numpy as np

GROUPS = ("fast", "general")
SIZES = (1, 2, 3, 63, 64, 65, 2047, 2048, 2049, 131073)
ROUND = 256     # lags of the first round


def max_lags(n):
    return (1, 63, 64, 65, 255, 256, 257, n - 1, n + 5)


def square_wave(n, half):
    """+1 / -1 in blocks of `half` values: its autocorrelation falls linearly and crosses zero where the table plants a break."""
    return np.where((np.arange(n) // half) % 2 == 0, 1.0, -1.0)


# (n, half period) of square waves whose scan breaks at lag 255 (the last lag of the first round: 254 lags used) and at lag 256
# (the first lag of the second round: 255 lags used); tests/test_budget_twin.py holds the twin to exactly that
BREAK_AT_ROUND_END = (1780, 445)
BREAK_AT_ROUND_START = (1788, 447)


def values(case):
    n, kind, rng = case["n"], case["series"], np.random.default_rng(case["seed"])
    if kind in ("ar_occ", "ar_soft", "ar_pos"):
        e = rng.standard_normal(n)
        x = np.empty(n)
        acc = 0.0
        for i in range(n):                      # AR(1), phi = 0.9
            acc = 0.9 * acc + e[i]
            x[i] = acc
        if kind == "ar_occ":
            return (x > 1.0).astype(np.float64)
        if kind == "ar_soft":
            return np.clip((x - 1.0) / 0.8, 0.0, None)
        return np.exp(0.5 * x)                  # positive: the logPositive cases
    if kind == "white":
        return rng.standard_normal(n)
    if kind == "alternating":
        return np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    if kind == "ramp":
        return np.arange(n, dtype=np.float64) * 0.25
    if kind == "square":
        return square_wave(n, case["half"])
    if kind == "const":
        return np.full(n, 2.5)
    if kind == "const_tenth":                   # the mean of n tenths is not a tenth: a variance of rounding errors
        return np.full(n, 0.1)
    if kind == "nan":
        x = rng.standard_normal(n)
        x[n // 3] = np.nan
        return x
    if kind == "inf":
        x = rng.standard_normal(n)
        x[n // 2] = np.inf
        return x
    if kind == "huge":                          # squares overflow: the variance is not finite
        return rng.standard_normal(n) * 1.0e200
    if kind == "pair_spike":                    # two adjacent large values among isolated active ones: rho(1) far above 1 under the mask
        x = rng.standard_normal(n) * 1.0e-3
        x[0] = x[1] = 10.0
        return x
    raise KeyError(kind)


def mask(case):
    n, kind = case["n"], case.get("mask")
    if kind is None:
        return None
    rng = np.random.default_rng(case["seed"] + 77)
    if kind == "random":
        return (rng.random(n) < 0.7).astype(np.uint8)
    if kind == "every4":                        # pairs exist at the multiples of 4 only
        return (np.arange(n) % 4 == 0).astype(np.uint8)
    if kind == "none_active":
        return np.zeros(n, np.uint8)
    if kind == "one_active":
        m = np.zeros(n, np.uint8)
        m[n // 2] = 1
        return m
    if kind == "all":
        return np.full(n, 3, np.uint8)          # any nonzero byte is active
    if kind == "pair_then_thirds":              # 0 and 1 active, then every third value: only one pair at lag 1
        m = (np.arange(n) % 3 == 0).astype(np.uint8)
        m[1] = 1
        return m
    if kind == "hide_bad":                      # the non-finite / non-positive values are inactive
        x = values(case)
        return (np.isfinite(x) & (x > 0.0)).astype(np.uint8)
    raise KeyError(kind)


def cases():
    cs = []

    def add(group, name, **kw):
        kw.setdefault("mask", None)
        kw.setdefault("log", False)
        kw.setdefault("window", 0)
        cs.append(dict(group=group, name=name, seed=1000 + len(cs), **kw))

    # -- fast path: every n x every maxLag on the default statistic's series; the other series at the tile edges
    for n in SIZES:
        for k, lag in enumerate(max_lags(n)):
            add("fast", f"fast_ar_occ_n{n}_lag{k}", series="ar_occ", n=n, max_lag=lag)
    for series in ("ar_soft", "white"):
        for n in (3, 65, 2049):
            for lag in (63, 257, n - 1):
                add("fast", f"fast_{series}_n{n}_lag{lag}", series=series, n=n, max_lag=lag)
    for n in (2, 3, 64, 65, 2049):
        add("fast", f"fast_alternating_n{n}", series="alternating", n=n, max_lag=5)
    for n, lag in ((2049, 255), (2049, 256), (2049, 257), (131073, 700), (65, 7)):
        add("fast", f"fast_ramp_n{n}_lag{lag}", series="ramp", n=n, max_lag=lag)
    add("fast", "fast_break_round_end", series="square", n=BREAK_AT_ROUND_END[0], half=BREAK_AT_ROUND_END[1], max_lag=BREAK_AT_ROUND_END[0] - 1)
    add("fast", "fast_break_round_start", series="square", n=BREAK_AT_ROUND_START[0], half=BREAK_AT_ROUND_START[1],
        max_lag=BREAK_AT_ROUND_START[0] - 1)
    for series in ("const", "const_tenth", "nan", "inf", "huge"):
        for n in (2, 65, 2049):
            add("fast", f"fast_{series}_n{n}", series=series, n=n, max_lag=64)
    add("fast", "fast_negative_lag", series="ar_soft", n=65, max_lag=-3)
    add("fast", "fast_n0", series="white", n=0, max_lag=4)
    # -- general path: masks, windows, the log
    for n in (2, 65, 2049):
        for lag in (1, 64, 257, n + 5):
            add("general", f"gen_random_mask_n{n}_lag{lag}", series="ar_soft", n=n, max_lag=lag, mask="random")
    add("general", "gen_random_mask_big", series="ar_occ", n=131073, max_lag=300, mask="random")
    for n in (65, 2049):
        add("general", f"gen_every4_n{n}", series="ar_soft", n=n, max_lag=257, mask="every4")
        add("general", f"gen_every4_window_n{n}", series="ar_soft", n=n, max_lag=257, mask="every4", window=300)
        add("general", f"gen_all_mask_n{n}", series="white", n=n, max_lag=70, mask="all")
    for n in (1, 65):
        add("general", f"gen_none_active_n{n}", series="white", n=n, max_lag=8, mask="none_active")
        add("general", f"gen_one_active_n{n}", series="white", n=n, max_lag=8, mask="one_active")
    for window in (1, 2, 64, 65, 256, 257, 5000):     # 5000: larger than maxLag
        for series in ("ar_soft", "ramp"):
            add("general", f"gen_window{window}_{series}", series=series, n=2049, max_lag=300, window=window)
    add("general", "gen_window_masked", series="ar_soft", n=2049, max_lag=300, window=64, mask="random")
    add("general", "gen_window_is_lag_plus_one", series="ramp", n=2049, max_lag=63, window=64)
    add("general", "gen_tau_clamped", series="pair_spike", n=301, max_lag=10, window=2, mask="pair_then_thirds")
    add("general", "gen_tau_unclamped", series="pair_spike", n=301, max_lag=10, window=0, mask="pair_then_thirds")
    for n in (3, 65, 2049):
        add("general", f"gen_log_n{n}", series="ar_pos", n=n, max_lag=65, log=True)
    add("general", "gen_log_masked", series="ar_pos", n=2049, max_lag=65, log=True, mask="random", window=40)
    add("general", "gen_log_bad_hidden", series="white", n=2049, max_lag=20, log=True, mask="hide_bad")
    add("general", "gen_nan_hidden", series="nan", n=65, max_lag=20, mask="hide_bad")
    add("general", "gen_const", series="const", n=65, max_lag=20, window=8)
    return cs


# what the reference answers with ValueError (name, series kwargs, text)
ERRORS = (
    ("err_window_negative", dict(series="white", n=9, max_lag=3, window=-1), "windowIntervals must be nonnegative"),
    ("err_mask_length", dict(series="white", n=9, max_lag=3, mask="short"), "activeMask length must match values length"),
    ("err_nan_active", dict(series="nan", n=9, max_lag=3, window=4), "active values must be finite"),
    ("err_inf_masked_in", dict(series="inf", n=9, max_lag=3, mask="all"), "active values must be finite"),
    ("err_log_nonpositive", dict(series="white", n=65, max_lag=3, log=True), "active values must be positive finite"),
    ("err_log_nan", dict(series="nan", n=9, max_lag=3, log=True), "active values must be positive finite"),
    ("err_variance", dict(series="huge", n=65, max_lag=3, window=4), "variance estimate must be finite"),
)


def error_cases():
    out = []
    for k, (name, kw, text) in enumerate(ERRORS):
        case = dict(name=name, seed=9000 + k, mask=None, log=False, window=0)
        case.update(kw)
        out.append((case, text))
    return out


def call(mod, case):
    m = np.ones(case["n"] - 1, np.uint8) if case.get("mask") == "short" else mask(case)
    return mod.cEstimateEffectiveSampleSize(values(case), case["max_lag"], m, case["log"], case["window"])


def run_case(mod, case):
    n_eff, tau, lags = call(mod, case)
    assert type(n_eff) is float and type(tau) is float and type(lags) is int
    return dict(out=np.asarray([n_eff, tau], np.float64), lags=np.asarray([lags], np.int64))


def same(a, b):
    return (np.array_equal(np.asarray(a["out"], np.float64).view(np.uint64), np.asarray(b["out"], np.float64).view(np.uint64))
            and np.array_equal(np.asarray(a["lags"], np.int64), np.asarray(b["lags"], np.int64)))


def load_group(path):
    out = {}
    with np.load(path) as z:
        for key in z.files:
            name, field = key.rsplit("/", 1)
            out.setdefault(name, {})[field] = z[key]
    return out
