"""Seeded inputs of the finished-track stages (tests/test_munc_track_twin.py, tests/test_gpu_munc_track.py,
tests/golden/make_munc_track_golden.py) -- TEST INFRASTRUCTURE.  Fixtures hold the reference's OUTPUTS only; the inputs come from
here."""
import numpy as np

F32_MAX = 3.4028234663852886e38
F32 = np.float32


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def ulp_distance(a, b):
    """Per element, how many float32 values lie between a and b (both finite and positive here)."""
    return np.abs(bits(np.asarray(a, F32)).astype(np.int64) - bits(np.asarray(b, F32)).astype(np.int64))


# -- trends ---------------------------------------------------------------------------------------------------------------------
def make_trend(degree, n_basis, seed, x_min=-2.5, x_max=4.0, repeat=False, beta_edit=None):
    """A clamped knot vector on [x_min, x_max] (degree + 1 equal knots at both ends) and smooth coefficients in log-variance
    units.  repeat: one interior knot twice.  beta_edit: {index: value} (a non-finite coefficient)."""
    rng = np.random.default_rng(seed)
    inner = n_basis - degree - 1
    mid = np.sort(rng.uniform(x_min, x_max, inner)) if inner > 0 else np.zeros(0)
    if repeat and inner >= 2:
        mid[inner // 2] = mid[inner // 2 - 1]
    knots = np.concatenate([np.full(degree + 1, x_min), mid, np.full(degree + 1, x_max)]).astype(np.float64)
    beta = (-3.0 + 0.8 * np.cumsum(rng.normal(0.0, 0.6, n_basis))).astype(np.float64)
    for k, v in (beta_edit or {}).items():
        beta[k] = v
    return knots, beta, int(degree), float(x_min), float(x_max)


def mean_track(n, seed, trend=None):
    """A float32 mean track: signed values whose predictor covers the trend's range and leaves it on both sides, zeros, NaN and
    infinities, and (with a trend) values whose predictor is exactly a knot."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_t(3, n) * 4.0).astype(F32)
    if n >= 8:
        x[1], x[2], x[3], x[4] = 0.0, np.nan, np.inf, -np.inf
        x[5], x[6] = 1.0e6, -40.0
    return x


EVAL_CASES = (
    # name, degree, basis functions, n, floor (eps), cap (maxVariance), options
    ("deg3_b60_n257", 3, 60, 257, 1.0e-6, None, {}),
    ("deg0_b7_n65", 0, 7, 65, 1.0e-6, None, {}),
    ("deg1_b9_n64", 1, 9, 64, 1.0e-6, None, {}),
    ("deg5_b12_n63", 5, 12, 63, 1.0e-6, None, {}),
    ("deg3_b256_n257", 3, 256, 257, 1.0e-6, None, {}),
    ("deg3_repeat_knot", 3, 16, 257, 1.0e-6, None, {"repeat": True}),
    ("deg3_beta_posinf", 3, 12, 65, 1.0e-6, None, {"beta_edit": {5: np.inf}}),
    ("deg3_beta_neginf", 3, 12, 65, 1.0e-6, None, {"beta_edit": {5: -np.inf}}),
    ("deg3_beta_nan", 3, 12, 65, 1.0e-6, None, {"beta_edit": {5: np.nan}}),
    ("deg2_clamps", 2, 10, 257, 0.5, 0.75, {"shift": 2.6}),      # both log bounds bind
    ("const_degree_m1", -1, 6, 64, 1.0e-6, None, {}),
    ("const_no_knots", 3, 6, 65, 1.0e-6, None, {"no_knots": True}),
    ("const_no_beta", 3, 0, 63, 1.0e-6, None, {"no_knots": True}),
    ("const_beta_inf", -1, 3, 17, 1.0e-6, 9.0, {"beta_edit": {0: np.inf}}),
    ("deg3_n0", 3, 12, 0, 1.0e-6, None, {}),
)


def eval_inputs(case):
    name, degree, nb, n, eps, cap, opt = case
    if degree < 0 or opt.get("no_knots"):
        rng = np.random.default_rng(len(name))
        beta = rng.normal(-2.0, 1.0, nb)
        for k, v in (opt.get("beta_edit") or {}).items():
            beta[k] = v
        trend = (np.zeros(0) if opt.get("no_knots") else np.linspace(-1.0, 1.0, 8), beta, degree, -1.0, 1.0)
    else:
        trend = make_trend(degree, nb, 100 + nb + degree, repeat=opt.get("repeat", False), beta_edit=opt.get("beta_edit"))
        trend = (trend[0], trend[1] + opt.get("shift", 0.0)) + trend[2:]
    mean = mean_track(n, 200 + n + max(degree, 0))
    return trend, mean, eps, cap


def eval_predictor(case, twin):
    """The float64 predictor track of a case, with values exactly on knots planted (what the native itself is called with)."""
    trend, mean, _eps, _cap = eval_inputs(case)
    pred = twin.predictor(mean)
    knots = trend[0]
    if knots.size and pred.size > 20:
        pick = knots[[0, knots.size // 2, knots.size // 3, knots.size - 1]]
        pred[10:14] = pick
        pred[14] = np.nextafter(trend[3], -np.inf)      # just below xMin
        pred[15] = np.nextafter(trend[4], np.inf)       # just above xMax
    return pred


# -- finalisation --------------------------------------------------------------------------------------------------------------
def final_base(n, seed):
    rng = np.random.default_rng(seed)
    local = rng.gamma(2.0, 0.3, n).astype(F32)
    prior = rng.gamma(2.0, 0.25, n).astype(F32)
    floor = rng.gamma(1.5, 0.05, n).astype(F32)
    floor[rng.random(n) < 0.3] = np.nan
    floor[rng.random(n) < 0.2] = 0.0
    return local, prior, floor


# name, n, keyword edits; every case runs with and without EB
FINAL_CASES = (
    ("plain_n257", 257, {}),
    ("n1", 1, {}),
    ("n63", 63, {}),
    ("n64_nofloor", 64, {"no_floor": True}),
    ("n65_cap", 65, {"varianceCap": 0.9, "varianceFloor": 0.05}),            # values on, below and above both bounds
    ("f32_params", 257, {"nuLocal": 6.1, "nuPrior": 33.3, "varianceFloor": 1.0e-3 / 3.0}),   # change when rounded to float32
    ("subnormal", 65, {"subnormal": True, "varianceFloor": 1.0e-45, "no_floor": True}),
    ("n0", 0, {}),
)


def final_inputs(case):
    name, n, opt = case
    local, prior, floor = final_base(n, 300 + n)
    kw = dict(nuLocal=opt.get("nuLocal", 8.0), nuPrior=opt.get("nuPrior", 40.0), varianceFloor=opt.get("varianceFloor", 1.0e-6),
              varianceCap=opt.get("varianceCap", F32_MAX))
    if n >= 8 and "varianceCap" in opt:
        lo, hi = F32(kw["varianceFloor"]), F32(kw["varianceCap"])
        local[:6] = [lo, np.nextafter(lo, F32(0)), np.nextafter(lo, F32(1)), hi, np.nextafter(hi, F32(0)), np.nextafter(hi, F32(9))]
        prior[2:8] = local[:6]
    if opt.get("subnormal"):
        local[:4] = [1.0e-45, 3.0e-45, 1.0e-40, 1.0e-38]
        prior[:4] = [2.0e-45, 1.0e-45, 5.0e-41, 1.0e-39]
    return local, prior, (None if opt.get("no_floor") else floor), kw


def final_error_cases():
    """(name, args, kwargs, text): parameter errors in the native's order, then each invalid kind at the first, a middle and the
    last index, and two kinds at one index."""
    local, prior, floor = final_base(65, 77)
    ok = dict(nuLocal=8.0, nuPrior=40.0)
    out = [
        ("floor_zero", (local, prior), dict(ok, varianceFloor=0.0), "varianceFloor must be positive and finite"),
        ("floor_nan", (local, prior), dict(ok, varianceFloor=np.nan), "varianceFloor must be positive and finite"),
        ("cap_below", (local, prior), dict(ok, varianceFloor=1.0, varianceCap=0.5), "varianceCap must be finite and at least varianceFloor"),
        ("cap_inf", (local, prior), dict(ok, varianceCap=np.inf), "varianceCap must be finite and at least varianceFloor"),
        ("no_prior", (local,), dict(ok), "priorVarianceTrack is required for MUNC EB finalization"),
        ("nu_local_zero", (local, prior), dict(nuLocal=0.0, nuPrior=40.0), "nuLocal must be positive and finite"),
        ("nu_prior_nan", (local, prior), dict(nuLocal=8.0, nuPrior=np.nan), "nuPrior must be positive and finite"),
        ("nu_local_f32_overflow", (local, prior), dict(nuLocal=1.0e39, nuPrior=40.0), "nuLocal must be positive and finite"),
        ("prior_length", (local, prior[:-1]), dict(ok), "priorVarianceTrack length must match localVarianceTrack length"),
        ("floor_length", (local, prior, floor[:-1]), dict(ok), "countFloor length must match localVarianceTrack length"),
    ]
    for where, idx in (("first", 0), ("middle", 31), ("last", 64)):
        for kind, value, text in (("local", 0.0, "localVarianceTrack must contain finite positive values at index {}"),
                                  ("prior", np.nan, "priorVarianceTrack must contain finite positive values at index {}"),
                                  ("floor", -1.0, "countFloor must be nonnegative where finite at index {}")):
            a = [local.copy(), prior.copy(), floor.copy()]
            a[("local", "prior", "floor").index(kind)][idx] = value
            out.append((f"bad_{kind}_{where}", tuple(a), dict(ok), text.format(idx)))
    a = [local.copy(), prior.copy(), floor.copy()]
    a[0][40], a[1][40], a[2][40], a[2][12] = np.inf, -1.0, np.inf, np.inf
    out.append(("two_kinds_floor_first", tuple(a), dict(ok), "countFloor must be nonnegative where finite at index 12"))
    a = [local.copy(), prior.copy(), floor.copy()]
    a[0][40], a[1][40], a[2][40] = np.inf, -1.0, np.inf
    out.append(("three_kinds_one_index", tuple(a), dict(ok), "localVarianceTrack must contain finite positive values at index 40"))
    a = [local.copy(), prior.copy(), floor.copy()]
    a[1][40], a[2][40] = 0.0, -2.0
    out.append(("prior_and_floor_one_index", tuple(a), dict(ok), "priorVarianceTrack must contain finite positive values at index 40"))
    a = [local.copy(), prior.copy(), floor.copy()]
    a[0][9] = np.nan
    out.append(("no_eb_bad_local", (a[0],), dict(useEB=False), "localVarianceTrack must contain finite positive values at index 9"))
    return out


# -- getMuncTrack and the blacklist floor ----------------------------------------------------------------------------------------
# name, n, use_eb, factor, prior from ("trend" | "track"), count floor, cap
TRACK_CASES = (
    ("eb_trend_n257", 257, True, 1.0, "trend", True, None),
    ("eb_factor_out", 257, True, 1.37, "trend", True, 2.0),
    ("eb_factor_in_band", 65, True, 1.0 + 5.0e-9, "track", False, None),
    ("eb_factor_edge", 65, True, 1.0 + 2.0e-8, "track", True, None),
    ("eb_floor_all_nan", 64, True, 1.0, "track", "nan", None),
    ("eb_floor_inf_cells", 64, True, 0.6, "track", "inf", None),
    ("no_eb_floor", 257, False, 1.0, "track", True, 1.5),
    ("no_eb_plain", 63, False, 1.0, "track", False, None),
)
TRACK_FLOOR, TRACK_NU0, TRACK_NUL = 1.0e-3 / 3.0, 1.0e4, 7.3       # (Nu_0 above 50 Nu_L: the cap binds; both change in float32)


def track_inputs(case):
    name, n, use_eb, factor, source, with_floor, cap = case
    local, prior, floor = final_base(n, 400 + n)
    trend = make_trend(3, 24, 500 + n)
    mean = mean_track(n, 600 + n)
    if with_floor == "nan":
        floor[:] = np.nan
    elif with_floor == "inf":
        floor[3], floor[9] = np.inf, -np.inf
    return dict(local=local, floor=TRACK_FLOOR, cap=cap, use_eb=use_eb, trend=trend, prior_mean=mean,
                prior_variance=prior if source == "track" else None, factor=factor, nu0=TRACK_NU0, nuL=TRACK_NUL,
                count_floor=floor if with_floor else None)


# name, m, n, masked fraction (None: no mask, 1.0: all), quantile
BLACKLIST_CASES = (
    ("no_mask", 3, 65, None, 0.05),
    ("all_masked", 3, 65, 1.0, 0.05),
    ("between_two", 3, 257, 0.2, 0.05),
    ("q0", 1, 64, 0.3, 0.0),
    ("q1", 1, 64, 0.3, 1.0),
    ("q_half_m17", 17, 63, 0.4, 0.5),
    ("one_unmasked", 3, 17, "one", 0.05),
    ("ties", 3, 257, 0.25, 0.37),
)


def blacklist_inputs(case):
    name, m, n, frac, q = case
    rng = np.random.default_rng(700 + n + m)
    x = rng.gamma(2.0, 0.4, (m, n)).astype(F32)
    if name == "ties":
        x = np.round(x * 4.0).astype(F32) / F32(4.0) + F32(0.25)
    if frac is None:
        mask = np.zeros(n, np.uint8)
    elif frac == "one":
        mask = np.ones(n, np.uint8)
        mask[n // 2] = 0
    else:
        mask = (rng.random(n) < frac).astype(np.uint8)
        if frac >= 1.0:
            mask[:] = 1
        else:
            mask[0] = 1
    return x, mask, q


# -- block sums ------------------------------------------------------------------------------------------------------------------
BLOCK_LENGTHS = (2, 7, 8, 9, 128, 129, 257)


def block_chain(m, n, seed, block_len):
    """Evidence, weights, exclude mask and float64 mean of one chain.  One block is all excluded, one has all-zero weights, one
    holds a NaN and an infinite mean, some cells have non-positive evidence or weight."""
    rng = np.random.default_rng(seed)
    ev = rng.gamma(2.0, 0.3, (m, n)).astype(F32)
    w = rng.uniform(0.05, 1.5, (m, n)).astype(F32)
    ex = (rng.random(n) < 0.1).astype(np.uint8)
    mean = (rng.standard_t(3, n) * 3.0).astype(F32)
    L = max(2, block_len)
    nb = n // L
    if nb >= 1:
        ex[0:L] = 1
    if nb >= 2:
        w[:, L:2 * L] = 0.0
    if nb >= 3:
        mean[2 * L], mean[2 * L + 1] = np.nan, np.inf
    hit = rng.random((m, n)) < 0.03
    ev[hit] = 0.0
    w[rng.random((m, n)) < 0.03] = -0.5
    ev[rng.random((m, n)) < 0.01] = np.nan
    return ev, w, ex, mean.astype(np.float64)


def planted_trigamma(x):
    """A stand-in with polygamma(1, .)'s leading behaviour, exact in float64 arithmetic everywhere: for the order and mask tests."""
    x = np.asarray(x, dtype=np.float64)
    return 1.0 / x + 0.5 / (x * x)
