"""GPU tests of the two device reductions behind the outer stop rule of `run_consenrich_batch` (run with -m gpu):

  * `DeviceBatch.objective_terms` (k_obj_wave / k_obj_fold + the bitwise median selection): robust-precision, roughness and
    negative-part penalties, effective observation count (core.py:4418-4538);
  * the weighted RMS triple of `DeviceBatch.background_update` (k_bg_wave_pass mode 3 + fold; core.py:5199-5243).

Every input is PLANTED (upload, upload_multipliers, set_background): no fit decides what the kernels see.  The reference is the
float64 twin in oracle/ (`driver.penalized_objective`, `driver.background_shift_gate`, `background.weight_rhs_tracks`).

Tolerance (derived, not measured).  Every per-chain sum is a sum of n non-negative float64 terms (v - log v >= 1, squares,
w d^2): in ANY summation order its relative error is at most (n - 1) 2^-53, plus a few ulps per term (one log, two or three
operations, no cancellation).  Gate: (n + 8) 2^-52 relative to the EXACT sum (math.fsum over the same float64 terms), n = number
of terms of that sum.  The twin's own value is held to the same gate, which anchors the gate to the reference and not to the code
under test.  The RMS values get the same gate with n = chain length (numerator and weight sum each carry it, the square root halves
it).  Counts, the weight median (both sides accumulate the same expression row by row, the selection is exact), support, weight
scale and every term that must vanish are compared with ==."""
import math

import numpy as np
import pytest

from conftest import gpu_available

pytestmark = pytest.mark.gpu

NU, LAM_FIRST, LAM_SECOND, MULT, PAD = 8.0, 3.0, 7.0, 2.0, 1.0e-4
BOUNDS = (0.25, 4.0)
TINY = float(np.finfo(np.float64).tiny)
# 1, 2, 3: the len == 1 kappa branch, first difference only, the first second difference; 63, 64, 65: one 64-bin group partly /
# exactly filled, the second group; 2047, 2048, 2049: one wavefront record holds 32 groups = 2048 bins; 4097: three records;
# 131073: 65 records, the second trip of the 64-lane fold loop.  Short chains sit between long ones: the pad bins after a 1-bin
# chain are followed by real data.
MAIN_LENS, MAIN_M = [131073, 1, 2049, 2, 4097, 3, 2048, 63, 2047, 64, 65], 3
SMALL_LENS, SMALL_M = [2049, 1, 65], 1
RMS_LENS = [131073, 1, 2049, 2, 65, 3, 64]
FIELDS = ("robust_observation_penalty", "robust_process_penalty", "first_difference_penalty", "second_difference_penalty",
          "negative_penalty")
TWIN_KEY = {"robust_observation_penalty": "robust_observation_penalty", "robust_process_penalty": "robust_process_penalty",
            "first_difference_penalty": "background_first_difference_penalty",
            "second_difference_penalty": "background_second_difference_penalty",
            "negative_penalty": "background_negative_penalty"}
WORST = {}          # field -> worst observed |error| / gate of the device (printed when the module is done; run with -s)


@pytest.fixture(scope="module")
def product():
    if not gpu_available():
        pytest.fail("GPU tests selected but no HIP device / library: the product has no CPU fallback")
    from consenrich_amd import cconsenrich

    yield cconsenrich
    print("\nworst |error| / gate per field: " + ", ".join(f"{k}={v:.4f}" for k, v in sorted(WORST.items())))


# ---- planted inputs ------------------------------------------------------------------------------------------------
def _plant(n, m, seed, dirty=True):
    """One chain: data, variances, lambda, kappa, background (float32).  dirty: the cells and entries no fit would leave
    (masked / non-finite variances, multipliers at and below zero); clean inputs can also go through a filter or a solve."""
    rng = np.random.default_rng(seed)
    k = np.arange(n)
    data = (0.4 * np.sin(k / 29.0) + rng.normal(0.0, 0.3, (m, n))).astype(np.float32)
    munc = (0.5 * np.exp(rng.normal(0.0, 0.4, (m, n)))).astype(np.float32)
    lam = np.exp(rng.normal(0.0, 1.2, n)).astype(np.float32)          # reaches both sides of lambda_bounds = (0.25, 4)
    kap = np.exp(rng.normal(0.0, 1.0, n)).astype(np.float32)
    bg = (0.3 * np.sin(k / 37.0) + rng.normal(0.0, 0.1, n)).astype(np.float32)
    if n == 1:
        bg[:] = [-0.7]
        lam[:] = [7.0]
    elif n == 2:
        bg[:] = [0.4, -0.2]
        lam[:] = [0.1, 1.0e-40] if dirty else [0.1, 7.0]
    elif n == 3:
        bg[:] = [-0.5, 0.0, 0.25]
        lam[:] = [0.0, -1.0, 5.0] if dirty else [0.1, 1.3, 5.0]
    else:
        bg[n // 3: n // 3 + max(8, n // 10)] = -np.abs(bg[n // 3: n // 3 + max(8, n // 10)]) - np.float32(0.05)   # negative stretch
        bg[[2, n // 2, n - 1]] = 0.0                                                                              # exact zeros
    if dirty:
        kap[0] = np.float32(1.0e30)          # must not count unless n == 1
        if n >= 2:
            kap[n // 2] = 0.0
        if n >= 63:
            lam[[5, 17, 40]] = [0.0, -1.0, 1.0e-40]
            munc[0, 3] = np.float32(1.0e30)              # masked cell
            munc[:, 7] = np.float32(1.0e30)              # whole masked bin
            munc[1 % m, 11] = np.nan
            munc[2 % m, 13] = np.inf
            munc[0, 19] = -np.inf
            munc[1 % m, 23] = -np.float32(PAD)
    return {"n": n, "data": data, "munc": munc, "lam": lam, "kap": kap, "bg": bg}


def _plants(lens, m, seed, dirty=True):
    return [_plant(n, m, seed + 17 * c, dirty) for c, n in enumerate(lens)]


@pytest.fixture(scope="module")
def planted():
    main, small = _plants(MAIN_LENS, MAIN_M, 100), _plants(SMALL_LENS, SMALL_M, 900)
    lam_all = np.concatenate([p["lam"] for p in main])
    assert lam_all.min() < BOUNDS[0] and lam_all.max() > BOUNDS[1]
    for p in main:
        assert (p["bg"] < 0).any()
    return {"main": (MAIN_LENS, MAIN_M, main), "small": (SMALL_LENS, SMALL_M, small)}


def _open(lens, m, plants, background=True):
    from consenrich_amd.batch import DeviceBatch, ModelParams

    b = DeviceBatch(0)
    b.configure(ModelParams(state_dim=2, pad=PAD, lambda_bounds=BOUNDS), m, lens)
    for c, p in enumerate(plants):
        b.upload(c, p["data"], p["munc"])
        b.upload_multipliers(c, p["lam"], p["kap"], np.ones(p["n"], np.float32))
        if background:
            b.set_background(c, p["bg"])
    return b


# ---- the reference: twin + exact sums ---------------------------------------------------------------------------------
def _fsum(a):
    a = np.asarray(a, np.float64).reshape(-1)
    return float("nan") if np.isnan(a).any() else math.fsum(a.tolist())


def _weight_track(munc, lam):
    """The float64 weight track of the twin's negative-part scale (oracle/driver.py `penalized_objective`), the same expression
    accumulated row by row; (median of the positive finite entries or 1.0, count of them)."""
    w = np.zeros(munc.shape[1])
    prec = None if lam is None else np.clip(np.asarray(lam, np.float64), *BOUNDS)
    for row in munc:
        inv = 1.0 / np.maximum(np.asarray(row, np.float64) + PAD, 1.0e-8)
        if prec is not None:
            inv *= prec
        w += inv
    pos = w[np.isfinite(w) & (w > 0.0)]
    scale = float(np.median(pos)) if pos.size else 1.0
    if not np.isfinite(scale) or scale <= 0.0:
        scale = 1.0
    return scale, np.sort(pos)


def _expected(p, *, use_lambda=True, use_kappa=True, nonneg=True, mult=MULT, have_bg=True):
    """Per field: (twin value, exact value, number of terms); plus the weight median and the count."""
    from oracle import driver as odrv

    bg = p["bg"] if have_bg else np.zeros(p["n"], np.float32)
    lam = p["lam"] if use_lambda else None
    cfg = dict(nu=NU, use_lambda=use_lambda, use_kappa=use_kappa, penalties=(LAM_FIRST, LAM_SECOND), neg_multiplier=mult,
               use_nonnegative=nonneg, lambda_bounds=BOUNDS, pad=PAD)
    with np.errstate(all="ignore"):
        twin = odrv.penalized_objective(0.0, p["munc"], bg, lam, p["kap"], cfg)
        n, b64 = p["n"], np.asarray(bg, np.float64)
        active = bool(nonneg and mult is not None and mult > 0.0)
        median, pos = _weight_track(p["munc"], lam) if active else (1.0, None)
        exact = {}
        v = np.maximum(np.asarray(p["lam"], np.float64), TINY)
        exact["robust_observation_penalty"] = 0.5 * NU * _fsum(v - np.log(v)) if use_lambda else 0.0
        v = np.maximum(np.asarray(p["kap"], np.float64), TINY)
        v = v[1:] if v.size > 1 else v
        exact["robust_process_penalty"] = 0.5 * NU * _fsum(v - np.log(v)) if use_kappa else 0.0
        exact["first_difference_penalty"] = 0.5 * LAM_FIRST * _fsum(np.diff(b64) ** 2)
        exact["second_difference_penalty"] = 0.5 * LAM_SECOND * _fsum(np.diff(b64, n=2) ** 2)
        neg_terms = np.minimum(b64, 0.0) ** 2
        exact["negative_penalty"] = 0.5 * (mult * median) * _fsum(neg_terms) if active else 0.0
        terms = {"robust_observation_penalty": n, "robust_process_penalty": max(n - 1, 1), "first_difference_penalty": n - 1,
                 "second_difference_penalty": n - 2, "negative_penalty": n}
        if active:      # the median restated here IS the twin's: the same expression gives the same bits
            assert twin["background_negative_penalty"] == 0.5 * float(mult * median) * float(np.sum(neg_terms, dtype=np.float64))
    return {"twin": twin, "exact": exact, "terms": terms, "weight_median": median, "pos": pos,
            "count": twin["effective_observation_count"]}


def _gate(value, exact, nterms, what):
    """|value - exact| / ((n + 8) 2^-52 |exact|); exact zeros and NaN are compared as such."""
    if math.isnan(exact):
        assert math.isnan(value), what
        return 0.0
    if exact == 0.0:
        assert value == 0.0, what
        return 0.0
    ratio = abs(value - exact) / ((nterms + 8) * 2.0 ** -52 * abs(exact))
    assert ratio <= 1.0, (what, value, exact, ratio)
    return ratio


def _check_terms(got, exp, what):
    for f in FIELDS:
        twin = exp["twin"][TWIN_KEY[f]]
        if math.isnan(twin):        # where the twin returns NaN the device does
            assert math.isnan(got[f]), (what, f, got[f])
            continue
        _gate(twin, exp["exact"][f], exp["terms"][f], (what, f, "twin"))
        r = _gate(got[f], exp["exact"][f], exp["terms"][f], (what, f, "device"))
        WORST[f] = max(WORST.get(f, 0.0), r)
    assert got["weight_median"] == exp["weight_median"], (what, got["weight_median"], exp["weight_median"])
    assert got["effective_observation_count"] == exp["count"], what


def _terms(b, **kw):
    args = dict(use_lambda_penalty=True, use_kappa_penalty=True, use_lambda_weights=True, use_nonnegative=True)
    args.update(kw)
    mult = args.pop("mult", MULT)
    return b.objective_terms(NU, LAM_FIRST, LAM_SECOND, mult, pad=PAD, **args)


# ---- objective_terms -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["main", "small"])
def test_every_objective_term_at_every_record_and_fold_shape(product, planted, which):
    """All seven fields per chain with every term on (lambda and kappa penalties, lambda weights, non-negative multiplier 2),
    no fit resident, on planted multipliers (0, -1, 1e-40, a huge kappa[0], kappa = 0), a background with a negative stretch and
    exact zeros and variance cells 1e30 / NaN / +-inf / -pad, against the twin and the exact sums."""
    lens, m, plants = planted[which]
    with _open(lens, m, plants) as b:
        got = _terms(b)
    for c, p in enumerate(plants):
        exp = _expected(p)
        _check_terms(got[c], exp, (which, c, p["n"]))
        if p["n"] > 1:          # the huge kappa[0] did not count
            assert got[c]["robust_process_penalty"] < 1.0e20, (which, c)
        else:
            assert got[c]["robust_process_penalty"] > 1.0e29 and got[c]["first_difference_penalty"] == 0.0
        if p["n"] < 3:
            assert got[c]["second_difference_penalty"] == 0.0
        assert got[c]["negative_penalty"] > 0.0


@pytest.mark.parametrize("which", ["main", "small"])
def test_objective_flag_paths(product, planted, which):
    """Kappa penalty alone (no lambda anywhere: weights without lambda); the negative part switched off by the flag and by a
    multiplier of None / 0 / NaN (penalty 0.0, weight_median at its fallback 1.0); a context whose background was never set
    (roughness and negative terms exactly 0.0, the rest what it is with a background)."""
    lens, m, plants = planted[which]
    with _open(lens, m, plants) as b:
        full = _terms(b)
        kap_only = _terms(b, use_lambda_penalty=False, use_lambda_weights=False)
        off = [_terms(b, use_nonnegative=False)] + [_terms(b, mult=v) for v in (None, 0.0, float("nan"))]
    for c, p in enumerate(plants):
        assert kap_only[c]["robust_observation_penalty"] == 0.0
        _check_terms(kap_only[c], _expected(p, use_lambda=False), (which, "kappa only", c))
        exp_off = _expected(p, nonneg=False)
        for i, run in enumerate(off):
            assert run[c]["negative_penalty"] == 0.0 and run[c]["weight_median"] == 1.0, (which, i, c)
            _check_terms(run[c], exp_off, (which, "negative part off", i, c))
    with _open(lens, m, plants, background=False) as b:
        bare = _terms(b)
    for c, p in enumerate(plants):
        for f in ("first_difference_penalty", "second_difference_penalty", "negative_penalty"):
            assert bare[c][f] == 0.0, (which, c, f)
        for f in ("robust_observation_penalty", "robust_process_penalty", "weight_median", "effective_observation_count"):
            assert bare[c][f] == full[c][f], (which, c, f)
        _check_terms(bare[c], _expected(p, have_bg=False), (which, "no background", c))


def test_weight_median_edges(product):
    """Even and odd counts of positive weights (2, 3, 64, 65 bins), a long run of identical weights around the middle (both middle
    order statistics equal), a chain of 1e30 cells only (count max(1, 0) = 1, a tiny positive median) and a chain of +inf
    variances only (no positive weight: the fallback 1.0)."""
    lens, m = [300, 2, 65, 70, 64, 3, 70], 3
    plants = _plants(lens, m, 300, dirty=False)
    run = plants[0]
    run["munc"][:, 50:250] = np.float32(0.5)
    run["lam"][50:250] = np.float32(1.0)
    plants[3]["munc"][:] = np.float32(1.0e30)
    plants[6]["munc"][:] = np.inf
    with _open(lens, m, plants) as b:
        got = _terms(b)
    for c, p in enumerate(plants):
        exp = _expected(p)
        _check_terms(got[c], exp, ("median", c, p["n"]))
        if c not in (3, 6):
            assert exp["pos"].size == p["n"]            # every weight positive: even and odd counts as listed
    pos = _expected(run)["pos"]
    assert pos[149] == pos[150] == got[0]["weight_median"] and pos[40] < pos[149] < pos[260]
    assert got[3]["effective_observation_count"] == 1 and 0.0 < got[3]["weight_median"] < 1.0e-29
    assert got[3]["negative_penalty"] > 0.0
    assert got[6]["effective_observation_count"] == 1 and got[6]["weight_median"] == 1.0


def test_non_finite_multipliers_reach_the_objective(product, planted):
    """np.maximum(x, tiny) of the reference propagates NaN (core.py:3172, 3175): a NaN in lambda / kappa makes that chain's penalty
    NaN, as in the twin -- `run_consenrich_batch` then never finds such a pass objective-stable (math.isfinite(cur)), like the
    reference.  Every other chain of the batch keeps its value bit for bit."""
    lens, m, plants = planted["main"]
    c_lam, c_kap = lens.index(2049), lens.index(4097)
    bad = [dict(p) for p in plants]
    bad[c_lam]["lam"] = plants[c_lam]["lam"].copy()
    bad[c_lam]["lam"][100] = np.nan
    bad[c_kap]["kap"] = plants[c_kap]["kap"].copy()
    bad[c_kap]["kap"][200] = np.nan
    with _open(lens, m, plants) as b:
        before = _terms(b)
        b.upload_multipliers(c_lam, bad[c_lam]["lam"], bad[c_lam]["kap"], None)
        b.upload_multipliers(c_kap, bad[c_kap]["lam"], bad[c_kap]["kap"], None)
        got = _terms(b)
    exp_lam, exp_kap = _expected(bad[c_lam]), _expected(bad[c_kap])
    assert math.isnan(exp_lam["twin"]["robust_observation_penalty"]) and math.isnan(exp_kap["twin"]["robust_process_penalty"])
    assert math.isnan(got[c_lam]["robust_observation_penalty"]), got[c_lam]
    assert math.isnan(got[c_kap]["robust_process_penalty"]), got[c_kap]
    _check_terms(got[c_lam], exp_lam, "NaN in lambda")
    _check_terms(got[c_kap], exp_kap, "NaN in kappa")
    for c in range(len(lens)):
        if c not in (c_lam, c_kap):
            assert got[c] == before[c], c


def test_objective_terms_disturb_nothing(product):
    """background_update -> objective_terms -> background_update on one context: the second update returns what the first did, bit
    for bit (the two calls share the per-chain sums, the selection answers and the rank buffer); two objective_terms calls in a row
    return equal dicts."""
    lens, m = [2049, 1, 131073, 65, 3], 3
    plants = _plants(lens, m, 500, dirty=False)
    kw = dict(use_nonnegative=True, negative_penalty_multiplier=MULT, use_initial=True, zero_state=True)
    with _open(lens, m, plants) as b:
        u1 = b.background_update(1800.0, 1.62e6, **kw)
        n1 = [b.download(c, "background_next") for c in range(len(lens))]
        t1 = _terms(b)
        t2 = _terms(b)
        u2 = b.background_update(1800.0, 1.62e6, **kw)
        n2 = [b.download(c, "background_next") for c in range(len(lens))]
    assert t1 == t2
    assert u1 == u2
    for c in range(len(lens)):
        assert np.array_equal(n1[c], n2[c]), c
        _check_terms(t1[c], _expected(plants[c]), ("between updates", c))


# ---- the RMS triple of background_update -----------------------------------------------------------------------------
def _check_rms(info, p, level, proposal, what):
    """shift / proposal / reference RMS of one chain against `oracle.driver.background_shift_gate` and the exact sums, from the
    host's rebuild of the weight track, the device's OWN proposal and the planted background."""
    from consenrich_amd import _lib as L
    from oracle import background as bgo
    from oracle import driver as odrv

    n = p["n"]
    w, _, _, _ = bgo.weight_rhs_tracks(p["data"], p["munc"], level, np.float32(PAD))
    assert info["status"] == L.BG_OK and info["support"] == int(np.count_nonzero(w > 0.0)), what
    assert info["weight_scale"] == float(np.median(w[w > 0.0])), what
    twin = odrv.background_shift_gate(w, proposal, p["bg"], 0.05)
    g1, g0 = np.asarray(proposal, np.float64), np.asarray(p["bg"], np.float64)
    sw = _fsum(w)
    for key, tkey, sq in (("shift_rms", "background_shift", (g1 - g0) ** 2), ("proposal_rms", "proposal_rms", g1 * g1),
                          ("reference_rms", "reference_rms", g0 * g0)):
        exact = math.sqrt(_fsum(w * sq) / sw)
        _gate(twin[tkey], exact, n, (what, key, "twin"))
        r = _gate(info[key], exact, n, (what, key, "device"))
        WORST[key] = max(WORST.get(key, 0.0), r)
    assert info["reference_rms"] > 0.0 and info["shift_rms"] != info["proposal_rms"], what


@pytest.mark.parametrize("level", ["zero_state", "resident_fit"])
def test_rms_triple_against_the_host_restatement(product, level):
    """A non-zero current background with a negative part on every chain; the level is zero (warm start, no fit) or the smoothed
    level of a resident fit.  The three RMS values are checked against the device's own proposal, so the solve's accuracy does not
    enter, and reference_rms > 0 and shift != proposal keep the test off the zero-background shortcut."""
    from consenrich_amd import _lib as L

    lens, m = RMS_LENS, 3
    plants = _plants(lens, m, 700, dirty=False)
    with _open(lens, m, plants) as b:
        if level == "resident_fit":
            b.stats()
            b.forward_backward(L.RETURN_NLL)
            b.export(L.EXPORT_SMOOTH)
            levels = [b.download(c, "xs")[:, 0].copy() for c in range(len(lens))]
        else:
            levels = [np.zeros(n, np.float32) for n in lens]
        info = b.background_update(1800.0, 1.62e6, use_nonnegative=True, negative_penalty_multiplier=MULT, use_initial=True,
                                   zero_state=level == "zero_state")
        nxt = [b.download(c, "background_next") for c in range(len(lens))]
    for c, p in enumerate(plants):
        assert (p["bg"] < 0).any()
        _check_rms(info[c], p, levels[c], nxt[c], (level, c, p["n"]))


def test_chain_without_support_inside_a_batch(product):
    """A chain whose every variance is +inf between ordinary chains (zero_state only: no filter kernel sees the infinite
    variances): nothing raises, the chain reports BG_NO_SUPPORT, support 0, an all-zero proposal (core.py:8150-8151) and 0.0 for
    the three RMS values; its neighbours are unaffected.

    The reference's driver would raise "shift RMS requires positive weights" for such a chain (core.py:5204);
    `run_consenrich_batch` does not: it takes the three zeros as a stable shift."""
    from consenrich_amd import _lib as L

    lens, m = [2049, 100, 65], 3
    plants = _plants(lens, m, 800, dirty=False)
    plants[1]["munc"][:] = np.inf
    with _open(lens, m, plants) as b:
        info = b.background_update(1800.0, 1.62e6, use_nonnegative=True, negative_penalty_multiplier=MULT, use_initial=True,
                                   zero_state=True, raise_on_error=True)
        nxt = [b.download(c, "background_next") for c in range(len(lens))]
    assert info[1]["status"] == L.BG_NO_SUPPORT and info[1]["support"] == 0
    assert not nxt[1].any()
    assert info[1]["shift_rms"] == 0.0 and info[1]["proposal_rms"] == 0.0 and info[1]["reference_rms"] == 0.0
    for c in (0, 2):
        _check_rms(info[c], plants[c], np.zeros(lens[c], np.float32), nxt[c], ("beside a chain without support", c))
