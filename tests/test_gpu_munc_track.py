"""From the seed loop to a finished `matrixMunc` on the device: the drop-ins (`cEvalPSplineLogVarianceTrend`,
`cFinalizeMuncEBTrack`, `munc_track.get_munc_track`, `apply_blacklist_munc_floor`, `munc_track.block_sums`) against the compiled
reference's fixtures and the twin (tests/twin_munc_track.py), and the resident route `munc_seed_batch -> munc_track_batch ->
forward_backward`.

Bit for bit: the valid counts, sum q, sum q * evidence, sum q * q, the finalisation with its counters and invalid indices, the
blacklist floor and the clamp.  Through the device's exp: every value of a prior track (and of a track composed on it) within one
float32 ulp of the reference's and at most 0.1 % of a case's values different at all.  Through the device's log1p: sum q * predictor,
|device - twin| / sum q |predictor| gated at ten times the worst ratio measured on these cases on the first GPU run
(profiles/munc_track_parity.json) and never looser than 1e-12.  With MUNC_TRACK_PARITY_OUT set, the measured values are also
written to that file."""
import json
import os

import numpy as np
import pytest

import munc_cases as SC
import munc_track_cases as MC
import twin_munc_track as T

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "munc_track")
PARITY = os.path.join(ROOT, "profiles", "munc_track_parity.json")
DIAG = ("supportCount", "supportFraction", "countFloorFiniteCount", "countFloorAddedCount", "countFloorMissingCount",
        "finalShrinkagePairCount", "finalShrinkagePairFraction")
QP_STANDING = 1.0e-12


@pytest.fixture(scope="module")
def dev():
    from consenrich_amd import _lib, munc_track

    _lib.require_gpu()
    return munc_track


@pytest.fixture(scope="module")
def gold():
    g = {}
    for group in ("eval", "final", "tracks", "blacklist"):
        with np.load(os.path.join(GOLD, f"munc_track_{group}.npz")) as z:
            g[group] = {k: z[k] for k in z.files}
    return g


@pytest.fixture(scope="module")
def parity():
    with open(PARITY) as fh:
        return json.load(fh)


def record(key, value):
    out = os.environ.get("MUNC_TRACK_PARITY_OUT")
    if not out:
        return
    rec = {}
    if os.path.exists(out):
        with open(out) as fh:
            rec = json.load(fh)
    rec[key] = max(float(value), rec.get(key, 0.0))
    with open(out, "w") as fh:
        json.dump(rec, fh, indent=1, sort_keys=True)


def within_one_ulp(name, got, want):
    """The two bounds of a track that passed through the device's exp; returns (worst ulp distance, share that differs)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float32 and got.shape == want.shape, name
    if got.size == 0:
        return 0, 0.0
    assert np.all(np.isfinite(got)), name
    dist = MC.ulp_distance(got, want)
    worst, share = int(dist.max()), float(np.count_nonzero(dist)) / got.size
    print(f"munc track parity {name}: worst {worst} ulp, {share:.6f} of {got.size} values differ")
    assert worst <= 1, (name, worst)
    assert share <= 1.0e-3, (name, share)
    return worst, share


# -- prior track -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", MC.EVAL_CASES, ids=[c[0] for c in MC.EVAL_CASES])
def test_trend_dropin_against_the_reference(dev, gold, case):
    trend, mean, eps, cap = MC.eval_inputs(case)
    lo, hi = T.log_bounds(eps, cap)
    got = dev.cEvalPSplineLogVarianceTrend(MC.eval_predictor(case, T), trend[0], trend[1], trend[2], trend[3], trend[4], lo, hi)
    worst, share = within_one_ulp(case[0], got, gold["eval"][f"{case[0]}/out"])
    got_mean = dev.eval_pspline_log_variance_trend(trend, mean, eps=eps, maxVariance=cap)
    w2, s2 = within_one_ulp(case[0] + "/mean", got_mean, gold["eval"][f"{case[0]}/mean/out"])
    record("prior_worst_ulp", max(worst, w2))
    record("prior_worst_share", max(share, s2))
    if case[0].startswith("const_"):        # the constant fallback is the C library's exp: every bit
        assert MC.same(got, gold["eval"][f"{case[0]}/out"])


def test_trend_limits_are_value_errors(dev):
    p = np.zeros(4)
    for trend, text in (((np.zeros(20), np.zeros(8), 6, 0.0, 1.0), "degree 6"), ((np.zeros(700), np.zeros(600), 3, 0.0, 1.0), "600 basis"),
                        ((np.zeros(9), np.zeros(8), 3, 0.0, 1.0), "do not describe")):
        with pytest.raises(ValueError, match=text):
            dev.cEvalPSplineLogVarianceTrend(p, trend[0], trend[1], trend[2], trend[3], trend[4], -10.0, 10.0)
    big = MC.make_trend(5, 512, 31)         # the largest the device takes
    pred = T.predictor(MC.mean_track(257, 32))
    lo, hi = T.log_bounds(1.0e-6, None)
    within_one_ulp("deg5_b512", dev.cEvalPSplineLogVarianceTrend(pred, big[0], big[1], big[2], big[3], big[4], lo, hi),
                   T.cEvalPSplineLogVarianceTrend(pred, big[0], big[1], big[2], big[3], big[4], lo, hi))


# -- finalisation ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", MC.FINAL_CASES, ids=[c[0] for c in MC.FINAL_CASES])
@pytest.mark.parametrize("eb", (True, False), ids=("eb", "noeb"))
def test_finalisation_dropin_equals_the_reference(dev, gold, case, eb):
    local, prior, floor, kw = MC.final_inputs(case)
    out, diag = dev.cFinalizeMuncEBTrack(local, prior if eb else None, floor, useEB=eb, **kw)
    key = f"{case[0]}/{'eb' if eb else 'noeb'}"
    assert MC.same(gold["final"][f"{key}/out"], out)
    assert MC.same(gold["final"][f"{key}/diag"], np.asarray([float(diag[k]) for k in DIAG]))
    assert all(type(diag[k]) is (float if "Fraction" in k else int) for k in DIAG)


def test_finalisation_error_texts(dev):
    for name, a, k, text in MC.final_error_cases():
        with pytest.raises(ValueError) as e:
            dev.cFinalizeMuncEBTrack(*a, **k)
        assert str(e.value) == text, name


@pytest.mark.parametrize("case", MC.TRACK_CASES, ids=[c[0] for c in MC.TRACK_CASES])
def test_get_munc_track_against_the_reference(dev, gold, case):
    a = MC.track_inputs(case)
    n = a["local"].shape[0]
    out, support = dev.get_munc_track("chrT", np.arange(n) * 200, np.zeros(n, np.float32), 200, EB_use=a["use_eb"], eps=a["floor"],
                                      varianceFloor=a["floor"], varianceCap=a["cap"], pooledTrend=a["trend"],
                                      priorMeanTrack=a["prior_mean"], priorVarianceTrack=a["prior_variance"],
                                      replicateVarianceFactor=a["factor"], EB_pooledNu0=a["nu0"], EB_effectiveNuL=a["nuL"],
                                      countModelVarianceFloor=a["count_floor"], localVarianceTrack=a["local"])
    assert MC.same(gold["tracks"][f"{case[0]}/support"], np.float64(support))
    if a["prior_variance"] is not None or not a["use_eb"]:
        assert MC.same(gold["tracks"][f"{case[0]}/out"], out)          # no exp on the way: every bit
    else:
        worst, share = within_one_ulp(case[0], out, gold["tracks"][f"{case[0]}/out"])
        record("composed_worst_ulp", worst)
        record("composed_worst_share", share)


def test_get_munc_track_branches_that_raise(dev):
    local = np.ones(5, np.float32)
    iv, vals = np.arange(5) * 200, np.zeros(5, np.float32)
    kw = dict(intervalSizeBP=200, localVarianceTrack=local, eps=1.0e-6, priorMeanTrack=vals)
    trend = MC.make_trend(3, 8, 1)
    for extra, text in ((dict(numNearest=3), "sparse-nearest MUNC is not supported by kalman MUNC"),
                        (dict(sparseIntervalIndices=np.arange(2)), "sparse-nearest MUNC is not supported by kalman MUNC"),
                        (dict(restrictLocalVarianceToSparseBed=True), "restrictLocalVarianceToSparseBed is not supported by kalman MUNC"),
                        (dict(), "kalman MUNC EB requires a pooled MUNC trend"),
                        (dict(pooledTrend=trend, EB_pooledNu0=40.0, EB_effectiveNuL=3.0), "EB_effectiveNuL must be finite and at least 4.0")):
        with pytest.raises(ValueError) as e:
            dev.get_munc_track("chrT", iv, vals, **dict(kw, **extra))
        assert str(e.value) == text
    with pytest.raises(NotImplementedError):
        dev.get_munc_track("chrT", iv, vals, **dict(kw, pooledTrend=trend, EB_pooledNu0=40.0, EB_effectiveNuL=8.0,
                                                  additiveCovariateModel=object(), covariateTrack=vals))
    with pytest.raises(NotImplementedError):
        dev.get_munc_track("chrT", iv, vals, **dict(kw, pooledTrend=trend, EB_effectiveNuL=8.0))     # Nu_0 would be estimated


@pytest.mark.parametrize("case", MC.BLACKLIST_CASES, ids=[c[0] for c in MC.BLACKLIST_CASES])
def test_blacklist_floor_dropin_equals_the_reference(dev, gold, case):
    x, mask, q = MC.blacklist_inputs(case)
    floors = dev.apply_blacklist_munc_floor(x, mask, 1.0e-12, q)
    assert MC.same(gold["blacklist"][f"{case[0]}/floors"], floors)
    assert MC.same(gold["blacklist"][f"{case[0]}/out"], x)


def test_blacklist_floor_with_cells_that_are_not_finite(dev):
    x, mask, q = MC.blacklist_inputs(MC.BLACKLIST_CASES[2])
    idx0, idx1 = np.flatnonzero(mask == 0)[:2]
    x[0, idx0], x[1, idx1] = np.nan, np.inf
    x[2, np.flatnonzero(mask)[0]] = np.nan
    want = x.copy()
    fw = T.apply_blacklist_munc_floor(want, mask, 0.05, q)
    fg = dev.apply_blacklist_munc_floor(x, mask, 0.05, q)
    assert MC.same(fw, fg) and MC.same(want, x)


# -- block sums --------------------------------------------------------------------------------------------------------------------
def check_sums(name, got, want_raw):
    """The bit-for-bit fields, and the ratio of the one that passes through log1p."""
    for key in ("valid", "q", "qe", "qq", "included", "starts", "ends"):
        assert MC.same(want_raw[key], got[key]), (name, key)
    scale = want_raw["abs_qp"]
    diff = np.abs(got["qp"] - want_raw["qp"])
    assert np.all(diff[scale == 0.0] == 0.0), name
    ratio = float(np.max(diff[scale > 0.0] / scale[scale > 0.0])) if np.any(scale > 0.0) else 0.0
    print(f"munc track parity {name}: sum q*predictor worst ratio {ratio:.3e}")
    return ratio


def twin_sums(ev, w, ex, mean, block_len):
    raw = T.block_loop(ev, w, ex, mean, block_len)["raw"]
    # the scale of the gate: sum q |predictor| over the same cells
    pred = T.predictor(mean)
    raw["abs_qp"] = T.block_loop(ev, w, ex, mean, block_len, pred=np.abs(pred))["raw"]["qp"]
    return raw


@pytest.mark.parametrize("block_len,m", [(2, 1), (7, 3), (8, 17), (9, 3), (128, 1), (129, 3), (257, 17), (600, 3)])
def test_block_sums_on_host_arrays(dev, parity, block_len, m):
    """Block lengths on the edges of NumPy's three summation regimes (and one staged by a single wavefront per workgroup), a
    dropped last block of length 1 and a kept one of length 2, an all-excluded block, an all-zero-weight block, a NaN and an
    infinite mean."""
    worst = 0.0
    for n in (5 * block_len + 1, 3 * block_len + 2):
        ev, w, ex, mean = MC.block_chain(m, n, 800 + n, block_len)
        got = dev.block_sums(ev, w, ex, mean, block_len)
        want = twin_sums(ev, w, ex, mean, block_len)
        assert got["starts"].size == (5 if n == 5 * block_len + 1 else 4)
        worst = max(worst, check_sums(f"L{block_len}_m{m}_n{n}", got, want))
        assert np.all(got["valid"][:, 0] == 0) and got["included"][0] == 0
    record("block_qp_worst_ratio", worst)
    gate = min(10.0 * parity["measured"]["block_qp_worst_ratio"], QP_STANDING)
    assert worst <= gate, (worst, gate)


def test_block_sums_without_a_mask_and_beyond_the_staged_length(dev):
    ev, w, _ex, mean = MC.block_chain(3, 100, 5, 9)
    got = dev.block_sums(ev, w, None, mean, 9)
    want = twin_sums(ev, w, np.zeros(100, np.uint8), mean, 9)
    check_sums("no_mask", got, want)
    with pytest.raises(ValueError, match="blocks of up to 2048"):
        dev.block_sums(ev, w, None, mean, 2049)


# -- the resident route ------------------------------------------------------------------------------------------------------------
LENS = (300, 2 * SC.ROLL_BLOCK + 1 + 64, 65)
M, PAD, WINDOW, BLOCK = 3, 1.0e-4, 9, 8
Q2 = np.array([[1.0e-3, 0.0], [0.0, 1.0e-4]], np.float32)
TREND = MC.make_trend(3, 24, 77, x_min=-1.5, x_max=2.5)
FIT = dict(trend=TREND, replicate_factors=[1.0, 1.3, 1.0 + 5.0e-9], nu0=[1.0e4, 40.0, 12.0], nuL=7.3)
FLOOR, CAP = 1.0e-3 / 3.0, 3.0


def chain_inputs(k, n):
    (data, munc, _l, _v), kw = SC.seed_inputs(dict(m=M, n=n, seed=9300 + k, opt=("floor",)))
    rng = np.random.default_rng(9400 + k)
    raw = kw["countFloor"].astype(np.float32).copy()
    raw[rng.random(raw.shape) < 0.2] = np.nan
    raw[rng.random(raw.shape) < 0.1] = 0.0
    excl = (rng.random(n) < 0.15).astype(np.uint8)
    return data, munc, raw, excl


@pytest.fixture(scope="module")
def seeded():
    """One batch after `munc_seed_batch` (three chains, the last one left out), its downloads, and the result of
    `munc_track_batch` with a planted fit -- shared by the tests below, which only read it."""
    from consenrich_amd import _lib, driver
    from consenrich_amd.batch import DeviceBatch, ModelParams

    _lib.require_gpu()
    chains = [chain_inputs(k, n) for k, n in enumerate(LENS)]
    take = [True, True, False]
    with DeviceBatch() as b:
        b.configure(ModelParams(), M, LENS)
        for c, ch in enumerate(chains):
            b.upload(c, ch[0], ch[1])
        driver.munc_seed_batch(b, pad=PAD, window=WINDOW, passes=1, count_floor=[ch[2] for ch in chains],
                               exclude=[ch[3] for ch in chains], chains=take, fit_background=False, q=[Q2] * len(LENS), fetch=())
        before = {c: dict(smooth=b.download_munc_seed(c, "seed_smooth"), weight=b.download_munc_seed(c, "seed_weight"),
                          exclude=b.download_munc_seed(c, "seed_exclude"), mean=b.download(c, "xs")[:, 0].copy(),
                          munc=b.download_inputs(c)[1].copy()) for c in range(len(LENS))}
        sums = b.munc_block_sums(BLOCK, chains=take)
        calls = []
        originals = {name: getattr(DeviceBatch, name) for name in ("download", "download_munc_seed", "download_inputs")}

        def counting(name):
            def wrapped(self, *a, **k):
                calls.append(name)
                return originals[name](self, *a, **k)
            return wrapped

        try:
            for name in originals:
                setattr(DeviceBatch, name, counting(name))
            seen = {}

            def fit_trend(pooled):
                seen["pooled"] = pooled
                return FIT

            done = driver.munc_track_batch(b, block_intervals=BLOCK, fit_trend=fit_trend, dependence_multiplier=2.0,
                                           trigamma=MC.planted_trigamma, count_floor=[ch[2] for ch in chains], floor=FLOOR, cap=CAP,
                                           chains=take)
        finally:
            for name, fn in originals.items():
                setattr(DeviceBatch, name, fn)
        after = {c: b.download_inputs(c)[1].copy() for c in range(len(LENS))}
        prior = {c: b.download_munc_seed(c, "seed_prior") for c in (0, 1)}
        gone = None
        try:
            b.munc_block_sums(BLOCK, chains=take)
        except _lib.ConsenrichAMDError as e:
            gone = str(e)
        b.stats()
        nll = b.forward_backward(want_sums=False)
        level = b.download(0, "xs")[:, 0].copy()
    return dict(chains=chains, take=take, before=before, sums=sums, calls=calls, done=done, pooled=seen["pooled"], after=after,
                prior=prior, gone=gone, nll=nll, level=level)


def test_resident_block_sums_equal_the_twin_on_the_downloads(seeded, parity):
    worst = 0.0
    assert seeded["sums"][2] is None
    for c in (0, 1):
        d = seeded["before"][c]
        want = twin_sums(d["smooth"], d["weight"], d["exclude"], d["mean"].astype(np.float64), BLOCK)
        assert want["starts"].size > 4          # more blocks than one workgroup of the launch takes
        worst = max(worst, check_sums(f"resident_chain{c}", seeded["sums"][c], want))
        assert int(np.sum(want["valid"])) > 0
    record("block_qp_worst_ratio", worst)
    assert worst <= min(10.0 * parity["measured"]["block_qp_worst_ratio"], QP_STANDING)


def test_resident_route_pools_the_rows_of_the_taken_chains(seeded):
    from consenrich_amd import munc_track as MT

    want = MT.pooled_block_rows(seeded["sums"], dependence_multiplier=2.0, trigamma=MC.planted_trigamma)
    got = seeded["pooled"]
    for key in ("means", "variances", "log_variance_noise", "sample_index", "chrom_index", "block_starts", "trend_weights"):
        assert MC.same(want[key], got[key]), key
    assert got["row_counts"][2] == 0 and got["row_counts"][0] > 0 and set(got["chrom_index"].tolist()) == {0, 1}
    loops = [T.block_loop(d["smooth"], d["weight"], d["exclude"], d["mean"].astype(np.float64), BLOCK) for d in
             (seeded["before"][0], seeded["before"][1])]
    twin = T.pooled_rows(loops + [None], MC.planted_trigamma)
    for key in ("variances", "log_variance_noise", "sample_index", "chrom_index", "block_starts", "trend_weights"):
        assert MC.same(twin[key], got[key]), key
    assert np.allclose(twin["means"], got["means"], rtol=1.0e-12, atol=1.0e-12)


def test_resident_route_leaves_the_finished_matrix_in_the_batch(seeded):
    """Against the twin on the downloaded local evidence, mean track, mask and raw floor: bit for bit on the device's own prior
    track, within the two bounds of a composed track on the twin's; the diagnostics and the blacklist floors likewise."""
    assert seeded["calls"] == []                # no download between the seed loop and the finished matrix
    worst = share = 0
    for c in (0, 1):
        d, raw = seeded["before"][c], seeded["chains"][c][2]
        got = seeded["after"][c]
        own, diags, floors = T.finished_matrix(d["smooth"], d["mean"], d["exclude"], raw, TREND, FIT["replicate_factors"], FIT["nu0"],
                                               FIT["nuL"], FLOOR, CAP, prior=seeded["prior"][c])
        assert MC.same(own, got)
        assert MC.same(floors, seeded["done"]["floors"][c])
        for j in range(M):
            assert seeded["done"]["diagnostics"][c][j] == diags[j], (c, j)
        within_one_ulp(f"resident_prior_chain{c}", seeded["prior"][c],
                       T.eval_pspline_log_variance_trend(TREND, d["mean"], eps=FLOOR, maxVariance=CAP))
        ref, _, ref_floors = T.finished_matrix(d["smooth"], d["mean"], d["exclude"], raw, TREND, FIT["replicate_factors"], FIT["nu0"],
                                               FIT["nuL"], FLOOR, CAP)
        w, s = within_one_ulp(f"resident_chain{c}", got, ref)
        worst, share = max(worst, w), max(share, s)
        assert np.all(floors > 1.0e-12) and np.all(got[:, d["exclude"] != 0] >= floors.astype(np.float32)[:, None])
        assert np.all(got >= np.float32(1.0e-12)) and np.all(got <= np.float32(CAP))
    record("composed_worst_ulp", worst)
    record("composed_worst_share", share)
    assert MC.same(seeded["after"][2], seeded["before"][2]["munc"])        # a chain left out keeps its munc
    assert seeded["done"]["diagnostics"][2] is None and seeded["done"]["floors"][2] is None


def test_resident_route_drops_the_fit_and_the_next_fit_runs(seeded):
    assert seeded["gone"] is not None and "no smoothed results" in seeded["gone"]
    assert np.all(np.isfinite(seeded["level"])) and seeded["level"].shape == (LENS[0],)


def small_batch():
    from consenrich_amd import driver
    from consenrich_amd.batch import DeviceBatch, ModelParams

    lens = (65, 130)
    chains = [chain_inputs(k + 5, n) for k, n in enumerate(lens)]
    b = DeviceBatch()
    b.configure(ModelParams(), M, lens)
    for c, ch in enumerate(chains):
        b.upload(c, ch[0], ch[1])
    driver.munc_seed_batch(b, pad=PAD, window=WINDOW, passes=0, exclude=[ch[3] for ch in chains], fit_background=False,
                           q=[Q2] * len(lens), fetch=())
    return b, lens, chains


def test_resident_finalisation_on_planted_arrays():
    """Planted local evidence, prior track and raw floor through `munc_track_finish`: the no-EB branch, a floor without a finite
    entry, the errors in the reference's order with the lowest index of a track, and a batch that is left as it was."""
    b, lens, chains = small_batch()
    with b:
        rng = np.random.default_rng(3)
        local = [rng.gamma(2.0, 0.3, (M, n)).astype(np.float32) for n in lens]
        prior = [rng.gamma(2.0, 0.25, n).astype(np.float32) for n in lens]
        floors = [np.full((M, n), np.nan, np.float32) for n in lens]
        floors[1][1, ::3] = 0.25
        floors[1][2, 5] = np.inf
        for c in range(2):
            b.munc_seed_upload(c, "seed_smooth", local[c])
            b.munc_seed_upload(c, "seed_prior", prior[c])
        assert MC.same(b.download_munc_seed(1, "seed_prior"), prior[1])
        munc0 = [b.download_inputs(c)[1].copy() for c in range(2)]
        excl = [ch[3] for ch in chains]
        # errors: the second chain's second sample holds the first invalid cells
        bad = local[1].copy()
        bad[1, 100], bad[1, 40], bad[2, 3] = 0.0, np.nan, -1.0
        b.munc_seed_upload(1, "seed_smooth", bad)
        with pytest.raises(ValueError) as e:
            b.munc_track_finish(8.0, 40.0, floor=1.0e-6)
        assert str(e.value) == "localVarianceTrack must contain finite positive values at index 40"
        b.munc_seed_upload(1, "seed_smooth", local[1])
        badp = prior[0].copy()
        badp[64], badp[7] = np.inf, 0.0
        b.munc_seed_upload(0, "seed_prior", badp)
        with pytest.raises(ValueError) as e:
            b.munc_track_finish(8.0, 40.0, floor=1.0e-6)
        assert str(e.value) == "localVarianceTrack must contain finite positive values at index 7"      # (as getMuncTrack passes it)
        b.munc_track_finish(8.0, 40.0, floor=1.0e-6, use_eb=False, chains=[False, True])               # no prior needed without EB
        assert MC.same(b.download_inputs(0)[1], munc0[0])
        b.munc_seed_upload(0, "seed_prior", prior[0])
        negf = [f.copy() for f in floors]
        negf[0][2, 11] = -0.5
        with pytest.raises(ValueError) as e:
            b.munc_track_finish(8.0, 40.0, count_floor=negf, floor=1.0e-6)
        assert str(e.value) == "countModelVarianceFloor must be nonnegative where finite"
        assert MC.same(b.download_inputs(0)[1], munc0[0])               # nothing of the batch changed
        with pytest.raises(ValueError, match="EB_effectiveNuL must be finite and at least 4.0"):
            b.munc_track_finish(3.0, 40.0, floor=1.0e-6)
        for use_eb in (True, False):
            done = b.munc_track_finish([8.0, 6.1, 9.0], 33.3, replicate_factors=[1.0, 0.7, 1.0 + 2.0e-8], count_floor=floors,
                                       floor=1.0e-3 / 3.0, cap=None, use_eb=use_eb, blacklist_quantile=0.37)
            for c in range(2):
                want, diags, fl = T.finished_matrix(local[c], None, excl[c], floors[c], TREND, [1.0, 0.7, 1.0 + 2.0e-8], 33.3,
                                                    [8.0, 6.1, 9.0], 1.0e-3 / 3.0, None, use_eb=use_eb, quantile=0.37, prior=prior[c])
                assert MC.same(want, b.download_inputs(c)[1]), (use_eb, c)
                assert MC.same(fl, done["floors"][c])
                assert done["diagnostics"][c] == diags
            assert done["diagnostics"][0][0]["countFloorMissingCount"] == 0         # a floor without a finite entry is no floor
            assert done["diagnostics"][1][1]["countFloorAddedCount"] > 0
            assert done["diagnostics"][1][2]["countFloorFiniteCount"] == 0          # the infinite cell counts as missing


def test_resident_prior_track_constant_fallback_and_limits():
    b, lens, _chains = small_batch()
    with b:
        b.stats()
        b.forward_backward(want_sums=False)
        mean = [b.download(c, "xs")[:, 0].copy() for c in range(2)]
        for trend in ((np.linspace(-1, 1, 8), np.array([-2.0, 1.0]), -1, -1.0, 1.0), (np.zeros(0), np.array([0.3]), 3, -1.0, 1.0)):
            b.munc_prior_track(trend, floor=1.0e-6, cap=None, chains=[True, False])
            want = T.eval_pspline_log_variance_trend(trend, mean[0], eps=1.0e-6)
            assert MC.same(want, b.download_munc_seed(0, "seed_prior"))
        assert np.all(b.download_munc_seed(1, "seed_prior") == 0.0)     # a chain not taken keeps what it had
        with pytest.raises(ValueError, match="degree 6"):
            b.munc_prior_track((np.zeros(20), np.zeros(8), 6, 0.0, 1.0))
        for degree, nb in ((0, 5), (1, 6), (5, 12)):
            trend = MC.make_trend(degree, nb, 40 + degree, x_min=-1.5, x_max=2.5)
            b.munc_prior_track(trend, floor=1.0e-6, cap=2.0)
            for c in range(2):
                within_one_ulp(f"resident_deg{degree}_chain{c}", b.download_munc_seed(c, "seed_prior"),
                               T.eval_pspline_log_variance_trend(trend, mean[c], eps=1.0e-6, maxVariance=2.0))
