"""`driver.munc_seed_batch`: the dense observation-variance seed loop (consenrich.py:7784-7945, background fit on and off) on one batch of
three chains of unequal length, end to end against the twin loop -- the oracle library's forward / backward passes and the NumPy
twin of the natives, of the per-cell glue and of `_updateSeedBackground` over the oracle's background solve (tests/twin_munc.py).

The loop is not bit for bit: the smoother agrees with the oracle to its documented tolerance, and
local = omega * rho * moment - pad - countFloor cancels near the floor.  So the difference of `local_evidence`, `seed_munc` and
`response_weight` is gated relative to the un-cancelled minuend |twin| + pad + countFloor (for the response weight: |twin|), at
10 x the worst ratio measured on these shapes on the first GPU run (profiles/munc_seed_parity.json, per case) and never looser than
the project's standing 1e-5.  The kernels inside the loop are proven bit for bit, stage by stage on the device's own inputs, in
tests/test_gpu_munc.py.  With MUNC_SEED_PARITY_OUT set, the measured ratios are also written to that file."""
import json
import os

import numpy as np
import pytest

import munc_cases as MC
import twin_munc as T

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARITY = os.path.join(ROOT, "profiles", "munc_seed_parity.json")
STANDING = 1.0e-5
PAD, WINDOW = 1.0e-4, 9
LENS = (300, 2 * MC.ROLL_BLOCK + 1, 65)
M = 5
Q2 = np.array([[1.0e-3, 0.0], [0.0, 1.0e-4]], np.float32)
F2 = np.array([[1.0, 1.0], [0.0, 1.0]], np.float32)
BG = dict(lam_first=25.0, lam=400.0, negative_penalty_multiplier=2.0)
# (name, state model, passes, weights: "student_t" | "gaussian" | "disabled", count floor, exclude mask, cap,
#  G-uncertainty mode with the background fit on, or None = fit_background off)
CASES = (
    ("trend_p3_t_floor_excl", 2, 3, "student_t", True, True, None, None),
    ("trend_p2_t_plain", 2, 2, "student_t", False, False, None, None),
    ("trend_p3_gauss_floor", 2, 3, "gaussian", True, False, 50.0, None),
    ("level_p3_t_excl", 1, 3, "student_t", False, True, None, None),
    ("level_p2_disabled", 1, 2, "disabled", False, False, None, None),
    ("trend_p3_t_bg_proxy", 2, 3, "student_t", True, True, None, "proxy"),
    ("trend_p2_t_bg_disabled", 2, 2, "student_t", False, False, None, "disabled"),
    ("level_p3_t_bg_proxy", 1, 3, "student_t", False, True, None, "proxy"),
    ("level_p2_gauss_bg_proxy", 1, 2, "gaussian", True, False, 50.0, "proxy"),
    ("trend_p2_disabled_bg_disabled", 2, 2, "disabled", False, False, None, "disabled"),
)


def inputs(k, n, floor, excl):
    (data, munc, _l, _v), kw = MC.seed_inputs(dict(m=M, n=n, seed=9100 + k, opt=("floor",)))
    rng = np.random.default_rng(9200 + k)
    return data, munc, (kw["countFloor"] if floor else None), ((rng.random(n) < 0.15).astype(np.uint8) if excl else None)


def twin_loop(orc, data, munc, floor, excl, d, passes, use_weights, cap, g_mode):
    n = data.shape[1]
    Q = np.ascontiguousarray(Q2[:d, :d])
    total, omega, rho = munc.copy(), np.ones(n, np.float32), np.ones(data.shape, np.float32)
    g, G = np.zeros(n, np.float32), np.zeros(n, np.float32)

    def smoother():
        work = T.seed_working_munc(total, omega, rho, G, PAD, use_weights)
        seed_data = np.ascontiguousarray(data - g.reshape(1, -1), dtype=np.float32)
        xf, Pf, pn, D = (np.empty((n, d), np.float32), np.empty((n, d, d), np.float32), np.empty((n, d, d), np.float32),
                         np.empty(n, np.float32))
        common = dict(matrixData=seed_data, matrixPluginMuncInit=work, matrixQ0=Q, intervalToBlockMap=np.zeros(n, np.int32), blockCount=1,
                      stateInit=0.0, stateCovarInit=1000.0, pad=PAD, stateForward=xf, stateCovarForward=Pf, pNoiseForward=pn,
                      vectorD=D, returnNLL=True, ECM_useObsPrecisionReweighting=False, ECM_useProcessPrecisionReweighting=False)
        if d == 1:
            orc.cforwardPassLevel(**common)
            bw = orc.cbackwardPassLevel(matrixData=seed_data, stateForward=xf, stateCovarForward=Pf, pNoiseForward=pn)
        else:
            orc.cforwardPass(matrixF=F2, **common)
            bw = orc.cbackwardPass(matrixData=seed_data, matrixF=F2, stateForward=xf, stateCovarForward=Pf, pNoiseForward=pn)
        return np.ascontiguousarray(bw[0][:, 0]), np.maximum(np.ascontiguousarray(bw[1][:, 0, 0]), np.float32(0.0))

    def seed_pass(update):
        mean, var = smoother()
        return mean, T.cMuncObservationMomentSeedPass(data, total, mean, var, background=g, gVariance=G, countFloor=floor, omegaIn=omega,
                                                      rhoIn=rho, pad=PAD, useSeedWeights=use_weights, updateWeights=update,
                                                      varianceCap=T.F32_MAX if cap is None else cap)

    for _ in range(passes):
        mean, (_mo, rho_n, _raw, omega_n, _local, total_n) = seed_pass(True)
        if g_mode is not None:
            g, G = T.update_seed_background(data, mean, total, omega, rho, PAD, use_weights, g_uncertainty=g_mode, **BG)[:2]
        total, omega, rho = total_n, omega_n, rho_n
        if not use_weights:
            omega, rho = np.ones_like(omega), np.ones_like(rho)
    _mean, (_mo, rho_s, _raw, omega_s, local_pt, _t) = seed_pass(False)
    smooth = T.cMuncSmoothDenseLocalEvidence(local_pt, WINDOW, excludeMask=excl)
    return dict(local_evidence=smooth, seed_munc=T.local_to_total_variance(smooth, floor, cap),
                response_weight=T.response_weight(rho_s, omega_s, use_weights))


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle as o

    o.lib()
    return o


@pytest.fixture(scope="module")
def gates():
    with open(PARITY) as fh:
        return json.load(fh)["cases"]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_loop_against_the_twin_loop(orc, gates, case):
    from consenrich_amd import _lib, driver
    from consenrich_amd.batch import DeviceBatch, ModelParams

    _lib.require_gpu()
    name, d, passes, weights, with_floor, with_excl, cap, g_mode = case
    use_weights = weights == "student_t"
    chains = [inputs(k, n, with_floor, with_excl) for k, n in enumerate(LENS)]
    model = ModelParams() if d == 2 else ModelParams(state_dim=1, Q0=((1e-3, 0), (0, 0)))
    with DeviceBatch() as b:
        b.configure(model, M, LENS)
        for c, ch in enumerate(chains):
            b.upload(c, ch[0], ch[1])
        got = driver.munc_seed_batch(b, pad=PAD, window=WINDOW, passes=passes, state_model="levelTrend" if d == 2 else "level",
                                     count_floor=[ch[2] for ch in chains] if with_floor else None,
                                     exclude=[ch[3] for ch in chains] if with_excl else None, weights=weights, cap=cap,
                                     fit_background=g_mode is not None, background=BG, g_uncertainty=g_mode or "proxy",
                                     q=[Q2] * len(LENS),
                                     fetch=("local_evidence", "seed_munc", "response_weight", "seed_mean", "omega", "g_variance"))
        stats = b.munc_seed_stats()
        with pytest.raises(ValueError):
            driver.munc_seed_batch(b, pad=PAD, window=WINDOW, fit_background=True)      # (no `background` arguments)
    assert stats["passes"] == passes + 1 and stats["rolls"] == 1
    worst = {}
    for c, ch in enumerate(chains):
        want = twin_loop(orc, ch[0], ch[1], ch[2], ch[3], d, passes, use_weights, cap, g_mode)
        assert bool(np.any(got[c]["g_variance"] > 0.0)) == (g_mode == "proxy")
        floor = ch[2] if ch[2] is not None else 0.0
        for field in ("local_evidence", "seed_munc", "response_weight"):
            w = want[field].astype(np.float64)
            scale = np.abs(w) + (PAD + floor if field != "response_weight" else 0.0)
            ratio = float(np.max(np.abs(got[c][field].astype(np.float64) - w) / scale))
            worst[field] = max(worst.get(field, 0.0), ratio)
        assert got[c]["seed_mean"].dtype == np.float64 and got[c]["seed_mean"].shape == (LENS[c],)
        if not use_weights:
            assert np.all(got[c]["response_weight"] == 1.0) and np.all(got[c]["omega"] == 1.0)
    print(f"munc seed parity {name}: {worst}")
    out = os.environ.get("MUNC_SEED_PARITY_OUT")
    if out:
        rec = {}
        if os.path.exists(out):
            with open(out) as fh:
                rec = json.load(fh)
        rec[name] = worst
        with open(out, "w") as fh:
            json.dump(rec, fh, indent=1, sort_keys=True)
    for field, ratio in worst.items():
        gate = min(10.0 * gates[name]["measured"][field], STANDING)
        assert ratio <= gate, (name, field, ratio, gate)


def test_loop_with_the_q0_seed_of_the_resident_batch(orc):
    """q=None: the Q0 of every chain comes from `DeviceBatch.qseed` on the resident data and seed munc; the batch's own munc holds
    the last working munc on exit."""
    from consenrich_amd import driver
    from consenrich_amd.batch import DeviceBatch, ModelParams

    chains = [inputs(k, n, False, False) for k, n in enumerate(LENS)]
    with DeviceBatch() as b:
        b.configure(ModelParams(), M, LENS)
        for c, ch in enumerate(chains):
            b.upload(c, ch[0], ch[1])
        got = driver.munc_seed_batch(b, pad=PAD, window=WINDOW, passes=1, chains=[True, False, True], fit_background=False,
                                     fetch=("seed_munc", "rho", "omega", "pointwise"))
        assert got[1] is None
        for c in (0, 2):
            assert np.all(np.isfinite(got[c]["seed_munc"])) and np.all(got[c]["seed_munc"] >= np.float32(1.0e-12))
            assert np.array_equal(got[c]["seed_munc"], b.download_munc_seed(c, "seed_total"))
        assert np.array_equal(b.download_inputs(1)[1], chains[1][1])        # a chain the loop leaves out keeps its munc
        assert not np.array_equal(b.download_inputs(0)[1], chains[0][1])    # the others hold the last working munc
