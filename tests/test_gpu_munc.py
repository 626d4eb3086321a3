"""The dense observation-variance seed natives on the device: the drop-ins (`consenrich_amd.cconsenrich.cMuncObservationMomentSeedPass`,
`cMuncSmoothDenseLocalEvidence`) against the compiled reference's fixtures, bit for bit and error text for error text, and the
resident forms (`DeviceBatch.munc_seed_*`) stage by stage: after each resident stage its inputs and outputs are downloaded and the
outputs must equal, bit for bit, the CPU twin of that stage alone on those inputs.  The rolling mean's fallback counter is asserted
with the bits: zero where every running-sum operation is exact, the planted rows where it is not (tests/test_munc_twin.py holds the
twin to the same condition on the CPU)."""
import os

import numpy as np
import pytest

import munc_cases as MC
import twin_munc as T

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "munc")
SEED = {c["name"]: c for c in MC.seed_cases()}
SMOOTH = {c["name"]: c for c in MC.smooth_cases()}
PAD = 1.0e-4
BG = dict(lam_first=25.0, lam=400.0, negative_penalty_multiplier=2.0)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def dev():
    from consenrich_amd import _lib, cconsenrich

    _lib.require_gpu()
    return cconsenrich


@pytest.fixture(scope="module")
def gold():
    g = {}
    for group in MC.SEED_GROUPS + MC.SMOOTH_GROUPS:
        g.update(MC.load_group(os.path.join(GOLD, f"munc_{group}.npz")))
    return g


@pytest.mark.parametrize("name", sorted(SEED))
def test_seed_pass_dropin_equals_the_reference(dev, gold, name):
    got = MC.run_seed(dev, SEED[name])
    for field in MC.SEED_FIELDS:
        assert np.array_equal(bits(got[field]), bits(gold[name][field])), field


@pytest.mark.parametrize("name", sorted(SMOOTH))
def test_smooth_dropin_equals_the_reference_and_counts_its_fallbacks(dev, gold, name):
    from consenrich_amd import munc

    case = SMOOTH[name]
    local, window, mask = MC.smooth_inputs(case)
    out = dev.cMuncSmoothDenseLocalEvidence(local, window, excludeMask=mask)
    assert np.array_equal(bits(out), bits(gold[name]["out"]))
    want = T.smooth_device(local, window, excludeMask=mask)[1]
    if case["fallback_rows"] is not None:
        assert want == case["fallback_rows"]
    assert munc.last_smooth_fallback_rows == want


def test_subnormal_results_are_kept(dev):
    got = MC.run_seed(dev, SEED["subnormal_m5"])
    assert 0.0 < got["moment"][0, 0] < np.finfo(np.float32).tiny
    assert 0.0 < got["local"][0, 0] < np.finfo(np.float32).tiny


def test_error_texts(dev):
    for name, a, k, text in MC.seed_error_cases():
        with pytest.raises(ValueError) as e:
            dev.cMuncObservationMomentSeedPass(*a, **k)
        assert str(e.value) == text, name
    for name, local, window, mask, eps, text in MC.smooth_error_cases():
        with pytest.raises(ValueError) as e:
            dev.cMuncSmoothDenseLocalEvidence(local, window, excludeMask=mask, eps=eps)
        assert str(e.value) == text, name


# ---------------------------------------------------------------------------------------------------------------
# resident forms, stage by stage on the device's own inputs
# ---------------------------------------------------------------------------------------------------------------
LENS = (65, 2 * MC.ROLL_BLOCK + 1, MC.ROLL_BLOCK - 1)


def chain_inputs(m, n, seed):
    (data, munc, _level, _var), kw = MC.seed_inputs(dict(m=m, n=n, seed=seed, opt=("floor", "rho", "omega", "g")))
    floor = kw["countFloor"]
    floor[0, 0] = np.nan                        # "no floor here": becomes 0 (consenrich.py:7354-7359)
    exclude = (np.random.default_rng(seed).random(n) < 0.2).astype(np.uint8)
    return data, munc, floor, exclude, kw["rhoIn"], kw["omegaIn"], kw["gVariance"]


def fit_tracks(b, c):
    xs, Ps = b.download(c, "xs"), b.download(c, "Ps")
    return np.ascontiguousarray(xs[:, 0]), np.maximum(np.ascontiguousarray(Ps[:, 0, 0]), np.float32(0.0))


def twin_pass(b, c, data, update, use_weights, cap):
    """The twin of one resident seed pass of chain c on what the device holds right now."""
    mean, var = fit_tracks(b, c)
    floor = b.download_munc_seed(c, "seed_count_floor")
    return T.cMuncObservationMomentSeedPass(
        data, b.download_munc_seed(c, "seed_total"), mean, var, background=b.download_munc_seed(c, "seed_g"),
        gVariance=b.download_munc_seed(c, "seed_gvar"), countFloor=floor, omegaIn=b.download_munc_seed(c, "seed_omega"),
        rhoIn=b.download_munc_seed(c, "seed_rho"), pad=PAD, studentTdf=8.0, useSeedWeights=use_weights, updateWeights=update,
        omegaMin=0.01, omegaMax=100.0, varianceFloor=1.0e-12, varianceCap=T.F32_MAX if cap is None else cap)


@pytest.mark.parametrize("m,state_dim,use_weights,cap", [(5, 2, True, None), (17, 1, True, 6.0), (17, 2, False, None)])
def test_resident_stages_equal_their_twins(dev, m, state_dim, use_weights, cap):
    from consenrich_amd.batch import DeviceBatch, ModelParams

    model = ModelParams() if state_dim == 2 else ModelParams(state_dim=1, Q0=((1e-3, 0), (0, 0)))
    chains = [chain_inputs(m, n, 8100 + k) for k, n in enumerate(LENS)]
    with DeviceBatch() as b:
        b.configure(model, m, LENS)
        for c, ch in enumerate(chains):
            b.upload(c, ch[0], ch[1])
        b.munc_seed_begin(count_floor=[ch[2] for ch in chains], exclude=[ch[3] for ch in chains])
        for c, ch in enumerate(chains):
            assert np.array_equal(bits(b.download_munc_seed(c, "seed_total")), bits(ch[1]))
            assert np.all(b.download_munc_seed(c, "seed_rho") == 1.0) and np.all(b.download_munc_seed(c, "seed_omega") == 1.0)
            assert b.download_munc_seed(c, "seed_count_floor")[0, 0] == 0.0
            b.munc_seed_upload(c, "seed_rho", ch[4])
            b.munc_seed_upload(c, "seed_omega", ch[5])
            b.munc_seed_upload(c, "seed_gvar", ch[6])
        # -- working munc into the batch's own munc
        b.munc_seed_working(PAD, use_weights)
        for c, ch in enumerate(chains):
            want = T.seed_working_munc(ch[1], ch[5], ch[4], ch[6], PAD, use_weights)
            assert np.array_equal(bits(b.download_inputs(c)[1]), bits(want)), c
        b.stats()
        b.forward_backward(want_sums=False)
        # -- a pass that updates the weights: "next" copies and the pointwise local evidence
        b.munc_seed_pass(PAD, True, use_weights=use_weights, cap=cap)
        nxt = []
        for c, ch in enumerate(chains):
            _mo, rho, _raw, omega, local, total = twin_pass(b, c, ch[0], True, use_weights, cap)
            for name, want in (("seed_rho_next", rho), ("seed_omega_next", omega), ("seed_local", local), ("seed_total_next", total)):
                assert np.array_equal(bits(b.download_munc_seed(c, name)), bits(want)), (c, name)
            assert np.array_equal(bits(b.download_munc_seed(c, "seed_rho")), bits(ch[4]))      # the current copies stand
            nxt.append((rho, omega, total))
        # -- the seed front of the background update, before the swap: weight / rhs tracks bit for bit against the oracle's
        #    weighted statistics on the twin's float32 inputs, G bit for bit given the device's own new background, g within the
        #    solve's standing contract (tests/test_gpu_parity.py: max(1e-5, 10 roundoff) of the largest |g|, + 1e-7)
        mode = "disabled" if cap else "proxy"
        means = [fit_tracks(b, c)[0] for c in range(len(LENS))]         # (the call drops the resident fit: the background changes)
        info = b.munc_seed_background(BG["lam_first"], BG["lam"], negative_penalty_multiplier=BG["negative_penalty_multiplier"],
                                      pad=PAD, use_weights=use_weights, g_uncertainty=mode)
        for c, ch in enumerate(chains):
            mean = means[c]
            total, rho, omega = (b.download_munc_seed(c, k) for k in ("seed_total", "seed_rho", "seed_omega"))
            g_t, _G, w_t, r_t, rinfo = T.update_seed_background(ch[0], mean, total, omega, rho, PAD, use_weights,
                                                                g_uncertainty=mode, **BG)
            inv64 = T.seed_background_inputs(ch[0], mean, total, omega, rho, PAD, use_weights)[2]
            w, r, w64 = b.munc_seed_background_tracks(c)
            assert np.array_equal(w.view(np.uint64), w_t.view(np.uint64)), (mode, c)
            assert np.array_equal(r.view(np.uint64), r_t.view(np.uint64)), (mode, c)
            assert np.array_equal(w64.view(np.uint64), np.sum(inv64, axis=0, dtype=np.float64).view(np.uint64)), (mode, c)
            g = b.download_munc_seed(c, "seed_g")
            assert info[c]["status"] == 0 and info[c]["passes"] == rinfo["passes"]
            scale = max(float(np.abs(g_t).max()), 1e-6)
            assert float(np.abs(g - g_t).max()) <= max(1e-5, 10 * rinfo["roundoff_index"]) * scale + 1e-7, (mode, c)
            G_want = T.seed_g_variance(inv64, total, g, BG["lam_first"], BG["lam"], True, BG["negative_penalty_multiplier"], mode)
            assert np.array_equal(bits(b.download_munc_seed(c, "seed_gvar")), bits(G_want)), (mode, c)
            assert np.array_equal(bits(b.download(c, "background")), bits(g)), (mode, c)     # what the next smoother subtracts
            assert np.any(G_want > 0.0) == (mode == "proxy")
        for c, ch in enumerate(chains):         # (the rest of this test goes on with the planted G and no background)
            b.munc_seed_upload(c, "seed_gvar", ch[6])
            b.munc_seed_upload(c, "seed_g", np.zeros(LENS[c], np.float32))
            b.set_background(c, None)
        b.munc_seed_swap(use_weights)
        for c in range(len(LENS)):
            rho, omega, total = nxt[c]
            if not use_weights:
                rho, omega = np.ones_like(rho), np.ones_like(omega)
            for name, want in (("seed_rho", rho), ("seed_omega", omega), ("seed_total", total)):
                assert np.array_equal(bits(b.download_munc_seed(c, name)), bits(want)), (c, name)
        # -- the pointwise pass and the finish
        b.munc_seed_working(PAD, use_weights)
        b.stats()
        b.forward_backward(want_sums=False)
        b.munc_seed_pass(PAD, False, use_weights=use_weights, cap=cap)
        window, redone = 7, 0
        keep = []
        for c, ch in enumerate(chains):
            _mo, rho, _raw, omega, local, _total = twin_pass(b, c, ch[0], False, use_weights, cap)
            assert np.array_equal(bits(b.download_munc_seed(c, "seed_local")), bits(local)), c
            assert np.array_equal(bits(b.download_munc_seed(c, "seed_rho_next")), bits(rho)), c
            assert np.array_equal(bits(b.download_munc_seed(c, "seed_omega_next")), bits(omega)), c
            keep.append((rho, omega, local))
        b.munc_seed_finish(window, cap=cap, use_weights=use_weights)
        for c, ch in enumerate(chains):
            rho, omega, local = keep[c]
            smooth, rows, _res = T.smooth_device(local, window, excludeMask=ch[3])
            redone += rows
            floor = b.download_munc_seed(c, "seed_count_floor")
            assert np.array_equal(bits(b.download_munc_seed(c, "seed_smooth")), bits(smooth)), c
            assert np.array_equal(bits(b.download_munc_seed(c, "seed_total")), bits(T.local_to_total_variance(smooth, floor, cap))), c
            assert np.array_equal(bits(b.download_munc_seed(c, "seed_weight")), bits(T.response_weight(rho, omega, use_weights))), c
        st = b.munc_seed_stats()
        assert st["passes"] == 2 and st["rolls"] == 1 and st["roll_rows"] == m * len(LENS)
        assert st["last_roll_fallback_rows"] == redone
        # -- a planted local evidence: the rows with an inexact running sum are redone, the others are not
        planted = []
        for c, n in enumerate(LENS):
            local, _w, _mask = MC.smooth_inputs(dict(m=m, n=n, window=5, seed=8200 + c, plant=((c % m, n // 2),)))
            b.munc_seed_upload(c, "seed_local", local)
            planted.append(local)
        b.munc_seed_finish(5, cap=cap, use_weights=use_weights)
        redone = 0
        for c, ch in enumerate(chains):
            smooth, rows, _res = T.smooth_device(planted[c], 5, excludeMask=ch[3])
            redone += rows
            assert np.array_equal(bits(b.download_munc_seed(c, "seed_smooth")), bits(smooth)), c
        assert b.munc_seed_stats()["last_roll_fallback_rows"] == redone
        # -- an invalid active cell: the reference's text, and the current arrays stand
        before = b.download_munc_seed(1, "seed_total")
        g = np.zeros(LENS[1], np.float32)
        g[3] = np.nan
        b.munc_seed_upload(1, "seed_g", g)
        with pytest.raises(ValueError) as e:
            b.munc_seed_pass(PAD, True, use_weights=use_weights, cap=cap)
        assert str(e.value) == T.SEED_INVALID
        assert np.array_equal(bits(b.download_munc_seed(1, "seed_total")), bits(before))


def test_resident_loop_on_a_subset_of_chains_leaves_the_others_alone(dev):
    from consenrich_amd.batch import DeviceBatch, ModelParams

    m = 2
    chains = [chain_inputs(m, n, 8300 + k) for k, n in enumerate(LENS)]
    with DeviceBatch() as b:
        b.configure(ModelParams(), m, LENS)
        for c, ch in enumerate(chains):
            b.upload(c, ch[0], ch[1])
        b.munc_seed_begin(chains=[True, False, True])
        b.munc_seed_working(PAD)
        b.stats()
        b.forward_backward(want_sums=False)
        b.munc_seed_pass(PAD, True)
        assert np.all(b.download_munc_seed(1, "seed_local") == 0.0)
        assert np.all(b.download_munc_seed(1, "seed_total_next") == 0.0)
        assert np.all(b.download_munc_seed(0, "seed_local") > 0.0)
        with pytest.raises(RuntimeError, match="nonnegative"):
            b.munc_seed_begin(count_floor=[np.full((m, LENS[0]), -1.0, np.float32), None, None])
        with pytest.raises(RuntimeError, match="finite or NaN"):
            b.munc_seed_begin(count_floor=[np.full((m, LENS[0]), np.inf, np.float32), None, None])


# ---------------------------------------------------------------------------------------------------------------
# the q99 half of G: a stage in which the clip binds on some intervals and not on others
# ---------------------------------------------------------------------------------------------------------------
CLIP_M, CLIP_LENS = 2, (65, 127, 257)       # (N - 1) 0.99 = 127.71 (lerp from the upper side), 250.47 (from the lower), 508.87


def clip_inputs(k, n):
    """Without penalties and with small weights omega * rho, G ~ total / (m omega rho) exceeds the q99 of total in its top part.
    Chain 0 also holds cells of total in (-pad, 0), which the seed pass accepts and which must sort BELOW the positive ones;
    chain 2 holds 2 % of +inf cells in the planted total, so its q99 is not finite and the clip is the 1.0 fallback."""
    (data, munc, _level, _var), _kw = MC.seed_inputs(dict(m=CLIP_M, n=n, seed=8400 + k, opt=()))
    rng = np.random.default_rng(8500 + k)
    rho = rng.uniform(0.02, 0.4, (CLIP_M, n)).astype(np.float32)
    omega = rng.uniform(0.5, 1.5, n).astype(np.float32)
    total = munc.copy()
    if k == 0:
        total[0, 3] = total[1, 40] = total[1, 41] = np.float32(-5.0e-5)
    if k == 2:
        total[0, rng.choice(n, 11, replace=False)] = np.inf          # (one track only: every interval keeps a positive weight)
    return data, munc, total, rho, omega


def test_g_proxy_is_clipped_at_the_q99_of_total(dev):
    from consenrich_amd.batch import DeviceBatch, ModelParams

    chains = [clip_inputs(k, n) for k, n in enumerate(CLIP_LENS)]
    kw = dict(lam_first=0.0, lam=0.0, negative_penalty_multiplier=0.05)     # (small: intervals with a negative g clip too)
    with DeviceBatch() as b:
        b.configure(ModelParams(), CLIP_M, CLIP_LENS)
        for c, ch in enumerate(chains):
            b.upload(c, ch[0], ch[1])
        b.munc_seed_begin()
        for c, ch in enumerate(chains):
            b.munc_seed_upload(c, "seed_total", ch[2])
            b.munc_seed_upload(c, "seed_rho", ch[3])
            b.munc_seed_upload(c, "seed_omega", ch[4])
        b.stats()
        b.forward_backward(want_sums=False)
        means = [fit_tracks(b, c)[0] for c in range(len(CLIP_LENS))]
        info = b.munc_seed_background(kw["lam_first"], kw["lam"], negative_penalty_multiplier=kw["negative_penalty_multiplier"], pad=PAD,
                                      g_uncertainty="proxy")
        for c, ch in enumerate(chains):
            assert info[c]["status"] == 0
            inv64 = T.seed_background_inputs(ch[0], means[c], ch[2], ch[4], ch[3], PAD, True)[2]
            g = b.download_munc_seed(c, "seed_g")
            with np.errstate(invalid="ignore"):
                q99 = float(np.quantile(ch[2].astype(np.float64), 0.99))
                want = T.seed_g_variance(inv64, ch[2], g, 0.0, 0.0, True, kw["negative_penalty_multiplier"], "proxy")
            clip = np.float32(q99 if np.isfinite(q99) and q99 > 0.0 else 1.0)
            assert np.isfinite(q99) == (c != 2)
            got = b.download_munc_seed(c, "seed_gvar")
            assert np.array_equal(bits(got), bits(want)), c
            clipped = int(np.count_nonzero(got == clip))
            assert 0 < clipped < CLIP_LENS[c], (c, clipped)            # the clip binds on some intervals and not on others
            assert float(got.max()) == float(clip)
