"""GPU tests (run with -m gpu) at sample counts above 64: the one dimension of a fit that selects other kernel code and another
LDS footprint (chain and block lengths only select geometry).

  * the residual kernels (`k_resid`, `k_resid_v4<K>` and their run-table forms): one slab of sample rows in LDS up to the edge of
    64 KB, slabs past it (csrc/csr_resid_form.h) -- against the definition, bit for bit, and pipelined against in order;
  * the statistics pass (`bin_stats4<4>`: groups of four rows, a scalar tail, a renormalisation every eighth row) and the whole
    fit against the CPU oracle, in the bit-exact and in the 2-ulp validation mode; the ECM on top of it;
  * the per-bin loops over the samples after a fit: diagnostics, gain summary, phase tracks, objective terms, background update.

M_EDGES: 65 (plain form; one tail row after 16 full groups of four), 68 (K = 2, no tail), 124 / 125 (the last K = 2 and its plain
neighbour), 128 (the first K = 1), 240 / 244 (the last one-slab K = 1 tile, 65280 bytes, and the first m past it), 251 / 253 (the
same pair for the plain form, 65260 bytes), 256 (a round cohort), 604 / 631 (three slabs).

Every reference is one the suite already states for the same quantity (the modules named in each test), with its tolerances."""
import numpy as np
import pytest

import cases
import test_gpu_gain_summary as gs
import test_gpu_stop_rule as sr
import test_gpu_tail_epilogue as te
from conftest import gpu_available
from test_gpu_parity import ATOL, RTOL, close_mostly

pytestmark = pytest.mark.gpu

M_EDGES = [65, 68, 124, 125, 128, 240, 244, 251, 253, 256, 604, 631]
RESID_LENS = [1, 63, 64, 65, 129, 193]      # odd and even numbers of 64-bin tiles: the K = 2 workgroups end half empty
POST_LENS = [64, 65, 1031]


@pytest.fixture(scope="module")
def product():
    if not gpu_available():
        pytest.fail("GPU tests selected but no HIP device / library: the product has no CPU fallback")
    from consenrich_amd import cconsenrich

    return cconsenrich


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as orc

    orc.lib()
    return orc


def _model(dim):
    from consenrich_amd.batch import ModelParams

    return ModelParams(state_dim=2) if dim == 2 else ModelParams(state_dim=1, Q0=((1e-3, 0), (0, 0)))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


# ---- B1: the residual kernel against its definition ------------------------------------------------------------------------
def _resid_definition(data, bg, xs):
    """pyx:6846-6848 on the device's own smoothed level: float32(float64(float32(data - background)) - float64(xs0)), (n, m)"""
    adj = data if bg is None else (data - bg[None, :]).astype(np.float32)
    return (adj.astype(np.float64) - xs[:, 0].astype(np.float64)[None, :]).astype(np.float32).T


@pytest.mark.parametrize("dim", [2, 1], ids=["levelTrend", "level"])
@pytest.mark.parametrize("m", M_EDGES)
def test_residuals_equal_their_definition_bit_for_bit(product, m, dim):
    """stats, forward_backward, export(SMOOTH | RESID) of six chains; every bin and every sample of `resid` equals the NumPy
    statement of the definition on the downloaded `xs`, without and then with a float32 background on two of the chains.  Row j
    of the data carries j / 64 on top, so a swapped, repeated or missing sample column cannot cancel."""
    from consenrich_amd import _lib as L
    from consenrich_amd.batch import DeviceBatch

    ramp = (np.arange(m, dtype=np.float32) * np.float32(2.0 ** -6))[:, None]
    sets = []
    for c, n in enumerate(RESID_LENS):
        d_, v_ = cases.synth(n, m, 7100 + 7 * m + c, mask_frac=0.02, outlier_frac=0.01)
        sets.append(((d_ + ramp).astype(np.float32), v_))
    bgs = {3: (0.3 * np.sin(np.arange(RESID_LENS[3]) / 9.0) - 0.1).astype(np.float32),
           5: (0.2 * np.cos(np.arange(RESID_LENS[5]) / 17.0) + 0.05).astype(np.float32)}
    with DeviceBatch(0) as b:
        b.configure(_model(dim), m, RESID_LENS)
        for c, (d_, v_) in enumerate(sets):
            b.upload(c, d_, v_)
        for with_bg in (False, True):
            if with_bg:
                for c, bg in bgs.items():
                    b.set_background(c, bg)
            b.stats()
            b.forward_backward(L.RETURN_NLL)
            b.export(L.EXPORT_SMOOTH | L.EXPORT_RESID)
            for c, n in enumerate(RESID_LENS):
                xs, resid = b.download(c, "xs"), b.download(c, "resid")
                assert xs.shape == (n, dim) and resid.shape == (n, m) and resid.dtype == np.float32
                assert np.all(np.isfinite(xs)), (m, dim, with_bg, c)
                want = _resid_definition(sets[c][0], bgs.get(c) if with_bg else None, xs)
                same = _bits(resid) == _bits(want)
                assert same.all(), (m, dim, with_bg, c, "first differing (bin, sample):", np.argwhere(~same)[:4].tolist())


# ---- B2: the run-table form, pipelined against in order -------------------------------------------------------------------
@pytest.fixture(scope="module")
def tail_inputs():
    """what tests/test_gpu_tail_epilogue.py's `_run` reads: per m, per chain of its N_LIST (data, munc); multipliers per chain"""
    mult = [cases.multipliers(n, 9300 + c) for c, n in enumerate(te.N_LIST)]
    return {}, mult


@pytest.mark.parametrize("m", [128, 253, 256])
def test_table_residuals_of_a_pipelined_step_equal_the_step_in_order(product, monkeypatch, tail_inputs, m):
    """The harness of tests/test_gpu_tail_epilogue.py (its environment pins, its chain lengths, two steps) at block 64, variant
    `plain`: with tail groups at 1 % (`k_resid_runs` / `k_resid_v4_runs<1>` serve them) every output of both steps equals the
    step in order bit for bit, nothing is replayed, and at least one group per step went out; the residuals of the pipelined steps
    equal their definition on the downloaded `xs` bit for bit as well."""
    sets, _ = tail_inputs
    if m not in sets:
        sets[m] = [cases.synth(n, m, 9100 + 10 * m + c, mask_frac=0.01, outlier_frac=0.01) for c, n in enumerate(te.N_LIST)]
    in_order = te._run(monkeypatch, tail_inputs, {"CONSENRICH_AMD_TAIL_SPLIT": "0"}, m, 64, "plain")
    assert in_order["stats"]["tail_groups"] == 0
    assert in_order["stats"]["pipeline_redos"] == 0 and in_order["stats"]["sb_bailouts"] == 0, in_order["stats"]
    got = te._run(monkeypatch, tail_inputs, {"CONSENRICH_AMD_TAIL_PCT": "1,1"}, m, 64, "plain")
    print(m, got["stats"])
    assert got["stats"]["pipeline_redos"] == 0 and got["stats"]["sb_bailouts"] == 0, got["stats"]
    if te._pipelines():
        assert got["stats"]["tail_groups"] >= 2, got["stats"]
    te._assert_same(got, in_order, (m, "against the step in order"))
    # ... and the table form against the definition itself (both steps run the same device function: equal is not yet right)
    for c, n in enumerate(te.N_LIST):
        for step in range(2):
            want = _resid_definition(sets[m][c][0], None, got[(c, "xs", step)])
            assert np.array_equal(_bits(got[(c, "resid", step)]), _bits(want)), (m, c, step)
    sets.pop(m)         # (33 000 bins x m: not kept for the rest of the module)


# ---- B3: the fit against the oracle ---------------------------------------------------------------------------------------
FIT_TRACKS = ("xf", "Pf", "pn", "D", "xs", "Ps", "lag", "resid")
_ORACLE_FITS, _PRODUCT_FITS = {}, {}


def _fit_case(m, dim):
    return cases._fb(f"fb_many_samples_m{m}_d{dim}", dim, 1000, m, 7700 + m, use_lam=True, use_kap=True, use_qs=True, mask=0.02,
                     outl=0.01)


def _oracle_fit(oracle, m, dim):
    """the oracle's fit of the case, computed once per (m, dim) and left unchanged"""
    if (m, dim) not in _ORACLE_FITS:
        _ORACLE_FITS[(m, dim)] = _freeze(cases.run_case(oracle, _fit_case(m, dim)))
    return _ORACLE_FITS[(m, dim)]


def _freeze(out):
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def _product_fit(product, m, dim, xtol):
    """the product's fit of the case in one validation mode, computed once and left unchanged"""
    if (m, dim, xtol) not in _PRODUCT_FITS:
        product.set_validation(xtol)
        try:
            _PRODUCT_FITS[(m, dim, xtol)] = _freeze(cases.run_case(product, _fit_case(m, dim)))
        finally:
            product.set_validation(0)
    return _PRODUCT_FITS[(m, dim, xtol)]


@pytest.mark.parametrize("dim", [2, 1], ids=["levelTrend", "level"])
@pytest.mark.parametrize("m", [65, 68, 128, 256, 631])
def test_exact_mode_fit_equals_the_oracle(product, oracle, m, dim):
    """One chain of 1000 bins with lambda, kappa, the process-noise scale, masked cells and outliers, validation at 0 ulps: Pf,
    pNoise, D, xs and resid equal the oracle's bit for bit (the tracks `test_exact_mode_is_bit_identical_to_the_oracle_at_full_size`
    holds so at m = 4); xf to that test's rtol 3e-7 / atol 1e-9; the float64 NLL to 1e-12.  (Measured: xf equals the oracle's
    bit for bit as well in all ten cases; the NLL differs by at most 2.2e-15 relative.  Ps and lag: the next test.)"""
    got, ref = _product_fit(product, m, dim, 0), _oracle_fit(oracle, m, dim)
    for name in FIT_TRACKS:
        print(m, dim, name, "differing elements:", int(np.count_nonzero(_bits(got[name]) != _bits(ref[name]))), "of", ref[name].size)
    print(m, dim, "nll", float(got["nll"]), float(ref["nll"]), abs(float(got["nll"]) - float(ref["nll"])) / abs(float(ref["nll"])))
    for name in ("Pf", "pn", "D", "xs", "resid"):
        assert np.array_equal(_bits(got[name]), _bits(ref[name])), (m, dim, name)
    np.testing.assert_allclose(got["xf"].astype(np.float64), ref["xf"].astype(np.float64), rtol=3e-7, atol=1e-9, err_msg="xf")
    assert float(got["nll"]) == pytest.approx(float(ref["nll"]), rel=1e-12)


@pytest.mark.parametrize("dim", [2, 1], ids=["levelTrend", "level"])
@pytest.mark.parametrize("m", [65, 68, 128, 256, 631])
def test_exact_mode_smoothed_covariances_within_3e_7_of_the_oracle(product, oracle, m, dim):
    """Ps and lag of the same fit to rtol 3e-7 / atol 1e-9 of the oracle's, the numbers of
    `test_exact_mode_is_bit_identical_to_the_oracle_at_full_size`.

    Measured: Ps and lag equal the oracle's bit for bit in all ten cases.  This test found the one place where they did not:
    bin 0 of a levelTrend chain, Ps[0][1,1], lag[0][1,0] and lag[0][1,1], off by 2.6e-5 (m = 65), 1.2e-6 (68), 1.2e-4 (128),
    8.7e-5 (256) relative on Ps[0][1,1] and up to 1.5e-3 on lag[0][1,0] -- at any m (the same case at m = 4, 32, 64: 5.4e-7,
    1.3e-6, 1.5e-6).  With lambda, kappa and the process-noise scale in the pass the filtered trend variance at bin 0 is 500
    against a smoothed one of 1e-3, and the predicted covariance the smoother inverts there has pp00 pp11 / det = 3e3 .. 4e5:
    the smoother gain's fused determinant, Newton-refined reciprocal and fused products, each within an ulp of the reference's
    operation, were amplified by that much.  `Gain` (csr_device.h) now performs the reference's operations in its order."""
    got, ref = _product_fit(product, m, dim, 0), _oracle_fit(oracle, m, dim)
    for name in ("Ps", "lag"):
        bad = np.argwhere(_bits(got[name]) != _bits(ref[name]))
        print(m, dim, name, "differs at", bad.tolist())
        for idx in map(tuple, bad):
            print("    device %.9e oracle %.9e relative %.3e" % (got[name][idx], ref[name][idx],
                                                              abs(float(got[name][idx]) - float(ref[name][idx])) / abs(float(ref[name][idx]))))
    for name in ("Ps", "lag"):
        np.testing.assert_allclose(got[name].astype(np.float64), ref[name].astype(np.float64), rtol=3e-7, atol=1e-9, err_msg=name)


@pytest.mark.parametrize("dim", [2, 1], ids=["levelTrend", "level"])
@pytest.mark.parametrize("m", [65, 68, 128, 256, 631])
def test_two_ulp_mode_fit_stays_within_the_parity_budget(product, oracle, m, dim):
    """The same chain with validation at 2 ulps (the batch default): every track within tests/test_gpu_parity.py's RTOL / ATOL,
    D through `close_mostly` with its defaults; sumNLL within 1e-7 relative of the oracle's -- a decade under the ECM stop rule's
    1e-6, its only consumer.  Measured (levelTrend / level): m = 65: 3.6e-9 / 3.7e-9, 68: 1.6e-10 / 1.6e-10, 128: 1.4e-9 /
    1.4e-9, 256: 9.7e-10 / 9.7e-10, 631: 6.3e-10 / 6.3e-10."""
    got, ref = _product_fit(product, m, dim, 2), _oracle_fit(oracle, m, dim)
    rel = abs(float(got["nll"]) - float(ref["nll"])) / abs(float(ref["nll"]))
    print(m, dim, "sumNLL relative difference:", rel)
    for name in FIT_TRACKS:
        if name == "D":
            close_mostly(got[name], ref[name], msg=f"{m} {dim} D")
        else:
            np.testing.assert_allclose(got[name].astype(np.float64), ref[name].astype(np.float64), rtol=RTOL, atol=ATOL,
                                       err_msg=f"{m} {dim} {name}")
    assert rel <= 1e-7, (m, dim, rel)


# ---- B4: ECM --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [65, 256])
def test_ecm_matches_the_oracle(product, oracle, m):
    """cfixedBackgroundECM with the arguments of `test_ecm_on_a_chromosome_sized_chain_matches_oracle` (the CLI defaults) on 3000
    bins in blocks of 500: the same iteration count and convergence flag, the objective path to 5e-8, the tracks within RTOL /
    ATOL with that test's scalings."""
    n = 3000
    data, munc = cases.synth(n, m, 2121 + m, outlier_frac=0.01)
    bm = (np.arange(n) // 500).astype(np.int32)
    kw = dict(matrixData=data, matrixPluginMuncInit=munc, matrixF=np.asarray(cases.F_TREND, np.float32),
              matrixQ0=np.diag([1e-3, 1e-4]).astype(np.float32), intervalToBlockMap=bm, blockCount=int(bm.max()) + 1,
              stateInit=0.0, stateCovarInit=1000.0, ECM_fixedBackgroundIters=50, ECM_fixedBackgroundRtol=1e-6, pad=1e-4,
              ECM_robustTNu=8.0, procPrecisionMultiplierMin=5e-3, procPrecisionMultiplierMax=5e3,
              ECM_useObsPrecisionReweighting=False, ECM_useProcessPrecisionReweighting=True, t_innerIters=5,
              returnIntermediates=True, returnDiagnostics=True, trackOptimizationPath=True, logIterations=False)
    g = product.cfixedBackgroundECM(**kw)
    o = oracle.cfixedBackgroundECM(**kw)
    print(m, "iterations", g[0], o[0], "nll", g[1], o[1])
    assert g[0] == o[0] and g[8]["converged"] == o[8]["converged"] and g[0] >= 2
    assert g[1] == pytest.approx(o[1], rel=5e-8)
    gp = [r["objective_value"] for r in g[8]["optimization_path"]]
    np.testing.assert_allclose(gp, o[8]["optimization_path"], rtol=5e-8)
    assert g[6] is None and o[6] is None
    close_mostly(g[7], o[7], msg="kappa")
    scale = np.abs(o[2]).max(axis=1, keepdims=True)
    assert np.all(np.abs(g[2].astype(np.float64) - o[2]) <= RTOL * scale + ATOL)      # smoothed state
    np.testing.assert_allclose(g[3], o[3], rtol=RTOL, atol=ATOL)                      # smoothed covariance
    np.testing.assert_allclose(g[4][: n - 1], o[4][: n - 1], rtol=RTOL, atol=ATOL)    # lag-one covariance
    assert np.all(np.abs(g[5].astype(np.float64) - o[5]) <= RTOL * np.abs(o[2][:, :1]) + ATOL)   # residuals


# ---- B5: the per-bin loops over the samples after a fit -----------------------------------------------------------------
@pytest.mark.parametrize("m", [65, 256])
def test_batch_diagnostics_at_many_samples(product, m):
    """`csr_batch_diagnostics` (k_diag_natural) as in `test_batch_diagnostics_from_resident_forward_pass`: against the oracle
    evaluated on the downloaded filter outputs, with the multipliers and without, rtol 1e-5."""
    from consenrich_amd import _lib as L
    from consenrich_amd.batch import DeviceBatch, ModelParams
    from oracle import diagnostics as orc

    mp = ModelParams(state_dim=2, Q0=((1e-3, 0.0), (0.0, 1e-4)))
    for flags in (L.USE_LAMBDA | L.USE_KAPPA | L.USE_QSCALE, 0):
        with DeviceBatch(0) as b:
            b.configure(mp, m, POST_LENS)
            ins = []
            for c, n in enumerate(POST_LENS):
                data, munc = cases.synth(n, m, 900 + m + c, mask_frac=0.02, outlier_frac=0.01)
                lam, kap, qs = cases.multipliers(n, 900 + m + c)
                b.upload(c, data, munc)
                b.upload_multipliers(c, lam, kap, qs)
                ins.append((munc, lam, kap, qs))
            b.stats()
            b.forward(L.RETURN_NLL | flags)
            b.diagnostics(flags)
            for c, n in enumerate(POST_LENS):
                munc, lam, kap, qs = ins[c]
                Pf, pn = b.download(c, "Pf"), b.download(c, "pnoise")
                use = flags != 0
                ref = orc.output_diagnostic_tracks(
                    stateCovarForward=Pf, matrixMunc=munc, matrixQ0=np.diag([1e-3, 1e-4]).astype(np.float32),
                    matrixF=np.asarray(cases.F_TREND, np.float32), stateCovarInit=mp.state_covar_init, state_dim=2,
                    lambdaExp=lam if use else None, processPrecExp=kap if use else None,
                    processQScale=qs if use else None, pNoiseForward=None if use else pn, pad=mp.pad,
                    obsPrecisionMultiplierMin=mp.lambda_bounds[0], obsPrecisionMultiplierMax=mp.lambda_bounds[1],
                    procPrecisionMultiplierMin=mp.kappa_bounds[0], procPrecisionMultiplierMax=mp.kappa_bounds[1])
                for k in ("sumGain0", "sumGain1", "effectiveQLevel", "effectiveQTrend", "muncTrace"):
                    np.testing.assert_allclose(b.download(c, k), ref[k], rtol=RTOL, atol=0, err_msg=f"{m} {flags} {c} {k}")


@pytest.mark.parametrize("dim", [2, 1], ids=["levelTrend", "level"])
@pytest.mark.parametrize("m", [65, 256])
def test_gain_summary_of_every_row_at_many_samples(product, m, dim):
    """One grid row per replicate, a histogram of m * GAIN_T * 256 words: EVERY row of every chain against `_reference` /
    `_compare` of tests/test_gpu_gain_summary.py.  The lambda track is one value per bin, so a NaN in it is a hole in every row
    of the chain: each chain has holes, and rows 64 and m - 1 (the last grid row) are asserted to have lost exactly them."""
    from consenrich_amd import _lib as L
    from consenrich_amd.batch import DeviceBatch

    mp = _model(dim)
    sets = [cases.synth(n, m, gs.SEED + 60 + m + c, mask_frac=0.02, outlier_frac=0.01) for c, n in enumerate(POST_LENS)]
    drops = [[0, 63], [7, 64], [0, 255, 256, 700, 1030]]
    lams = [gs._lambda(n, gs.SEED + 60 + c, drops[c]) for c, n in enumerate(POST_LENS)]
    with DeviceBatch(0) as b:
        b.configure(mp, m, POST_LENS)
        for c, (d_, v_) in enumerate(sets):
            b.upload(c, d_, v_)
            b.upload_multipliers(c, lams[c], None, None)
        b.stats()
        b.forward(L.RETURN_NLL)
        b.export(L.EXPORT_FORWARD | L.EXPORT_MULT)
        for c, n in enumerate(POST_LENS):
            Pf, lam = b.download(c, "Pf"), b.download(c, "lambda")
            assert Pf.shape == (n, dim, dim) and np.all(np.isfinite(Pf)), c         # the filter alone removes values
            assert np.array_equal(lam.view(np.uint32), lams[c].view(np.uint32)), c
            p00 = np.maximum(Pf.astype(np.float64)[:, 0, 0], 0.0)
            got = b.gain_summary(c, gs.PAD, use_lambda=True, lambda_bounds=mp.lambda_bounds)
            assert len(got["count"]) == m
            for j in range(m):
                g = gs._reference(p00, lam, mp.lambda_bounds, sets[c][1][j], gs.PAD)
                gs._compare(got, j, g, (m, dim, c, j))
            for j in (64, m - 1):
                assert got["count"][j] == n - len(drops[c]), (m, dim, c, j, got["count"][j])


@pytest.mark.parametrize("dim", [2, 1], ids=["levelTrend", "level"])
@pytest.mark.parametrize("m", [65, 256])
def test_phase_tracks_at_many_samples(product, m, dim):
    """`phase_tracks(with_fit=True)` (k_phase_tracks) as in `test_phase_tracks_equal_the_whole_matrix_restatement`
    (tests/test_core_api.py): the weighted-mean track bit for bit, the per-bin objective sums to 1e-14, the cell counts exactly,
    on the same fit (level, multipliers, background and proposal downloaded from the device)."""
    from consenrich_amd import _lib as L
    from consenrich_amd.batch import DeviceBatch
    from oracle import passdiag as pdg

    rng = np.random.default_rng(3 + m)
    mp = _model(dim)
    with DeviceBatch(0) as b:
        b.configure(mp, m, POST_LENS)
        host = []
        for c, n in enumerate(POST_LENS):
            sig = np.sin(np.arange(n) / 40.0)
            data = (sig[None, :] + 0.3 * rng.normal(size=(m, n))).astype(np.float32)
            munc = (0.2 * np.exp(rng.normal(0, 0.4, size=(m, n)))).astype(np.float32)
            munc[1, 10:20] = np.float32(1.0e30)
            munc[m - 1, 30:33] = np.float32(1.0e30)
            munc[:, 50] = np.float32(1.0e30)
            b.upload(c, data, munc)
            b.set_background(c, (0.05 * np.cos(np.arange(n) / 90.0)).astype(np.float32))
            host.append((data, munc))
        b.stats()
        b.ecm(max_iters=2, inner_iters=2, rtol=1e-6, nu=8.0, use_lambda=True, use_kappa=True)
        b.background_update(16.0, 256.0, use_lambda=True, use_initial=True)
        b.export(L.EXPORT_SMOOTH | L.EXPORT_MULT)
        pad32 = float(np.float32(mp.pad))
        for c, n in enumerate(POST_LENS):
            data, munc = host[c]
            rel, fit, cnt = b.phase_tracks(c, 1.0e-4, with_fit=True, use_lambda=True)
            level, lam = b.download(c, "xs")[:, 0], b.download(c, "lambda")
            cur, nxt = b.download(c, "background"), b.download(c, "background_next")
            assert np.abs(cur).max() > 0.01 and float(np.abs(nxt - cur).max()) > 0.0
            np.testing.assert_array_equal(rel, pdg.relative_level_track(level, data, munc, background=cur, pad=1.0e-4))
            inv, res = pdg.update_matrices(data, munc, level, lam, pad32, mp.lambda_bounds)
            inv64, fr = inv.astype(np.float64), res.astype(np.float64) - nxt.astype(np.float64)[None, :]
            np.testing.assert_allclose(fit, np.sum(inv64 * fr * fr, axis=0), rtol=1e-14)
            np.testing.assert_array_equal(cnt, np.count_nonzero(np.isfinite(res) & np.isfinite(inv) & (inv > 0.0), axis=0))
            want = pdg.background_fit_objective(res, inv, nxt, 16.0, 256.0, True, 1.0)
            assert 0.5 * float(fit.sum()) == pytest.approx(want["background_weighted_residual_objective"], rel=1e-12)
            assert int(cnt.sum()) == int(want["background_effective_observation_count"]) == m * n


@pytest.mark.parametrize("m", [65, 256])
def test_objective_terms_at_many_samples(product, m):
    """`objective_terms` (k_obj_wave: the weight track is a sum over the m variance rows) on the planted inputs of
    tests/test_gpu_stop_rule.py against its twin and exact sums, with its gate (n + 8) 2^-52; weight median and count with ==."""
    plants = sr._plants(POST_LENS, m, 1100 + m)
    with sr._open(POST_LENS, m, plants) as b:
        got = sr._terms(b)
    for c, p in enumerate(plants):
        sr._check_terms(got[c], sr._expected(p), ("many samples", m, c, p["n"]))
        assert got[c]["negative_penalty"] > 0.0


@pytest.mark.parametrize("m", [65, 256])
def test_background_update_at_many_samples(product, oracle, m):
    """`background_update`, mode `irls` (k_bg_batch_stats: weights and right-hand side are sums over the m rows), against the
    oracle's restatement on the downloaded smoothed level, as in `test_batch_background_update_matches_oracle`."""
    from consenrich_amd import _lib as L
    from consenrich_amd.batch import DeviceBatch, ModelParams
    from oracle import background as bgo
    from test_gpu_parity import _bg_batch_fixture

    mp = ModelParams(state_dim=2)
    ins = _bg_batch_fixture(POST_LENS, m, 4100 + m)
    lam_first, lam = bgo.penalties(60, 2.0)
    with DeviceBatch(0) as b:
        b.configure(mp, m, POST_LENS)
        for c, (data, munc) in enumerate(ins):
            b.upload(c, data, munc)
        b.stats()
        b.forward_backward(L.RETURN_NLL)
        b.export(L.EXPORT_SMOOTH)
        xs = [b.download(c, "xs") for c in range(len(POST_LENS))]
        kw = dict(zero_center=False, use_nonnegative=True, negative_penalty_multiplier=2.0, use_lambda=False, use_initial=True)
        info = b.background_update(lam_first, lam, **kw)
        nxt = [b.download(c, "background_next") for c in range(len(POST_LENS))]
    for c, (data, munc) in enumerate(ins):
        w, r, _, _ = bgo.weight_rhs_tracks(data, munc, xs[c][:, 0], np.float32(mp.pad), None, mp.lambda_bounds)
        ref, rinfo = bgo.solve_background(w, r, 0, zero_center=False, use_nonnegative=True, multiplier=2.0,
                                          initial=np.zeros(POST_LENS[c], np.float32), penalties_override=(lam_first, lam),
                                          return_info=True)
        scale = max(float(np.abs(ref).max()), 1e-6)
        assert info[c]["status"] == L.BG_OK and info[c]["support"] == int(np.count_nonzero(w > 0))
        assert info[c]["weight_sum"] == pytest.approx(float(w.sum()), rel=1e-12)
        assert info[c]["passes"] == rinfo["passes"], (m, c)
        assert info[c]["weight_scale"] == float(np.median(w[w > 0.0])), (m, c)      # exact order statistics
        assert info[c]["roundoff_index"] == pytest.approx(rinfo["roundoff_index"], rel=1e-9)
        assert float(np.abs(nxt[c] - ref).max()) <= max(1e-5, 10 * rinfo["roundoff_index"]) * scale + 1e-7, (m, c)
        shift = np.sqrt(np.dot(w, ref.astype(np.float64) ** 2) / w.sum())
        assert info[c]["shift_rms"] == pytest.approx(shift, rel=1e-4)
