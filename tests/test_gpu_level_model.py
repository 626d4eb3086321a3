"""GPU tests of the level model (state_dim = 1) through every stage that runs after the fit and reads the resident arrays (run
with -m gpu).  The resident arrays have another layout than the levelTrend ones (xs and Ps are one float per bin), the export
converts them along another path, and none of the state_dim == 2 fast paths is taken; the post-fit kernels index by the state
dimension.  Every stage is held to a reference of its own: the CPU oracle run chain by chain at state_dim = 1 (the project's
gate RTOL / ATOL), the pure-Python twin of the peak selection (bit for bit), the NumPy restatement of the gain summary, the
oracle of the output diagnostics, the reference's pandas call and tests/writer_refs.py for the track writers."""
import numpy as np
import pytest

import cases
import twin_rocco
import writer_refs as wr
from conftest import gpu_available
from test_gpu_parity import ATOL, RTOL, close_mostly

pytestmark = pytest.mark.gpu

CHAINS = [1, 2, 63, 64, 65, 1031, 4097]      # one bin, two, around one 64-bin block, an end inside a block, past 64 blocks of 64
M = 3
SEED = 6100
SHIFTED = 5                                  # this chain's data is moved by -50: its smoothed level is negative everywhere
Q_LEVEL = np.asarray([[1e-3, 0.0], [0.0, 1.0]], np.float32)     # what the oracle's level entry points read is [0, 0]
FIT = ("D", "xf", "Pf", "pnoise", "xs", "Ps", "lag", "resid")


def _model():
    from consenrich_amd.batch import ModelParams

    return ModelParams(state_dim=1, Q0=((1e-3, 0), (0, 0)))


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


@pytest.fixture(scope="module")
def sets():
    out = []
    for c, n in enumerate(CHAINS):
        d_, v_ = cases.synth(n, M, SEED + c, mask_frac=0.02, outlier_frac=0.01)
        out.append((d_ - np.float32(50.0) if c == SHIFTED else d_, v_))
    return out


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint32 if x.dtype == np.float32 else np.uint64)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _new_batch(sets_, chains=None):
    from consenrich_amd.batch import DeviceBatch

    take = range(len(sets_)) if chains is None else chains
    b = DeviceBatch(0)
    b.configure(_model(), M, [sets_[c][0].shape[1] for c in take])
    for k, c in enumerate(take):
        b.upload(k, *sets_[c])
    return b


def _downloads(b, names=FIT):
    return {(c, a): b.download(c, a) for c in range(len(b.chain_lens)) for a in names}


@pytest.fixture(scope="module")
def level(product, sets):
    """the fitted level batch, smoothed and exported: (batch, downloads of the fit)"""
    from consenrich_amd import _lib as L

    b = _new_batch(sets)
    b.stats()
    sums = b.forward_backward(L.RETURN_NLL)
    b.export(L.EXPORT_FORWARD | L.EXPORT_SMOOTH | L.EXPORT_RESID)
    yield b, _downloads(b), sums
    b.close()


def test_entry_points_agree_and_agree_with_the_oracle(level, oracle, sets):
    """forward + backward, forward_backward, step and (for the forward arrays) step_forward: the same bits in every array and the
    same per-chain sums, shapes (n, 1) / (n, 1, 1) / (n - 1, 1, 1), every chain within the gate of the oracle's level passes"""
    from consenrich_amd import _lib as L

    what = L.EXPORT_FORWARD | L.EXPORT_SMOOTH | L.EXPORT_RESID
    _b, base, base_sums = level
    runs = {"forward_backward": (base, base_sums)}
    with _new_batch(sets) as b:
        b.stats()
        sums = b.forward(L.RETURN_NLL)
        b.backward()
        b.export(what)
        runs["forward+backward"] = (_downloads(b), sums)
    with _new_batch(sets) as b:
        sums = b.step(L.RETURN_NLL, what)
        runs["step"] = (_downloads(b), sums)
    with _new_batch(sets) as b:
        sums = b.step_forward(L.RETURN_NLL, L.EXPORT_FORWARD)
        runs["step_forward"] = (_downloads(b, FIT[:4]), sums)
    for c, n in enumerate(CHAINS):
        shapes = {"D": (n,), "xf": (n, 1), "Pf": (n, 1, 1), "pnoise": (n - 1, 1, 1), "xs": (n, 1), "Ps": (n, 1, 1),
                  "lag": (n - 1, 1, 1), "resid": (n, M)}
        for a in FIT:
            assert base[(c, a)].shape == shapes[a] and base[(c, a)].dtype == np.float32
    for entry, (got, sums) in runs.items():
        for key, v in got.items():
            assert _same_bits(v, base[key]), (entry, key)
        for k in range(2):
            assert np.array_equal(_bits(np.asarray(sums[k])), _bits(np.asarray(base_sums[k]))), (entry, k, sums[k], base_sums[k])
    for c, n in enumerate(CHAINS):
        d_, v_ = sets[c]
        xf, Pf, pn, D = np.zeros((n, 1), np.float32), np.zeros((n, 1, 1), np.float32), np.zeros((n, 1, 1), np.float32), np.zeros(n, np.float32)
        r = oracle.cforwardPassLevel(matrixData=d_, matrixPluginMuncInit=v_, matrixQ0=Q_LEVEL, intervalToBlockMap=np.zeros(n, np.int32),
                                     blockCount=1, stateInit=0.0, stateCovarInit=1000.0, stateForward=xf, stateCovarForward=Pf,
                                     pNoiseForward=pn, vectorD=D, returnNLL=True)
        bw = oracle.cbackwardPassLevel(matrixData=d_, stateForward=xf, stateCovarForward=Pf, pNoiseForward=pn)
        ref = dict(D=D, xf=xf, Pf=Pf, pnoise=pn[: n - 1], xs=bw[0], Ps=bw[1], lag=bw[2][: n - 1], resid=bw[3])
        for a in FIT:
            np.testing.assert_allclose(base[(c, a)], ref[a], rtol=RTOL, atol=ATOL, err_msg=f"chain {c} {a}")
        assert base_sums[1][c] == pytest.approx(r[3], rel=1e-8, abs=1e-8), c
    assert float(np.max(base[(SHIFTED, "xs")])) < 0.0


def test_multi_chain_ecm_equals_chain_by_chain_and_the_oracle(product, oracle):
    """chains of other lengths in one lock-step loop: each equals its own batch of one bit for bit (iteration count, NLL path,
    smoothed moments, kappa) and the oracle's level ECM within the gate"""
    from consenrich_amd import _lib as L

    n_list = [1031, 65, 64, 2]
    ecm_sets = [cases.synth(n, M, SEED + 50 + c, mask_frac=0.02, outlier_frac=0.01) for c, n in enumerate(n_list)]
    kw = dict(max_iters=3, inner_iters=2, rtol=0.0, use_kappa=True)

    def run(chains):
        with _new_batch(ecm_sets, chains) as b:
            b.stats()
            outs, paths = b.ecm(**kw)
            b.export(L.EXPORT_SMOOTH | L.EXPORT_MULT)
            return [(int(o.iters_done), int(o.skipped), paths[k].copy(), b.download(k, "xs"), b.download(k, "Ps"), b.download(k, "kappa"))
                    for k, o in enumerate(outs)]

    together = run(None)
    for c, n in enumerate(n_list):
        alone = run([c])[0]
        assert together[c][:2] == alone[:2], (c, together[c][:2], alone[:2])
        for k, what in ((2, "nll path"), (3, "xs"), (4, "Ps"), (5, "kappa")):
            assert _same_bits(together[c][k], alone[k]), (c, what)
        d_, v_ = ecm_sets[c]
        r = oracle.cfixedBackgroundECMLevel(matrixData=d_, matrixPluginMuncInit=v_, matrixQ0=Q_LEVEL, intervalToBlockMap=np.zeros(n, np.int32),
                                            blockCount=1, stateInit=0.0, stateCovarInit=1000.0, ECM_fixedBackgroundIters=3,
                                            ECM_fixedBackgroundRtol=0.0, ECM_useObsPrecisionReweighting=False,
                                            ECM_useProcessPrecisionReweighting=True, procPrecisionMultiplierMin=5e-3,
                                            procPrecisionMultiplierMax=5e3, t_innerIters=2, returnIntermediates=True,
                                            returnDiagnostics=True, trackOptimizationPath=True, logIterations=False)
        assert together[c][0] == r[0] and bool(together[c][1]) == bool(r[8]["skipped"]), (c, together[c][:2], r[0], r[8])
        assert together[c][3].shape == (n, 1) and together[c][4].shape == (n, 1, 1)
        np.testing.assert_allclose(together[c][3], r[2], rtol=RTOL, atol=ATOL, err_msg=f"xs chain {c}")
        np.testing.assert_allclose(together[c][4], r[3], rtol=RTOL, atol=ATOL, err_msg=f"Ps chain {c}")
        close_mostly(together[c][5], r[7], msg=f"kappa chain {c}")
    assert together[0][0] == 3 and not together[0][1]


def _record(b, c, r):
    return (b.rocco_solution(c), r["objective"], r["penalized_objective"], r["selected_count"], r["selection_penalty"])


def _same_tuple(got, ref, tag):
    """the 5-tuple of csolveChromROCCOExact, exactly"""
    assert np.array_equal(got[0], ref[0]) and got[0].dtype == np.uint8, tag
    assert got[3] == ref[3], tag
    f = lambda t: np.asarray([t[1], t[2], t[4]], np.float64).view(np.uint64)  # noqa: E731
    assert np.array_equal(f(got), f(ref)), (tag, got[1:], ref[1:])


@pytest.mark.parametrize("mode", ["state", "lower_confidence"])
def test_scores_and_selection_from_the_resident_level_fit(level, mode):
    b, base, _sums = level
    z = 0.5
    b.rocco_scores(mode, z=z)
    res = b.rocco(budget=0.1, gamma=0.5)
    floored = []
    for c, n in enumerate(CHAINS):
        xs, Ps = base[(c, "xs")], base[(c, "Ps")]
        unc = np.sqrt(Ps[:, 0, 0])
        assert unc.dtype == np.float32
        sc = twin_rocco.score_track(xs[:, 0], unc, mode, z)
        mx = float(np.max(xs[:, 0]))
        floored.append(mode == "lower_confidence" and mx > 0.0 and bool(np.any(sc == -2.0 * mx)))     # read off the twin's track
        assert _same_bits(b.download_scores(c), sc), (mode, c)
        _same_tuple(_record(b, c, res[c]), twin_rocco.csolveChromROCCOExact(sc, budget=0.1, gamma=0.5), (mode, c))
        sol = b.rocco_solution(c)
        for gap in (0, 1):
            got, ref = b.rocco_runs(c, gap), twin_rocco.cBooleanRunBounds(sol, gap)
            assert got[0].dtype == np.int64 and np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), (mode, c, gap)
    if mode == "lower_confidence":
        assert any(floored) and not floored[SHIFTED] and float(np.max(base[(SHIFTED, "xs")])) <= 0.0
    for key, v in base.items():         # the scores read the fit and change none of its arrays
        assert _same_bits(b.download(*key), v), key


def test_peak_driver_on_the_level_batch_equals_the_twin(level):
    from consenrich_amd import driver

    b, base, _sums = level
    peaks = driver.call_peaks_batch(b, budget=0.05, gamma=0.5, score_mode="lower_confidence", z=1.0, max_gap_bins=1)
    for c, r in enumerate(peaks):
        sc = twin_rocco.score_track(base[(c, "xs")][:, 0], np.sqrt(base[(c, "Ps")][:, 0, 0]), "lower_confidence", 1.0)
        ref = twin_rocco.csolveChromROCCOExact(sc, budget=0.05, gamma=0.5)
        _same_tuple(_record(b, c, r), ref, c)
        runs = twin_rocco.cBooleanRunBounds(ref[0], 1)
        assert np.array_equal(r["starts"], runs[0]) and np.array_equal(r["ends"], runs[1]) and r["selected_count"] == int(ref[0].sum())
    for key, v in base.items():
        assert _same_bits(b.download(*key), v), key


@pytest.mark.parametrize("use_lambda", [False, True], ids=["plain", "lambda"])
def test_gain_summary_of_the_level_model_equals_the_reference_expression(product, use_lambda):
    """`_finalForwardReplicateGainContigSummary` (core.py:7671-7731) restated with NumPy on the downloaded (n, 1, 1) covariance, as
    tests/test_gpu_residency.py does for the levelTrend model, with that test's tolerances"""
    from consenrich_amd import _lib as L

    n_list = [1, 2, 5, 64, 65, 1031]
    mp = _model()
    g_sets = [cases.synth(n, M, SEED + 100 + c, mask_frac=0.02, outlier_frac=0.01) for c, n in enumerate(n_list)]
    with _new_batch(g_sets) as b:
        if use_lambda:
            for c, n in enumerate(n_list):
                b.upload_multipliers(c, cases.multipliers(n, SEED + 100 + c)[0], None, None)
        b.stats()
        b.forward(L.RETURN_NLL | (L.USE_LAMBDA if use_lambda else 0))
        b.export(L.EXPORT_FORWARD | L.EXPORT_MULT)
        for c, n in enumerate(n_list):
            got = b.gain_summary(c, 1.0e-4, use_lambda=use_lambda, lambda_bounds=mp.lambda_bounds)
            Pf = b.download(c, "Pf")
            assert Pf.shape == (n, 1, 1)
            p00 = np.maximum(Pf.astype(np.float64)[:, 0, 0], 0.0)
            prec = np.clip(b.download(c, "lambda").astype(np.float64), *mp.lambda_bounds) if use_lambda else np.ones(n)
            for j in range(M):
                g = (p00 * prec) / np.maximum(g_sets[c][1][j].astype(np.float64) + 1.0e-4, 1.0e-12)
                g = g[np.isfinite(g)]
                assert got["count"][j] == g.size == n
                q25, q75 = np.quantile(g, [0.25, 0.75])
                assert got["median"][j] == float(np.median(g)), (c, j)
                assert got["iqr"][j] == float(q75 - q25), (c, j)
                assert got["mean"][j] == pytest.approx(float(np.mean(g)), rel=1e-12)
                assert got["sd"][j] == pytest.approx(float(np.std(g)), rel=1e-10, abs=1e-300)


def test_batch_diagnostics_of_the_level_model_equal_the_oracle(product, sets):
    from consenrich_amd import _lib as L
    from oracle import diagnostics as orc

    mp = _model()
    for flags in (L.USE_LAMBDA | L.USE_KAPPA | L.USE_QSCALE, 0):
        with _new_batch(sets) as b:
            mult = [cases.multipliers(n, SEED + c) for c, n in enumerate(CHAINS)]
            for c, (lam, kap, qs) in enumerate(mult):
                b.upload_multipliers(c, lam, kap, qs)
            b.stats()
            b.forward(L.RETURN_NLL | flags)
            b.diagnostics(flags)
            for c, n in enumerate(CHAINS):
                lam, kap, qs = mult[c]
                Pf, pn = b.download(c, "Pf"), b.download(c, "pnoise")
                assert Pf.shape == (n, 1, 1) and pn.shape == (n - 1, 1, 1)
                use = flags != 0
                ref = orc.output_diagnostic_tracks(
                    stateCovarForward=Pf, matrixMunc=sets[c][1], matrixQ0=np.asarray(mp.Q0, np.float32),
                    matrixF=np.asarray(cases.F_TREND, np.float32), stateCovarInit=mp.state_covar_init, state_dim=1,
                    lambdaExp=lam if use else None, processPrecExp=kap if use else None,
                    processQScale=qs if use else None, pNoiseForward=None if use else pn, pad=mp.pad,
                    obsPrecisionMultiplierMin=mp.lambda_bounds[0], obsPrecisionMultiplierMax=mp.lambda_bounds[1],
                    procPrecisionMultiplierMin=mp.kappa_bounds[0], procPrecisionMultiplierMax=mp.kappa_bounds[1])
                for k in ("sumGain0", "sumGain1", "effectiveQLevel", "effectiveQTrend", "muncTrace"):
                    np.testing.assert_allclose(b.download(c, k), ref[k], rtol=RTOL, atol=0, err_msg=f"{flags} {c} {k}")


def test_writers_of_the_level_tracks(level):
    """state (4-decimal float32 rounding) and uncertainty (sqrt of the variance) tracks of every chain: bedGraph text against the
    reference's pandas call, bigWig items, section headers, summary and zoom records against tests/writer_refs.py; 200-base
    intervals, the last one clipped"""
    from consenrich_amd import _lib as L

    b, base, _sums = level
    step = 200
    for c, n in enumerate(CHAINS):
        cap = n * step - 13
        wr.check_resident_track(b, c, "xs", 0, "round4", np.ascontiguousarray(base[(c, "xs")][:, 0]), c + 1, 0, step, cap, ("xs", c))
        wr.check_resident_track(b, c, "Ps", 0, "sqrt", np.ascontiguousarray(base[(c, "Ps")][:, 0, 0]), c + 1, 0, step, cap, ("Ps", c))
        for name in ("xs", "Ps"):
            with pytest.raises(L.ConsenrichAMDError, match="component out of range"):
                b.bedgraph_bytes(c, name, "chr1", 0, step, comp=1)
