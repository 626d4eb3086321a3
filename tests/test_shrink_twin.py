"""State shrinkage without a GPU: the pure-Python twin against the fixtures the compiled reference wrote, the product's EM loop
(`shrink.fit_state_shrinkage_prior`) over the sequential twin against every fixture prior bit for bit -- which pins the M-step,
the back-tracking path and both stop rules -- the apply step's metadata, the reference's error texts before any launch, the new
symbols, and the loud failure without a device."""
import json
import os

import numpy as np
import pytest

import shrink_cases as sc
import twin_shrink as tw
from consenrich_amd import _lib as L
from consenrich_amd import cconsenrich as cc
from consenrich_amd import shrink as S

FIT_IDS = [sc.fit_name(*f) for f in sc.FITS]


@pytest.fixture(scope="module")
def inputs():
    return {name: sc.make_input(name) for name in sc.INPUTS}


def _quadrature(fx):
    return (fx["nodes"], fx["weights"]) if "nodes" in fx else None


def _dumps(d):
    return json.dumps(d, sort_keys=True)


def test_symbols_and_exports():
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "consenrich_amd.h")) as fh:
        header = fh.read()
    for name in ("csr_shrink_stage", "csr_batch_shrink_prepare", "csr_shrink_initial_sums", "csr_shrink_em_step", "csr_shrink_posterior",
                 "csr_batch_shrink_posterior", "csr_batch_shrink_download", "csr_batch_shrink_medians", "csr_batch_set_export_signal"):
        assert name in L.SYMBOLS and hasattr(L.lib(), name) and f"int {name}(" in header
    for name in ("cstateShrinkInitialSums", "cstateShrinkMixtureEMStep", "cstateShrinkMixtureEMStepPrepared",
                 "cstateShrinkMixturePosterior", "cstateShrinkMixturePosteriorPrepared"):
        assert name in cc.__all__ and getattr(cc, name) is getattr(S, name)
    assert S.fitStateShrinkagePrior is S.fit_state_shrinkage_prior and S.shrinkStateEB is S.shrink_state_eb


@pytest.mark.parametrize("fit", sc.FITS, ids=FIT_IDS)
def test_twin_sums_against_fixture(fit, inputs):
    """The sequential twin equals the natives' sums; the device's tree over the same terms stays within 1e-12 of the sum of
    |terms| (measured here: below 1e-15), which is the gate the device is held to."""
    fx = sc.load_fixture(*fit)
    chunks, block = inputs[fit[0]]
    pi0, tau, lsp = float(fx["em_pi0"]), fx["em_tau"], fx["em_lsp"]
    seq, tree = tw.SequentialPasses(chunks, block), tw.TreePasses(chunks, block)
    assert np.array_equal(np.array(seq.initial_rows(1.5)), fx["init_sums"])
    assert np.array_equal(np.array(seq.em_rows(pi0, tau, lsp)), fx["em_sums"])
    assert np.array_equal(np.array(tree.abs_initial_rows(1.5)), fx["init_abs"])
    assert np.array_equal(np.array(tree.abs_rows(pi0, tau, lsp)), fx["em_abs"])
    for got, want, scale in ((np.array(tree.initial_rows(1.5)), fx["init_sums"], fx["init_abs"]),
                             (np.array(tree.em_rows(pi0, tau, lsp)), fx["em_sums"], fx["em_abs"])):
        assert np.all(np.abs(got - want) <= 1.0e-12 * scale)
    assert np.array_equal(np.array(tree.em_rows(pi0, tau, lsp))[:, 3], fx["em_sums"][:, 3])       # finiteCount: exact


@pytest.mark.parametrize("fit", sc.FITS, ids=FIT_IDS)
def test_fit_loop_reproduces_the_reference_prior(fit, inputs):
    fx = sc.load_fixture(*fit)
    chunks, block = inputs[fit[0]]
    passes = tw.SequentialPasses(chunks, block)
    prior = S.fit_state_shrinkage_prior(passes=passes, blockSize=block, quadrature=_quadrature(fx), **sc.fit_kwargs(fit[1], fit[2]))
    want = json.loads(str(fx["prior_json"]))
    got = {"model": prior.model, "priorSpikeProp": prior.priorSpikeProp, "priorScale": prior.priorScale,
           "priorVariance": prior.priorVariance, "blockSize": prior.blockSize, "slabVariance": list(prior.slabVariance),
           "slabWeight": list(prior.slabWeight), "componentWeights": list(prior.componentWeights)}
    assert _dumps(got) == _dumps(want)
    assert _dumps(prior.metadata) == _dumps(json.loads(str(fx["meta_json"])))
    assert list(prior.metadata) == list(json.loads(str(fx["meta_json"])))          # every key, in the reference's order


def test_fixtures_cover_the_paths():
    """What the case table has to exercise: a Student-t fit that ends after one iteration through twelve rejected trials, fits that
    converge and fits that reach the cap, every slab count, and an adaptive mixture that is not stable against 1e-11."""
    metas = {f: json.loads(str(sc.load_fixture(*f)["meta_json"])) for f in sc.FITS}
    one = metas[("a_b1", sc.STUDENT, 16)]
    assert one["iterations"] == 1 and one["converged"] is True
    passes = tw.SequentialPasses(*sc.make_input("a_b1"))
    fx = sc.load_fixture("a_b1", sc.STUDENT, 16)
    S.fit_state_shrinkage_prior(passes=passes, blockSize=1, quadrature=_quadrature(fx), model=sc.STUDENT, studentTQuadratureOrder=16)
    assert passes.passes == 1 + 1 + S.BACKTRACK_TRIALS       # the E-step, the proposal, twelve trials
    assert {m["slab_count"] for m in metas.values()} == {1, 5, 8, 12, 16, 96}
    assert any(m["iterations"] == 96 and not m["converged"] for m in metas.values())
    assert any(1 < m["iterations"] < 96 and m["converged"] for m in metas.values())
    stable = {f: bool(sc.load_fixture(*f)["stable"]) for f in sc.FITS}
    assert all(v for f, v in stable.items() if f[1] != sc.MIXTURE)
    assert not stable[("c_b7", sc.MIXTURE, 0)] and any(v for f, v in stable.items() if f[1] == sc.MIXTURE)


@pytest.mark.parametrize("fit", sc.POSTERIORS, ids=[sc.fit_name(*f) for f in sc.POSTERIORS])
def test_twin_posterior_and_apply_metadata(fit, inputs):
    fx = sc.load_fixture(*fit)
    chunks, _ = inputs[fit[0]]
    want = json.loads(str(fx["prior_json"]))
    prior = S.stateShrinkPrior(want["model"], want["priorSpikeProp"], want["priorScale"], want["priorVariance"], want["blockSize"],
                               json.loads(str(fx["meta_json"])), tuple(want["slabVariance"]), tuple(want["slabWeight"]),
                               tuple(want["componentWeights"]))
    assert float(fx["ratio_max"]) <= 1.0e6
    metas, at = json.loads(str(fx["apply_json"])), 0
    for (x, v), meta in zip(chunks, metas):
        res = S.apply_state_shrinkage_prior(x, v, prior, stateShrinkageSpikeOddsMultiplier=2.0, posterior=tw.posterior)
        got = [res.shrunkState, res.posteriorSd, res.spikeProp, res.slabPosteriorMean, res.slabPosteriorWeight]
        for k in range(5):
            assert np.array_equal(got[k].view(np.uint32), fx["post"][k, at:at + x.size].view(np.uint32)), k
        assert _dumps(res.metadata) == _dumps(meta) and list(res.metadata) == list(meta)
        at += x.size


def test_floor_case_in_the_twin():
    x, v = sc.floor_case()
    tau, w = np.array([0.5, 4.0]), np.array([0.5, 0.5])
    out = tw.posterior(x, v, 0.9, tau, S.log_slab_prior(0.9, w))
    assert np.all(np.isfinite(out[1])) and np.all(out[1] >= np.float32(1.0e-6))


# ---------------------------------------------------------------------------------------------------------------
# argument checks: the reference's texts, raised before anything reaches a device
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture
def no_device(monkeypatch):
    """Any path that reaches the device fails the test: the checks below must come first."""
    def boom(*a, **k):
        raise AssertionError("a device call was reached before the argument check")

    monkeypatch.setattr(L, "require_gpu", boom)
    monkeypatch.setattr(S, "_stage", boom)


X, V = np.array([0.5, -1.0, 2.0]), np.array([1.0, 0.5, 0.25])


@pytest.mark.parametrize("call, text", [
    (lambda: S.cstateShrinkInitialSums(X, V[:2], 1.5, 1), "state and variance must have the same length"),
    (lambda: S.cstateShrinkMixtureEMStepPrepared(X, V[:2], 0.5, [1.0], [0.0], 1), "state and variance must have the same length"),
    (lambda: S.cstateShrinkMixtureEMStepPrepared(X, V, 0.5, [[1.0]], [0.0], 1), "slabVariance must be one-dimensional"),
    (lambda: S.cstateShrinkMixtureEMStepPrepared(X, V, 0.5, [1.0], [[0.0]], 1), "logSlabPrior must be one-dimensional"),
    (lambda: S.cstateShrinkMixtureEMStepPrepared(X, V, 0.5, [], [], 1), "slab arrays must be nonempty"),
    (lambda: S.cstateShrinkMixtureEMStepPrepared(X, V, 0.5, [1.0, 2.0], [0.0], 1), "slabVariance and logSlabPrior must have the same length"),
    (lambda: S.cstateShrinkMixtureEMStepPrepared(X, V, 1.0, [1.0], [0.0], 1), "priorSpikeProp must be finite with 0 < priorSpikeProp < 1"),
    (lambda: S.cstateShrinkMixtureEMStepPrepared(X, V, float("nan"), [1.0], [0.0], 1), "priorSpikeProp must be finite with 0 < priorSpikeProp < 1"),
    (lambda: S.cstateShrinkMixtureEMStepPrepared(X, V, 0.5, [0.0], [0.0], 1), "slabVariance must contain only positive finite values"),
    (lambda: S.cstateShrinkMixtureEMStepPrepared(X, V, 0.5, np.ones(97), np.zeros(97), 1), "slab arrays must hold 1 to 96 slabs"),
    (lambda: S.cstateShrinkMixtureEMStep(X, V, 0.5, [1.0], [[1.0]], 1), "slabWeight must be one-dimensional"),
    (lambda: S.cstateShrinkMixtureEMStep(X, V, 0.5, [1.0, 2.0], [1.0], 1), "slabVariance and slabWeight must have the same length"),
    (lambda: S.cstateShrinkMixtureEMStep(X, V, 0.5, [1.0], [-1.0], 1), "slabWeight must contain only finite nonnegative values with positive sum"),
    (lambda: S.cstateShrinkMixtureEMStep(X, V, 0.5, [1.0], [0.0], 1), "slabWeight must contain only finite nonnegative values with positive sum"),
    (lambda: S.cstateShrinkMixtureEMStep(X, V, 0.5, [np.inf], [1.0], 1), "slabVariance must contain only positive finite values"),
    (lambda: S.cstateShrinkMixturePosteriorPrepared(X, V, 0.0, [1.0], [0.0]), "priorSpikeProp must be finite with 0 < priorSpikeProp < 1"),
    (lambda: S.cstateShrinkMixturePosteriorPrepared(X, V, 0.5, [-1.0], [0.0]), "slabVariance must contain only positive finite values"),
    (lambda: S.cstateShrinkMixturePosterior(X, V, 0.5, [1.0], [np.nan]), "slabWeight must contain only finite nonnegative values with positive sum"),
    (lambda: S.fit_state_shrinkage_prior([]), "state shrinkage prior fit requires at least one chunk"),
    (lambda: S.fit_state_shrinkage_prior([(X, V)], model="nope"), "Unsupported state shrinkage model 'nope'"),
    (lambda: S.fit_state_shrinkage_prior([(X, V)], studentTDF=0.5), "`studentTDF` must be numeric with 1 <= studentTDF <= 30"),
    (lambda: S.fit_state_shrinkage_prior([(X, V)], studentTQuadratureOrder=7), "`studentTQuadratureOrder` must be an integer with 8 <= order <= 96"),
    (lambda: S.fit_state_shrinkage_prior([(X, V[:2])]), "`state` and `stateVariance` must have the same length"),
    (lambda: S.fit_state_shrinkage_prior([(X.reshape(1, 3), V)]), "`state` must be one-dimensional"),
    (lambda: S.fit_state_shrinkage_prior([{"state": X}]), "state shrinkage item is missing `state`/`variance`"),
    (lambda: S.fit_state_shrinkage_prior([(X, V)], minNull=0.6, maxNull=0.5), "`minNull` must be smaller than `maxNull`"),
    (lambda: S.apply_state_shrinkage_prior(X, V, S.stateShrinkPrior("spikeAndNormal", 0.5, 1.0, 1.0, 1, {}),
                                           stateShrinkageSpikeOddsMultiplier=0.0), "`stateShrinkageSpikeOddsMultiplier` must be finite and positive"),
    (lambda: S.apply_state_shrinkage_prior(X, V, S.stateShrinkPrior("spikeAndNormal", 1.5, 1.0, 1.0, 1, {})),
     "`priorSpikeProp` must be finite and strictly between 0 and 1"),
])
def test_error_texts_come_before_any_launch(no_device, call, text):
    with pytest.raises(ValueError) as e:
        call()
    assert text in str(e.value)


def test_late_errors_of_the_fit_with_an_injected_evaluator():
    """No valid bin anywhere, bad fixed parameters: the reference's texts, decided from the evaluator's sums."""
    x, v = np.array([np.nan, 1.0, np.inf]), np.array([1.0, -1.0, 1.0])
    with pytest.raises(ValueError, match="state shrinkage prior fit has no finite positive-variance intervals"):
        S.fit_state_shrinkage_prior(passes=tw.SequentialPasses([(x, v)], 1))
    ok = tw.SequentialPasses([(X, V)], 1)
    with pytest.raises(ValueError, match="`priorScale` must be finite and positive"):
        S.fit_state_shrinkage_prior(passes=ok, priorScale=-1.0)
    with pytest.raises(ValueError, match="`priorSpikeProp` must be finite and strictly between 0 and 1"):
        S.fit_state_shrinkage_prior(passes=ok, priorSpikeProp=1.0)
    with pytest.raises(ValueError, match="`stateShrinkageSpikePseudoCount` must be nonnegative"):
        S.fit_state_shrinkage_prior(passes=ok, stateShrinkageSpikePseudoCount=-1.0)
    with pytest.raises(ValueError, match="Student-t quadrature produced invalid nodes or weights"):
        S.fit_state_shrinkage_prior(passes=ok, quadrature=(np.ones(11), np.ones(11)))


def test_fixed_parameters_skip_the_loop():
    """spikeAndNormal with both parameters given: nothing is estimated, no EM pass runs, the reference's `iterations` of 0."""
    passes = tw.SequentialPasses([(X, V)], 1)
    prior = S.fit_state_shrinkage_prior(passes=passes, model=sc.NORMAL, priorSpikeProp=0.7, priorScale=2.0)
    assert passes.passes == 0 and prior.metadata["iterations"] == 0 and prior.metadata["converged"] is True
    assert prior.priorSpikeProp == 0.7 and prior.slabVariance == (4.0,) and prior.slabWeight == (1.0,)


def test_no_device_fails_loudly(monkeypatch):
    """Without a device the natives and the fit raise the library's error; nothing is computed on the host instead."""
    monkeypatch.setattr(L, "device_count", lambda: 0)
    for call in (lambda: S.cstateShrinkInitialSums(X, V, 1.5, 1),
                 lambda: S.cstateShrinkMixtureEMStep(X, V, 0.5, [1.0], [1.0], 1),
                 lambda: S.cstateShrinkMixturePosterior(X, V, 0.5, [1.0], [1.0]),
                 lambda: S.fit_state_shrinkage_prior([(X, V)], model=sc.NORMAL),
                 lambda: S.shrink_state_eb(X, V, model=sc.NORMAL)):
        with pytest.raises(L.ConsenrichAMDError, match="no CPU fallback"):
            call()
