"""State shrinkage on the device against the fixtures the compiled reference wrote (tests/golden/make_shrink_golden.py) and against
the twin (tests/twin_shrink.py).  Bit for bit is not available -- the reference adds bin after bin with the C library's log and
exp, the device adds in a fixed tree with its own -- so the contract is split:

  (a) every per-pass sum within 1e-12 of the sum of |terms| (the twin supplies it; for the positive sums that is the sum itself),
      finiteCount exact; the worst ratio seen is printed (measured 1e-15 .. 1.85e-13; the two cases above a tenth of the gate are
      the reference's own drift -- adding the same 1 / block thousands of times -- not the device's: against exact sums the
      sequential form is off by 1.85e-13 on the 20 000-bin chain, the device's tree by 5.7e-16; CHANGELOG);
  (b) a whole fit: iterations and converged equal, every float of the prior and of the metadata within 1e-9 relative, everything
      else equal -- for the adaptive mixture only on the cases whose fixture says the reference's own loop is stable against
      noise of 1e-11 (it re-sorts its slabs in the M-step; tests/test_shrink_twin.py pins which cases are not);
  (c) posterior tracks with the same prior: NaN pattern and the invalid bins' float32(x) bit-equal, every valid bin within 1
      float32 ulp and at most 0.1 % of them different at all, the posterior sd within 2 ulps (every bin of these cases has
      postSecond / postVariance <= 1e6), and the floor case finite and >= 1e-6;
  (d) exact relations: two identical calls return identical bits; one staged call for all chunks equals the chunk-by-chunk calls;
      the resident path equals the host-array path on the downloaded tracks; the medians equal np.median of the downloaded tracks;
      narrowPeak and broadPeak rows with signal="shrunk" equal the twins fed with the downloaded shrunk track, and with
      signal="state" what they returned before.
Tile edges: chains of W - 1, W, W + 1 and 2 W + 1 bins for the pass kernels' tile width W = 256, a block size that does not divide
W, one larger than the chain, and slab counts on both sides of the register / recompute switch (16 | 17)."""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import shrink_cases as sc  # noqa: E402
import twin_shrink as tw  # noqa: E402

pytestmark = pytest.mark.gpu
GATE = 1.0e-12
FIT_IDS = [sc.fit_name(*f) for f in sc.FITS]
# (b) is asserted where the reference's own loop is stable (the flag of the fixture)
STABLE_FITS = [f for f in sc.FITS if bool(sc.load_fixture(*f)["stable"])]


@pytest.fixture(scope="module")
def S():
    from consenrich_amd import _lib, shrink

    _lib.require_gpu()
    return shrink


@pytest.fixture(scope="module")
def inputs():
    return {name: sc.make_input(name) for name in sc.INPUTS}


def quadrature(fx):
    return (fx["nodes"], fx["weights"]) if "nodes" in fx else None


def em_row(t):
    return np.array([t[0], t[1], t[4], float(t[5]), *t[2], *t[3]], dtype=np.float64)


def init_row(t):
    return np.array([*t[:4], float(t[4])], dtype=np.float64)


def worst_ratio(got, want, scale):
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.abs(got - want) / scale
    return float(np.nanmax(np.where(scale > 0.0, r, np.where(got == want, 0.0, np.inf)))) if got.size else 0.0


def ulps32(a, b):
    """Distance in float32 ulps (finite values)."""
    def key(x):
        i = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


def bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------
# (a) per-pass sums
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fit", sc.FITS, ids=FIT_IDS)
def test_pass_sums_against_the_reference(S, fit, inputs):
    fx = sc.load_fixture(*fit)
    chunks, block = inputs[fit[0]]
    pi0, tau, lsp = float(fx["em_pi0"]), fx["em_tau"], fx["em_lsp"]
    init = np.array([init_row(S.cstateShrinkInitialSums(x, v, 1.5, block)) for x, v in chunks])
    em = np.array([em_row(S.cstateShrinkMixtureEMStepPrepared(x, v, pi0, tau, lsp, block)) for x, v in chunks])
    r_init, r_em = worst_ratio(init, fx["init_sums"], fx["init_abs"]), worst_ratio(em, fx["em_sums"], fx["em_abs"])
    print(f"{sc.fit_name(*fit)}: worst |device - reference| / sum|terms|: initial {r_init:.3g}, EM pass {r_em:.3g} (gate {GATE:g})")
    assert np.array_equal(init[:, 4], fx["init_sums"][:, 4]) and np.array_equal(em[:, 3], fx["em_sums"][:, 3])
    assert r_init <= GATE and r_em <= GATE
    # one staged call for all chunks, and the same call again: identical bits
    passes = S.HostArrayPasses(chunks, block)
    for _ in range(2):
        assert np.array_equal(np.array([init_row(t) for t in passes.initial_sums(1.5)]), init)
        assert np.array_equal(np.array([em_row(t) for t in passes.em_step(pi0, tau, lsp)]), em)


def test_em_step_from_weights_builds_the_same_prior(S, inputs):
    chunks, block = inputs["a_b64"]
    x, v = chunks[1]
    tau, w, pi0 = np.array([0.3, 2.0, 11.0]), np.array([2.0, 0.0, 6.0]), 0.7
    lsp = np.array([np.log(0.3) + np.log(0.25), -np.inf, np.log(0.3) + np.log(0.75)])
    a = em_row(S.cstateShrinkMixtureEMStep(x, v, pi0, tau, w, block))
    want = tw.TreePasses([(x, v)], block)
    b = np.array(want.em_rows(pi0, tau, lsp))[0]
    assert worst_ratio(a, b, np.array(want.abs_rows(pi0, tau, lsp))[0]) <= GATE
    assert a[4 + 1] == 0.0 and a[4 + 3 + 1] == 0.0          # a slab of weight zero takes no mass


EDGE_LENS = (255, 256, 257, 513)


@pytest.mark.parametrize("block", [1, 7, 1000])
@pytest.mark.parametrize("k", [1, 16, 17])
def test_tile_edges(S, block, k):
    rng = np.random.default_rng(100 + k)
    chunks = [sc.synth_chunk(n, rng, (7, 14) if block == 7 else None) for n in EDGE_LENS]
    tau = np.geomspace(0.2, 30.0, k)
    lsp = S.log_slab_prior(0.8, np.linspace(1.0, 2.0, k))
    seq, tree = tw.SequentialPasses(chunks, block), tw.TreePasses(chunks, block)
    passes = S.HostArrayPasses(chunks, block)
    got_i = np.array([init_row(t) for t in passes.initial_sums(1.5)])
    got_e = np.array([em_row(t) for t in passes.em_step(0.8, tau, lsp)])
    r_i = worst_ratio(got_i, np.array(seq.initial_rows(1.5)), np.array(tree.abs_initial_rows(1.5)))
    r_e = worst_ratio(got_e, np.array(seq.em_rows(0.8, tau, lsp)), np.array(tree.abs_rows(0.8, tau, lsp)))
    print(f"tile edges block {block} K {k}: worst ratio initial {r_i:.3g}, EM pass {r_e:.3g}")
    assert r_i <= GATE and r_e <= GATE
    assert np.array_equal(got_e[:, 3], np.array(seq.em_rows(0.8, tau, lsp))[:, 3])
    # the initial sums hold products and sums of the inputs only: the tree twin is the device, bit for bit
    assert np.array_equal(got_i, np.array(tree.initial_rows(1.5)))


# ---------------------------------------------------------------------------------------------------------------
# (b) whole fits
# ---------------------------------------------------------------------------------------------------------------
def assert_close_meta(got, want, where=""):
    assert list(got) == list(want), where
    for key, w in want.items():
        g = got[key]
        if isinstance(w, float) and not isinstance(w, bool):
            assert isinstance(g, float) and (abs(g - w) <= 1.0e-9 * abs(w) or (g != g and w != w)), (where, key, g, w)
        elif isinstance(w, list):
            assert len(g) == len(w) and all(abs(a - b) <= 1.0e-9 * abs(b) for a, b in zip(g, w)), (where, key)
        else:
            assert g == w and type(g) is type(w), (where, key, g, w)


@pytest.mark.parametrize("fit", STABLE_FITS, ids=[sc.fit_name(*f) for f in STABLE_FITS])
def test_whole_fit_against_the_reference(S, fit, inputs):
    fx = sc.load_fixture(*fit)
    chunks, block = inputs[fit[0]]
    prior = S.fit_state_shrinkage_prior(chunks, blockSize=block, quadrature=quadrature(fx), **sc.fit_kwargs(fit[1], fit[2]))
    want, meta = json.loads(str(fx["prior_json"])), json.loads(str(fx["meta_json"]))
    assert prior.metadata["iterations"] == meta["iterations"] and prior.metadata["converged"] == meta["converged"]
    assert_close_meta(prior.metadata, meta, sc.fit_name(*fit))
    assert prior.model == want["model"] and prior.blockSize == want["blockSize"]
    for got, ref in ((prior.priorSpikeProp, want["priorSpikeProp"]), (prior.priorScale, want["priorScale"])):
        assert abs(got - ref) <= 1.0e-9 * abs(ref)
    assert (prior.priorVariance != prior.priorVariance) if want["priorVariance"] != want["priorVariance"] else \
        abs(prior.priorVariance - want["priorVariance"]) <= 1.0e-9 * abs(want["priorVariance"])
    for key in ("slabVariance", "slabWeight", "componentWeights"):
        got = np.array(getattr(prior, key))
        assert got.shape == np.array(want[key]).shape and np.all(np.abs(got - want[key]) <= 1.0e-9 * np.abs(want[key])), key
    worst = max(float(np.max(np.abs(np.array(getattr(prior, k)) / np.array(want[k]) - 1.0))) for k in ("slabVariance", "slabWeight"))
    print(f"{sc.fit_name(*fit)}: iterations {meta['iterations']}, worst relative parameter difference {worst:.3g} (gate 1e-9)")


def test_scipy_quadrature_is_the_default(S, inputs):
    """Without `quadrature` the rule comes from SciPy (imported lazily): the same prior as with the fixture's rule as data."""
    fx = sc.load_fixture("c_b7", sc.STUDENT, 16)
    chunks, block = inputs["c_b7"]
    a = S.fit_state_shrinkage_prior(chunks, blockSize=block, studentTQuadratureOrder=16)
    b = S.fit_state_shrinkage_prior(chunks, blockSize=block, studentTQuadratureOrder=16, quadrature=quadrature(fx))
    assert json.dumps(a.metadata) == json.dumps(b.metadata) and a.slabVariance == b.slabVariance


def test_invalid_chunks(S):
    """A chunk without a valid bin contributes nothing and the others still fit; no valid bin anywhere is the reference's error."""
    rng = np.random.default_rng(3)
    good = [sc.synth_chunk(300, rng), sc.synth_chunk(200, rng)]
    dead = (np.full(150, np.nan), np.full(150, -1.0))
    with_dead = S.fit_state_shrinkage_prior([good[0], dead, good[1]], blockSize=16, model=sc.NORMAL)
    without = S.fit_state_shrinkage_prior(good, blockSize=16, model=sc.NORMAL)
    assert with_dead.slabVariance == without.slabVariance and with_dead.priorSpikeProp == without.priorSpikeProp
    assert with_dead.metadata["finite_count"] == without.metadata["finite_count"]
    assert with_dead.metadata["chunk_count"] == 3 and with_dead.metadata["interval_count"] == 650
    assert S.cstateShrinkInitialSums(*dead, 1.5, 16) == (0.0, 0.0, 0.0, 0.0, 0)
    assert S.cstateShrinkInitialSums([], [], 1.5, 4) == (0.0, 0.0, 0.0, 0.0, 0)              # the natives take an empty vector
    empty = S.cstateShrinkMixtureEMStepPrepared([], [], 0.5, [1.0, 2.0], [0.0, 0.0], 0)
    assert empty[0] == 0.0 and empty[5] == 0 and empty[2].tolist() == [0.0, 0.0] and empty[3].tolist() == [0.0, 0.0]
    assert [a.shape for a in S.cstateShrinkMixturePosterior([], [], 0.5, [1.0], [1.0])] == [(0,)] * 5
    with pytest.raises(ValueError, match="state shrinkage prior fit has no finite positive-variance intervals"):
        S.fit_state_shrinkage_prior([dead, dead], blockSize=4)
    res = S.shrink_state_eb(*good[0], model=sc.NORMAL, blockSize=16)
    assert res.shrunkState.dtype == np.float32 and res.metadata["scope"] == "contig_apply" and np.isnan(res.shrunkState[3])


# ---------------------------------------------------------------------------------------------------------------
# (c) posterior tracks
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fit", sc.POSTERIORS, ids=[sc.fit_name(*f) for f in sc.POSTERIORS])
def test_posterior_tracks_against_the_reference(S, fit, inputs):
    fx = sc.load_fixture(*fit)
    chunks, _ = inputs[fit[0]]
    pi0, tau, lsp = float(fx["post_pi0"]), fx["post_tau"], fx["post_lsp"]
    at, differing, valid_total, worst, worst_sd = 0, 0, 0, 0, 0
    for x, v in chunks:
        got = S.cstateShrinkMixturePosteriorPrepared(x, v, pi0, tau, lsp)
        again = S.cstateShrinkMixturePosteriorPrepared(x, v, pi0, tau, lsp)
        want = fx["post"][:, at:at + x.size]
        ok = tw.valid_mask(x, v)
        for k in range(5):
            assert got[k].dtype == np.float32 and np.array_equal(bits32(got[k]), bits32(again[k]))
            assert np.array_equal(bits32(got[k][~ok]), bits32(want[k][~ok])), k         # float32(x) and the NaNs, bit for bit
            assert not np.any(np.isnan(got[k][ok]))
            d = ulps32(got[k][ok], want[k][ok])
            if k == 1:
                worst_sd = max(worst_sd, int(d.max()) if d.size else 0)
                assert np.all(d <= 2), k
            else:
                worst = max(worst, int(d.max()) if d.size else 0)
                differing += int(np.count_nonzero(d))
                assert np.all(d <= 1), k
        valid_total += 4 * int(np.count_nonzero(ok))
        at += x.size
    print(f"{sc.fit_name(*fit)}: {differing} of {valid_total} valid values differ (worst {worst} ulp; posterior sd worst {worst_sd} ulp)")
    assert differing <= 1.0e-3 * valid_total


def test_posterior_floor(S):
    x, v = sc.floor_case()
    tau, w = np.array([0.5, 4.0]), np.array([0.5, 0.5])
    out = S.cstateShrinkMixturePosterior(x, v, 0.9, tau, w)
    assert np.all(np.isfinite(out[1])) and np.all(out[1] >= np.float32(1.0e-6))
    assert np.all(np.isfinite(out[0]))


# ---------------------------------------------------------------------------------------------------------------
# the resident path
# ---------------------------------------------------------------------------------------------------------------
FIT_ARRAYS = ("D", "xf", "Pf", "pnoise", "xs", "Ps", "lag")
LENS = [700, 1300, 257, 513]
TAKE = [True, True, False, True]


def float32_variance(unc):
    """The reference CLI's three float32 steps (consenrich.py:9634-9641)."""
    v = np.ascontiguousarray(unc, dtype=np.float32).copy()
    np.multiply(v, v, out=v)
    np.maximum(v, np.float32(1.0e-12), out=v)
    return v


def prior_key(p):
    return json.dumps([p.model, p.priorSpikeProp, p.priorScale, p.priorVariance, p.blockSize, p.slabVariance, p.slabWeight, p.metadata])


@pytest.fixture(scope="module")
def fitted():
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import cases
    from consenrich_amd import _lib as L
    from consenrich_amd.batch import DeviceBatch, ModelParams

    L.require_gpu()
    with DeviceBatch(0) as b:
        b.configure(ModelParams(state_dim=2), 3, LENS)
        for c, n in enumerate(LENS):
            b.upload(c, *cases.synth(n, 3, 770 + c))
        b.stats()
        b.forward_backward(L.RETURN_NLL)
        b.export(L.EXPORT_FORWARD | L.EXPORT_SMOOTH)
        yield b


@pytest.mark.parametrize("source", ["fit", "uncertainty"])
@pytest.mark.parametrize("model, order", [(sc.STUDENT, 16), (sc.MIXTURE, 0)])
def test_resident_fit_and_apply_equal_the_host_arrays(S, fitted, source, model, order):
    from consenrich_amd import _lib as L

    b = fitted
    nc = len(LENS)
    before = {(c, a): b.download(c, a) for c in range(nc) for a in FIT_ARRAYS}
    xs = [before[(c, "xs")][:, 0].astype(np.float64) for c in range(nc)]
    if source == "fit":
        unc = [np.sqrt(before[(c, "Ps")][:, 0, 0]) for c in range(nc)]
        variance = "fit"
    else:
        rng = np.random.default_rng(9)
        unc = [rng.uniform(0.2, 1.5, n).astype(np.float32) for n in LENS]
        unc[0][11], unc[0][12] = np.nan, 0.0                 # an invalid bin and one on the float32 floor
        variance = [unc[0], unc[1], None, unc[3]]
    var = [float32_variance(u) for u in unc]
    kw = sc.fit_kwargs(model, order)
    if model == sc.MIXTURE:
        kw["maxIter"] = 12
    prior = b.shrink_fit(chains=TAKE, variance=variance, block_size=64, **kw)
    chunks = [(xs[c], var[c].astype(np.float64)) for c in range(nc) if TAKE[c]]
    host = S.fit_state_shrinkage_prior(chunks, blockSize=64, **kw)
    assert prior_key(prior) == prior_key(host)              # the same kernels in the same tree: bit for bit
    assert prior.metadata["chunk_count"] == 3 and prior.metadata["interval_count"] == sum(n for n, t in zip(LENS, TAKE) if t)
    for c in range(nc):
        if TAKE[c]:
            assert np.array_equal(bits32(b.download_shrunk(c, "variance")), bits32(var[c])), c
    # a chain that is left out does not enter the sums
    every = b.shrink_fit(variance="fit" if source == "fit" else [unc[0], unc[1], unc[2], unc[3]], block_size=64, **kw)
    assert every.metadata["chunk_count"] == 4 and every.metadata["finite_count"] > prior.metadata["finite_count"]

    metas = b.shrink_apply(prior, spike_odds_multiplier=2.0, chains=TAKE, variance=variance, want_slab=True)
    assert metas[2] is None
    names = ("shrunk", "posterior_sd", "spike_prop", "slab_mean", "slab_weight")
    for c in range(nc):
        if not TAKE[c]:
            continue
        # (float32 inputs, as the reference's CLI passes them: np.median then combines its two middle values in float32)
        res = S.apply_state_shrinkage_prior(np.ascontiguousarray(before[(c, "xs")][:, 0]), var[c], prior,
                                            stateShrinkageSpikeOddsMultiplier=2.0)
        want = (res.shrunkState, res.posteriorSd, res.spikeProp, res.slabPosteriorMean, res.slabPosteriorWeight)
        tracks = [b.download_shrunk(c, name) for name in names]
        for t, w, name in zip(tracks, want, names):
            assert np.array_equal(bits32(t), bits32(w)), (c, name)
        # the four medians: np.median of the downloaded tracks, bit for bit (and so the host result's metadata)
        ok = tw.valid_mask(xs[c], var[c].astype(np.float64))
        x32 = before[(c, "xs")][:, 0]
        med = [float(np.median(a[ok])) for a in (np.abs(x32), np.abs(tracks[0]), tracks[2], tracks[1])]
        m = metas[c]
        assert [m["state_abs_median_before"], m["state_abs_median_after"], m["spike_prop_median"], m["posterior_sd_median"]] == med, c
        assert json.dumps(m) == json.dumps(res.metadata) and list(m) == list(res.metadata), c
        assert m["finite_count"] == int(np.count_nonzero(ok)) and m["interval_count"] == LENS[c]
    # nothing of the fit has changed
    for (c, a), v in before.items():
        assert np.array_equal(b.download(c, a).view(np.uint32), v.view(np.uint32)), (c, a)
    with pytest.raises(ValueError, match="Unknown shrinkage track"):
        b.download_shrunk(0, "nope")
    with pytest.raises(ValueError, match="priorSpikeProp must be finite"):
        L.check_value(b._lib.csr_shrink_em_step(b._ctx, 1.5, 1, L.dp(np.ones(1)), L.dp(np.zeros(1)), L.dp(np.zeros(4 * 6))))
    with pytest.raises(L.ConsenrichAMDError, match="block must be at least 1"):
        L.check_value(b._lib.csr_batch_shrink_prepare(b._ctx, None, None, 0))


def test_resident_chain_without_a_valid_bin(S, fitted):
    """One chain of the batch has no valid bin (its uploaded uncertainty is NaN throughout): it contributes nothing, the others
    still fit, and applying the prior leaves it float32(state) and NaNs, with a finite count of 0 and no medians."""
    b = fitted
    rng = np.random.default_rng(21)
    unc = [rng.uniform(0.2, 1.5, n).astype(np.float32) for n in LENS]
    unc[1][:] = np.nan
    xs = [b.download(c, "xs")[:, 0] for c in range(len(LENS))]
    prior = b.shrink_fit(chains=TAKE, variance=[unc[0], unc[1], None, unc[3]], block_size=16, model=sc.NORMAL)
    host = S.fit_state_shrinkage_prior([(xs[c].astype(np.float64), float32_variance(unc[c]).astype(np.float64)) for c in (0, 3)],
                                       blockSize=16, model=sc.NORMAL)
    assert prior.slabVariance == host.slabVariance and prior.priorSpikeProp == host.priorSpikeProp
    assert prior.metadata["chunk_count"] == 3 and prior.metadata["finite_count"] == LENS[0] + LENS[3]
    metas = b.shrink_apply(prior, chains=TAKE, variance=[unc[0], unc[1], None, unc[3]])
    assert metas[1]["finite_count"] == 0 and metas[1]["interval_count"] == LENS[1]
    assert [metas[1][k] for k in ("state_abs_median_before", "state_abs_median_after", "spike_prop_median", "posterior_sd_median")] == [None] * 4
    assert np.array_equal(bits32(b.download_shrunk(1, "shrunk")), bits32(xs[1]))
    assert np.all(np.isnan(b.download_shrunk(1, "posterior_sd"))) and np.all(np.isnan(b.download_shrunk(1, "spike_prop")))
    assert metas[0]["finite_count"] == LENS[0] and metas[0]["state_abs_median_after"] is not None
    with pytest.raises(ValueError, match="state shrinkage prior fit has no finite positive-variance intervals"):
        b.shrink_fit(chains=[False, True, False, False], variance=[None, unc[1], None, None], block_size=16)


def test_shrunk_signal_through_the_export_stages(S):
    """narrowPeak and broadPeak rows with signal="shrunk" equal the twins fed with the downloaded shrunk track; with signal="state"
    they equal what they returned before the shrinkage; a chain without a shrunk track is refused."""
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import broad_cases as BC
    import cases
    import twin_broad as TB
    import twin_narrowpeak as TN
    from consenrich_amd import _lib as L
    from consenrich_amd import driver
    from consenrich_amd.batch import DeviceBatch, ModelParams

    lens, step, names = [1500, 700, 900], 50, ["chrA", "chrB", "chrC"]
    take = [True, False, True]
    with DeviceBatch(0) as b:
        b.configure(ModelParams(state_dim=2), 3, lens)
        for c, n in enumerate(lens):
            b.upload(c, *cases.synth(n, 3, 660 + c))
        b.stats()
        b.forward_backward(L.RETURN_NLL)
        b.export(L.EXPORT_FORWARD | L.EXPORT_SMOOTH)
        b.rocco_scores("state")
        scores = [b.download_scores(c) for c in range(3)]
        strong = [(s > np.quantile(s, 0.85)).astype(np.uint8) for s in scores]
        weak = [(s > np.quantile(s, 0.70)).astype(np.uint8) for s in scores]
        for c in range(3):
            b.upload_solution(c, strong[c])
            b.upload_weak_solution(c, weak[c])
        pens, gammas = [0.05, 0.05, 0.02], [0.4, 0.4, 0.8]
        common = dict(interval_bp=step, chroms=names, prefix="cs")
        state_before = b.narrowpeak_rows(pens, gammas, **common)
        with pytest.raises(L.ConsenrichAMDError, match="chain 0 has no shrunk track"):
            b.narrowpeak_rows(pens, gammas, signal="shrunk", **common)
        with pytest.raises(L.ConsenrichAMDError, match="chain 1 has no shrunk track"):
            b.download_shrunk(1)
        fit = {(c, a): b.download(c, a) for c in range(3) for a in FIT_ARRAYS}
        prior, metas = driver.shrink_state_batch(b, block_size=25, chains=take, studentTQuadratureOrder=16)
        assert prior.metadata["chunk_count"] == 2 and metas[1] is None and metas[0]["scope"] == "contig_apply"
        with pytest.raises(L.ConsenrichAMDError, match="chain 1 has no shrunk track"):
            b.narrowpeak_rows(pens, gammas, signal="shrunk", **common)
        with pytest.raises(ValueError, match="Unknown export signal"):
            b.narrowpeak_rows(pens, gammas, signal="raw", **common)
        got = b.narrowpeak_rows(pens, gammas, signal="shrunk", chains=take, **common)
        differs = 0
        for c in (0, 2):
            x = b.download_shrunk(c, "shrunk").astype(np.float64)
            u = np.sqrt(b.download(c, "Ps")[:, 0, 0]).astype(np.float64)
            iv = np.arange(lens[c], dtype=np.int64) * step
            want = TN.rows(names[c], iv, iv + step, x, scores[c], strong[c], "cs", 0.5, uncertainty=u, trimScoreFloor=0.0,
                           subpeakSelectionPenalty=pens[c], subpeakBoundaryCost=0.25 * gammas[c], minSubpeakBins=5,
                           returnExportDetails=True, form="steps")
            assert TN.differences((got[c]["rows"], got[c]["peak_meta"], got[c]["export_details"]), want) == [], c
            assert got[c]["decided_on_host"] is False and len(want[0]) > 0
            differs += int(TN.differences(got[c]["rows"], state_before[c]["rows"]) != [])
        assert differs > 0                                  # the shrunk signal is another signal
        # the default is the state, and it returns what it returned before
        after = b.narrowpeak_rows(pens, gammas, **common)
        for c in range(3):
            assert TN.differences((after[c]["rows"], after[c]["peak_meta"], after[c]["export_details"]),
                                  (state_before[c]["rows"], state_before[c]["peak_meta"], state_before[c]["export_details"])) == [], c
        # broad rows
        b.broad_parents(float(np.quantile(scores[0], 0.6)), 0.05, 0.2, max_gap_bp=10 * step, **{k: v for k, v in common.items() if k != "prefix"},
                        chains=take)
        rows_state = b.broadpeak_rows(chains=take, **common)
        rows = b.broadpeak_rows(chains=take, signal="shrunk", **common)
        for c in (0, 2):
            x = b.download_shrunk(c, "shrunk").astype(np.float64)
            u = np.sqrt(b.download(c, "Ps")[:, 0, 0]).astype(np.float64)
            iv = np.arange(lens[c], dtype=np.int64) * step
            want = TB.rows(names[c], iv, iv + step, x, scores[c], b.broad_parent_solution(c), strong[c], "cs", uncertainty=u,
                           returnExportDetails=True)
            r = rows[c]
            assert BC.differences(BC.canon((r["broad_rows"], r["gapped_rows"], r["peak_meta"], r["export_details"])), BC.canon(want)) == [], c
            xs = b.download(c, "xs")[:, 0].astype(np.float64)
            want_s = TB.rows(names[c], iv, iv + step, xs, scores[c], b.broad_parent_solution(c), strong[c], "cs", uncertainty=u,
                             returnExportDetails=True)
            s = rows_state[c]
            assert BC.differences(BC.canon((s["broad_rows"], s["gapped_rows"], s["peak_meta"], s["export_details"])), BC.canon(want_s)) == [], c
        # the writers take the resident tracks by name: the text and the bigWig body of the downloaded track
        import writer_refs as wr
        from oracle import writers as ow

        for c in (0, 2):
            iv = np.arange(lens[c], dtype=np.int64) * step
            for name, track in (("shrunk", "shrunk"), ("shrunk_posterior_sd", "posterior_sd"), ("shrunk_spike_prop", "spike_prop")):
                v = b.download_shrunk(c, track)
                for transform in (None, "round4"):
                    assert b.bedgraph_bytes(c, name, names[c], 0, step, transform=transform) == \
                        ow.bedgraph_bytes(names[c], iv, iv + step, v, transform), (c, name, transform)
            piece = b.bigwig_track(c, "shrunk", 3, 0, step, zoom_bases=[4 * step])
            wr.check_piece(piece, 3, iv, iv + step, b.download_shrunk(c, "shrunk"), [4], step, c)
        with pytest.raises(L.ConsenrichAMDError, match="chain 1 has no shrunk track"):
            b.bedgraph_bytes(1, "shrunk", "chrB", 0, step)
        with pytest.raises(L.ConsenrichAMDError, match="component out of range"):
            b.bedgraph_bytes(0, "shrunk", "chrA", 0, step, comp=1)
        # nothing resident has changed: the fit, the scores, the masks
        for (c, a), v in fit.items():
            assert np.array_equal(b.download(c, a).view(np.uint32), v.view(np.uint32)), (c, a)
        for c in range(3):
            assert np.array_equal(b.download_scores(c).view(np.uint64), scores[c].view(np.uint64)), c
            assert np.array_equal(b.rocco_solution(c), strong[c]) and np.array_equal(b.weak_solution(c), weak[c]), c
