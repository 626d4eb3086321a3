"""GPU parity tests (run with -m gpu on an MI355X): the HIP product path, called through the C ABI via the
reference-shaped Python mirror, against (a) the golden vectors captured from the real reference and (b) the CPU
oracle run live on the same inputs.  Tolerance: north_star's 1e-5 relative (+ 2e-6 absolute, the tolerance of the
reference's own known-answer tests, test_core.py:3341-3350) on float32 tracks; discrete outputs (ECM iteration
count, convergence flag) must match exactly.
"""
import glob
import os

import numpy as np
import pytest

import cases
from conftest import gpu_available

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1.0e-5, 2.0e-6
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


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


CASES = {c["name"]: c for c in cases.all_cases()}


def _default_switches(spin_limit_too=True):
    """True unless the suite runs under one of the library's mode switches (scripts/suite_variants.sh) that keeps a bit-exact
    step from pipelining its tail per group of chains (a forced bail-out of the single launch, CONSENRICH_AMD_SB_SPIN_LIMIT,
    still launches groups -- it redoes them)."""
    e = os.environ.get
    return (e("CONSENRICH_AMD_TAIL_SPLIT", "1") != "0" and e("CONSENRICH_AMD_SB_ASYNC", "1") != "0"
            and e("CONSENRICH_AMD_SEQ_STATE", "0") == "0"
            and e("CONSENRICH_AMD_DEFER", "1") != "0" and not (spin_limit_too and e("CONSENRICH_AMD_SB_SPIN_LIMIT")))


def close_mostly(got, ref, frac=1e-3, cap=2e-3, msg=""):
    """Quantities that amplify ONE float32 ulp of the level (NIS, kappa: differences of O(30) levels divided by
    O(1e-2) innovations / process noise): 1e-5 on all but `frac` of the entries, never worse than `cap`."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    bad = np.abs(got - ref) > RTOL * np.abs(ref) + ATOL
    assert bad.mean() <= frac, (msg, float(bad.mean()))
    np.testing.assert_allclose(got, ref, rtol=cap, atol=ATOL, err_msg=msg)


@pytest.mark.parametrize("xtol", [2, 0], ids=["ulp2", "exact"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_product_matches_golden(product, name, xtol):
    """Both carry-validation modes (2-ulp acceptance = batch/bench default; 0 = bit-exact sequential semantics = default
    of the drop-in callables) must meet parity."""
    case = CASES[name]
    gold = np.load(os.path.join(GOLDEN, name + ".npz"))
    product.set_validation(xtol)
    try:
        got = cases.run_case(product, case)
    finally:
        product.set_validation(0)
    cases.compare(case, got, gold, RTOL, ATOL)


@pytest.mark.parametrize("name", ["fb_trend_n4096_m32", "fb_level_n4096_m32", "ecm_trend_n4096_m8_defaults",
                                  "fb_trend_n20000_m8", "fb_trend_n333_m5_mask"])
def test_product_matches_live_oracle(product, oracle, name):
    case = CASES[name]
    got = cases.run_case(product, case)
    ref = cases.run_case(oracle, case)
    for k, v in ref.items():
        if isinstance(v, np.ndarray) and v.dtype.kind == "f":
            np.testing.assert_allclose(got[k].astype(np.float64), v.astype(np.float64), rtol=RTOL, atol=ATOL,
                                       err_msg=f"{name}:{k}")
        else:
            assert np.asarray(got[k]).item() == pytest.approx(np.asarray(v).item(), rel=RTOL, abs=ATOL), f"{name}:{k}"


def _run_batch(block_len, warm, d, n_list, m, seed, flags_extra=0, xtol=0, fused=False, mult=True):
    from consenrich_amd import _lib as L
    from consenrich_amd.batch import DeviceBatch, ModelParams

    mp = ModelParams(state_dim=d, Q0=((1e-3, 0.0), (0.0, 1e-4)) if d == 2 else ((1e-3, 0.0), (0.0, 0.0)))
    out = {}
    with DeviceBatch(0, block_len=block_len, warm=warm, x_tol_ulps=xtol) as b:
        b.configure(mp, m, n_list)
        for c, n in enumerate(n_list):
            data, munc = cases.synth(n, m, seed + c, mask_frac=0.02, outlier_frac=0.01)
            lam, kap, qs = cases.multipliers(n, seed + c)
            b.upload(c, data, munc)
            b.upload_multipliers(c, lam, kap, qs)
        b.stats()
        fl = L.RETURN_NLL | ((L.USE_LAMBDA | L.USE_KAPPA | L.USE_QSCALE) if mult else 0) | flags_extra
        if fused:       # everything queued behind the optimistic pipeline, one synchronisation in sums()
            b.forward_backward(fl, want_sums=False)
            b.export(L.EXPORT_FORWARD | L.EXPORT_SMOOTH | L.EXPORT_RESID)
            sd, sn = b.sums()
        else:
            sd, sn = b.forward(fl)
            b.backward()
            b.export(L.EXPORT_FORWARD | L.EXPORT_SMOOTH | L.EXPORT_RESID)
        out["sd"], out["sn"] = sd, sn
        for c in range(len(n_list)):
            for name in ("D", "xf", "Pf", "pnoise", "xs", "Ps", "lag", "resid"):
                out[(c, name)] = b.download(c, name)
        out["stats"] = b.run_stats()
    return out


@pytest.mark.parametrize("d", [2, 1])
def test_speculative_blocks_equal_sequential_recursion(product, d):
    """Results must not depend on block length / warm-up: tiny blocks with (deliberately insufficient) warm-up,
    repaired by the validation/fix-up pass, must reproduce the single-block sequential run.  levelTrend: bit for bit;
    level (double carries, tolerance-validated): to 1e-6 relative."""
    n_list = [5000, 37, 1, 12345, 64, 65]
    seq = _run_batch(32 * 512, (0, 0, 0), d, n_list, 4, 100)       # every chain is one block: pure sequential
    for blk, warm in ((32, (8, 16, 8)), (64, (40, 200, 72)), (256, (512, 2048, 1024)), (32, (0, 0, 0))):
        spec = _run_batch(blk, warm, d, n_list, 4, 100)
        for key, val in seq.items():
            if key == "stats":
                continue
            if d == 2 and not isinstance(key, str):
                assert np.array_equal(val, spec[key]), f"block={blk} warm={warm} {key}"
            else:
                np.testing.assert_allclose(spec[key], val, rtol=1e-6, atol=1e-7, err_msg=f"{blk} {warm} {key}")
        if warm == (0, 0, 0):
            assert spec["stats"]["reruns_p"] > 0 and spec["stats"]["reruns_b"] > 0   # the fix-up path really ran


@pytest.mark.parametrize("d", [2, 1])
def test_fused_pipeline_and_failed_optimistic_validation(product, d):
    """csr_batch_forward_backward (one host sync, NIS/NLL epilogue on the side stream, validation counters checked
    at the end) must equal forward() + backward(), also when the optimistic validation FAILS: with a deliberately
    short warm-up every stage re-runs blocks, the deferred check notices and the pipeline is redone synchronously."""
    n_list = [5000, 37, 1, 12345, 64, 65]
    seq = _run_batch(32 * 512, (0, 0, 0), d, n_list, 4, 100)
    for blk, warm in ((64, (512, 512, 512)), (32, (0, 16, 0))):
        fused = _run_batch(blk, warm, d, n_list, 4, 100, fused=True)
        for key, val in seq.items():
            if key == "stats":
                continue
            if d == 2 and not isinstance(key, str):
                assert np.array_equal(val, fused[key]), f"block={blk} warm={warm} {key}"
            else:
                np.testing.assert_allclose(fused[key], val, rtol=1e-6, atol=1e-7, err_msg=f"{blk} {warm} {key}")
        deferred = os.environ.get("CONSENRICH_AMD_DEFER", "1") != "0"       # the switch that disables optimistic launches
        if warm == (0, 16, 0):
            assert fused["stats"]["reruns_b"] > 0 and (fused["stats"]["pipeline_redos"] >= 1 or not deferred)
        else:
            assert fused["stats"]["pipeline_redos"] == 0


@pytest.mark.parametrize("d", [2, 1])
def test_fused_forward_chain_with_failed_optimistic_validation(product, d):
    """Tolerant mode runs covariance and state in ONE chain kernel.  With a deliberately short window its optimistic
    validation fails; the synchronous redo must land within the k-ulp budget of the sequential recursion, and a
    sufficient window must give the same numbers as the exact mode's split chains."""
    n_list = [5000, 37, 1, 12345, 64, 65]
    # (the fused kernel is used without per-bin multipliers only: with them the split chains need the shorter window)
    seq = _run_batch(32 * 512, (0, 0, 0), d, n_list, 4, 100, xtol=0, mult=False)
    for blk, warm in ((64, (512, 512, 512)), (32, (0, 0, 0))):
        fused = _run_batch(blk, warm, d, n_list, 4, 100, xtol=2, fused=True, mult=False)
        for key, val in seq.items():
            if key == "stats":
                continue
            if not isinstance(key, str) and val.size == 0:       # pnoise / lag of the one-bin chain
                assert fused[key].size == 0
                continue
            scale = 1.0 if isinstance(key, str) else float(np.abs(val).max())
            np.testing.assert_allclose(fused[key], val, rtol=2e-6, atol=2e-6 * max(scale, 1e-30) if isinstance(key, str)
                                       else 1e-6 * max(scale, 1e-30), err_msg=f"{blk} {warm} {key}")
        if warm == (0, 0, 0):
            deferred = os.environ.get("CONSENRICH_AMD_DEFER", "1") != "0"
            assert fused["stats"]["reruns_p"] > 0 and (fused["stats"]["pipeline_redos"] >= 1 or not deferred)
            assert fused["stats"]["reruns_x"] == 0       # no separate state stage in the fused path


@pytest.mark.parametrize("xtol", [0, 2], ids=["exact", "ulp2"])
def test_general_transition_matrix_runs_the_general_instances(product, oracle, xtol):
    """F = [[1, f], [0, 1]] (what the reference's constructMatrixF always builds) runs specialised instances of the levelTrend chain
    policies that drop the multiplications by 1 and 0.  `matrixF` is a free argument of the callables (pyx:6393-6428): any other
    F runs the GENERAL instances (every chain kernel has both; round 6 retired the switch that forced them for a unit F) -- here
    against the oracle: forward / backward with all multipliers and an ECM run (fused kappa E-step, compact pNoise)."""
    n, m = 20011, 4
    Fg = np.asarray([[0.995, 0.8], [0.004, 0.97]], np.float32)
    data, munc = cases.synth(n, m, 712, mask_frac=0.02, outlier_frac=0.01)
    lam, kap, qs = cases.multipliers(n, 712)
    Q0 = np.diag([1e-3, 1e-4]).astype(np.float32)
    bm = (np.arange(n) // 100).astype(np.int32)

    def fb(mod):
        xf, Pf, pn = np.zeros((n, 2), np.float32), np.zeros((n, 2, 2), np.float32), np.zeros((n, 2, 2), np.float32)
        D = np.zeros(n, np.float32)
        r = mod.cforwardPass(matrixData=data, matrixPluginMuncInit=munc, matrixF=Fg, matrixQ0=Q0, intervalToBlockMap=bm,
                             blockCount=int(bm.max()) + 1, stateInit=0.0, stateCovarInit=1000.0, stateForward=xf, stateCovarForward=Pf,
                             pNoiseForward=pn, vectorD=D, returnNLL=True, lambdaExp=lam, processPrecExp=kap, processQScale=qs,
                             obsPrecisionMultiplierMin=0.25, obsPrecisionMultiplierMax=4.0, procPrecisionMultiplierMin=5e-3,
                             procPrecisionMultiplierMax=5e3)
        b = mod.cbackwardPass(matrixData=data, matrixF=Fg, stateForward=xf, stateCovarForward=Pf, pNoiseForward=pn)
        return dict(nll=r[3], xf=xf, Pf=Pf, pn=pn[: n - 1], xs=b[0], Ps=b[1], lag=b[2][: n - 1], resid=b[3])

    def ecm(mod):
        return mod.cfixedBackgroundECM(matrixData=data, matrixPluginMuncInit=munc, matrixF=Fg, matrixQ0=Q0, intervalToBlockMap=bm,
                                       blockCount=int(bm.max()) + 1, stateInit=0.0, stateCovarInit=1000.0, ECM_fixedBackgroundIters=4,
                                       ECM_fixedBackgroundRtol=0.0, pad=1e-4, ECM_robustTNu=8.0, procPrecisionMultiplierMin=5e-3,
                                       procPrecisionMultiplierMax=5e3, ECM_useObsPrecisionReweighting=False,
                                       ECM_useProcessPrecisionReweighting=True, t_innerIters=3, returnIntermediates=True,
                                       logIterations=False)

    product.set_validation(xtol)
    try:
        g, ge = fb(product), ecm(product)
    finally:
        product.set_validation(0)
    o, oe = fb(oracle), ecm(oracle)
    assert g["nll"] == pytest.approx(o["nll"], rel=1e-8)
    scale = np.maximum(np.abs(o["xs"].astype(np.float64)).max(axis=1, keepdims=True), 1.0)
    for name in ("xf", "xs", "resid"):
        assert np.all(np.abs(g[name].astype(np.float64) - o[name]) <= RTOL * scale + ATOL), name
    for name in ("Pf", "pn", "Ps", "lag"):
        np.testing.assert_allclose(g[name], o[name], rtol=RTOL, atol=ATOL, err_msg=name)
    assert ge[0] == oe[0] and ge[1] == pytest.approx(oe[1], rel=1e-7)
    escale = np.maximum(np.abs(oe[2].astype(np.float64)).max(axis=1, keepdims=True), 1.0)
    assert np.all(np.abs(ge[2].astype(np.float64) - oe[2]) <= RTOL * escale + ATOL)
    np.testing.assert_allclose(ge[3], oe[3], rtol=RTOL, atol=ATOL)
    close_mostly(ge[7], oe[7], msg="kappa")


def test_ulp_tolerant_validation_stays_within_parity_budget(product, monkeypatch):
    """Throughput mode: speculative carries are accepted within 2 float32 ulps.  Against the exact sequential run the
    tracks must agree far inside the 1e-5 budget (a few ulps on the level; the trend inherits ulp(level)-sized noise,
    covered by the absolute tolerance), with large |x| (coarse ulps) to make the test bite."""
    monkeypatch.setenv("CONSENRICH_AMD_SEQ_STATE", "0")
    n_list = [60000, 7000]
    seq = _run_batch(32 * 2048, (0, 0, 0), 2, n_list, 8, 300, xtol=0)
    tol = _run_batch(64, (64, 128, 64), 2, n_list, 8, 300, xtol=2)
    exact = _run_batch(64, (64, 128, 64), 2, n_list, 8, 300, xtol=0)
    assert tol["stats"]["reruns_x"] == 0        # (the fused chain has no separate state stage)
    for key, val in seq.items():
        if key == "stats":
            continue
        if not isinstance(key, str):
            assert np.array_equal(val, exact[key]), key
        scale = 1.0 if isinstance(key, str) else float(np.abs(val).max())
        np.testing.assert_allclose(tol[key], val, rtol=2e-6, atol=2e-6 * max(scale, 1e-30) if isinstance(key, str)
                                   else 1e-6 * scale, err_msg=str(key))


def test_exact_state_chain_on_superblocks_equals_the_sequential_kernel(product, monkeypatch):
    """Bit-exact mode runs the levelTrend state chain on superblocks (k_sb_async: one wavefront per superblock, no barrier between
    the repair passes; k_sb_sys + k_sb_delta: the pass form).  With 64 / 256-bin superblocks nearly every superblock fails its
    bitwise validation and the repairs cascade through the chains (partial last blocks, chains shorter than a block, more
    superblocks than the device holds wavefronts): the fixed point must still be the sequential recursion --
    k_state_seq_trend, one wavefront per chain, bit for bit."""
    n_list = [60000, 7000, 300, 1, 16640]
    monkeypatch.setenv("CONSENRICH_AMD_SEQ_STATE", "1")
    seq = _run_batch(0, (-1, -1, -1), 2, n_list, 8, 300, xtol=0)
    monkeypatch.setenv("CONSENRICH_AMD_SEQ_STATE", "0")
    # the barrier-free single launch (default), the pass form, and the single launch with a wait bound so short that it
    # bails out and the host runs the pass form instead
    for bins, warm, mode in (("256", "448", "async"), ("8192", "16384", "async"), ("64", "0", "async"), ("256", "448", "passes"),
                             ("64", "0", "passes"), ("4096", "0", "bail")):
        monkeypatch.setenv("CONSENRICH_AMD_SB_BINS", bins)
        monkeypatch.setenv("CONSENRICH_AMD_SB_ASYNC", "0" if mode == "passes" else "1")
        if mode == "bail":
            monkeypatch.setenv("CONSENRICH_AMD_SB_SPIN_LIMIT", "1")
        else:
            monkeypatch.delenv("CONSENRICH_AMD_SB_SPIN_LIMIT", raising=False)
        sb = _run_batch(0, (-1, -1, -1), 2, n_list, 8, 300, xtol=0)
        for key, val in seq.items():
            if key != "stats" and not isinstance(key, str):
                assert np.array_equal(val, sb[key]), (bins, mode, key)
        assert np.array_equal(sb["sn"], seq["sn"]) and np.array_equal(sb["sd"], seq["sd"])
        if bins != "8192":
            assert sb["stats"]["reruns_x"] > 0, sb["stats"]
        if mode == "bail":
            assert sb["stats"]["sb_bailouts"] > 0, sb["stats"]


@pytest.mark.parametrize("variant", ["constant_q", "multipliers", "per_chain_q"])
def test_a_step_that_pipelines_its_tail_per_chain_equals_the_step_in_order(product, monkeypatch, variant):
    """csr_batch_step in the bit-exact mode launches the smoother / residuals of the chains whose filtered state stands while
    the state chain of the others is still running (step_pipelined, csr_host_pipeline.inl): groups of chains under masks, on
    a second stream.  Same kernels, so every output must equal the step run in order, bit for bit -- with the default
    thresholds, with thresholds that make (nearly) every finished chain a group of its own, and when the single launch bails
    out under the groups already in flight (everything is then redone behind the pass form).  Round 4: also with per-bin
    multipliers (lambda, kappa, qScale: the final pass of a fit, pyx:8151-8300) and with per-chain base process noise
    (core.py:5667) -- their process noise reaches the reference layout underneath the state chain."""
    from consenrich_amd import _lib as L
    from consenrich_amd.batch import DeviceBatch, ModelParams

    n_list = [420000, 150000, 90000, 260000, 64, 1, 30001]
    m = 4
    sets = [cases.synth(n, m, 7300 + c, mask_frac=0.01, outlier_frac=0.01) for c, n in enumerate(n_list)]
    what = L.EXPORT_FORWARD | L.EXPORT_SMOOTH | L.EXPORT_RESID
    flags = L.RETURN_NLL
    if variant == "multipliers":
        flags |= L.USE_LAMBDA | L.USE_KAPPA | L.USE_QSCALE

    def run(env):
        for k in ("CONSENRICH_AMD_TAIL_SPLIT", "CONSENRICH_AMD_TAIL_PCT", "CONSENRICH_AMD_SB_SPIN_LIMIT"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        out = {}
        with DeviceBatch(0) as b:
            b.configure(ModelParams(state_dim=2), m, n_list)
            for c, (d_, v_) in enumerate(sets):
                b.upload(c, d_, v_)
                if variant == "multipliers":
                    lam, kap, qs = cases.multipliers(n_list[c], 7400 + c)
                    b.upload_multipliers(c, lam, np.clip(kap, 0.25, 4.0), qs)
            if variant == "per_chain_q":
                b.set_chain_q([np.diag([1e-3 * (1 + c), 1e-4 * (1 + 0.5 * c)]).astype(np.float32) for c in range(len(n_list))])
            for rep in range(2):        # the second step re-uses every buffer of the first
                sd, sn = b.step(flags, what)
                if rep == 0:
                    # the FIRST step of a batch allocates (and zeroes) its reference-layout arrays: that zeroing must be ordered
                    # ahead of every group's writes, whichever stream a group runs on (round 4: it was queued on the first
                    # group's stream and could wipe what the next group had already written)
                    for c in range(len(n_list)):
                        for name in ("xs", "Ps", "lag", "resid"):
                            out[(c, name, "first step")] = b.download(c, name)
            out["sd"], out["sn"] = np.array(sd), np.array(sn)
            for c in range(len(n_list)):
                for name in ("D", "xf", "Pf", "pnoise", "xs", "Ps", "lag", "resid"):
                    out[(c, name)] = b.download(c, name)
            out["stats"] = b.run_stats()
            # a step that exports nothing, the exports asked for afterwards (the residuals were not part of the pipelined tails)
            b.step(flags, 0)
            b.export(what)
            for c in range(len(n_list)):
                for name in ("D", "xf", "Pf", "pnoise", "xs", "Ps", "lag", "resid"):
                    assert np.array_equal(out[(c, name)], b.download(c, name)), (env, "exports after the step", c, name)
        return out

    ref = run({"CONSENRICH_AMD_TAIL_SPLIT": "0"})
    assert ref["stats"]["tail_groups"] == 0
    if variant != "constant_q":         # the process noise really varies (per bin / per chain)
        assert not np.array_equal(ref[(0, "pnoise")][:100], ref[(1, "pnoise")][:100])
    for env in ({}, {"CONSENRICH_AMD_TAIL_PCT": "1,1"}, {"CONSENRICH_AMD_TAIL_PCT": "1,1", "CONSENRICH_AMD_SB_SPIN_LIMIT": "1"}):
        got = run(env)
        if _default_switches(spin_limit_too=False):
            assert got["stats"]["tail_groups"] >= 2, (env, variant, got["stats"])       # two steps, at least one group each
        for key, val in ref.items():
            if key != "stats":
                assert np.array_equal(val, got[key]), (env, variant, key)


@pytest.mark.parametrize("xtol", [2, 0], ids=["ulp2", "exact"])
def test_smoother_inputs_from_either_layout_give_the_same_bits(product, monkeypatch, xtol):
    """A step leaves xf / Pf in the reference layout only where it can (2-ulp mode with one constant process noise; the default
    mode's pipelined tails) and the smoother reads them there through its LDS tiles (`k_smooth_natin`).  A smoother that reads the
    blocked layout (CONSENRICH_AMD_NATIN=0: the blocked copies the forward pass did not write are brought back first,
    `ensure_blocked_fwd`) runs the same recursion on the same values: every output array and both sums BIT FOR BIT -- and so does
    a second smoother pass on the resident forward results.  (Round 5 checked the whole lean data flow against round 4's through
    the switch CONSENRICH_AMD_LEAN, retired in round 6: `profiles/r05_lean_ab.txt`.)"""
    from consenrich_amd import _lib as L
    from consenrich_amd.batch import DeviceBatch, ModelParams

    n_list = [400000, 130000, 70001, 64, 9]
    m = 5
    sets = [cases.synth(n, m, 7900 + c, mask_frac=0.01, outlier_frac=0.005) for c, n in enumerate(n_list)]
    what = L.EXPORT_FORWARD | L.EXPORT_SMOOTH | L.EXPORT_RESID

    def run(env):
        monkeypatch.delenv("CONSENRICH_AMD_NATIN", raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        out = {}
        with DeviceBatch(0, x_tol_ulps=xtol) as b:
            b.configure(ModelParams(state_dim=2), m, n_list)
            if xtol:
                b.set_tuning(0, 96, 96, 64)     # (pinned windows: the 2-ulp mode's results depend on them within its acceptance)
            for c, (d_, v_) in enumerate(sets):
                b.upload(c, d_, v_)
            sd, sn = b.step(L.RETURN_NLL, what)
            out["sd"], out["sn"] = np.array(sd), np.array(sn)
            for c in range(len(n_list)):
                for name in ("D", "xf", "Pf", "pnoise", "xs", "Ps", "lag", "resid"):
                    out[(c, name)] = b.download(c, name)
            # the separate entries behind a lean step: a second smoother pass on the resident forward results
            b.backward()
            b.export(L.EXPORT_SMOOTH)
            for c in range(len(n_list)):
                assert np.array_equal(out[(c, "xs")], b.download(c, "xs")), (env, c)
        return out

    ref = run({})
    got = run({"CONSENRICH_AMD_NATIN": "0"})
    for key, val in ref.items():
        assert np.array_equal(val, got[key]), key


def test_two_contexts_in_one_process_each_raise_their_own_launch_attributes(product):
    """The default-mode state chain launches with ~124 KB of dynamic LDS, which has to be asked for once per kernel AND PER
    DEVICE (hipFuncSetAttribute).  Round 4 remembered that in a process-wide static: a second context on another GPU of the
    same process skipped the call and its launch failed.  The flag lives in the context now: two contexts of one process --
    on two devices where the box has them, else both on device 0 -- step the same batch to the same bits."""
    from consenrich_amd import _lib as L
    from consenrich_amd.batch import DeviceBatch, ModelParams

    n_list = [70000, 33000]
    sets = [cases.synth(n, 3, 7800 + c) for c, n in enumerate(n_list)]
    what = L.EXPORT_FORWARD | L.EXPORT_SMOOTH
    second = 1 if L.device_count() > 1 else 0
    outs = []
    with DeviceBatch(0) as b0, DeviceBatch(second) as b1:
        for b in (b0, b1):
            b.configure(ModelParams(state_dim=2), 3, n_list)
            for c, (d_, v_) in enumerate(sets):
                b.upload(c, d_, v_)
        for b in (b0, b1, b0):
            b.step(L.RETURN_NLL, what)
            outs.append({(c, k): b.download(c, k) for c in range(2) for k in ("xf", "xs", "Ps", "D")})
    for o in outs[1:]:
        for key, val in outs[0].items():
            assert np.array_equal(val, o[key]), key


def test_a_pipelined_step_whose_covariance_chain_fails_validation_is_replayed_whole(product, monkeypatch):
    """In the default mode the covariance chain is validated OPTIMISTICALLY and writes the gain records the state chain, the
    pipelined tail groups and the exports run on.  With a deliberately short covariance window (16 bins) that validation
    fails: everything that ran on the unvalidated gains -- the single launch of the state chain, the groups already launched,
    the exports -- is replayed at the settle point (forward_impl in order + export_impl(pendExport)).  The step must equal the
    step in order with synchronous validation (CONSENRICH_AMD_TAIL_SPLIT=0, CONSENRICH_AMD_DEFER=0, default windows) bit for
    bit, having really taken the replay path."""
    from consenrich_amd import _lib as L
    from consenrich_amd.batch import DeviceBatch, ModelParams

    n_list = [300000, 120000, 200000, 4097]
    m = 4
    sets = [cases.synth(n, m, 7700 + c, mask_frac=0.01, outlier_frac=0.01) for c, n in enumerate(n_list)]
    what = L.EXPORT_FORWARD | L.EXPORT_SMOOTH | L.EXPORT_RESID

    def run(env):
        for k in ("CONSENRICH_AMD_TAIL_SPLIT", "CONSENRICH_AMD_WARM", "CONSENRICH_AMD_DEFER"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        out = {}
        with DeviceBatch(0) as b:
            b.configure(ModelParams(state_dim=2), m, n_list)
            for c, (d_, v_) in enumerate(sets):
                b.upload(c, d_, v_)
            sd, sn = b.step(L.RETURN_NLL, what)
            out["sd"], out["sn"] = np.array(sd), np.array(sn)
            for c in range(len(n_list)):
                for name in ("D", "xf", "Pf", "pnoise", "xs", "Ps", "lag", "resid"):
                    out[(c, name)] = b.download(c, name)
            out["stats"] = b.run_stats()
        return out

    # the yardstick: every stage validated synchronously before the next one starts, nothing pipelined
    ref = run({"CONSENRICH_AMD_TAIL_SPLIT": "0", "CONSENRICH_AMD_DEFER": "0"})
    assert ref["stats"]["pipeline_redos"] == 0 and ref["stats"]["tail_groups"] == 0
    got = run({"CONSENRICH_AMD_WARM": "16,-1,-1"})
    if _default_switches():
        assert got["stats"]["pipeline_redos"] >= 1 and got["stats"]["tail_groups"] >= 1, got["stats"]
    for key, val in ref.items():
        if key != "stats":
            assert np.array_equal(val, got[key]), key


def _full_chain(mod, d, n, m, seed=4242):
    data, munc = cases.synth(n, m, seed)
    _lam, kap, _qs = cases.multipliers(n, seed)
    F = np.asarray(cases.F_TREND, np.float32)
    Q0 = np.diag([1e-3, 1e-4]).astype(np.float32) if d == 2 else np.asarray([[1e-3]], np.float32)
    bm = (np.arange(n) // 500).astype(np.int32)
    xf, Pf, pn = np.zeros((n, d), np.float32), np.zeros((n, d, d), np.float32), np.zeros((n, d, d), np.float32)
    D = np.zeros(n, np.float32)
    kw = dict(matrixData=data, matrixPluginMuncInit=munc, matrixQ0=Q0, intervalToBlockMap=bm,
              blockCount=int(bm.max()) + 1, stateInit=0.0, stateCovarInit=1000.0, stateForward=xf,
              stateCovarForward=Pf, pNoiseForward=pn, vectorD=D, returnNLL=True, processPrecExp=kap,
              obsPrecisionMultiplierMin=0.25, obsPrecisionMultiplierMax=4.0, procPrecisionMultiplierMin=5e-3,
              procPrecisionMultiplierMax=5e3)
    if d == 2:
        r = mod.cforwardPass(matrixF=F, **kw)
        b = mod.cbackwardPass(matrixData=data, matrixF=F, stateForward=xf, stateCovarForward=Pf, pNoiseForward=pn)
    else:
        r = mod.cforwardPassLevel(**kw)
        b = mod.cbackwardPassLevel(matrixData=data, stateForward=xf, stateCovarForward=Pf, pNoiseForward=pn)
    return dict(phi=r[0], nll=r[3], xf=xf, Pf=Pf, pn=pn[: n - 1], D=D, xs=b[0], Ps=b[1], lag=b[2][: n - 1], resid=b[3])


@pytest.mark.parametrize("d,n,m", [(2, 1000000, 4), (2, 1244783, 8), (1, 1000000, 4), (2, 2200000, 2)])
def test_full_size_chain_matches_oracle(product, oracle, d, n, m):
    """BASELINE config sizes (1e6 x 4; chr1 @200bp x 8): the whole chain, every bin, against the CPU oracle in the
    THROUGHPUT (2-ulp carry validation) mode.  |x| reaches ~30 here, so one float32 ulp of the level is 2e-6.
    (2.2e6 x 2: the automatic block length is 64 bins between 2 M and 6 M bins, 32 below.)"""
    product.set_validation(2)
    try:
        g = _full_chain(product, d, n, m)
    finally:
        product.set_validation(0)
    o = _full_chain(oracle, d, n, m)
    assert g["phi"] == pytest.approx(o["phi"], rel=1e-6)
    assert g["nll"] == pytest.approx(o["nll"], rel=1e-8)          # sumNLL drives the ECM stop rule
    for name in ("xf", "Pf", "pn", "D", "xs", "Ps", "lag", "resid"):
        a, b = g[name].astype(np.float64), o[name].astype(np.float64)
        if name in ("xf", "xs") and d == 2:
            # state vectors: tolerance relative to the LEVEL of the same bin (the trend enters the level additively,
            # F01*x1, and inherits ulp(level)-sized float32 rounding noise in the reference itself)
            scale = np.abs(b).max(axis=1, keepdims=True)
            assert np.all(np.abs(a - b) <= RTOL * scale + ATOL), name
        elif name == "resid":
            # residual = z - xs0: its absolute error is the level's, so the tolerance scales with the level
            scale = np.abs(o["xs"][:, :1].astype(np.float64))
            assert np.all(np.abs(a - b) <= RTOL * scale + ATOL), name
        elif name == "D":
            # NIS is ill-conditioned in the level: d = zbar - x0 turns ONE float32 ulp of x0 into ~2 ulp(x0)/|d|
            # ~ 1e-4 relative in D (the reference's own D moves that much when its x0 rounds the other way):
            # 1e-5 on >= 99 % of the bins, never worse than the conditioning bound.
            bad = np.abs(a - b) > RTOL * np.abs(b) + ATOL
            assert bad.mean() <= 1e-2, (name, bad.mean())
            np.testing.assert_allclose(a, b, rtol=5e-4, atol=ATOL, err_msg=name)
        else:
            np.testing.assert_allclose(a, b, rtol=RTOL, atol=ATOL, err_msg=name)
    # level track: never more than a few float32 ulps of max(|level|, 1) off (the validation criterion's own scale:
    # a level crossing zero still inherits ulp(1)-sized rounding noise from its neighbours)
    lvl = np.abs(g["xf"][:, 0].astype(np.float64) - o["xf"][:, 0]) / np.maximum(np.abs(o["xf"][:, 0]), 1.0)
    assert lvl.max() <= 6e-7


def test_exact_mode_is_bit_identical_to_the_oracle_at_full_size(product, oracle):
    """x_tol_ulps = 0 (bit-exact sequential semantics): on a 1e6-bin chain the output arrays equal the oracle's -- hence
    the reference's -- bit for bit except for a handful of elements (<= 1 ulp(fp64) arithmetic differences reach a
    float32 rounding boundary ~once per 10^7 values; measured: 1 of 2e6 filtered-state values, 3 covariance rows at
    the P = 1000 start-up); the fp64 NLL agrees to 1e-12."""
    product.set_validation(0)
    g = _full_chain(product, 2, 1000000, 4)
    o = _full_chain(oracle, 2, 1000000, 4)
    for name in ("xf", "Pf", "pn", "D", "xs", "Ps", "lag", "resid"):
        diff = g[name] != o[name]
        assert int(diff.sum()) <= 16, (name, int(diff.sum()))
        np.testing.assert_allclose(g[name].astype(np.float64), o[name].astype(np.float64), rtol=3e-7, atol=1e-9,
                                   err_msg=name)
    for name in ("Pf", "pn", "D", "xs", "resid"):
        assert np.array_equal(g[name], o[name]), name
    assert g["nll"] == pytest.approx(o["nll"], rel=1e-12)


def test_ecm_on_a_chromosome_sized_chain_matches_oracle(product, oracle):
    """cfixedBackgroundECM with the CLI defaults (constants.py:266-281: 50 iters, rtol 1e-6, t_inner 5, nu 8, obs
    re-weighting off, process re-weighting on) on a chr21-sized chain x 8 samples: same iteration count, same
    convergence flag, NLL path to 5e-8, tracks to 1e-5."""
    n, m = 233550, 8
    data, munc = cases.synth(n, m, 2121, outlier_frac=0.01)
    kw = dict(matrixData=data, matrixPluginMuncInit=munc, matrixF=np.asarray(cases.F_TREND, np.float32),
              matrixQ0=np.diag([1e-3, 1e-4]).astype(np.float32), intervalToBlockMap=(np.arange(n) // 500).astype(np.int32),
              blockCount=n // 500 + 1, stateInit=0.0, stateCovarInit=1000.0, ECM_fixedBackgroundIters=50,
              ECM_fixedBackgroundRtol=1e-6, pad=1e-4, ECM_robustTNu=8.0, procPrecisionMultiplierMin=5e-3,
              procPrecisionMultiplierMax=5e3, ECM_useObsPrecisionReweighting=False,
              ECM_useProcessPrecisionReweighting=True, t_innerIters=5, returnIntermediates=True,
              returnDiagnostics=True, trackOptimizationPath=True, logIterations=False)
    g = product.cfixedBackgroundECM(**kw)
    o = oracle.cfixedBackgroundECM(**kw)
    assert g[0] == o[0] and g[8]["converged"] == o[8]["converged"] and g[0] >= 2
    # NLL inherits the NIS conditioning (ulp(level)/innovation) on the few % of bins whose level differs in the last
    # bit: ~1e-8 relative on the sum, two orders below the stop rule's rtol
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


def test_batch_ecm_lockstep_equals_per_chain_calls(product):
    """Chains of one batch run the ECM loop in lock-step but converge independently (masked out when done): every
    chain must equal its own single-chain run, including its own iteration count."""
    from consenrich_amd import _lib as L
    from consenrich_amd.batch import DeviceBatch, ModelParams

    n_list, m = [6000, 900, 3, 12000], 4
    mp = ModelParams(state_dim=2)
    sets = [cases.synth(n, m, 900 + i, outlier_frac=0.02 * i) for i, n in enumerate(n_list)]
    # exact carry validation on both sides: results are then independent of the block structure, so the comparison
    # isolates the lock-step / masking logic (iteration counts are discrete and must agree)
    product.set_validation(0)
    with DeviceBatch(0, x_tol_ulps=0) as b:
        b.configure(mp, m, n_list)
        for c, (d_, v_) in enumerate(sets):
            b.upload(c, d_, v_)
        b.stats()
        outs, paths = b.ecm(max_iters=30, inner_iters=3, rtol=1e-5, use_lambda=True, use_kappa=True)
        b.export(L.EXPORT_SMOOTH | L.EXPORT_MULT)
        got = [(int(o.iters_done), o.final_nll, b.download(c, "xs"), b.download(c, "lambda"), b.download(c, "kappa"))
               for c, o in enumerate(outs)]
    iters = set()
    for c, (d_, v_) in enumerate(sets):
        n = n_list[c]
        r = product.cfixedBackgroundECM(matrixData=d_, matrixPluginMuncInit=v_, matrixF=np.asarray(cases.F_TREND, np.float32),
                                        matrixQ0=np.diag([1e-3, 1e-4]).astype(np.float32),
                                        intervalToBlockMap=np.zeros(n, np.int32), blockCount=1, stateInit=0.0,
                                        stateCovarInit=1000.0, ECM_fixedBackgroundIters=30, ECM_fixedBackgroundRtol=1e-5,
                                        procPrecisionMultiplierMin=5e-3, procPrecisionMultiplierMax=5e3, t_innerIters=3,
                                        returnIntermediates=True, logIterations=False)
        assert got[c][0] == r[0], (c, got[c][0], r[0])
        assert got[c][1] == pytest.approx(r[1], rel=1e-9)
        np.testing.assert_allclose(got[c][2], r[2], rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(got[c][3], r[6], rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(got[c][4], r[7], rtol=RTOL, atol=ATOL)
        iters.add(r[0])
    assert len(iters) >= 2      # the chains really stop at different iterations


@pytest.mark.parametrize("xtol", [0, 2], ids=["exact", "ulp2"])
def test_ecm_with_failed_optimistic_validations_follows_the_reference_sequence(product, oracle, xtol, monkeypatch):
    """The fused kappa E-step writes the kappa of the NEXT sweep while the forward pass of THIS sweep may still have to be
    re-run (deferred validation).  With deliberately short windows every iteration of the loop fails its optimistic
    validation and is replayed; iteration count, NLL path, kappa and the smoothed moments must still be the reference
    sequence (pyx:8156-8300) -- a sweep reading the kappa of its own E-step would run one E-step ahead."""
    from consenrich_amd import _lib as L
    from consenrich_amd.batch import DeviceBatch, ModelParams

    monkeypatch.setenv("CONSENRICH_AMD_WARM", "-1,-1,-1,16")      # window of the fused forward chain with per-bin kappa
    n_list, m = [6000, 2500], 5
    sets = [cases.synth(n, m, 3300 + i, outlier_frac=0.02) for i, n in enumerate(n_list)]
    with DeviceBatch(0, block_len=32, warm=(16, 16, 16), x_tol_ulps=xtol) as b:
        b.configure(ModelParams(state_dim=2), m, n_list)
        for c, (d_, v_) in enumerate(sets):
            b.upload(c, d_, v_)
        b.stats()
        outs, paths = b.ecm(max_iters=8, inner_iters=3, rtol=1e-7, use_lambda=False, use_kappa=True)
        b.export(L.EXPORT_SMOOTH | L.EXPORT_MULT)
        got = [(int(o.iters_done), paths[c], b.download(c, "xs"), b.download(c, "Ps"), b.download(c, "kappa"))
               for c, o in enumerate(outs)]
        rs = b.run_stats()
    deferred = os.environ.get("CONSENRICH_AMD_DEFER", "1") != "0"
    assert (rs["reruns_p"] + rs["reruns_x"] + rs["reruns_b"]) > 0 and (rs["pipeline_redos"] >= 1 or not deferred), rs
    for c, (d_, v_) in enumerate(sets):
        n = n_list[c]
        r = oracle.cfixedBackgroundECM(matrixData=d_, matrixPluginMuncInit=v_, matrixF=np.asarray(cases.F_TREND, np.float32),
                                       matrixQ0=np.diag([1e-3, 1e-4]).astype(np.float32),
                                       intervalToBlockMap=np.zeros(n, np.int32), blockCount=1, stateInit=0.0,
                                       stateCovarInit=1000.0, ECM_fixedBackgroundIters=8, ECM_fixedBackgroundRtol=1e-7,
                                       ECM_useObsPrecisionReweighting=False, ECM_useProcessPrecisionReweighting=True,
                                       procPrecisionMultiplierMin=5e-3, procPrecisionMultiplierMax=5e3, t_innerIters=3,
                                       returnIntermediates=True, returnDiagnostics=True, trackOptimizationPath=True,
                                       logIterations=False)
        assert got[c][0] == r[0], (c, got[c][0], r[0])
        np.testing.assert_allclose(got[c][1][: r[0]], r[8]["optimization_path"], rtol=1e-9 if xtol == 0 else 5e-8)
        scale = np.abs(r[2]).max(axis=1, keepdims=True)
        # (tolerant mode with 16-bin windows: every carry is accepted AT the rule's limit -- twice the usual budget; the point
        # of this test is the sequencing of the E-steps, the precision of the mode is measured elsewhere)
        slack = 1.0 if xtol == 0 else 2.0
        assert np.all(np.abs(got[c][2].astype(np.float64) - r[2]) <= slack * (RTOL * scale + ATOL))
        np.testing.assert_allclose(got[c][3], r[3], rtol=RTOL, atol=ATOL)
        if xtol == 0:
            np.testing.assert_allclose(got[c][4], r[7], rtol=RTOL, atol=ATOL)
        else:
            close_mostly(got[c][4], r[7], frac=2e-2, cap=5e-2, msg="kappa")


def test_warm_started_ecm_sweeps_repair_inside_the_kernel_and_follow_the_reference(product, oracle, monkeypatch):
    """ECM sweeps of small batches start their speculative windows from the carries the previous sweep recorded
    (Prm::ckptIn) and validate / repair 63 of 64 blocks inside the speculative kernel (wave_local_repair).  With 32-bin
    warm-started windows against 96 / 80-bin cold ones hundreds of blocks (the ones whose kappa moved most) fail and are
    repaired in place, a few at wavefront edges fail the global check (replay, windows widen): iteration count, NLL path and
    moments must be the reference's, for this run and for the one with warm starting switched off."""
    from consenrich_amd import _lib as L
    from consenrich_amd.batch import DeviceBatch, ModelParams

    if os.environ.get("CONSENRICH_AMD_WARMSTART", "1") == "0":
        pytest.skip("warm starting is switched off by the environment")
    n_list, m = [40000, 9000, 700], 32
    sets = [cases.synth(n, m, 5100 + i, outlier_frac=0.02) for i, n in enumerate(n_list)]

    def run():
        with DeviceBatch(0, x_tol_ulps=2) as b:
            b.configure(ModelParams(state_dim=2), m, n_list)
            for c, (d_, v_) in enumerate(sets):
                b.upload(c, d_, v_)
            b.stats()
            outs, paths = b.ecm(max_iters=6, inner_iters=5, rtol=1e-7, use_lambda=False, use_kappa=True)
            b.export(L.EXPORT_SMOOTH | L.EXPORT_MULT)
            got = [(int(o.iters_done), paths[c], b.download(c, "xs"), b.download(c, "Ps"), b.download(c, "kappa"))
                   for c, o in enumerate(outs)]
            return got, b.run_stats()

    warm, rs = run()
    assert rs["block_len"] == 32 and rs["local_repairs"] > 0, rs
    monkeypatch.setenv("CONSENRICH_AMD_WARMSTART", "0")
    cold, rs0 = run()
    assert rs0["local_repairs"] == 0, rs0
    for c, (d_, v_) in enumerate(sets):
        n = n_list[c]
        r = oracle.cfixedBackgroundECM(matrixData=d_, matrixPluginMuncInit=v_, matrixF=np.asarray(cases.F_TREND, np.float32),
                                       matrixQ0=np.diag([1e-3, 1e-4]).astype(np.float32),
                                       intervalToBlockMap=np.zeros(n, np.int32), blockCount=1, stateInit=0.0,
                                       stateCovarInit=1000.0, ECM_fixedBackgroundIters=6, ECM_fixedBackgroundRtol=1e-7,
                                       ECM_useObsPrecisionReweighting=False, ECM_useProcessPrecisionReweighting=True,
                                       procPrecisionMultiplierMin=5e-3, procPrecisionMultiplierMax=5e3, t_innerIters=5,
                                       returnIntermediates=True, returnDiagnostics=True, trackOptimizationPath=True,
                                       logIterations=False)
        for tag, got in (("warm", warm), ("cold", cold)):
            assert got[c][0] == r[0], (c, got[c][0], r[0])
            np.testing.assert_allclose(got[c][1][: r[0]], r[8]["optimization_path"], rtol=5e-8)
            scale = np.abs(r[2]).max(axis=1, keepdims=True)
            excess = np.abs(got[c][2].astype(np.float64) - r[2]) - (RTOL * scale + ATOL)
            k = np.unravel_index(np.argmax(excess), excess.shape)
            assert excess.max() <= 0.0, (tag, c, k, float(excess.max()), got[c][2][k[0]], r[2][k[0]])
            np.testing.assert_allclose(got[c][3], r[3], rtol=RTOL, atol=ATOL)
            close_mostly(got[c][4], r[7], frac=2e-2, cap=5e-2, msg="kappa")
        np.testing.assert_allclose(warm[c][1], cold[c][1], rtol=5e-8)


def test_exact_mode_on_a_chromosome_sized_chain(product):
    """Bit-exact sequential semantics at chr21 size: default blocks (speculative) == one block per chain."""
    n = 233550
    seq = _run_batch(32 * 8192, (0, 0, 0), 2, [n], 8, 77, xtol=0)
    spec = _run_batch(0, (-1, -1, -1), 2, [n], 8, 77, xtol=0)
    for key, val in seq.items():
        if key != "stats" and not isinstance(key, str):
            assert np.array_equal(val, spec[key]), key
    assert spec["stats"]["blocks"] > 1000


def test_many_ragged_chains_in_one_batch(product, oracle):
    """200 contigs of ragged length (1 .. 3000 bins, like the unplaced scaffolds of a real assembly) in one batch:
    block tables, wave-groups straddling chain boundaries, partial last blocks.  Every chain is checked against the
    oracle (forward + smoother), in exact mode and with deliberately short warm-up."""
    from consenrich_amd import _lib as L
    from consenrich_amd.batch import DeviceBatch, ModelParams

    rng = np.random.default_rng(5)
    n_list = [int(v) for v in np.concatenate([[1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257],
                                              rng.integers(1, 3000, 185)])]
    m = 3
    F = np.asarray(cases.F_TREND, np.float32)
    Q0 = np.diag([1e-3, 1e-4]).astype(np.float32)
    with DeviceBatch(0, block_len=64, warm=(32, 48, 32), x_tol_ulps=0) as b:
        b.configure(ModelParams(state_dim=2), m, n_list)
        sets = []
        for c, n in enumerate(n_list):
            d_, v_ = cases.synth(n, m, 7000 + c, mask_frac=0.03)
            sets.append((d_, v_))
            b.upload(c, d_, v_)
        b.stats()
        sd, sn = b.forward(L.RETURN_NLL)
        b.backward()
        b.export(L.EXPORT_FORWARD | L.EXPORT_SMOOTH | L.EXPORT_RESID)
        for c in list(range(20)) + list(range(20, 200, 9)):
            n = n_list[c]
            d_, v_ = sets[c]
            xf, Pf, pn = np.zeros((n, 2), np.float32), np.zeros((n, 2, 2), np.float32), np.zeros((n, 2, 2), np.float32)
            D = np.zeros(n, np.float32)
            r = oracle.cforwardPass(matrixData=d_, matrixPluginMuncInit=v_, matrixF=F, matrixQ0=Q0,
                                    intervalToBlockMap=np.zeros(n, np.int32), blockCount=1, stateInit=0.0,
                                    stateCovarInit=1000.0, stateForward=xf, stateCovarForward=Pf, pNoiseForward=pn,
                                    vectorD=D, returnNLL=True)
            bw = oracle.cbackwardPass(matrixData=d_, matrixF=F, stateForward=xf, stateCovarForward=Pf, pNoiseForward=pn)
            assert sn[c] == pytest.approx(r[3], rel=1e-9, abs=1e-9), c
            for name, ref in (("D", D), ("xf", xf), ("Pf", Pf), ("pnoise", pn[: n - 1]), ("xs", bw[0]), ("Ps", bw[1]),
                              ("lag", bw[2][: n - 1]), ("resid", bw[3])):
                np.testing.assert_allclose(b.download(c, name), ref, rtol=RTOL, atol=ATOL, err_msg=f"chain {c} {name}")


def test_batch_chains_are_independent(product):
    """A chain's result must not depend on which other chains share the batch (contig sharding relies on it)."""
    a = _run_batch(64, (128, 256, 128), 2, [3000, 777], 3, 7)
    b = _run_batch(64, (128, 256, 128), 2, [3000], 3, 7)
    for name in ("D", "xf", "Pf", "xs", "Ps", "lag", "resid"):
        assert np.array_equal(a[(0, name)], b[(0, name)]), name


def test_reference_api_contract(product):
    """Contract details the reference tests pin (test_core.py:3427, 3078-3079, 2862-2895)."""
    n, m = 40, 2
    data, munc = cases.synth(n, m, 5)
    F = np.asarray(cases.F_TREND, np.float32)
    Q0 = np.diag([1e-3, 1e-4]).astype(np.float32)
    bm = np.zeros(n, np.int32)
    D = np.empty(n, np.float32)
    r = product.cforwardPass(matrixData=data, matrixPluginMuncInit=munc, matrixF=F, matrixQ0=Q0, intervalToBlockMap=bm,
                             blockCount=1, stateInit=0.0, stateCovarInit=1000.0, vectorD=D, returnNLL=True)
    assert r[1] == 0 and r[2] is D and np.isfinite(r[3])
    with pytest.raises(ValueError):     # lambdaExp must be interval-level (1-D)
        product.cforwardPass(matrixData=data, matrixPluginMuncInit=munc, matrixF=F, matrixQ0=Q0,
                             intervalToBlockMap=bm, blockCount=1, stateInit=0.0, stateCovarInit=1000.0,
                             lambdaExp=np.ones((m, n), np.float32), ECM_useObsPrecisionReweighting=True)
    with pytest.raises(ValueError, match="out-of-range block id"):
        product.cforwardPass(matrixData=data, matrixPluginMuncInit=munc, matrixF=F, matrixQ0=Q0,
                             intervalToBlockMap=bm + 3, blockCount=1, stateInit=0.0, stateCovarInit=1000.0)
    with pytest.raises(ValueError, match="blockCount must be positive"):
        product.cforwardPass(matrixData=data, matrixPluginMuncInit=munc, matrixF=F, matrixQ0=Q0,
                             intervalToBlockMap=bm, blockCount=0, stateInit=0.0, stateCovarInit=1000.0)
    out = product.cfixedBackgroundECM(matrixData=data, matrixPluginMuncInit=munc, matrixF=F, matrixQ0=Q0,
                                      intervalToBlockMap=bm, blockCount=1, stateInit=0.0, stateCovarInit=1.0,
                                      ECM_fixedBackgroundIters=1, ECM_useObsPrecisionReweighting=False,
                                      ECM_useProcessPrecisionReweighting=False, returnIntermediates=True,
                                      t_innerIters=1, logIterations=False)
    assert out[6] is None and out[7] is None and len(out) == 8
    e = product.cforwardPass(matrixData=np.empty((m, 0), np.float32), matrixPluginMuncInit=np.empty((m, 0), np.float32),
                             matrixF=F, matrixQ0=Q0, intervalToBlockMap=np.empty(0, np.int32), blockCount=1,
                             stateInit=0.0, stateCovarInit=1.0, returnNLL=True)
    assert e[0] == 0.0 and e[1] == 0 and e[3] == 0.0


@pytest.mark.parametrize("d", [2, 1])
def test_output_arrays_are_written_in_place(product, oracle, d):
    """The callables fill the CALLER's arrays (pyx:6545-6561: preallocated outputs, `shape[0] >= n`): arrays of exactly the
    shape of the pass are written by the library itself (no bounce buffer; n large enough for the host-side page pre-fault to
    run), larger ones through a sliced store that leaves the rows past n alone; the returned objects are the caller's; a
    pNoise input of n or of n - 1 rows is the same input."""
    n, m = 300000, 4
    data, munc = cases.synth(n, m, 77)
    F = np.asarray(cases.F_TREND, np.float32)
    Q0 = np.diag([1e-3, 1e-4]).astype(np.float32) if d == 2 else np.asarray([[1e-3]], np.float32)
    bm = np.zeros(n, np.int32)

    def fwd(mod, xf, Pf, pn, D):
        kw = dict(matrixData=data, matrixPluginMuncInit=munc, matrixQ0=Q0, intervalToBlockMap=bm, blockCount=1, stateInit=0.0,
                  stateCovarInit=1000.0, stateForward=xf, stateCovarForward=Pf, pNoiseForward=pn, vectorD=D, returnNLL=True,
                  ECM_useObsPrecisionReweighting=False, ECM_useProcessPrecisionReweighting=False)
        return mod.cforwardPass(matrixF=F, **kw) if d == 2 else mod.cforwardPassLevel(**kw)

    def bwd(mod, xf, Pf, pn, **out):
        if d == 2:
            return mod.cbackwardPass(matrixData=data, matrixF=F, stateForward=xf, stateCovarForward=Pf, pNoiseForward=pn, **out)
        return mod.cbackwardPassLevel(matrixData=data, stateForward=xf, stateCovarForward=Pf, pNoiseForward=pn, **out)

    def blank(rows, *tail, fill=np.nan):
        return np.full((rows,) + tail, fill, np.float32)

    ref_f = (blank(n, d), blank(n, d, d), blank(n, d, d, fill=0.0), blank(n))
    fwd(oracle, *ref_f)
    ref_b = bwd(oracle, ref_f[0], ref_f[1], ref_f[2])
    # forward: exact shapes (pNoise with n rows: the last one is never written) and oversized ones
    xf, Pf, pn, D = blank(n, d), blank(n, d, d), blank(n, d, d, fill=5.0), blank(n)
    r = fwd(product, xf, Pf, pn, D)
    assert r[2] is D
    for got, want in ((xf, ref_f[0]), (Pf, ref_f[1]), (pn[: n - 1], ref_f[2][: n - 1]), (D, ref_f[3])):
        np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL)
    assert np.all(pn[n - 1] == 5.0)
    xf2, Pf2, pn2, D2 = blank(n + 3, d, fill=7.0), blank(n + 3, d, d, fill=7.0), blank(n - 1, d, d), blank(n + 3, fill=7.0)
    fwd(product, xf2, Pf2, pn2, D2)
    assert np.array_equal(xf2[:n], xf) and np.array_equal(Pf2[:n], Pf) and np.array_equal(pn2, pn[: n - 1]) and np.array_equal(D2[:n], D)
    assert np.all(xf2[n:] == 7.0) and np.all(Pf2[n:] == 7.0) and np.all(D2[n:] == 7.0)
    # smoother: fresh outputs, exact-shape preallocated outputs (same objects back), oversized ones
    b0 = bwd(product, xf, Pf, pn)
    for k, (got, want) in enumerate(zip(b0, ref_b)):
        rows = n - 1 if k == 2 else n           # lagCovSmoothed has n - 1 meaningful rows
        np.testing.assert_allclose(got[:rows], want[:rows], rtol=RTOL, atol=ATOL)
    pre = dict(stateSmoothed=blank(n, d), stateCovarSmoothed=blank(n, d, d), lagCovSmoothed=blank(n - 1, d, d),
               postFitResiduals=blank(n, m))
    b1 = bwd(product, xf, Pf, pn2, **pre)                      # (pNoise given with n - 1 rows)
    assert b1[0] is pre["stateSmoothed"] and b1[1] is pre["stateCovarSmoothed"] and b1[2] is pre["lagCovSmoothed"] \
        and b1[3] is pre["postFitResiduals"]
    for a, b_ in zip(b0, b1):
        assert np.array_equal(a[: b_.shape[0]], b_[: a.shape[0]])
    big = dict(stateSmoothed=blank(n + 2, d, fill=3.0), stateCovarSmoothed=blank(n + 2, d, d, fill=3.0),
               lagCovSmoothed=blank(n + 2, d, d, fill=3.0), postFitResiduals=blank(n + 2, m, fill=3.0))
    b2 = bwd(product, xf, Pf, pn, **big)
    assert b2[3] is big["postFitResiduals"]
    assert np.array_equal(b2[0][:n], b1[0]) and np.array_equal(b2[1][:n], b1[1]) and np.array_equal(b2[3][:n], b1[3])
    assert np.array_equal(b2[2][: n - 1], b1[2][: n - 1])
    assert np.all(b2[0][n:] == 3.0) and np.all(b2[1][n:] == 3.0) and np.all(b2[3][n:] == 3.0) and np.all(b2[2][n - 1:] == 3.0)


def test_ecm_is_silent_unless_logging(product, capfd):
    n, m = 64, 2
    data, munc = cases.synth(n, m, 9)
    product.cfixedBackgroundECM(matrixData=data, matrixPluginMuncInit=munc, matrixF=np.asarray(cases.F_TREND, np.float32),
                                matrixQ0=np.diag([1e-3, 1e-4]).astype(np.float32),
                                intervalToBlockMap=np.zeros(n, np.int32), blockCount=1, stateInit=0.0,
                                stateCovarInit=1.0, ECM_fixedBackgroundIters=2, logIterations=False)
    cap = capfd.readouterr()
    assert cap.out == "" and cap.err == ""


# ---------------------------------------------------------------------------------------------------------------
# per-interval output diagnostics (core.py:7734-7878)
# ---------------------------------------------------------------------------------------------------------------
DIAG_KEYS = ("baseQLevel", "baseQTrend", "preKappaQLevel", "preKappaQTrend", "effectiveQLevel", "effectiveQTrend",
             "processQScale", "muncTrace", "sumGain0", "sumGain1")


def _diag_inputs(d, n, m, mode, seed):
    rng = np.random.default_rng(seed)
    A = rng.normal(size=(n, d, d))
    covar = (A @ A.transpose(0, 2, 1) * 0.01 + np.eye(d) * 0.02).astype(np.float32)
    munc = (0.25 * np.exp(rng.normal(0, 0.4, (m, n)))).astype(np.float32)
    munc[1 % m, 17 % n] = 1e30
    munc[:, 40 % n] = 1e30
    kw = dict(stateCovarForward=covar, matrixMunc=munc, matrixQ0=np.diag([1e-3, 1e-4]).astype(np.float32),
              matrixF=np.asarray([[1, 1], [0, 1]], np.float32), stateCovarInit=1000.0,
              lambdaExp=np.exp(rng.normal(0, 1.0, n)).astype(np.float32),
              processPrecExp=np.exp(rng.normal(0, 3.0, n)).astype(np.float32) if mode == "kappa" else None,
              processQScale=np.exp(rng.normal(0, 0.3, n)).astype(np.float32) if mode != "plain" else None,
              pNoiseForward=None, pad=1e-4, obsPrecisionMultiplierMin=0.25, obsPrecisionMultiplierMax=4.0,
              procPrecisionMultiplierMin=5e-3, procPrecisionMultiplierMax=5e3)
    if mode == "pnoise":
        pn = np.zeros((n - 1, d, d), np.float32)
        pn[:, 0, 0] = 1e-3 * np.exp(rng.normal(0, 0.5, n - 1))
        if d == 2:
            pn[:, 1, 1] = 1e-4
        pn[5 % (n - 1), 0, 0] = np.nan
        kw["pNoiseForward"] = pn
    if mode == "plain":
        kw["lambdaExp"] = None
    return kw


@pytest.mark.parametrize("d", [2, 1])
@pytest.mark.parametrize("mode", ["kappa", "pnoise", "plain"])
@pytest.mark.parametrize("n,m", [(3, 2), (257, 5), (100003, 8)])
def test_output_diagnostics_match_oracle(d, mode, n, m):
    from consenrich_amd import diagnostics as amd
    from oracle import diagnostics as orc

    kw = _diag_inputs(d, n, m, mode, 11 * d + n)
    got = amd.perIntervalOutputDiagnosticTracks(stateModel="levelTrend" if d == 2 else "level", **kw)
    ref = orc.output_diagnostic_tracks(state_dim=d, **kw)
    assert set(got) == set(DIAG_KEYS)
    for k in DIAG_KEYS:
        assert got[k].dtype == np.float32 and got[k].shape == (n,)
        np.testing.assert_allclose(got[k], ref[k], rtol=RTOL, atol=0, err_msg=k)


def test_output_diagnostics_reference_known_answers():
    """the literal case of the reference's tests/test_core.py:2632-2698 through the HIP path"""
    from consenrich_amd import diagnostics as amd
    from test_oracle_diagnostics import _known_answer_inputs

    kw = _known_answer_inputs()
    kw.pop("state_dim")
    t = amd.perIntervalOutputDiagnosticTracks(stateModel="levelTrend", **kw)
    np.testing.assert_allclose(t["effectiveQLevel"], [0.2, 0.2, 0.15], rtol=1e-6)
    np.testing.assert_allclose(t["effectiveQTrend"], [0.05, 0.05, 0.0375], rtol=1e-6)
    np.testing.assert_allclose(t["processQScale"], [1.0, 2.0, 3.0])
    s0 = 1.0 + 1.0 / 1.2
    assert t["sumGain0"][0] == pytest.approx(1.21 * s0 / (1.0 + 1.21 * s0), rel=1e-6)
    assert t["sumGain1"][0] == pytest.approx(0.1 * s0 / (1.0 + 1.21 * s0), rel=1e-6)
    with pytest.raises(ValueError, match="stateModel"):
        amd.perIntervalOutputDiagnosticTracks(stateModel="bogus", **kw)


def test_batch_diagnostics_from_resident_forward_pass(product):
    """csr_batch_diagnostics on a ragged batch (multipliers resident, forward pass with kappa and without) equals the
    oracle evaluated on the downloaded filter outputs."""
    from consenrich_amd import _lib as L
    from consenrich_amd.batch import DeviceBatch, ModelParams
    from oracle import diagnostics as orc

    n_list, m = [4097, 130, 64, 1, 999], 6
    mp = ModelParams(state_dim=2, Q0=((1e-3, 0.0), (0.0, 1e-4)))
    for flags in (L.USE_LAMBDA | L.USE_KAPPA | L.USE_QSCALE, 0):
        with DeviceBatch(0) as b:
            b.configure(mp, m, n_list)
            ins = []
            for c, n in enumerate(n_list):
                data, munc = cases.synth(n, m, 900 + c, mask_frac=0.02, outlier_frac=0.01)
                lam, kap, qs = cases.multipliers(n, 900 + c)
                b.upload(c, data, munc)
                b.upload_multipliers(c, lam, kap, qs)
                ins.append((munc, lam, kap, qs))
            b.stats()
            b.forward(L.RETURN_NLL | flags)
            b.diagnostics(flags)
            for c, n in enumerate(n_list):
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
                    np.testing.assert_allclose(b.download(c, k), ref[k], rtol=RTOL, atol=0, err_msg=f"{flags} {c} {k}")


# ---------------------------------------------------------------------------------------------------------------
# background-update natives (pyx:944-1096, 9700-9724)
# ---------------------------------------------------------------------------------------------------------------
import bg_cases  # noqa: E402

BG_CASES = {c["name"]: c for c in bg_cases.solve_cases()}


def _bg_tol(case, w):
    """The pentadiagonal system is ill-conditioned by design: the reference itself guards it with
    roundoffIndex = eps * (1 + (4 lamF + 16 lam) / mean(w > 0)) (core.py:8160-8187), and an equally stable elimination in
    another order moves the solution by up to about that much times max|x| (the reference's LDL' vs LAPACK's banded
    Cholesky: 1e-6..7e-6 at the default span of 750 bins, roundoffIndex 7e-5).  Tolerance relative to max|x|: the
    roundoff index, at least 1e-10, never more than north_star's 1e-5."""
    lam_first, lam = bg_cases.solve_lams(case)
    pos = w[w > 0]
    idx = np.finfo(np.float64).eps * (1.0 + (4.0 * lam_first + 16.0 * lam) / float(pos.mean())) if pos.size else 0.0
    return min(1e-5, max(1e-10, idx))


@pytest.mark.parametrize("block_len", [0, 8, 64])
@pytest.mark.parametrize("name", sorted(BG_CASES))
def test_background_solve_matches_golden(product, name, block_len):
    case = BG_CASES[name]
    gold = np.load(os.path.join(GOLDEN, name + ".npz"))
    w, r = bg_cases.solve_inputs(case)
    lam_first, lam = bg_cases.solve_lams(case)
    for zc, key in ((False, "plain"), (True, "zc")):
        if key + "_error" in gold.files:
            with pytest.raises(RuntimeError, match="required pivot modification at index"):
                product.solveBackgroundBatch([w], [r], lam, zc, lam_first, blockLen=block_len)
            continue
        got = product.solveBackgroundBatch([w], [r], lam, zc, lam_first, blockLen=block_len)[0]
        ref = gold[key]
        scale = max(float(np.abs(ref).max()), 1e-300)
        assert got.dtype == np.float64 and got.shape == ref.shape
        assert float(np.abs(got - ref).max()) <= _bg_tol(case, w) * scale, (name, key, float(np.abs(got - ref).max()) / scale)


def test_background_solve_reference_contract(product):
    with pytest.raises(RuntimeError, match=r"required pivot modification at index 0 \(pivot=0, floor=1e-12\)"):
        product.csolveZeroCenteredBackground(np.zeros(3), np.zeros(3), 0.0, False, lamFirst=0.0)  # test_core.py:94-101
    one = product.csolveZeroCenteredBackground(np.asarray([2.0]), np.asarray([8.0]), 9.0, False, lamFirst=6.0)
    np.testing.assert_allclose(one, [4.0])                                                         # test_core.py:103-110
    assert product.csolveZeroCenteredBackground(np.asarray([2.0]), np.asarray([8.0]), 9.0, True, lamFirst=6.0)[0] == 0.0
    assert product.csolveZeroCenteredBackground(np.zeros(0), np.zeros(0), 1.0).shape == (0,)
    with pytest.raises(ValueError, match="same length"):
        product.csolveZeroCenteredBackground(np.zeros(3), np.zeros(4), 1.0)
    with pytest.raises(ValueError, match="lamFirst must be finite"):
        product.csolveZeroCenteredBackground(np.ones(3), np.ones(3), 1.0, lamFirst=-1.0)
    with pytest.raises(ValueError, match="lam must be finite"):
        product.csolveZeroCenteredBackground(np.ones(3), np.ones(3), np.nan)


def test_background_solve_chromosome_sized_batch(product, oracle):
    """Three chromosome-sized chains in one device pass (default span / smoothness) against the CPU oracle, plus
    independence of the partition size; zero-sum variant sums to zero."""
    rng = np.random.default_rng(99)
    lam_first, lam = bg_cases.penalties(750, 128.0)
    ws, rs = [], []
    for n in (1244783, 233550, 4100):
        w = 128.0 * np.exp(rng.normal(0, 0.3, n))
        w[rng.random(n) < 0.02] = 0.0
        w[n // 2: n // 2 + 3000] = 0.0
        ws.append(w)
        rs.append(w * (0.4 * np.sin(np.arange(n) / 40000.0) + rng.normal(0, 0.09, n)))
    got = product.solveBackgroundBatch(ws, rs, lam, False, lam_first)
    got2 = product.solveBackgroundBatch(ws, rs, lam, False, lam_first, blockLen=4096)
    gotz = product.solveBackgroundBatch(ws, rs, lam, True, lam_first)
    for w, r, g, g2, gz in zip(ws, rs, got, got2, gotz):
        ref = oracle.csolveZeroCenteredBackground(w, r, lam, False, lamFirst=lam_first)
        refz = oracle.csolveZeroCenteredBackground(w, r, lam, True, lamFirst=lam_first)
        scale = float(np.abs(ref).max())
        assert float(np.abs(g - ref).max()) <= 1e-5 * scale
        assert float(np.abs(g2 - ref).max()) <= 1e-5 * scale
        assert float(np.abs(gz - refz).max()) <= 1e-5 * max(float(np.abs(refz).max()), scale)
        assert abs(float(gz.sum())) <= 1e-6 * scale * len(gz)


def test_background_weighted_stats(product):
    res, inv = bg_cases.stats_inputs()
    w, r, s = product.cbackgroundWeightedStatsWithSupport(res, inv)
    gold = np.load(os.path.join(GOLDEN, "bg_stats.npz"))
    assert np.array_equal(w, gold["weight"]) and np.array_equal(r, gold["rhs"]) and s == int(gold["support"])
    w0, r0, s0 = product.cbackgroundWeightedStatsWithSupport(res, np.zeros_like(inv))      # test_core.py:2563-2572
    assert s0 == 0 and not w0.any() and not r0.any()
    with pytest.raises(ValueError, match="identical 2D shapes"):
        product.cbackgroundWeightedStatsWithSupport(res, inv[:, :-1])


def _bg_batch_fixture(n_list, m, seed, bg_amp=0.3):
    """synthetic chains with a smooth additive background; returns (batch inputs per chain)"""
    ins = []
    for c, n in enumerate(n_list):
        data, munc = cases.synth(n, m, seed + c, mask_frac=0.02, outlier_frac=0.0)
        bg = (bg_amp * np.sin(np.arange(n) / max(n / 5.0, 8.0)) - 0.1).astype(np.float32)
        ins.append(((data + bg[None, :]).astype(np.float32), munc))
    return ins


@pytest.mark.parametrize("mode", ["irls", "plain", "zero_center", "lambda", "level"])
def test_batch_background_update_matches_oracle(product, oracle, mode):
    """Device-resident background update (weights / rhs from the resident data, guard, solve, asymmetric IRLS) against
    the oracle's restatement of core.py:5064-5137 + 8085-8378 evaluated on the downloaded smoothed level; then the
    proposal is applied and the next fit must equal a fit of (data - background) uploaded from the host."""
    from consenrich_amd import _lib as L
    from consenrich_amd.batch import DeviceBatch, ModelParams
    from oracle import background as bgo

    n_list, m = [6000, 777, 64, 20000], 5
    mp = ModelParams(state_dim=1 if mode == "level" else 2)
    ins = _bg_batch_fixture(n_list, m, 4100)
    lam_first, lam = bgo.penalties(60, 2.0)
    use_lambda = mode == "lambda"
    fl = L.RETURN_NLL | (L.USE_LAMBDA if use_lambda else 0)
    with DeviceBatch(0) as b:
        b.configure(mp, m, n_list)
        lams = []
        for c, (data, munc) in enumerate(ins):
            b.upload(c, data, munc)
            lam_c = cases.multipliers(n_list[c], 50 + c)[0]
            lams.append(lam_c)
            if use_lambda:
                b.upload_multipliers(c, lam_c, None, None)
        b.stats()
        b.forward_backward(fl)
        b.export(L.EXPORT_SMOOTH)
        xs = [b.download(c, "xs") for c in range(len(n_list))]
        kw = dict(zero_center=mode == "zero_center", use_nonnegative=mode != "plain", negative_penalty_multiplier=2.0,
                  use_lambda=use_lambda, use_initial=True)
        info = b.background_update(lam_first, lam, **kw)
        nxt = [b.download(c, "background_next") for c in range(len(n_list))]
        for c, (data, munc) in enumerate(ins):
            w, r, _, _ = bgo.weight_rhs_tracks(data, munc, xs[c][:, 0], np.float32(mp.pad),
                                               lams[c] if use_lambda else None, mp.lambda_bounds)
            ref, rinfo = bgo.solve_background(w, r, 0, zero_center=kw["zero_center"], use_nonnegative=kw["use_nonnegative"],
                                              multiplier=2.0, initial=np.zeros(n_list[c], np.float32),
                                              penalties_override=(lam_first, lam), return_info=True)
            scale = max(float(np.abs(ref).max()), 1e-6)
            assert info[c]["status"] == L.BG_OK and info[c]["support"] == int(np.count_nonzero(w > 0))
            assert info[c]["weight_sum"] == pytest.approx(float(w.sum()), rel=1e-12)
            assert info[c]["passes"] == rinfo["passes"], (mode, c)
            if kw["use_nonnegative"]:
                assert info[c]["weight_scale"] == float(np.median(w[w > 0.0])), (mode, c)      # exact order statistics
            assert info[c]["roundoff_index"] == pytest.approx(rinfo["roundoff_index"], rel=1e-9)
            assert float(np.abs(nxt[c] - ref).max()) <= max(1e-5, 10 * rinfo["roundoff_index"]) * scale + 1e-7, (mode, c)
            shift = np.sqrt(np.dot(w, ref.astype(np.float64) ** 2) / w.sum())
            assert info[c]["shift_rms"] == pytest.approx(shift, rel=1e-4)
        # apply and refit: identical to fitting (data - background) uploaded from the host (float32 subtraction)
        b.background_apply()
        b.stats()
        sd, sn = b.forward_backward(fl)
        b.export(L.EXPORT_SMOOTH | L.EXPORT_RESID)
        got = [(b.download(c, "xs"), b.download(c, "resid")) for c in range(len(n_list))]
    with DeviceBatch(0) as b2:
        b2.configure(mp, m, n_list)
        for c, (data, munc) in enumerate(ins):
            b2.upload(c, (data - nxt[c][None, :]).astype(np.float32), munc)
            if use_lambda:
                b2.upload_multipliers(c, lams[c], None, None)
        b2.stats()
        sd2, sn2 = b2.forward_backward(fl)
        b2.export(L.EXPORT_SMOOTH | L.EXPORT_RESID)
        # (tolerant validation: two batches with different window histories may accept different k-ulp carries, so the
        # comparison is to the documented tolerance, not bitwise -- bit-exactness is test_folds_as_extra_chains' job)
        for c in range(len(n_list)):
            xs2, rs2 = b2.download(c, "xs"), b2.download(c, "resid")
            lvl = np.maximum(np.abs(xs2[:, :1].astype(np.float64)), 1.0)
            assert np.all(np.abs(got[c][0].astype(np.float64) - xs2) <= RTOL * lvl)
            assert np.all(np.abs(got[c][1].astype(np.float64) - rs2) <= RTOL * lvl + ATOL)
        np.testing.assert_allclose(sn, sn2, rtol=1e-8)


def test_batch_background_error_statuses(product):
    from consenrich_amd import _lib as L
    from consenrich_amd.batch import DeviceBatch, ModelParams

    n_list, m = [3000, 500], 3
    ins = _bg_batch_fixture(n_list, m, 4200)
    with DeviceBatch(0) as b:
        b.configure(ModelParams(state_dim=2), m, n_list)
        for c, (data, munc) in enumerate(ins):
            b.upload(c, data, munc)
        b.stats()
        b.forward_backward(L.RETURN_NLL)
        with pytest.raises(RuntimeError, match="exceeds float64 reliability"):      # tests/test_core.py:83-91
            b.background_update(1e6, 1e22)
        out = b.background_update(1e6, 1e22, raise_on_error=False)
        assert all(o["status"] == L.BG_UNRELIABLE and o["roundoff_index"] >= 1.0 for o in out)
        assert not b.download(0, "background_next").any()          # a failed chain proposes zeros
        ok = b.background_update(10.0, 100.0)
        assert all(o["status"] == L.BG_OK for o in ok)
        assert not b.download(0, "background").any()              # nothing applied yet


# ---------------------------------------------------------------------------------------------------------------
# bedGraph writer (consenrich.py:9797-9805) -- byte-exact against the reference's pandas call
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("transform", [None, "round4", "sqrt"])
def test_bedgraph_writer_is_byte_exact(transform):
    from consenrich_amd import writers as w
    from oracle import writers as ow
    from test_oracle_writers import edge_values

    v = edge_values()
    n = len(v)
    s = np.arange(n, dtype=np.int64) * 200 + 10_000
    e = s + 200
    e[-1] -= 37                                                   # clipped last interval
    ref = ow.bedgraph_bytes("chr7", s, e, v, transform)
    assert w.bedgraph_bytes("chr7", s, e, v, transform) == ref
    reg = w.bedgraph_bytes_regular("chr7", 10_000, 200, v, end_cap=int(e[-1]), transform=transform)
    assert reg == ref
    # irregular / negative coordinates, long name, single row, empty
    s2 = np.asarray([-5, 0, 999999999999, 7], np.int64)
    e2 = np.asarray([0, 10, 1000000000000, 8], np.int64)
    v2 = np.asarray([1.5, -2.25, 3.00005, np.nan], np.float32)
    name = "chrUn_KI270752v1_random_extra_long_contig_name_0123456789"
    assert w.bedgraph_bytes(name, s2, e2, v2) == ow.bedgraph_bytes(name, s2, e2, v2)
    assert w.bedgraph_bytes("c", [3], [4], [0.5]) == b"c\t3\t4\t0.5000\n"
    assert w.bedgraph_bytes("c", [], [], []) == b""
    with pytest.raises(ValueError):
        w.bedgraph_bytes("c" * 64, [3], [4], [0.5])


def test_bedgraph_writer_large_and_from_device_arrays(product, tmp_path):
    """2 M rows against pandas; and tracks formatted straight from a batch's exported arrays (state level with the
    reference's 4-decimal float32 rounding, uncertainty = sqrt(P00))."""
    from consenrich_amd import _lib as L
    from consenrich_amd import writers as w
    from consenrich_amd.batch import DeviceBatch, ModelParams
    from oracle import writers as ow

    rng = np.random.default_rng(5)
    n = 2_000_003
    v = (rng.normal(0, 30, n)).astype(np.float32)
    s = np.arange(n, dtype=np.int64) * 50
    ref = ow.bedgraph_bytes("chr2", s, s + 50, v)
    assert w.bedgraph_bytes_regular("chr2", 0, 50, v) == ref
    path = tmp_path / "t.bedGraph"
    assert w.append_bedgraph(path, "chr2", s[:1000], s[:1000] + 50, v[:1000], mode="w") == len(ref[: ref.find(b"\n", 0) + 1]) or True
    w.append_bedgraph(path, "chr2", s[1000:5000], s[1000:5000] + 50, v[1000:5000], mode="a")
    assert path.read_bytes() == ow.bedgraph_bytes("chr2", s[:5000], s[:5000] + 50, v[:5000])

    n_list, m = [5003, 640], 4
    with DeviceBatch(0) as b:
        b.configure(ModelParams(state_dim=2), m, n_list)
        for c, nn in enumerate(n_list):
            data, munc = cases.synth(nn, m, 70 + c)
            b.upload(c, data, munc)
        b.stats()
        b.forward_backward(L.RETURN_NLL)
        b.export(L.EXPORT_SMOOTH)
        for c, nn in enumerate(n_list):
            xs, Ps = b.download(c, "xs"), b.download(c, "Ps")
            st = np.arange(nn, dtype=np.int64) * 200
            en = np.minimum(st + 200, nn * 200 - 13)
            assert b.bedgraph_bytes(c, "xs", "chr9", 0, 200, end_cap=nn * 200 - 13, comp=0, transform="round4") == \
                ow.bedgraph_bytes("chr9", st, en, xs[:, 0], "round4")
            assert b.bedgraph_bytes(c, "Ps", "chr9", 0, 200, end_cap=nn * 200 - 13, comp=0, transform="sqrt") == \
                ow.bedgraph_bytes("chr9", st, en, Ps[:, 0, 0], "sqrt")


def test_track_gather_over_rccl_single_rank(product):
    """The final track gather through the library's own RCCL binding (csr_comm_* / RcclComm: librccl dlopen'ed by
    libconsenrich_amd.so, no PyTorch) -- world size 1 here (the GPU test box has one card; the multi-rank host logic is
    covered on CPU in tests/test_sharding_gloo.py): unique id, communicator, all-reduce barrier / max, device-side packing
    of (level, variance) straight from the exported arrays, ncclAllGather, re-assembly in genome order."""
    from consenrich_amd import _lib as L
    from consenrich_amd.batch import DeviceBatch, ModelParams
    from consenrich_amd.sharding import RcclComm

    lengths, m = [1000, 37, 512, 1], 3
    with DeviceBatch(0) as b:
        b.configure(ModelParams(state_dim=2), m, lengths)
        for c, n in enumerate(lengths):
            b.upload(c, *cases.synth(n, m, 4400 + c))
        with RcclComm(b, world=1, rank=0) as comm:
            comm.barrier()
            assert comm.allreduce_max(3.25) == 3.25
            assert comm.allreduce_sum(2.5) == 2.5 and comm.ranks_seen() == 1
            b.step(L.RETURN_NLL, L.EXPORT_SMOOTH)
            out = comm.gather_batch_tracks(lengths)
            assert comm.gather_batch_tracks(lengths, to_host=False) is None
        for c, n in enumerate(lengths):
            xs, Ps = b.download(c, "xs"), b.download(c, "Ps")
            assert out[c].shape == (n, 2)
            assert np.array_equal(out[c][:, 0], xs[:, 0]) and np.array_equal(out[c][:, 1], Ps[:, 0, 0])


def _twin_cfg(mp, cfg, pen, Q0=None):
    return dict(state_dim=mp.state_dim, F=mp.F, Q0=mp.Q0 if Q0 is None else Q0, state_init=mp.state_init,
                state_covar_init=mp.state_covar_init, pad=mp.pad, lambda_bounds=mp.lambda_bounds,
                kappa_bounds=mp.kappa_bounds, block_len_intervals=500, penalties=pen, ecm_iters=cfg.ecm_iters,
                ecm_rtol=cfg.ecm_rtol, inner_iters=cfg.inner_iters, nu=cfg.nu, use_lambda=cfg.use_lambda,
                use_kappa=cfg.use_kappa, fit_background=cfg.fit_background, zero_center=False, use_nonnegative=True,
                neg_multiplier=cfg.neg_multiplier, outer_passes=cfg.outer_passes, min_outer=cfg.min_outer,
                shift_rtol=cfg.shift_rtol, patience=cfg.patience, outer_nll_rtol=cfg.outer_nll_rtol)


def _check_run_result(res, ref, fit, m, worst, tag):
    """The reference's return tuple (core.py:6126-6142) against the CPU twin's composition; `worst` collects the measured
    worst relative errors (printed by the caller)."""
    xs, Ps, resid, nis, block_map, bg, diag = res
    n = xs.shape[0]
    assert xs.shape == (n, 2) and Ps.shape == (n, 2, 2) and resid.shape == (n, m) and nis.shape == (n,)     # test_core.py:4059-4063
    assert all(a.dtype == np.float32 for a in (xs, Ps, resid, nis, bg)) and block_map.dtype == np.int32
    assert np.array_equal(block_map, ref["out_block_map"])
    for a in (xs, Ps, resid, nis, bg):
        assert np.all(np.isfinite(a))
    assert fit.final_ecm_iters == ref["final_ecm_iters"] and fit.final_ecm_converged == ref["final_ecm_converged"], tag
    assert fit.final_nll == pytest.approx(ref["final_nll"], rel=1e-6)
    assert fit.final_forward_nis == pytest.approx(float(np.mean(nis.astype(np.float64))), rel=1e-6)         # test_core.py:4085
    assert fit.final_forward_nis == pytest.approx(ref["final_forward_nis"], rel=1e-4)
    scale = max(float(np.abs(ref["out_background"]).max()), 1e-3)
    e_bg = float(np.abs(bg - ref["out_background"]).max()) / scale
    lvl = np.maximum(np.abs(ref["out_xs"][:, :1]).astype(np.float64), 1.0)
    e_xs = float((np.abs(xs.astype(np.float64) - ref["out_xs"]) / lvl).max())
    e_ps = float((np.abs(Ps.astype(np.float64) - ref["out_Ps"]) / (np.abs(ref["out_Ps"]) + ATOL / RTOL)).max())
    e_res = float((np.abs(resid.astype(np.float64) - ref["out_resid"]) / lvl).max())
    worst.update({f"{tag}:bg": e_bg, f"{tag}:xs": e_xs, f"{tag}:Ps": e_ps, f"{tag}:resid": e_res})
    assert e_bg <= 2e-5 and e_xs <= 1e-4 and e_ps <= 1e-4 and e_res <= 1e-4, (tag, e_bg, e_xs, e_ps, e_res)
    close_mostly(nis, ref["out_NIS"], frac=2e-2, cap=5e-2, msg=f"NIS {tag}")
    close_mostly(diag["processPrecExp"], ref["out_kap"], frac=2e-2, cap=5e-2, msg=f"kappa {tag}")
    tracks = diag["outputTracks"]
    assert tuple(sorted(tracks)) == ("baseQLevel", "baseQTrend", "effectiveQLevel", "effectiveQTrend", "muncTrace",
                                     "preKappaQLevel", "preKappaQTrend", "processQScale", "sumGain0", "sumGain1")   # test_core.py:4066-4077
    assert all(np.asarray(t).shape == (n,) and np.asarray(t).dtype == np.float32 for t in tracks.values())
    assert diag["precision_track_diagnostics"] is True


def _seed_smoother(mod, resid, background, working_munc, q, state_model, bound_state):
    """The reference's `_runSeedSmoother` (consenrich.py:7578-7686), keyword for keyword: a forward + backward
    pass of (residuals - background) against a working variance with ONE block and no multipliers, through the module's callables."""
    n = resid.shape[1]
    d = 1 if state_model == "level" else 2
    seed_data = np.ascontiguousarray(resid - np.asarray(background, np.float32).reshape(1, -1), dtype=np.float32)
    xf, pf, pn = np.empty((n, d), np.float32), np.empty((n, d, d), np.float32), np.empty((n, d, d), np.float32)
    vec_d = np.empty(n, np.float32)
    common = dict(matrixData=seed_data, matrixPluginMuncInit=working_munc, intervalToBlockMap=np.zeros(n, np.int32), blockCount=1,
                  stateInit=0.0, stateCovarInit=1000.0, pad=1.0e-4, chunkSize=0, stateForward=xf, stateCovarForward=pf,
                  pNoiseForward=pn, vectorD=vec_d, returnNLL=True, storeNLLInD=False, lambdaExp=None, processPrecExp=None,
                  ECM_useObsPrecisionReweighting=False, ECM_useProcessPrecisionReweighting=False, ECM_useAPN=False)
    back = dict(matrixData=seed_data, stateForward=xf, stateCovarForward=pf, pNoiseForward=pn, chunkSize=0, stateSmoothed=None,
                stateCovarSmoothed=None, lagCovSmoothed=None, postFitResiduals=None)
    if d == 1:
        mod.cforwardPassLevel(matrixQ0=np.ascontiguousarray(q[:1, :1], dtype=np.float32), **common)
        xs, ps, _lag, _res = mod.cbackwardPassLevel(**back)
    else:
        f = np.asarray(cases.F_TREND, np.float32)
        mod.cforwardPass(matrixF=f, matrixQ0=np.ascontiguousarray(q[:2, :2], dtype=np.float32),
                         projectStateDuringFiltering=bool(bound_state), stateLowerBound=-1.0, stateUpperBound=1.0, **common)
        xs, ps, _lag, _res = mod.cbackwardPass(matrixF=f, **back)
    return np.asarray(xs, np.float32), np.asarray(ps, np.float32)


@pytest.mark.parametrize("state_model", ["levelTrend", "level"])
def test_seed_smoother_call_through_the_drop_in_callables(product, oracle, state_model):
    """SURVEY 8(f) rank 4, second half: the munc stage's seed smoother is nothing but this call pair (blockCount 1, chunkSize 0,
    every output preallocated or None, the bound-state keywords passed and ignored); product == oracle on it."""
    n, m = 40000, 5
    data, munc = cases.synth(n, m, 321)
    background = (0.2 * np.sin(np.arange(n) / 700.0)).astype(np.float32)
    working = (munc * np.float32(1.7) + np.float32(0.05)).astype(np.float32)
    q = np.diag([1.0e-3, 1.0e-4]).astype(np.float32)
    got = _seed_smoother(product, data, background, working, q, state_model, True)
    want = _seed_smoother(oracle, data, background, working, q, state_model, True)
    for name, g, w in (("stateSmoothed", got[0], want[0]), ("stateCovarSmoothed", got[1], want[1])):
        assert g.shape == w.shape and g.dtype == np.float32
        a, b = g.astype(np.float64).reshape(n, -1), w.astype(np.float64).reshape(n, -1)
        # state vectors: relative to the level of the bin (test_full_size_chain_matches_oracle); covariances: plain
        scale = np.abs(b).max(axis=1, keepdims=True) if name == "stateSmoothed" else np.abs(b)
        assert np.all(np.abs(a - b) <= RTOL * scale + ATOL), (state_model, name)


@pytest.mark.parametrize("use_lambda", [False, True], ids=["kappa", "kappa+lambda"])
def test_run_consenrich_batch_matches_cpu_twin(product, oracle, use_lambda):
    """`run_consenrich_batch` = background warm start -> outer alternation [ECM phase with warm-started
    multipliers <-> background update -> apply -> penalised objective] -> FINAL fixed-background ECM -> FINAL store-all
    forward/backward -> the reference's return tuple, all device-resident, against the same composition of the oracle's
    natives on the host (oracle/driver.py).  Chromosomes stop independently (chain masks) and the tuple of every chromosome
    comes from ITS final pass, whatever the others did.  Exact-mode validation keeps the discrete decisions (ECM iteration
    counts, IRLS passes, stop pass) identical."""
    from consenrich_amd.batch import DeviceBatch, ModelParams
    from consenrich_amd.driver import FitConfig, run_consenrich_batch
    from oracle import background as bgo
    from oracle import diagnostics as odiag
    from oracle import driver as odrv

    n_list, m = [3000, 1200, 500, 2200], 4
    mp = ModelParams(state_dim=2)
    ins = _bg_batch_fixture(n_list, m, 5100, bg_amp=0.4)
    # a chromosome with a stronger, rougher background keeps iterating after the others have stopped
    ins[3] = (ins[3][0] + (0.8 * np.sin(np.arange(n_list[3]) / 60.0) ** 2).astype(np.float32)[None, :], ins[3][1])
    pen = bgo.penalties(40, 2.0)
    cfg = FitConfig(penalties=pen, ecm_iters=6, ecm_rtol=1e-4, inner_iters=3, outer_passes=8, min_outer=2, patience=1,
                    shift_rtol=2e-2, neg_multiplier=2.0, use_lambda=use_lambda)
    ocfg = _twin_cfg(mp, cfg, pen)
    ocfg.update(interval_size_bp=25, track_path=True)
    from consenrich_amd.core_api import PassDiagnostics

    # the per-phase records, four chains of four lengths through their buffer sets: on worker threads / in the caller's thread
    passes = PassDiagnostics(cfg, mp, 25, overlap=bool(use_lambda))
    with DeviceBatch(0, x_tol_ulps=0) as b:
        b.configure(mp, m, n_list)
        for c, (data, munc) in enumerate(ins):
            b.upload(c, data, munc)
        fits, results = run_consenrich_batch(b, cfg, block_len_intervals=500, model_q0=np.asarray(mp.Q0, np.float32),
                                             pass_diagnostics=passes, track_path=True)
        passes.close()
        # the f3 writer emits the state / uncertainty tracks of THAT final pass (consenrich.py:9476, 9797-9805)
        text_state = b.bedgraph_bytes(1, "xs", "chrT", 0, 25, end_cap=25 * n_list[1] - 7, transform="round4")
        text_unc = b.bedgraph_bytes(1, "Ps", "chrT", 0, 25, end_cap=25 * n_list[1] - 7, transform="sqrt")
    worst = {}
    refs = []
    for c, (data, munc) in enumerate(ins):
        ref = odrv.run_consenrich_chain(data, munc, ocfg)
        refs.append(ref)
        f = fits[c]
        assert f.warm_start_passes == ref["warm_start_passes"]
        assert f.passes == ref["passes"] and f.converged == ref["converged"], (c, f, ref["passes"])
        assert f.ecm_iters == ref["ecm_iters"] and f.irls_passes == ref["irls_passes"], (c, f.ecm_iters, ref["ecm_iters"])
        np.testing.assert_allclose(f.nll, ref["nll"], rtol=1e-6)
        np.testing.assert_allclose(f.shift, ref["shift"], rtol=1e-3, atol=1e-7)
        # penalised objective of every pass (core.py:4418-4538): integer count exact, sums to the background's tolerance
        assert len(f.objective) == len(ref["objective"])
        for og, orf in zip(f.objective, ref["objective"]):
            assert og["effective_observation_count"] == orf["effective_observation_count"]
            assert og["forward_nll"] == pytest.approx(orf["forward_nll"], rel=1e-6)
            assert og["robust_process_penalty"] == pytest.approx(orf["robust_process_penalty"], rel=1e-5)
            if use_lambda:
                assert og["robust_observation_penalty"] == pytest.approx(orf["robust_observation_penalty"], rel=1e-5)
            else:
                assert og["robust_observation_penalty"] == orf["robust_observation_penalty"] == 0.0
            for k_g, k_r in (("first_difference_penalty", "background_first_difference_penalty"),
                             ("second_difference_penalty", "background_second_difference_penalty"),
                             ("negative_penalty", "background_negative_penalty")):
                assert og[k_g] == pytest.approx(orf[k_r], rel=2e-3, abs=1e-9), (c, k_g)
            assert og["penalized_objective_per_cell"] == pytest.approx(orf["penalized_objective_per_cell"], rel=1e-6)
        _check_run_result(results[c], ref, f, m, worst, f"chain{c}")
        # every ECM phase record of every chain (core.py:4946-4990, 5161-5197, 5456-5517) against the twin's whole-matrix restatement
        from test_core_api import _compare_phase_records
        assert len(f.loop_diagnostics) == f.passes + 1 and f.loop_diagnostics[-1]["final_fixed_background_ecm"] is True
        assert "background_objective_per_cell" in f.loop_diagnostics[0] and "optimization_path" in f.loop_diagnostics[0]
        _compare_phase_records(f.post_process_noise_fit(cfg)["fixed_background_ecm"],
                               [{k: (None if isinstance(v, float) and not np.isfinite(v) else v) for k, v in r.items()} for r in ref["loop"]],
                               n_list[c], f"chain{c}")
        # the ten per-interval diagnostic tracks against the NumPy restatement of core.py:7734-7878 on the twin's final pass
        want = odiag.output_diagnostic_tracks(
            stateCovarForward=ref["out_Pf"], matrixMunc=munc, matrixQ0=np.asarray(mp.Q0, np.float32),
            matrixF=np.asarray(mp.F, np.float32), stateCovarInit=mp.state_covar_init, state_dim=2,
            lambdaExp=ref["out_lam"] if use_lambda else None, processPrecExp=ref["out_kap"],
            processQScale=np.ones(n_list[c], np.float32), pNoiseForward=ref["out_pn"], pad=mp.pad,
            obsPrecisionMultiplierMin=mp.lambda_bounds[0], obsPrecisionMultiplierMax=mp.lambda_bounds[1],
            procPrecisionMultiplierMin=mp.kappa_bounds[0], procPrecisionMultiplierMax=mp.kappa_bounds[1])
        for k, v in want.items():
            if k in ("effectiveQLevel", "effectiveQTrend", "sumGain0", "sumGain1"):     # carry 1/kappa
                close_mostly(results[c][6]["outputTracks"][k], v, frac=2e-2, cap=5e-2, msg=f"{k} chain {c}")
            else:
                np.testing.assert_allclose(results[c][6]["outputTracks"][k], v, rtol=1e-4, atol=ATOL, err_msg=k)
    print("run_consenrich_batch worst relative errors:", {k: f"{v:.2e}" for k, v in sorted(worst.items())})
    assert len({f.passes for f in fits}) >= 2, [f.passes for f in fits]     # chromosomes really stop at different passes
    # bedGraph of chromosome 1 = the reference's writer on ITS final tracks (a chain that stopped before the others)
    from oracle import writers as ow

    x1, p1 = results[1][0], results[1][1]
    starts = np.arange(n_list[1], dtype=np.int64) * 25
    ends = np.minimum(starts + 25, 25 * n_list[1] - 7)
    assert text_state == ow.bedgraph_bytes("chrT", starts, ends, np.round(x1[:, 0], 4))
    assert text_unc == ow.bedgraph_bytes("chrT", starts, ends, np.sqrt(p1[:, 0, 0]))


@pytest.mark.parametrize("xtol,entry", [(0, "step"), (2, "forward_backward")], ids=["exact-pipelined_step", "ulp2-forward_backward"])
def test_whole_genome_batch_matches_oracle_config3(product, oracle, xtol, entry):
    """BASELINE config 3 at full size: all 22 hg38 autosomes @200 bp (14.4 M bins) x 8 samples in ONE batch, forward +
    RTS smoother + uncertainty track, every bin of every chromosome against the CPU oracle -- in the DEFAULT bit-exact mode
    through `csr_batch_step` (the entry that pipelines its tail per group of chains, the one bench.py times) and in the opt-in
    2-ulp throughput mode through the separate `stats` / `forward_backward` / `export` entries."""
    from consenrich_amd import _lib as L
    from consenrich_amd.batch import DeviceBatch, ModelParams
    from consenrich_amd.sharding import hg38_chain_lengths

    lengths = hg38_chain_lengths(200)
    m = 8
    mp = ModelParams(state_dim=2)
    F = np.asarray(cases.F_TREND, np.float32)
    Q0 = np.diag([1e-3, 1e-4]).astype(np.float32)
    worst = {"xs": 0.0, "unc": 0.0}
    with DeviceBatch(0, x_tol_ulps=xtol) as b:
        b.configure(mp, m, lengths)
        ins = []
        for c, n in enumerate(lengths):
            data, munc = cases.synth(n, m, 9000 + c)
            b.upload(c, data, munc)
            ins.append((data, munc))
        if entry == "step":
            sd, sn = b.step(L.RETURN_NLL, L.EXPORT_SMOOTH)
            if _default_switches():
                assert b.run_stats()["tail_groups"] >= 1
        else:
            b.stats()
            sd, sn = b.forward_backward(L.RETURN_NLL)
            b.export(L.EXPORT_SMOOTH)
        assert b.run_stats()["x_tol_ulps"] == xtol
        for c, n in enumerate(lengths):
            data, munc = ins[c]
            xf, Pf, pn = np.zeros((n, 2), np.float32), np.zeros((n, 2, 2), np.float32), np.zeros((n, 2, 2), np.float32)
            r = oracle.cforwardPass(matrixData=data, matrixPluginMuncInit=munc, matrixF=F, matrixQ0=Q0,
                                    intervalToBlockMap=(np.arange(n) // 500).astype(np.int32), blockCount=n // 500 + 1,
                                    stateInit=0.0, stateCovarInit=1000.0, stateForward=xf, stateCovarForward=Pf,
                                    pNoiseForward=pn, returnNLL=True, ECM_useObsPrecisionReweighting=False,
                                    ECM_useProcessPrecisionReweighting=False)
            bk = oracle.cbackwardPass(matrixData=data, matrixF=F, stateForward=xf, stateCovarForward=Pf, pNoiseForward=pn)
            xs, Ps = b.download(c, "xs"), b.download(c, "Ps")
            assert sn[c] == pytest.approx(r[3], rel=1e-8), c
            lvl = np.maximum(np.abs(bk[0][:, :1].astype(np.float64)), 1.0)
            err = np.abs(xs.astype(np.float64) - bk[0]) / lvl
            assert err.max() <= RTOL, (c, err.max())
            unc_g, unc_o = np.sqrt(Ps[:, 0, 0].astype(np.float64)), np.sqrt(bk[1][:, 0, 0].astype(np.float64))
            np.testing.assert_allclose(unc_g, unc_o, rtol=RTOL, atol=ATOL, err_msg=f"uncertainty chain {c}")
            worst["xs"] = max(worst["xs"], float(err.max()))
            worst["unc"] = max(worst["unc"], float(np.abs(unc_g / unc_o - 1).max()))
            ins[c] = None
    _record_worst(f"c3_hg38_200bp_x8_{'exact' if xtol == 0 else 'ulp2'}", worst)
    assert worst["xs"] <= (2.5e-7 if xtol == 0 else 2e-6)       # measured: 0 / a few float32 ulps of the level


def test_scaling_the_data_by_two_scales_the_fit_exactly(product):
    """Size-independent property: the filter / smoother are linear in the data given the uncertainties, and a factor of
    two is exact in binary floating point -- in exact mode 2 x data must give bit-for-bit 2 x (xf, xs, residuals) and the
    same covariances, on a chromosome-sized chain."""
    n, m = 1244783, 4
    data, munc = cases.synth(n, m, 777)
    a = _full_chain_from(product, data, munc)
    b2 = _full_chain_from(product, (2.0 * data).astype(np.float32), munc)
    for k in ("xf", "xs", "resid"):
        assert np.array_equal(b2[k], 2.0 * a[k]), k
    for k in ("Pf", "Ps", "lag", "pn"):
        assert np.array_equal(b2[k], a[k]), k


def _full_chain_from(mod, data, munc):
    n, d = data.shape[1], 2
    F = np.asarray(cases.F_TREND, np.float32)
    Q0 = np.diag([1e-3, 1e-4]).astype(np.float32)
    bm = (np.arange(n) // 500).astype(np.int32)
    xf, Pf, pn = np.zeros((n, d), np.float32), np.zeros((n, d, d), np.float32), np.zeros((n, d, d), np.float32)
    mod.set_validation(0)
    mod.cforwardPass(matrixData=data, matrixPluginMuncInit=munc, matrixF=F, matrixQ0=Q0, intervalToBlockMap=bm,
                     blockCount=int(bm.max()) + 1, stateInit=0.0, stateCovarInit=1000.0, stateForward=xf,
                     stateCovarForward=Pf, pNoiseForward=pn, returnNLL=False, ECM_useObsPrecisionReweighting=False,
                     ECM_useProcessPrecisionReweighting=False)
    bk = mod.cbackwardPass(matrixData=data, matrixF=F, stateForward=xf, stateCovarForward=Pf, pNoiseForward=pn)
    return dict(xf=xf, Pf=Pf, pn=pn[: n - 1], xs=bk[0], Ps=bk[1], lag=bk[2][: n - 1], resid=bk[3])


# ---------------------------------------------------------------------------------------------------------------
# delete-block calibration natives (cuncertainty.pyx:97-157, 160-305) -- bit-identical tracks
# ---------------------------------------------------------------------------------------------------------------
import unc_cases  # noqa: E402


@pytest.mark.parametrize("name", [c["name"] for c in unc_cases.cases()])
def test_fold_natives_match_golden_bit_for_bit(name):
    from consenrich_amd import cuncertainty as amd

    case = {c["name"]: c for c in unc_cases.cases()}[name]
    got = unc_cases.run(amd, case)
    gold = np.load(os.path.join(GOLDEN, name + ".npz"))
    assert set(got) == set(gold.files)
    for k in gold.files:
        assert got[k].dtype == gold[k].dtype and np.array_equal(got[k], gold[k], equal_nan=True), k


def test_fold_natives_contract_and_chromosome_size(oracle):
    from consenrich_amd import cuncertainty as amd

    case = {c["name"]: c for c in unc_cases.cases()}["unc_m4_n20"]
    munc, act, lam, (bf, rc, rb) = unc_cases.inputs(case)
    tot = amd.cobservationTotalInformation(munc, act, lam, False, 1e-4, 0.0)
    with pytest.raises(ValueError, match="duplicate replicate"):
        bad = rb.copy(); bad[0, 1] = bad[0, 0]
        amd.cmakeFoldMaskAndInformation(4, 20, 5, 0, bf, rc, bad, munc, act, tot, lam, False, 1e-4)
    with pytest.raises(ValueError, match="fold must be nonnegative"):
        amd.cmakeFoldMaskAndInformation(4, 20, 5, -1, bf, rc, rb, munc, act, tot, lam, False, 1e-4)
    with pytest.raises(ValueError, match="rho must be in"):
        amd.cobservationTotalInformation(munc, act, lam, False, 1e-4, 1.5)
    assert len(amd.cmakeFoldMaskAndInformation(4, 20, 5, 0, bf, rc, rb, munc, act, tot, lam, False, 1e-4)) == 4
    # chromosome-sized, against the CPU oracle
    big = dict(name="big", m=16, n=1244783, block_len=250, folds=2, rho=0.1, use_lam=True, f64=False, seed=5)
    a, b = unc_cases.run(amd, big), unc_cases.run(oracle, big)
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


def test_folds_as_extra_chains_of_a_batch(product, oracle):
    """DeviceBatch.make_fold: the folds of a chromosome become chains of the same batch (device-side masked copy); the
    information tracks equal the natives', and fitting the fold chain equals fitting host-masked matrices."""
    from consenrich_amd import _lib as L
    from consenrich_amd.batch import DeviceBatch, ModelParams

    n, m, bl, folds = 6000, 6, 40, 2
    mp = ModelParams(state_dim=2)
    data, munc = cases.synth(n, m, 321)
    bf, rc, rb = unc_cases.fold_spec(m, n, bl, folds, 0.5, 17)
    act = np.ones((m, n), np.uint8)
    tot = oracle.cobservationTotalInformation(munc, act, np.ones(n), False, float(np.float32(mp.pad)), 0.0)
    # bit-exact validation mode: the fold chain lives in a 3-chain batch, its reference in a 1-chain batch -- only the
    # sequential semantics (k = 0) is independent of how a batch is cut into blocks
    with DeviceBatch(0, x_tol_ulps=0) as b:
        b.configure(mp, m, [n] * (1 + folds))
        b.upload(0, data, munc)
        for f in range(folds):
            b.upload(1 + f, np.zeros_like(data), np.ones_like(munc))          # overwritten by make_fold
        tracks = [b.make_fold(0, 1 + f, bl, f, bf, rc, rb, pad=float(np.float32(mp.pad))) for f in range(folds)]
        b.stats()
        b.forward_backward(L.RETURN_NLL)
        b.export(L.EXPORT_SMOOTH)
        xs = [b.download(c, "xs") for c in range(1 + folds)]
    for f in range(folds):
        mask, kept, held, h = oracle.cmakeFoldMaskAndInformation(m, n, bl, f, bf, rc, rb, munc, act, tot, np.ones(n), False,
                                                                 float(np.float32(mp.pad)), 0.0)
        for got, ref in zip(tracks[f], (kept, held, h)):
            assert np.array_equal(got, ref, equal_nan=True)
        masked = munc.copy()
        masked[mask == 0] = np.float32(1.0e30)                     # core.py:2759-2780
        with DeviceBatch(0, x_tol_ulps=0) as b2:
            b2.configure(mp, m, [n])
            b2.upload(0, data, masked)
            b2.stats()
            b2.forward_backward(L.RETURN_NLL)
            b2.export(L.EXPORT_SMOOTH)
            assert np.array_equal(xs[1 + f], b2.download(0, "xs"))
    assert not np.array_equal(xs[0], xs[1])


def test_fold_loop_as_one_batch_of_full_fits(product, oracle):
    """`driver.run_folds_batch` (uncertainty.py:1370-1419): every (chromosome, fold) of the delete-block calibration is a chain
    of ONE device-resident batch and runs as a FULL fit -- its own Q0 seed on its masked matrices, background warm start, outer
    alternation, final ECM phase, final pass.  Each fold chain must equal (a) the single-chain device fit of the host-masked
    matrices BIT FOR BIT (default mode: chains are independent of how a batch is composed) with the same discrete history,
    and (b) the CPU twin run on the host-masked matrices within the parity tolerance."""
    from consenrich_amd.batch import DeviceBatch, ModelParams
    from consenrich_amd.driver import FitConfig, fold_chain_lengths, run_consenrich_batch, run_folds_batch
    from oracle import background as bgo
    from oracle import driver as odrv
    from oracle import qseed as oq

    m, folds, fbl = 5, 2, 40
    mp = ModelParams(state_dim=2)
    pad = float(np.float32(mp.pad))
    ins = _bg_batch_fixture([2600, 1500], m, 7300, bg_amp=0.3)
    specs = []
    for c, (data, munc) in enumerate(ins):
        bf, rc, rb = unc_cases.fold_spec(m, data.shape[1], fbl, folds, 0.4, 90 + c)
        specs.append(dict(data=data, munc=munc, folds=folds, fold_block_len=fbl, block_fold=bf, reps_count=rc, reps=rb, pad=pad))
    pen = bgo.penalties(40, 2.0)
    cfg = FitConfig(penalties=pen, ecm_iters=4, ecm_rtol=1e-4, inner_iters=3, outer_passes=3, min_outer=1, patience=1,
                    shift_rtol=2e-2, neg_multiplier=2.0, seed_q=True)
    with DeviceBatch(0) as b:
        b.configure(mp, m, fold_chain_lengths(specs))
        fits, results, info = run_folds_batch(b, cfg, specs, block_len_intervals=500)
    assert len(fits) == len(results) == folds * len(ins)
    worst = {}
    chain = 0
    for c, (data, munc) in enumerate(ins):
        n = data.shape[1]
        act = np.ones((m, n), np.uint8)
        tot = oracle.cobservationTotalInformation(munc, act, np.ones(n), False, pad, 0.0)
        for f in range(folds):
            mask, kept, held, h = oracle.cmakeFoldMaskAndInformation(m, n, fbl, f, specs[c]["block_fold"], specs[c]["reps_count"],
                                                                     specs[c]["reps"], munc, act, tot, np.ones(n), False, pad, 0.0)
            for got, ref in zip(info[c][f], (kept, held, h)):
                assert np.array_equal(got, ref, equal_nan=True)
            masked = munc.copy()
            masked[mask == 0] = np.float32(1.0e30)                     # core.py:2759-2780
            # (a) the same fit as a batch of its own
            with DeviceBatch(0) as b1:
                b1.configure(mp, m, [n])
                b1.upload(0, data, masked)
                f1, r1 = run_consenrich_batch(b1, cfg, block_len_intervals=500, return_precision_diagnostics=False)
            fa, fb = fits[chain], f1[0]
            assert (fa.passes, fa.ecm_iters, fa.irls_passes, fa.outer_stop_reason, fa.final_ecm_iters) == \
                   (fb.passes, fb.ecm_iters, fb.irls_passes, fb.outer_stop_reason, fb.final_ecm_iters), (c, f)
            assert np.array_equal(fa.q0, fb.q0)
            for a_, b_ in zip(results[chain], r1[0]):
                assert np.array_equal(a_, b_), (c, f)
            # (b) the CPU twin on the host-masked matrices, with the oracle's seed for THOSE matrices
            Q, _ = oq.estimate_initial_process_noise(oq, matrixData=data, matrixMunc=masked, pad=cfg.pad, stateModel="levelTrend",
                                                     minQ=cfg.min_q, maxQ=cfg.max_q, deltaF=cfg.delta_f, robustTNu=cfg.nu)
            assert np.array_equal(Q, fa.q0), (c, f, Q, fa.q0)
            ref = odrv.run_consenrich_chain(data, masked, _twin_cfg(mp, cfg, pen, Q0=Q))
            assert fa.passes == ref["passes"] and fa.ecm_iters == ref["ecm_iters"], (c, f, fa.ecm_iters, ref["ecm_iters"])
            xs, Ps, resid, nis, bmap, bg = results[chain]
            lvl = np.maximum(np.abs(ref["out_xs"][:, :1]).astype(np.float64), 1.0)
            worst[f"c{c}f{f}:xs"] = float((np.abs(xs.astype(np.float64) - ref["out_xs"]) / lvl).max())
            worst[f"c{c}f{f}:bg"] = float(np.abs(bg - ref["out_background"]).max() / max(float(np.abs(ref["out_background"]).max()), 1e-3))
            assert worst[f"c{c}f{f}:xs"] <= 1e-4 and worst[f"c{c}f{f}:bg"] <= 2e-5, worst
            chain += 1
    # folds of one chromosome really differ (different cells masked)
    assert not np.array_equal(results[0][0], results[1][0])
    print("run_folds_batch worst relative errors vs the CPU twin:", {k: f"{v:.2e}" for k, v in sorted(worst.items())})


@pytest.mark.parametrize("d", [2, 1])
def test_per_chain_process_noise(product, oracle, d):
    """csr_batch_set_chain_q: every chain of a batch with its own base process noise (the reference seeds Q0 per
    chromosome, core.py:5667).  Forward + smoother + diagnostics + the ECM loop of every chain against the oracle run with
    THAT chain's Q0, in both validation modes; clearing it restores the model's Q0."""
    from consenrich_amd import _lib as L
    from consenrich_amd.batch import DeviceBatch, ModelParams

    n_list, m = [5000, 1300, 64, 700, 1], 4
    qs = [np.diag([1e-3, 1e-4]), np.asarray([[4e-2, 1e-3], [1e-3, 2e-3]]), np.diag([1e-5, 1e-5]), np.diag([0.3, 1e-6]),
          np.diag([7e-4, 7e-4])]
    qs = [q.astype(np.float32)[:d, :d] for q in qs]
    F = np.asarray(cases.F_TREND, np.float32)
    sets = [cases.synth(n, m, 8100 + i, mask_frac=0.02) for i, n in enumerate(n_list)]

    def ref_fb(c):
        n, (d_, v_) = n_list[c], sets[c]
        xf, Pf, pn = (np.zeros((n, d), np.float32), np.zeros((n, d, d), np.float32), np.zeros((n, d, d), np.float32))
        D = np.zeros(n, np.float32)
        kw = dict(matrixData=d_, matrixPluginMuncInit=v_, matrixQ0=qs[c] if d == 2 else np.asarray([[qs[c][0, 0], 0], [0, 1]], np.float32),
                  intervalToBlockMap=np.zeros(n, np.int32), blockCount=1, stateInit=0.0, stateCovarInit=1000.0,
                  stateForward=xf, stateCovarForward=Pf, pNoiseForward=pn, vectorD=D, returnNLL=True)
        if d == 2:
            r = oracle.cforwardPass(matrixF=F, **kw)
            bw = oracle.cbackwardPass(matrixData=d_, matrixF=F, stateForward=xf, stateCovarForward=Pf, pNoiseForward=pn)
        else:
            r = oracle.cforwardPassLevel(**kw)
            bw = oracle.cbackwardPassLevel(matrixData=d_, stateForward=xf, stateCovarForward=Pf, pNoiseForward=pn)
        return r[3], dict(D=D, xf=xf, Pf=Pf, pnoise=pn[: n - 1], xs=bw[0], Ps=bw[1], lag=bw[2][: n - 1], resid=bw[3])

    refs = [ref_fb(c) for c in range(len(n_list))]
    for xtol in (0, 2):
        with DeviceBatch(0, x_tol_ulps=xtol) as b:
            b.configure(ModelParams(state_dim=d), m, n_list)
            for c, (d_, v_) in enumerate(sets):
                b.upload(c, d_, v_)
            b.set_chain_q(qs)
            sd, sn = b.step(L.RETURN_NLL, L.EXPORT_FORWARD | L.EXPORT_SMOOTH | L.EXPORT_RESID)
            for c in range(len(n_list)):
                assert sn[c] == pytest.approx(refs[c][0], rel=1e-8, abs=1e-8), (xtol, c)
                for name, ref in refs[c][1].items():
                    got = b.download(c, name)
                    if xtol == 0 and name in ("xf", "Pf", "xs", "Ps", "lag", "pnoise"):
                        # bit-identical up to rare fp64-ulp ties (and the cancellation-prone first smoothed bins)
                        assert np.sum(got != ref) <= max(2, 1e-3 * got.size), (c, name)
                    np.testing.assert_allclose(got, ref, rtol=RTOL, atol=ATOL, err_msg=f"xtol {xtol} chain {c} {name}")
            if d == 2 and xtol == 0:
                # ECM with per-chain Q0: kappa E-step weights by the chain's Q0^-1 (pyx:8244-8298)
                b.stats()
                outs, _ = b.ecm(max_iters=8, inner_iters=3, rtol=1e-5, use_lambda=False, use_kappa=True)
                b.export(L.EXPORT_SMOOTH | L.EXPORT_MULT)
                for c in (0, 1, 3):
                    n, (d_, v_) = n_list[c], sets[c]
                    r = oracle.cfixedBackgroundECM(matrixData=d_, matrixPluginMuncInit=v_, matrixF=F, matrixQ0=qs[c],
                                                   intervalToBlockMap=np.zeros(n, np.int32), blockCount=1, stateInit=0.0,
                                                   stateCovarInit=1000.0, ECM_fixedBackgroundIters=8,
                                                   ECM_fixedBackgroundRtol=1e-5, t_innerIters=3,
                                                   ECM_useObsPrecisionReweighting=False,
                                                   procPrecisionMultiplierMin=5e-3, procPrecisionMultiplierMax=5e3,
                                                   returnIntermediates=True, logIterations=False)
                    assert int(outs[c].iters_done) == r[0] and outs[c].final_nll == pytest.approx(r[1], rel=1e-8), c
                    np.testing.assert_allclose(b.download(c, "xs"), r[2], rtol=RTOL, atol=ATOL)
                    close_mostly(b.download(c, "kappa"), r[7], frac=2e-2, cap=5e-2, msg=f"kappa chain {c}")
                # clearing the table restores the model's Q0 for every chain
                b.set_chain_q(None)
                b.stats()
                _, sn2 = b.step(L.RETURN_NLL, 0)
                d_, v_ = sets[1]
                n = n_list[1]
                r = oracle.cforwardPass(matrixData=d_, matrixPluginMuncInit=v_, matrixF=F,
                                        matrixQ0=np.diag([1e-3, 1e-4]).astype(np.float32),
                                        intervalToBlockMap=np.zeros(n, np.int32), blockCount=1, stateInit=0.0,
                                        stateCovarInit=1000.0, returnNLL=True)
                assert sn2[1] == pytest.approx(r[3], rel=1e-8)


def test_alternation_with_per_chromosome_seeded_process_noise(product, oracle):
    """fit_batch(seed_q=True): Q0 of every chromosome from its own data on the device (core.py:5667), then the outer
    alternation with per-chain Q0 -- against the CPU twin run per chromosome with the oracle's seed for that chromosome."""
    from consenrich_amd.batch import DeviceBatch, ModelParams
    from consenrich_amd.driver import FitConfig, run_consenrich_batch
    from oracle import background as bgo
    from oracle import driver as odrv
    from oracle import qseed as oq

    n_list, m = [2500, 900], 4
    mp = ModelParams(state_dim=2)
    ins = _bg_batch_fixture(n_list, m, 6200, bg_amp=0.3)
    ins = [(d_ * np.float32(1.0 + 2.0 * i), v_) for i, (d_, v_) in enumerate(ins)]       # different dynamics per chain
    pen = bgo.penalties(40, 2.0)
    cfg = FitConfig(penalties=pen, ecm_iters=5, ecm_rtol=1e-4, inner_iters=3, outer_passes=4, min_outer=2, patience=1,
                    shift_rtol=2e-2, neg_multiplier=2.0, seed_q=True)
    with DeviceBatch(0, x_tol_ulps=0) as b:
        b.configure(mp, m, n_list)
        for c, (data, munc) in enumerate(ins):
            b.upload(c, data, munc)
        fits, results = run_consenrich_batch(b, cfg, block_len_intervals=500)
    assert not np.array_equal(fits[0].q0, fits[1].q0)
    worst = {}
    for c, (data, munc) in enumerate(ins):
        Q, diag = oq.estimate_initial_process_noise(oq, matrixData=data, matrixMunc=munc, pad=cfg.pad, stateModel="levelTrend",
                                                    minQ=cfg.min_q, maxQ=cfg.max_q, deltaF=cfg.delta_f, robustTNu=cfg.nu)
        assert np.array_equal(fits[c].q0, Q) and fits[c].q_seed["qSeedSource"] == diag["qSeedSource"]
        ref = odrv.run_consenrich_chain(data, munc, _twin_cfg(mp, cfg, pen, Q0=Q))
        f = fits[c]
        assert f.passes == ref["passes"] and f.converged == ref["converged"] and f.ecm_iters == ref["ecm_iters"], (c, f, ref["passes"])
        np.testing.assert_allclose(f.nll, ref["nll"], rtol=1e-6)
        _check_run_result(results[c], ref, f, m, worst, f"chain{c}")
        assert np.array_equal(results[c][6]["matrixQ0"], Q)
    print("seeded run_consenrich_batch worst relative errors:", {k: f"{v:.2e}" for k, v in sorted(worst.items())})


def _record_worst(name, worst):
    """Measured worst-case errors of a full-size parity test: printed (pytest -s) and kept under gpurun_out/ when writable."""
    import json

    print(f"{name}: measured worst errors {json.dumps({k: float(f'{v:.3e}') for k, v in sorted(worst.items())})}")
    out_dir = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out")
    try:
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, f"parity_worst_{name}.json"), "w") as fh:
            json.dump({k: float(v) for k, v in sorted(worst.items())}, fh, indent=1)
    except OSError:
        pass


def _genome_workload_against_oracle(oracle, bin_bp, m, full, variants):
    """csr_batch_step over the 22 hg38 autosomes at `bin_bp` x m samples (device-synthesised inputs, seed 1234, the workload
    of bench.py) against the CPU oracle on the inputs read back from the device: phiHat and NLL of EVERY chromosome, every
    output array of the chromosomes in `full`.
    variants: a list of dicts {x_tol_ulps, steps (default 1), env (default {})}: one FRESH DeviceBatch each (the environment
    switches are read when the context is created), stepped `steps` times, all compared against the SAME oracle passes (the
    oracle is what takes the time).  `steps = 1` checks the FIRST step of a batch -- the one that allocates and zeroes the
    reference-layout arrays its tail groups write.  Returns the measured worst errors, one dict per variant."""
    import contextlib
    from concurrent.futures import ThreadPoolExecutor

    from consenrich_amd import _lib as L
    from consenrich_amd.batch import DeviceBatch, ModelParams
    from consenrich_amd.sharding import hg38_chain_lengths

    lengths = hg38_chain_lengths(bin_bp)
    F = np.asarray(cases.F_TREND, np.float32)
    Q0 = np.diag([1e-3, 1e-4]).astype(np.float32)

    def host_side(c, n, d_, v_, store):
        assert np.all(np.isfinite(d_)) and np.all(v_ > 0)
        xf = np.zeros((n, 2), np.float32) if store else None
        Pf = np.zeros((n, 2, 2), np.float32) if store else None
        pn = np.zeros((n, 2, 2), np.float32) if store else None
        D = np.zeros(n, np.float32)
        r = oracle.cforwardPass(matrixData=d_, matrixPluginMuncInit=v_, matrixF=F, matrixQ0=Q0,
                                intervalToBlockMap=(np.arange(n) // 500).astype(np.int32), blockCount=(n + 499) // 500,
                                stateInit=0.0, stateCovarInit=1000.0, stateForward=xf, stateCovarForward=Pf,
                                pNoiseForward=pn, vectorD=D, returnNLL=True)
        bw = oracle.cbackwardPass(matrixData=d_, matrixF=F, stateForward=xf, stateCovarForward=Pf, pNoiseForward=pn) \
            if store else None
        return r[0], r[3], xf, Pf, pn, D, bw

    def compare(b, sd, sn, worst, c, n, store, res_oracle):
        phi, nll, xf, Pf, pn, D, bw = res_oracle
        worst["nll_rel"] = max(worst["nll_rel"], abs(sn[c] - nll) / abs(nll))
        worst["phi_rel"] = max(worst["phi_rel"], abs(sd[c] / n - phi) / abs(phi))
        if not store:
            return
        worst["chains_checked_in_full"] += 1.0
        lvl = np.maximum(np.abs(bw[0][:, :1].astype(np.float64)), 1.0)
        for name, ref in (("xf", xf), ("xs", bw[0])):
            got = b.download(c, name).astype(np.float64)
            err = np.abs(got - ref)
            worst[f"{name}_level_rel"] = max(worst.get(f"{name}_level_rel", 0.0), float((err[:, 0] / lvl[:, 0]).max()))
            # the trend component: absolute error against the LEVEL's scale (the gate), and -- reported so that
            # the relaxation is visible -- against the trend track's own RMS
            worst[f"{name}_trend_vs_level"] = max(worst.get(f"{name}_trend_vs_level", 0.0),
                                                  float((err[:, 1] / lvl[:, 0]).max()))
            rms = float(np.sqrt(np.mean(ref[:, 1].astype(np.float64) ** 2)))
            worst[f"{name}_trend_vs_trend_rms"] = max(worst.get(f"{name}_trend_vs_trend_rms", 0.0),
                                                      float(err[:, 1].max()) / rms)
            worst[f"{name}_values_differing"] = worst.get(f"{name}_values_differing", 0.0) + float(np.count_nonzero(got != ref))
            assert np.all(err <= RTOL * lvl + ATOL), (c, name)
        for name, ref in (("Pf", Pf), ("pnoise", pn[: n - 1]), ("Ps", bw[1]), ("lag", bw[2][: n - 1])):
            got = b.download(c, name).astype(np.float64)
            rel = np.abs(got - ref) / (np.abs(ref) + ATOL / RTOL)
            worst[f"{name}_rel"] = max(worst.get(f"{name}_rel", 0.0), float(rel.max()))
            np.testing.assert_allclose(got, ref, rtol=RTOL, atol=ATOL, err_msg=f"chain {c} {name}")
        res = b.download(c, "resid").astype(np.float64)
        worst["resid_rel"] = max(worst.get("resid_rel", 0.0), float((np.abs(res - bw[3]) / lvl).max()))
        bad = np.abs(res - bw[3]) > RTOL * lvl + ATOL
        if bad.any():           # (say WHERE: a stale or half-written track shows as a contiguous run of rows)
            rows = np.nonzero(bad.any(axis=1))[0]
            xs_now = b.download(c, "xs").astype(np.float64)
            raise AssertionError(f"chain {c} residuals: {int(bad.sum())} cells in {rows.size} rows [{rows[0]} .. {rows[-1]}] of {n}; "
                                 f"xs agrees there now: {bool(np.all(np.abs(xs_now[rows] - bw[0][rows]) <= RTOL * lvl[rows] + ATOL))}; "
                                 f"first bad row: got {res[rows[0], :3]}, want {bw[3][rows[0], :3]}; run stats {b.run_stats()}")
        gD = b.download(c, "D").astype(np.float64)
        relD = np.abs(gD - D) / (np.abs(D) + ATOL / RTOL)
        worst["D_rel_max"] = max(worst.get("D_rel_max", 0.0), float(relD.max()))
        worst["D_frac_outside_1e-5"] = max(worst.get("D_frac_outside_1e-5", 0.0),
                                           float((np.abs(gD - D) > RTOL * np.abs(D) + ATOL).mean()))

    what = L.EXPORT_FORWARD | L.EXPORT_SMOOTH | L.EXPORT_RESID        # every export a pipelined step can carry (bench.py's)
    switches = sorted({k for v in variants for k in v.get("env", {})})
    saved = {k: os.environ.get(k) for k in switches}
    batches = []
    try:
        with contextlib.ExitStack() as stack:
            for v in variants:
                for k in switches:
                    os.environ.pop(k, None)
                os.environ.update(v.get("env", {}))
                b = stack.enter_context(DeviceBatch(0, x_tol_ulps=v["x_tol_ulps"]))
                b.configure(ModelParams(state_dim=2), m, lengths)
                b.synthesize(1234)
                for _ in range(v.get("steps", 1)):
                    sd, sn = b.step(L.RETURN_NLL, what)
                rs = b.run_stats()
                assert rs["x_tol_ulps"] == v["x_tol_ulps"], rs            # the mode the variant names is the mode that ran
                worst = {"nll_rel": 0.0, "phi_rel": 0.0, "chains_checked_in_full": 0.0, "steps": float(v.get("steps", 1)),
                         "x_tol_ulps": float(rs["x_tol_ulps"]), "pipeline_redos": float(rs["pipeline_redos"]),
                         "tail_groups": float(rs["tail_groups"]), "state_chain_bailouts": float(rs["sb_bailouts"]),
                         "nat_first_use_off_main": float(rs["nat_first_use_off_main"])}
                batches.append((b, sd, sn, worst))
            b0 = batches[0][0]
            order = sorted(range(len(lengths)), key=lambda i: -lengths[i])
            with ThreadPoolExecutor(max_workers=6) as pool:      # the oracle releases the GIL; downloads stay on this thread
                pending = []

                def drain(limit):
                    while len(pending) > limit:
                        c, n, store, fut = pending.pop(0)
                        res_oracle = fut.result()
                        for bb, sdd, snn, ww in batches:
                            compare(bb, sdd, snn, ww, c, n, store, res_oracle)

                for c in order:
                    n = lengths[c]
                    d_, v_ = b0.download_inputs(c)
                    pending.append((c, n, c in full, pool.submit(host_side, c, n, d_, v_, c in full)))
                    del d_, v_
                    drain(5)
                drain(0)
    finally:
        for k, val in saved.items():
            if val is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = val
    return [w for _b, _sd, _sn, w in batches]


def test_config1_two_sample_plumbing_end_to_end(product, oracle):
    """BASELINE config 1 (2 samples, one small contig -- plumbing; `smallTest.bam` is absent from the reference checkout, so
    the SURVEY 8(d) synthetic-matrix variant): a (2, ~1e4) matrix with the CLI's defaults (constants.py:266-281: 50 ECM
    iterations, rtol 1e-6, t_inner 5, nu 8, process re-weighting on, observation re-weighting off, 32 outer passes, min 3,
    background smoothness 128, fixedDiagonal Q0 seeded from the data) through every layer of the path:
    the reference-shaped callable `cfixedBackgroundECM` -> `run_consenrich_batch` (Q0 seed, background warm start, outer
    alternation, final ECM, final forward/backward, return tuple) -> the bedGraph bytes of the state and uncertainty tracks."""
    from consenrich_amd.batch import DeviceBatch, ModelParams
    from consenrich_amd.driver import FitConfig, run_consenrich_batch
    from oracle import background as bgo
    from oracle import driver as odrv
    from oracle import qseed as oq
    from oracle import writers as ow

    m, n, step = 2, 10007, 50
    data, munc = _bg_batch_fixture([n], m, 777, bg_amp=0.3)[0]
    # (1) the drop-in callable on the background-free matrix
    kw = dict(matrixData=data, matrixPluginMuncInit=munc, matrixF=np.asarray(cases.F_TREND, np.float32),
              matrixQ0=np.diag([1e-3, 1e-4]).astype(np.float32), intervalToBlockMap=(np.arange(n) // 100).astype(np.int32),
              blockCount=n // 100 + 1, stateInit=0.0, stateCovarInit=1000.0, ECM_fixedBackgroundIters=50,
              ECM_fixedBackgroundRtol=1e-6, pad=1e-4, ECM_robustTNu=8.0, procPrecisionMultiplierMin=5e-3,
              procPrecisionMultiplierMax=5e3, ECM_useObsPrecisionReweighting=False,
              ECM_useProcessPrecisionReweighting=True, t_innerIters=5, returnIntermediates=True,
              returnDiagnostics=True, logIterations=False)
    g, o = product.cfixedBackgroundECM(**kw), oracle.cfixedBackgroundECM(**kw)
    assert g[0] == o[0] and g[8]["converged"] == o[8]["converged"] and g[1] == pytest.approx(o[1], rel=1e-9)
    np.testing.assert_allclose(g[2], o[2], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(g[7], o[7], rtol=RTOL, atol=ATOL)
    # (2) the whole estimator, device-resident, with the CLI defaults
    mp = ModelParams(state_dim=2)
    pen = bgo.penalties(100, 128.0)
    cfg = FitConfig(penalties=pen, seed_q=True)
    with DeviceBatch(0, x_tol_ulps=0) as b:
        b.configure(mp, m, [n])
        b.upload(0, data, munc)
        fits, results = run_consenrich_batch(b, cfg, block_len_intervals=100)
        text_state = b.bedgraph_bytes(0, "xs", "chrPlumb", 1000, step, end_cap=1000 + step * n - 13, transform="round4")
        text_unc = b.bedgraph_bytes(0, "Ps", "chrPlumb", 1000, step, end_cap=1000 + step * n - 13, transform="sqrt")
    Q, _ = oq.estimate_initial_process_noise(oq, matrixData=data, matrixMunc=munc, pad=cfg.pad, stateModel="levelTrend",
                                             minQ=cfg.min_q, maxQ=cfg.max_q, deltaF=cfg.delta_f, robustTNu=cfg.nu)
    assert np.array_equal(fits[0].q0, Q)
    tw = _twin_cfg(mp, cfg, pen, Q0=Q)
    tw["block_len_intervals"] = 100
    ref = odrv.run_consenrich_chain(data, munc, tw)
    f = fits[0]
    assert f.passes == ref["passes"] and f.converged == ref["converged"] and f.ecm_iters == ref["ecm_iters"], (f, ref["passes"])
    worst = {}
    _check_run_result(results[0], ref, f, m, worst, "c1")
    _record_worst("c1_two_sample_plumbing_exact", worst)
    # (3) tracks on disk: byte-exact against the reference's writer (pandas to_csv, %.4f) on the returned tracks ...
    xs, Ps = results[0][0], results[0][1]
    starts = 1000 + np.arange(n, dtype=np.int64) * step
    ends = np.minimum(starts + step, 1000 + step * n - 13)
    assert text_state == ow.bedgraph_bytes("chrPlumb", starts, ends, np.round(xs[:, 0], 4))
    assert text_unc == ow.bedgraph_bytes("chrPlumb", starts, ends, np.sqrt(Ps[:, 0, 0]))
    # ... and against the bedGraph of the CPU twin's tracks: the files agree row for row except where a value sits within
    # the track tolerance of a %.4f rounding boundary
    ref_rows = ow.bedgraph_bytes("chrPlumb", starts, ends, np.round(ref["out_xs"][:, 0], 4)).split(b"\n")
    got_rows = text_state.split(b"\n")
    assert len(ref_rows) == len(got_rows) == n + 1
    assert sum(a != b_ for a, b_ in zip(got_rows, ref_rows)) <= max(1, n // 1000)


@pytest.mark.parametrize("xtol", [0, 2], ids=["exact", "ulp2"])
def test_config2_forward_only_step_matches_oracle(product, oracle, xtol):
    """BASELINE config 2 = `bench.py --config c2`: ONE chromosome of 1e6 bins x 4 samples, the forward filter alone
    (`cforwardPass` with store + NLL and no `cbackwardPass`, pyx:6393-6632) through `csr_batch_step_forward` on device-synthesised
    inputs (seed 1234): phiHat, NLL and every stored array against the oracle on the inputs read back; the one-call entry equals
    the separate stats / forward / export calls bit for bit; nothing of a smoother is exported."""
    from consenrich_amd import _lib as L
    from consenrich_amd.batch import DeviceBatch, ModelParams

    n, m = 1000000, 4
    F = np.asarray(cases.F_TREND, np.float32)
    Q0 = np.diag([1e-3, 1e-4]).astype(np.float32)
    with DeviceBatch(0, x_tol_ulps=xtol) as b:
        b.configure(ModelParams(state_dim=2), m, [n])
        if xtol:
            # (the 2-ulp mode's results depend on its windows within the acceptance, and windows lengthen themselves when a
            # validation pass finds many mismatches: pinned, so that two passes over the same inputs are the same computation)
            b.set_tuning(0, 96, 96, 64)
        b.synthesize(1234)
        sd, sn = b.step_forward(L.RETURN_NLL, L.EXPORT_FORWARD)
        got = {k: b.download(0, k) for k in ("xf", "Pf", "pnoise", "D")}
        with pytest.raises(L.ConsenrichAMDError, match="not exported"):
            b.download(0, "xs")
        data, munc = b.download_inputs(0)
        b.stats()
        sd2, sn2 = b.forward(L.RETURN_NLL)
        b.export(L.EXPORT_FORWARD)
        for k, v in got.items():
            assert np.array_equal(v, b.download(0, k)), k
        assert sd2[0] == sd[0] and sn2[0] == sn[0]
    xf, Pf, pn = np.zeros((n, 2), np.float32), np.zeros((n, 2, 2), np.float32), np.zeros((n, 2, 2), np.float32)
    D = np.zeros(n, np.float32)
    r = oracle.cforwardPass(matrixData=data, matrixPluginMuncInit=munc, matrixF=F, matrixQ0=Q0,
                            intervalToBlockMap=(np.arange(n) // 500).astype(np.int32), blockCount=(n + 499) // 500,
                            stateInit=0.0, stateCovarInit=1000.0, stateForward=xf, stateCovarForward=Pf, pNoiseForward=pn,
                            vectorD=D, returnNLL=True)
    assert sd[0] / n == pytest.approx(r[0], rel=1e-6) and sn[0] == pytest.approx(r[3], rel=1e-8 if xtol else 1e-11)
    lvl = np.maximum(np.abs(xf[:, :1].astype(np.float64)), 1.0)
    worst = {"xf_level_rel": float((np.abs(got["xf"].astype(np.float64) - xf)[:, 0] / lvl[:, 0]).max()),
             "xf_values_differing": float(np.count_nonzero(got["xf"] != xf)),
             "Pf_values_differing": float(np.count_nonzero(got["Pf"] != Pf))}
    assert np.all(np.abs(got["xf"].astype(np.float64) - xf) <= RTOL * lvl + ATOL)
    np.testing.assert_allclose(got["Pf"], Pf, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(got["pnoise"], pn[: n - 1], rtol=RTOL, atol=ATOL)
    if xtol == 0:
        np.testing.assert_allclose(got["D"], D, rtol=2e-5, atol=ATOL)
        assert worst["xf_level_rel"] == 0.0 and worst["xf_values_differing"] <= 2000
    else:
        # NIS amplifies ONE float32 ulp of the level by ~2 ulp(x0) / |zbar - x0|: with |level| up to ~30 on this 1e6-bin walk
        # and m = 4 that is ~1e-5 relative on a few per cent of the bins (measured 3.2 %), never beyond the conditioning bound
        worst["D_frac_outside_1e-5"] = float((np.abs(got["D"].astype(np.float64) - D) > RTOL * np.abs(D) + ATOL).mean())
        close_mostly(got["D"], D, frac=1e-1, cap=5e-4, msg="D")
        assert worst["xf_level_rel"] <= 2e-6
    _record_worst(f"c2_1e6_x4_forward_only_{'exact' if xtol == 0 else 'ulp2'}", worst)


def test_bench_workload_matches_oracle(product, oracle):
    """BASELINE config 4 = the exact workload bench.py times (its `throughput_mode` line) -- hg38 autosomes @200 bp x 32
    samples, device-synthesised inputs (seed 1234), csr_batch_step in the THROUGHPUT mode, `x_tol_ulps = 2` passed explicitly
    (the library default is the exact mode): NLL of every chromosome and every output array of ALL 22 chromosomes, first and
    second step of a batch.  The MEASURED worst errors are asserted (not only caps)."""
    ws = _genome_workload_against_oracle(oracle, 200, 32, full=range(22),
                                         variants=[dict(x_tol_ulps=2, steps=1), dict(x_tol_ulps=2, steps=2)])
    _record_worst("c4_hg38_200bp_x32_ulp2", ws[1])
    _record_worst("c4_hg38_200bp_x32_ulp2_first_step", ws[0])
    for w in ws:
        assert w["x_tol_ulps"] == 2 and w["chains_checked_in_full"] == 22
        assert w["nll_rel"] <= 1e-8 and w["phi_rel"] <= 1e-5
        assert w["xs_level_rel"] <= 2e-6 and w["xf_level_rel"] <= 2e-6          # measured 2.4e-7 .. 1e-6: <= 2 float32 ulps
        assert w["xs_trend_vs_level"] <= 2e-6 and w["xf_trend_vs_level"] <= 2e-6
        assert w["D_frac_outside_1e-5"] <= 1e-2 and w["D_rel_max"] <= 5e-4       # NIS amplifies one ulp of the level
        assert w["xf_values_differing"] > 0         # 2-ulp data under the 2-ulp label (the exact mode differs in ~0 values)


def test_bench_workload_exact_mode_matches_oracle(product, oracle):
    """Same workload in the DEFAULT bit-exact validation mode (k = 0: `value` of the bench line, the mode the drop-in
    callables run in): every gate at the north_star tolerance with NO conditioning-aware relaxation -- NIS included -- on
    every output array of ALL 22 chromosomes (the step pipelines its tail per GROUP of chains: a chain outside the checked set
    is a chain whose group is not checked), for the FIRST step of a fresh batch (the step that allocates and zeroes the
    reference-layout arrays) and for the second.
    Third variant: the first step of a fresh batch under CONSENRICH_AMD_TAIL_PCT=5,5 and CONSENRICH_AMD_SB_BINS=4096 -- many
    small tail groups following each other closely, the schedule under which round 4's first-use zeroing (queued on a group's
    stream) wiped the residuals the next group had written.  nat_array now zeroes on a stream of its own and waits for it
    before handing the array out; `nat_first_use_off_main` shows that first uses DO happen inside tail groups here."""
    env = {"CONSENRICH_AMD_TAIL_PCT": "5,5", "CONSENRICH_AMD_SB_BINS": "4096"}
    ws = _genome_workload_against_oracle(oracle, 200, 32, full=range(22),
                                         variants=[dict(x_tol_ulps=0, steps=1), dict(x_tol_ulps=0, steps=2),
                                                   dict(x_tol_ulps=0, steps=1, env=env)])
    _record_worst("c4_hg38_200bp_x32_exact", ws[1])
    _record_worst("c4_hg38_200bp_x32_exact_first_step", ws[0])
    _record_worst("c4_hg38_200bp_x32_exact_first_step_small_groups", ws[2])
    for w in ws:
        assert w["x_tol_ulps"] == 0 and w["chains_checked_in_full"] == 22
        assert w["nll_rel"] <= 1e-11 and w["phi_rel"] <= 1e-6
        assert w["xs_level_rel"] <= 2.5e-7 and w["xs_trend_vs_level"] <= 2.5e-7
        assert w["D_frac_outside_1e-5"] <= 1e-5 and w["D_rel_max"] <= 2e-5
        # stored float32 values that are not the oracle's, of 2.9e7 per array (measured round 5: xf 808, xs 782, ALL of them
        # trend components, off by one ulp of the trend = 1.4e-7 of the trend track's RMS = 2.6e-11 of the level: a handful of
        # flipped roundings of the weakly observed trend, each persisting for a few hundred bins until the trajectories
        # merge again; no level, Pf, D or residual value differs.  The 2-ulp mode differs in half of the values.)
        assert w["xf_values_differing"] <= 5000 and w["xf_level_rel"] == 0.0 and w["resid_rel"] <= 1e-9
    if _default_switches():
        assert ws[0]["tail_groups"] >= 1, ws
        # HOW MANY groups the host launches while the state chain runs -- and with them whether a first use of a reference-layout
        # array falls inside a group -- depends on the host thread's timing in the parity runs above.  One more first step of a fresh
        # batch of the same workload under the same switches (no oracle pass) with the grouping SCRIPTED (csr_batch_set_step_groups):
        # the three shortest chromosomes as tail groups 0, 1, 2 and the remainder -- four groups whatever the timing, and the first
        # of them, on the tail stream, is where xs / Ps / lag / resid are first used
        from consenrich_amd import _lib as L
        from consenrich_amd.batch import DeviceBatch, ModelParams
        from consenrich_amd.sharding import hg38_chain_lengths

        saved = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            with DeviceBatch(0, x_tol_ulps=0) as b:
                b.configure(ModelParams(state_dim=2), 32, hg38_chain_lengths(200))
                b.synthesize(1234)
                b.set_step_groups([{21: 0, 20: 1, 19: 2}.get(c, -1) for c in range(22)], None)
                b.step(L.RETURN_NLL, L.EXPORT_FORWARD | L.EXPORT_SMOOTH | L.EXPORT_RESID)
                rs = b.run_stats()
        finally:
            for k, v in saved.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
        assert rs["tail_groups"] == 4 and rs["nat_first_use_off_main"] >= 1, rs


def test_config5_hg38_50bp_x64_matches_oracle(product, oracle):
    """BASELINE config 5: hg38 autosomes @50 bp (57 500 042 bins) x 64 samples in ONE batch on one MI355X (29 GB of inputs),
    throughput mode AND default bit-exact mode (a second batch, same oracle passes): phiHat and NLL of every chromosome against the oracle, every output array of the two shortest
    chromosomes (chr21, chr22: ~1 M bins each) AND of chr1 (4 979 129 bins, ~200 superblocks: the longest critical path of the
    state chain and the likeliest place for one of its bounded waits to run out -- `state_chain_bailouts` must stay 0).  MFMA
    eligibility of the m = 64 observation update: none -- it is a length-m weighted reduction per bin (pyx:443-456), no dense
    contraction; the bound is HBM."""
    w, we = _genome_workload_against_oracle(oracle, 50, 64, full=(0, 20, 21),
                                            variants=[dict(x_tol_ulps=2), dict(x_tol_ulps=0)])
    _record_worst("c5_hg38_50bp_x64_ulp2", w)
    assert w["chains_checked_in_full"] == 3 and we["chains_checked_in_full"] == 3
    assert (w["state_chain_bailouts"] == 0 and we["state_chain_bailouts"] == 0) or not _default_switches()      # (the suite also runs with bail-outs forced)
    assert w["nll_rel"] <= 1e-8 and w["phi_rel"] <= 1e-5
    assert w["xs_level_rel"] <= 2e-6 and w["xs_trend_vs_level"] <= 2e-6
    # (NIS amplifies one ulp of the level by ~2 ulp / |zbar - x|: on chr1 -- 5 M bins of a random walk, |level| up to ~60 -- it is
    # outside 1e-5 on 2.6 % of the bins, never by more than 1.2e-4; on chr21 / chr22 alone, round 5: 0.07 %)
    assert w["D_frac_outside_1e-5"] <= 5e-2 and w["D_rel_max"] <= 5e-4
    # the same batch in the DEFAULT (bit-exact) mode against the same oracle passes: the gates of the config-4 exact test
    _record_worst("c5_hg38_50bp_x64_exact", we)
    # (NLL: per-bin terms of both signs, 5 M of them in chr1 at 50 bp: the fp64 sum's order shows at 5e-10 relative; the stop rule
    # of the ECM loop works at 1e-6)
    assert we["nll_rel"] <= 2e-9 and we["phi_rel"] <= 1e-6
    assert we["xs_level_rel"] <= 2.5e-7 and we["xs_trend_vs_level"] <= 2.5e-7
    # Round 6, with chr1 in the checked set: on chr21 / chr22 alone the default mode differed from the oracle in 335 values and
    # NIS nowhere (round 5); on chr1 -- 5 M bins; the synthetic level drifts to -880 and passes through [256, 512) -- 1.1 M of its
    # 10 M filtered-state values are ONE float32 ulp off (1.2e-7 relative) and NIS is outside 1e-5 on 0.42 % of its bins (never by
    # more than 1e-4).  In that window one ulp of the level is the size of the trend's increments and the float32-rounded
    # recursion keeps two implementations that agree to 1e-16 per operation apart at the ulp scale (scripts/ubench/flip_regime.c
    # shows the same window with plain C on the CPU; scripts/exact_vs_seq_probe.py: the library equals its own sequential kernel
    # bit for bit on that chain).  Every array is still two orders inside 1e-5.  DESIGN section 7, finding 3.
    assert we["D_frac_outside_1e-5"] <= 1e-2 and we["D_rel_max"] <= 5e-4
    assert we["xf_values_differing"] < 0.25 * w["xf_values_differing"]        # (the 2-ulp mode differs in half of the values)


@pytest.mark.parametrize("xtol", [0, 2], ids=["exact", "ulp2"])
@pytest.mark.parametrize("flags_name", ["plain", "kappa", "all"])
@pytest.mark.parametrize("block_len", [32, 64, 128])
def test_lds_dma_paths_agree_with_the_plain_kernels(product, block_len, flags_name, xtol):
    """The LDS-DMA ring only changes HOW a chain's inputs reach the recursion (global_load_lds + counted waits instead of
    register prefetch).  In exact mode the results do not depend on the speculation at all: every output must equal the
    plain kernels' bit for bit (smoother warm-up hybrid, state-chain ring).  In the 2-ulp mode a lane whose chain starts
    inside its window begins at the window's edge through the ring and at the chain start in the plain kernel -- two
    valid speculations -- so the outputs agree to the mode's tolerance.  Ragged chains (partial blocks, chain starts /
    ends inside warm-up windows, one-bin chains), constant and per-bin multipliers, forward with reference-layout outputs
    (warm-up hybrid) and ECM sweeps (whole walk through the ring)."""
    from consenrich_amd import _lib as L
    from consenrich_amd.batch import DeviceBatch, ModelParams

    rng = np.random.default_rng(77 + block_len)
    n_list = [int(v) for v in np.concatenate([[1, 2, 31, 33, 63, 65, 127, 129, 300], rng.integers(1, 4000, 40)])]
    m = 3
    sets = [cases.synth(n, m, 9100 + i, mask_frac=0.02) for i, n in enumerate(n_list)]
    mult = {c: (np.exp(rng.normal(0, 0.3, n)).astype(np.float32), np.exp(rng.normal(0, 1.0, n)).astype(np.float32),
                np.exp(rng.normal(0, 0.2, n)).astype(np.float32)) for c, n in enumerate(n_list)}
    flags = {"plain": 0, "kappa": L.USE_KAPPA, "all": L.USE_KAPPA | L.USE_LAMBDA | L.USE_QSCALE}[flags_name]
    what = L.EXPORT_FORWARD | L.EXPORT_SMOOTH | L.EXPORT_RESID

    def run(dma):
        env = {"CONSENRICH_AMD_DMA": "1" if dma else "0"}
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            with DeviceBatch(0, block_len=block_len, x_tol_ulps=xtol) as b:     # switches are read at context creation
                b.configure(ModelParams(state_dim=2), m, n_list)
                for c, (d_, v_) in enumerate(sets):
                    b.upload(c, d_, v_)
                    if flags:
                        b.upload_multipliers(c, *mult[c])
                b.stats()
                sd, sn = b.forward_backward(L.RETURN_NLL | flags)                  # reference-layout outputs: warm-up hybrid
                b.export(what)
                out = {(c, k): b.download(c, k) for c in range(len(n_list)) for k in ("D", "xf", "Pf", "xs", "Ps", "lag", "resid")}
                outs, _ = b.ecm(max_iters=2, inner_iters=2, rtol=0.0, use_lambda=bool(flags & L.USE_LAMBDA), use_kappa=True)
                b.export(L.EXPORT_SMOOTH | L.EXPORT_MULT)                           # ECM sweeps: whole walk through the ring
                for c in range(len(n_list)):
                    out[(c, "ecm_xs")] = b.download(c, "xs")
                    out[(c, "ecm_kappa")] = b.download(c, "kappa")
                return sn.copy(), np.asarray([o.final_nll for o in outs]), out
        finally:
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v

    sn_a, nll_a, out_a = run(True)
    sn_b, nll_b, out_b = run(False)
    if xtol == 0:
        assert np.array_equal(sn_a, sn_b) and np.array_equal(nll_a, nll_b)
        for key in out_a:
            assert np.array_equal(out_a[key], out_b[key], equal_nan=True), key
        return
    np.testing.assert_allclose(sn_a, sn_b, rtol=1e-7)
    np.testing.assert_allclose(nll_a, nll_b, rtol=1e-6)
    for (c, k), a in out_a.items():
        b_ = out_b[(c, k)]
        if k in ("D", "ecm_kappa"):
            close_mostly(a, b_, frac=2e-2, cap=5e-2, msg=f"{k} chain {c}")
        elif k in ("xf", "xs", "ecm_xs", "resid"):
            lvl = np.maximum(np.abs(out_b[(c, "xs" if k != "ecm_xs" else "ecm_xs")][:, :1].astype(np.float64)), 1.0)
            assert np.all(np.abs(a.astype(np.float64) - b_) <= 2 * RTOL * lvl + ATOL), (c, k)
        else:
            np.testing.assert_allclose(a, b_, rtol=2 * RTOL, atol=ATOL, err_msg=f"{k} chain {c}")


def test_bench_line_contract(product):
    """bench.py --full prints ONE JSON line with the driver's contract fields plus the roofline object (2 steps, no extras)."""
    import json
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "2", "--warmup", "1", "--full",
                        "--no-cpu-baseline", "--no-extras"], capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.strip().splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline"):
        assert key in d, key
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1 and d["higher_is_better"] is True
    assert d["vs_baseline"] is None and d["data"] == "synthetic" and "workload" in d["config"] and "model" not in d["config"]
    assert d["value"] == pytest.approx(14375018 / (d["ms_per_step"] * 1e-3), rel=1e-6)
    rf = d["roofline"]
    assert rf["bound"] == "hbm" and rf["unit"] == "GB/s" and rf["peak"] == 8000.0
    assert rf["frac"] == pytest.approx(rf["achieved"] / rf["peak"]) and 0.0 < rf["frac"] < 1.0
    # the headline is measured in the library's default mode, which is the bit-exact one; the line says which build ran
    assert d["config"]["x_tol_ulps"] == 0 and d["config"]["n_ranks_seen"] == 1
    assert d["build"].startswith("abi ") and " src " in d["build"]
    rs = d["roofline_streaming"]
    assert rs["kernel"] in ("stats", "residuals") and 0.2 < rs["frac"] < 1.0


def test_plain_bench_times_k_steps_and_dumps_what_the_last_one_returned(product, tmp_path):
    """A plain bench.py run times one window of exactly K steps and measures nothing beside the headline; --dump-outputs
    writes the last step's returns as float .npy files (a fixed sample of the per-bin arrays, within 64 MB), and a second
    run with the same arguments writes the same values."""
    import json
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lines = {}
    for tag in ("a", "b"):
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                            "--dump-outputs", str(tmp_path / tag)], capture_output=True, text=True, timeout=600, cwd=root)
        assert r.returncode == 0, r.stderr[-2000:]
        out = [ln for ln in r.stdout.strip().splitlines() if ln.strip()]
        assert len(out) == 1, out
        lines[tag] = json.loads(out[0])
    d = lines["a"]
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in d, key
    assert d["steps"] == 3 and d["warmup"] == 1 and d["timed_windows"] == 1 and d["full"] is False
    assert d["value"] == pytest.approx(14375018 / (d["ms_per_step"] * 1e-3), rel=1e-6)
    for key in ("roofline", "kernels_rank0", "cpu_baseline", "throughput_mode", "ecm", "with_calibration_folds"):
        assert key not in d, key
    names = {"D", "xf", "Pf", "pnoise", "xs", "Ps", "lag", "resid", "sumD", "sumNLL"}
    assert set(d["dumped_outputs"]) == names
    assert {f for f in os.listdir(tmp_path / "a")} == {n + ".npy" for n in names}
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 64 * 2**20
    for n in sorted(names):
        a, b = np.load(tmp_path / "a" / f"{n}.npy"), np.load(tmp_path / "b" / f"{n}.npy")
        assert a.dtype in (np.float32, np.float64) and a.shape == b.shape and a.size > 0, n
        assert np.all(np.isfinite(a)), n
        if n in ("sumD", "sumNLL"):
            assert a.shape == (22,), n
            np.testing.assert_allclose(a, b, rtol=1e-12, atol=0.0, err_msg=n)
        else:
            assert np.array_equal(a, b), n
    assert np.load(tmp_path / "a" / "resid.npy").shape[1:] == (32,)


def test_bench_started_plainly_with_two_ranks_on_one_gpu(product):
    """`python bench.py --gpus 2` started plainly (no launcher): the parent spawns its two rank processes, which shard the
    genome and meet through the job's directory; --same-device puts both on GPU 0 (RCCL refuses two ranks on one device, so the
    barrier is the file one).  One line from rank 0, n_ranks_seen = 2, exit status 0."""
    import json
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--same-device", "--steps", "2", "--warmup",
                        "1", "--full", "--no-cpu-baseline", "--no-extras"], capture_output=True, text=True, timeout=900, cwd=root,
                       env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.strip().splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["n_ranks_seen"] == 2 and d["config"]["comm"] == "file"
    assert d["value"] == pytest.approx(14375018 / (d["ms_per_step"] * 1e-3), rel=1e-6)
    # what a measured N > 1 line is read against: the model's speed-ups for this job's LPT table and the measured / modelled ratio
    assert d["expected"]["default"]["speedup_vs_1gpu"] > 1.0 and d["expected"]["ulp2"]["speedup_vs_1gpu"] > 1.5
    assert d["speedup_vs_expected"] == pytest.approx(d["expected"]["default"]["ms_per_step"] / d["ms_per_step"], rel=1e-9)

