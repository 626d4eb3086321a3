"""GPU tests (run with -m gpu) of the default-mode step whose NIS / NLL epilogue runs in groups of its own on the side stream while
the state chain is still running (step_pipelined, csr_host_pipeline.inl): `k_fwd_dstat<natXf>` reads the previous filtered state
where the state chain wrote it (no blocked copy of xf), and a tail group's residuals are ONE launch over a table of runs
(`k_resid_runs`, `k_resid_v4_runs`).  Same arithmetic in the same order: every output equals, bit for bit, the step in order
(CONSENRICH_AMD_TAIL_SPLIT=0).

Small shapes on purpose: chains shorter than, equal to and just past one block of every block length, a chain of one bin, chains of
several superblocks (CONSENRICH_AMD_SB_BINS=4096); m = 4 takes the 16-byte residual kernel, m = 5 the plain one.

The smoother's speculation window is pinned at 384 bins (CONSENRICH_AMD_WARM=-1,-1,384).  With one constant process noise the
default 128 bins do not validate bit for bit on this data at any of the three block lengths -- the step in order of the commit
before this one re-runs 2 to 72 smoother blocks in its first step, widens the window to 192 / 384 bins and replays the pipeline
once (pipeline_redos = 1), after which the second step validates.  A replayed step's outputs come from the in-order kernels of
settle(), so such a first step would compare nothing of the pipelined path; at 384 bins both steps validate and both are compared
with `pipeline_redos == 0`."""
import os

import numpy as np
import pytest

from conftest import gpu_available
from tail_cases import N_LIST, OWN, assert_same as _assert_same, bits as _bits, make_inputs, pipelines as _pipelines, run as _run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def product():
    if not gpu_available():
        pytest.fail("GPU tests selected but no HIP device / library: the product has no CPU fallback")
    from consenrich_amd import cconsenrich

    return cconsenrich


@pytest.fixture(scope="module")
def inputs():
    return make_inputs()


@pytest.mark.parametrize("variant", ["plain", "multipliers", "nll_in_d", "per_chain_q"])
@pytest.mark.parametrize("block", [64, 128, 256])
@pytest.mark.parametrize("m", [4, 5])
def test_epilogue_groups_and_table_residuals_equal_the_step_in_order_and_the_old_tails(product, monkeypatch, inputs, m, block, variant):
    """D, xf, Pf, pNoise, xs, Ps, lag, resid, sumD and sumNLL of the first and of the second step of a fresh batch, bit for bit:
    the default step (tail thresholds unset, and at 1 % so that nearly every finished chain is a group) against the step in
    order; no replay and no bail-out in any of them.  Then with a wait bound of one poll (CONSENRICH_AMD_SB_SPIN_LIMIT=1): the
    single launch gives up under the groups in flight, everything is redone behind the pass form, and the outputs equal the step
    in order."""
    in_order = _run(monkeypatch, inputs, {"CONSENRICH_AMD_TAIL_SPLIT": "0"}, m, block, variant)
    assert in_order["stats"]["tail_groups"] == 0
    assert in_order["stats"]["pipeline_redos"] == 0 and in_order["stats"]["sb_bailouts"] == 0, in_order["stats"]
    for env in ({}, {"CONSENRICH_AMD_TAIL_PCT": "1,1"}, {"CONSENRICH_AMD_TAIL_PCT": "1,1", "CONSENRICH_AMD_EPILOGUE_PCT": "1"}):
        got = _run(monkeypatch, inputs, env, m, block, variant)
        print(m, block, variant, env, got["stats"])
        assert got["stats"]["pipeline_redos"] == 0 and got["stats"]["sb_bailouts"] == 0, (env, got["stats"])
        if _pipelines():
            assert got["stats"]["tail_groups"] >= 2, (env, got["stats"])        # two steps, at least one group each
        _assert_same(got, in_order, (env, "against the step in order"))
    bail = _run(monkeypatch, inputs, {"CONSENRICH_AMD_TAIL_PCT": "1,1", "CONSENRICH_AMD_EPILOGUE_PCT": "1", "CONSENRICH_AMD_SB_SPIN_LIMIT": "1"},
                m, block, variant)
    print(m, block, variant, "bail-out", bail["stats"])
    if _pipelines():
        assert bail["stats"]["sb_bailouts"] >= 1, bail["stats"]
    _assert_same(bail, in_order, "forced bail-out against the step in order")


@pytest.mark.parametrize("m", [4, 5])
def test_a_pipelined_step_launches_no_blocked_copy_of_xf_and_one_residual_kernel_per_group(product, monkeypatch, inputs, m):
    """One constant process noise: the smoother of every tail group reads the reference layout, so nothing of the step reads a
    blocked xf -- no `state_reblock_out` launch; the residuals are one launch per tail group; the epilogue ran at least once per
    step."""
    if not _pipelines() or os.environ.get("CONSENRICH_AMD_NATIN", "1") == "0":
        return      # (a mode switch of the whole suite: the step does not pipeline, or its smoother reads blocks)
    new = _run(monkeypatch, inputs, {"CONSENRICH_AMD_TAIL_PCT": "1,1", "CONSENRICH_AMD_EPILOGUE_PCT": "1"}, m, 128, "plain", profile=True)
    print(new["launches"], new["stats"])
    assert new["launches"].get("state_reblock_out", 0) == 0, new["launches"]
    assert new["launches"]["residuals"] == new["stats"]["tail_groups"], (new["launches"], new["stats"])
    assert new["launches"]["fwd_dstat"] >= 2, new["launches"]


@pytest.mark.parametrize("block", [64, 128, 256])
def test_a_masked_forward_pass_after_such_a_step_leaves_the_other_chains_as_they_were(product, monkeypatch, inputs, block):
    """After a pipelined step with one constant process noise the blocked xf is not resident (csr_ctx::where[] says so).  A masked
    forward pass on one chain rewrites the blocked copies of ITS blocks: the other chains' blocks come back from the reference
    layout first (need_blocked), so xf / D of another chain are unchanged -- as downloaded at once and, for xf / Pf and the
    smoothed arrays, after a smoother pass and a new export of every chain."""
    from consenrich_amd import _lib as L
    from consenrich_amd.batch import DeviceBatch, ModelParams

    sets, _ = inputs
    for k in OWN:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("CONSENRICH_AMD_BLOCK", str(block))
    monkeypatch.setenv("CONSENRICH_AMD_SB_BINS", "4096")
    monkeypatch.setenv("CONSENRICH_AMD_WARM", "-1,-1,384")
    m = 4
    what = L.EXPORT_FORWARD | L.EXPORT_SMOOTH | L.EXPORT_RESID
    mask = [c == 9 for c in range(len(N_LIST))]         # the chain of 8193 bins
    with DeviceBatch(0) as b:
        b.configure(ModelParams(state_dim=2), m, N_LIST)
        for c, (d_, v_) in enumerate(sets[m]):
            b.upload(c, d_, v_)
        b.step(L.RETURN_NLL, what)
        before = {(c, a): b.download(c, a) for c in range(len(N_LIST)) for a in ("D", "xf", "Pf", "xs", "Ps", "lag")}
        b.forward_masked(L.RETURN_NLL, mask)
        for c in (8, 10, 0):
            for a in ("xf", "D"):
                assert np.array_equal(_bits(before[(c, a)]), _bits(b.download(c, a))), (block, c, a)
        b.backward()
        b.export(L.EXPORT_FORWARD | L.EXPORT_SMOOTH)
        for c in range(len(N_LIST)):
            for a in ("xf", "Pf", "xs", "Ps", "lag"):
                assert np.array_equal(_bits(before[(c, a)]), _bits(b.download(c, a))), (block, "after the smoother", c, a)
