"""GPU tests (run with -m gpu) of the pipelined step (step_pipelined, csr_host_pipeline.inl) under SCRIPTED groupings of its
chains (csr_batch_set_step_groups / DeviceBatch.set_step_groups).  Which chains share a tail group or an NIS / NLL epilogue
group is otherwise decided by the host's clock, and at the small shapes where a comparison bit for bit is cheap the state chain
may well end before the first poll: no early group, one remainder of everything, and none of the code that only a grouping
selects runs -- `chain_runs` with several runs, `group_span` over blocks of chains outside the group, the bisection of the
run-table residual kernels, a mask that trims a span, the mask / run-table slots past the first, a chain whose epilogue is early
and whose tail is not.  A script fixes the grouping (not whether a group overlaps the running state chain: that stays with the
full-size test, tests/test_gpu_parity.py); the cases below walk those edges.

Shapes and set-up are those of tests/test_gpu_tail_epilogue.py (tests/tail_cases.py): 11 chains of 1 to 20000 bins, 4096-bin
superblocks, the smoother's window pinned at 384 bins so that both steps of a fresh batch validate, m = 4 (16-byte residual
kernel) and m = 5 (plain one).  Every case compares D, xf, Pf, pnoise, xs, Ps, lag, resid, sumD and sumNLL of both steps with the
step in order (CONSENRICH_AMD_TAIL_SPLIT=0), bit for bit; the step in order of a (m, block, variant) is computed once per module."""
import os

import numpy as np
import pytest

import cases
from conftest import gpu_available
from tail_cases import N_LIST, WARM, assert_same, bits, fill, make_inputs, pipelines, run, set_env

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1.0e-5, 2.0e-6         # tests/test_gpu_parity.py
NC = len(N_LIST)


def _groups(*sets):
    """Per chain the index of the set that holds it, -1 where none does."""
    g = [-1] * NC
    for k, chains in enumerate(sets):
        for c in chains:
            assert g[c] == -1
            g[c] = k
    return g


# script -> (tail group per chain, epilogue group per chain); None = that kind is left to the host's clock
SCRIPTS = {
    # the caps: six tail groups, eight epilogue groups -- every mask / run-table slot, the remainder's included
    "singletons": (_groups([10], [9], [8], [7], [6], [5]), _groups(*[[c] for c in range(8)])),
    # {0, 5, 10}: three runs, a span over the whole batch; {2, 3}: two adjacent chains, one run; {1}
    "scattered": (_groups([0, 5, 10], [2, 3], [1]), _groups([1, 3, 5, 7, 9], [0])),
    "all_early": (_groups(range(NC)), _groups(range(NC))),          # the remainder is empty: `rest` launches nothing
    "none": (_groups(), _groups()),
    "crossed": (_groups(range(0, 6)), _groups(range(6, NC))),       # a chain's epilogue is early and its tail is not, and the reverse
    "one_bin_alone": (_groups([0], [10]), None),                    # a run of 64 padded bins that hold one
}


def _expected_groups(script):
    """Groups per step of each kind: the scripted ones and the remainder unless it is empty (None: unscripted)."""
    return [None if g is None else max(g) + 1 + (1 if -1 in g else 0) for g in script]


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
def inputs():
    return make_inputs()


@pytest.fixture(scope="module")
def in_order(inputs):
    """The step in order of (m, block, variant, window): two steps of a fresh batch, computed at first use, never changed."""
    cache = {}

    def get(m, block, variant, warm=WARM):
        key = (m, block, variant, warm)
        if key not in cache:
            with pytest.MonkeyPatch.context() as mp:
                ref = run(mp, inputs, {"CONSENRICH_AMD_TAIL_SPLIT": "0"}, m, block, variant, warm=warm)
            assert ref["stats"]["tail_groups"] == 0 and ref["stats"]["sb_bailouts"] == 0, ref["stats"]
            if warm == WARM:
                assert ref["stats"]["pipeline_redos"] == 0, ref["stats"]
            for v in ref.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
            cache[key] = ref
        return cache[key]

    return get


def _natin():
    return os.environ.get("CONSENRICH_AMD_NATIN", "1") != "0"


def _check_script(monkeypatch, inputs, in_order, name, m, block, variant):
    """Two scripted steps of a fresh batch against the step in order, bit for bit; no replay, no bail-out; the number of groups of
    each kind is the script's, in both steps (profiled launch census at block 128)."""
    script = SCRIPTS[name]
    ref = in_order(m, block, variant)
    got = run(monkeypatch, inputs, {}, m, block, variant, profile=block == 128, script=script)
    print(name, m, block, variant, got["stats"], got.get("launches"))
    assert got["stats"]["pipeline_redos"] == 0 and got["stats"]["sb_bailouts"] == 0, got["stats"]
    assert_same(got, ref, (name, "against the step in order"))
    if not pipelines():
        return got
    tails, epis = _expected_groups(script)
    assert got["stats"]["tail_groups"] == 2 * tails, (name, got["stats"])
    if block == 128:
        launches = got["launches"]
        assert launches["residuals"] == got["stats"]["tail_groups"], (launches, got["stats"])
        if epis is not None:
            assert launches["fwd_dstat"] == 2 * epis, (name, launches)
        else:
            assert launches["fwd_dstat"] >= 2, (name, launches)
        if variant == "plain" and _natin():
            assert launches.get("state_reblock_out", 0) == 0, launches
    return got


@pytest.mark.parametrize("variant", ["plain", "multipliers", "nll_in_d", "per_chain_q"])
@pytest.mark.parametrize("block", [64, 128, 256])
@pytest.mark.parametrize("m", [4, 5])
def test_scattered_groups_equal_the_step_in_order(product, monkeypatch, inputs, in_order, m, block, variant):
    """Tail groups {0, 5, 10} (three runs: the residual kernel's bisection over a table of three, a span of wavefront-groups over the
    whole batch that the mask trims), {2, 3} (one run of two chains), {1}, remainder {4, 6, 7, 8, 9}; epilogue groups {1, 3, 5, 7, 9},
    {0} and the rest.  With multipliers / per-chain Q the smoother reads blocks: `group_span` decides which get a blocked xf."""
    _check_script(monkeypatch, inputs, in_order, "scattered", m, block, variant)


@pytest.mark.parametrize("variant", ["plain", "multipliers"])
@pytest.mark.parametrize("m", [4, 5])
@pytest.mark.parametrize("name", ["singletons", "all_early", "none", "crossed", "one_bin_alone"])
def test_scripted_groups_equal_the_step_in_order(product, monkeypatch, inputs, in_order, name, m, variant):
    """The caps (six tail groups, eight epilogue groups: every slot), everything in one early group (nothing remains), nothing early,
    tails and epilogues of a chain in groups of different kinds, and a tail group that is one bin."""
    _check_script(monkeypatch, inputs, in_order, name, m, 128, variant)


@pytest.mark.parametrize("m", [4, 5])
def test_scattered_groups_match_the_oracle(product, oracle, monkeypatch, inputs, m):
    """Against a reference that shares no code with the step (a bug that the step in order shares does not hide there): every chain
    of both scripted steps against the oracle's cforwardPass + cbackwardPass at the parity tolerance, sumNLL to 1e-9."""
    sets, _ = inputs
    got = run(monkeypatch, inputs, {}, m, 128, "plain", script=SCRIPTS["scattered"])
    assert got["stats"]["pipeline_redos"] == 0 and got["stats"]["sb_bailouts"] == 0, got["stats"]
    if pipelines():
        assert got["stats"]["tail_groups"] == 8, got["stats"]
    F = np.asarray(cases.F_TREND, np.float32)
    Q0 = np.diag([1e-3, 1e-4]).astype(np.float32)
    for c, n in enumerate(N_LIST):
        d_, v_ = sets[m][c]
        xf, Pf, pn = np.zeros((n, 2), np.float32), np.zeros((n, 2, 2), np.float32), np.zeros((n, 2, 2), np.float32)
        D = np.zeros(n, np.float32)
        r = oracle.cforwardPass(matrixData=d_, matrixPluginMuncInit=v_, matrixF=F, matrixQ0=Q0, intervalToBlockMap=np.zeros(n, np.int32),
                                blockCount=1, stateInit=0.0, stateCovarInit=1000.0, stateForward=xf, stateCovarForward=Pf,
                                pNoiseForward=pn, vectorD=D, returnNLL=True)
        bw = oracle.cbackwardPass(matrixData=d_, matrixF=F, stateForward=xf, stateCovarForward=Pf, pNoiseForward=pn)
        for step in range(2):
            assert got[("sumNLL", step)][c] == pytest.approx(r[3], rel=1e-9, abs=1e-9), (c, step)
            for name, ref in (("D", D), ("xf", xf), ("Pf", Pf), ("pnoise", pn[: n - 1]), ("xs", bw[0]), ("Ps", bw[1]),
                              ("lag", bw[2][: n - 1]), ("resid", bw[3])):
                np.testing.assert_allclose(got[(c, name, step)], ref, rtol=RTOL, atol=ATOL, err_msg=f"chain {c} {name} step {step}")


@pytest.mark.parametrize("variant", ["plain", "multipliers"])
@pytest.mark.parametrize("m", [4, 5])
def test_a_bail_out_under_a_script_redoes_everything_in_one_remainder(product, monkeypatch, inputs, in_order, m, variant):
    """A wait bound of one poll (CONSENRICH_AMD_SB_SPIN_LIMIT=1, the bounded bail-out of the single launch): whatever scripted groups
    went out are redone behind the pass form, none goes out after it, and the outputs equal the step in order."""
    bail = run(monkeypatch, inputs, {"CONSENRICH_AMD_SB_SPIN_LIMIT": "1"}, m, 128, variant, script=SCRIPTS["scattered"])
    print(m, variant, "bail-out", bail["stats"])
    if pipelines():
        assert bail["stats"]["sb_bailouts"] >= 1, bail["stats"]
    assert_same(bail, in_order(m, 128, variant), "scripted groups, forced bail-out, against the step in order")


@pytest.mark.parametrize("m", [4, 5])
def test_a_replayed_step_under_a_script_equals_the_step_in_order(product, monkeypatch, inputs, in_order, m):
    """The smoother's window at its default: the first step's optimistic validation fails (tests/test_gpu_tail_epilogue.py's
    docstring), the window widens and settle() replays the pipeline once, over every chain whatever the groups were; the second
    step validates under the script.  Same switches in order: the same bits and as many replays."""
    default_window = "CONSENRICH_AMD_WARM" not in os.environ        # (a mode switch of the whole suite may pin another one)
    ref = in_order(m, 128, "plain", warm=None)
    got = run(monkeypatch, inputs, {}, m, 128, "plain", script=SCRIPTS["scattered"], warm=None)
    print(m, "default window", got["stats"], ref["stats"])
    assert got["stats"]["sb_bailouts"] == 0, got["stats"]
    assert_same(got, ref, "scripted groups, default smoother window, against the step in order")
    assert got["stats"]["pipeline_redos"] == ref["stats"]["pipeline_redos"], (got["stats"], ref["stats"])
    if pipelines() and default_window:
        assert got["stats"]["pipeline_redos"] >= 1, got["stats"]
        assert got["stats"]["tail_groups"] == 8, got["stats"]


def test_a_script_lasts_until_it_is_cleared_or_the_batch_is_configured_again(product, monkeypatch, inputs, in_order):
    """The script belongs to the batch: it holds for every step until set_step_groups(None, None) or configure; a rejected script
    (ValueError, a text of its own) leaves the previous one in force.  CONSENRICH_AMD_TAIL_PCT=100,100: an unscripted step hands
    every chain out as ONE group whatever the timing, so the increments of `tail_groups` tell which grouping a step ran under."""
    from consenrich_amd import _lib as L
    from consenrich_amd.batch import DeviceBatch

    m, block = 4, 128
    tails, epis = SCRIPTS["scattered"]
    set_env(monkeypatch, {"CONSENRICH_AMD_TAIL_PCT": "100,100"}, block)
    what = L.EXPORT_FORWARD | L.EXPORT_SMOOTH | L.EXPORT_RESID
    ref = in_order(m, block, "plain")
    seen = []

    def step(b):
        before = b.run_stats()["tail_groups"]
        sd, sn = b.step(L.RETURN_NLL, what)
        assert np.array_equal(bits(np.array(sn)), bits(ref[("sumNLL", 0)])) and np.array_equal(bits(np.array(sd)), bits(ref[("sumD", 0)]))
        for c in (0, 5, 10, 4):
            for a in ("xs", "resid", "D"):
                assert np.array_equal(bits(b.download(c, a)), bits(ref[(c, a, 0)])), (len(seen), c, a)
        seen.append(b.run_stats()["tail_groups"] - before)
        return seen[-1]

    scripted, unscripted = (4, 1) if pipelines() else (0, 0)
    with DeviceBatch(0) as b:
        fill(b, inputs, m, "plain")
        assert step(b) == unscripted
        b.set_step_groups(tails, epis)
        assert step(b) == scripted and step(b) == scripted          # it survives a second step
        b.set_step_groups(None, None)
        assert step(b) == unscripted
        b.set_step_groups(tails, None)                               # one kind alone
        assert step(b) == scripted
        for bad, text in ((dict(tail_groups=tails[:-1], epilogue_groups=epis[:-1]), "10 entries for a batch of 11 chains"),
                          (dict(tail_groups=[-2] + tails[1:]), "below -1"),
                          (dict(tail_groups=[6] + tails[1:]), "at or above the cap"),
                          (dict(epilogue_groups=[8] + epis[1:]), "at or above the cap"),
                          (dict(tail_groups=[g + 1 if g >= 1 else g for g in tails]), "hole"),
                          (dict(tail_groups=[-1] * NC, epilogue_groups=[1] + [-1] * (NC - 1)), "hole")):
            with pytest.raises(ValueError, match=text):
                b.set_step_groups(**bad)
            assert step(b) == scripted, (bad, seen)                  # nothing changed: the previous script is in force
        b.set_step_groups([-1] * NC, None)                           # all -1 is a script: one remainder
        assert step(b) == unscripted
        b.set_step_groups(tails, epis)
        fill(b, inputs, m, "plain")                                  # configure drops it with the rest of the batch's state
        assert step(b) == unscripted
        print("tail_groups per step:", seen)


@pytest.mark.parametrize("how", ["ulp2", "level", "in_order"])
def test_a_step_that_does_not_pipeline_ignores_the_script(product, monkeypatch, inputs, how):
    """The 2-ulp mode, the level model and CONSENRICH_AMD_TAIL_SPLIT=0: no groups, and the same bits as without a script."""
    from consenrich_amd.batch import ModelParams

    kw = {"ulp2": dict(x_tol_ulps=2), "level": dict(model=ModelParams(state_dim=1)), "in_order": {}}[how]
    env = {"CONSENRICH_AMD_TAIL_SPLIT": "0"} if how == "in_order" else {}
    plain = run(monkeypatch, inputs, env, 4, 128, "plain", **kw)
    scripted = run(monkeypatch, inputs, env, 4, 128, "plain", script=SCRIPTS["scattered"], **kw)
    assert plain["stats"]["tail_groups"] == 0 and scripted["stats"]["tail_groups"] == 0, (plain["stats"], scripted["stats"])
    assert_same(scripted, plain, (how, "with a script against without"))


@pytest.mark.parametrize("block", [64, 128, 256])
def test_a_masked_forward_pass_after_a_scripted_step_leaves_the_other_chains_as_they_were(product, monkeypatch, inputs, block):
    """As test_gpu_tail_epilogue's masked pass, after a step whose groups were scattered: the blocked xf is not resident, a masked
    forward pass on chain 9 (in the remainder, between chains of three different groups) rewrites its own blocks only."""
    from consenrich_amd import _lib as L
    from consenrich_amd.batch import DeviceBatch

    set_env(monkeypatch, {}, block)
    what = L.EXPORT_FORWARD | L.EXPORT_SMOOTH | L.EXPORT_RESID
    mask = [c == 9 for c in range(NC)]
    with DeviceBatch(0) as b:
        fill(b, inputs, 4, "plain")
        b.set_step_groups(*SCRIPTS["scattered"])
        b.step(L.RETURN_NLL, what)
        if pipelines():
            assert b.run_stats()["tail_groups"] == 4, b.run_stats()
        before = {(c, a): b.download(c, a) for c in range(NC) for a in ("D", "xf", "Pf", "xs", "Ps", "lag")}
        b.forward_masked(L.RETURN_NLL, mask)
        for c in (8, 10, 0):
            for a in ("xf", "D"):
                assert np.array_equal(bits(before[(c, a)]), bits(b.download(c, a))), (block, c, a)
        b.backward()
        b.export(L.EXPORT_FORWARD | L.EXPORT_SMOOTH)
        for c in range(NC):
            for a in ("xf", "Pf", "xs", "Ps", "lag"):
                assert np.array_equal(bits(before[(c, a)]), bits(b.download(c, a))), (block, "after the smoother", c, a)
