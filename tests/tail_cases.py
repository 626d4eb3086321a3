"""Shapes, inputs and the two-step run shared by the GPU tests of the pipelined step (tests/test_gpu_tail_epilogue.py,
tests/test_gpu_step_schedules.py).  A plain module: no fixtures, no tests.

Small shapes on purpose: chains shorter than, equal to and just past one block of every block length, a chain of one bin, chains of
several superblocks (CONSENRICH_AMD_SB_BINS=4096); m = 4 takes the 16-byte residual kernel, m = 5 the plain one.  33 k bins in all."""
import os

import numpy as np

import cases

N_LIST = [1, 63, 64, 65, 127, 128, 129, 257, 4097, 8193, 20000]
NAMES = ("D", "xf", "Pf", "pnoise", "xs", "Ps", "lag", "resid")
OWN = ("CONSENRICH_AMD_TAIL_SPLIT", "CONSENRICH_AMD_TAIL_PCT", "CONSENRICH_AMD_SB_SPIN_LIMIT", "CONSENRICH_AMD_EPILOGUE_PCT")
WARM = "-1,-1,384"      # the smoother's window at which both steps of a fresh batch validate (test_gpu_tail_epilogue's docstring)


def pipelines():
    """False when the suite runs under a mode switch (scripts/suite_variants.sh) that keeps a bit-exact step from pipelining at all:
    the comparisons still hold, the counts of groups and bail-outs do not apply."""
    e = os.environ.get
    return (e("CONSENRICH_AMD_SB_ASYNC", "1") != "0" and e("CONSENRICH_AMD_SEQ_STATE", "0") == "0" and e("CONSENRICH_AMD_DEFER", "1") != "0"
            and e("CONSENRICH_AMD_XTOL_ULPS", "0") == "0")


def make_inputs():
    """The chains' data (computed once, never changed): per m, per chain (data, munc); multipliers per chain."""
    sets = {m: [cases.synth(n, m, 9100 + 10 * m + c, mask_frac=0.01, outlier_frac=0.01) for c, n in enumerate(N_LIST)] for m in (4, 5)}
    mult = [cases.multipliers(n, 9300 + c) for c, n in enumerate(N_LIST)]
    return sets, mult


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def flags_of(variant):
    from consenrich_amd import _lib as L

    flags = L.RETURN_NLL
    if variant == "multipliers":
        flags |= L.USE_LAMBDA | L.USE_KAPPA | L.USE_QSCALE
    if variant == "nll_in_d":
        flags |= L.NLL_IN_D
    return flags


def set_env(monkeypatch, env, block, warm=WARM):
    """The switches of a run: the module's own unset, the block length, 4096-bin superblocks, the smoother's window (None: the
    library's default), then `env`."""
    for k in OWN:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("CONSENRICH_AMD_BLOCK", str(block))
    monkeypatch.setenv("CONSENRICH_AMD_SB_BINS", "4096")
    if warm is None:
        monkeypatch.delenv("CONSENRICH_AMD_WARM", raising=False)
    else:
        monkeypatch.setenv("CONSENRICH_AMD_WARM", warm)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def fill(b, inputs, m, variant, model=None):
    """Configure `b` for the chains of N_LIST with m samples and upload what `variant` needs."""
    from consenrich_amd.batch import ModelParams

    sets, mult = inputs
    b.configure(model if model is not None else ModelParams(state_dim=2), m, N_LIST)
    for c, (d_, v_) in enumerate(sets[m]):
        b.upload(c, d_, v_)
        if variant == "multipliers":
            lam, kap, qs = mult[c]
            b.upload_multipliers(c, lam, np.clip(kap, 0.25, 4.0), qs)
    if variant == "per_chain_q":
        b.set_chain_q([np.diag([1e-3 * (1 + c), 1e-4 * (1 + 0.5 * c)]).astype(np.float32) for c in range(len(N_LIST))])


def step_outputs(b, flags, what, out, step):
    """One step of `b`: both sums and every array of every chain go to `out` under (.., step)."""
    sd, sn = b.step(flags, what)
    out[("sumD", step)], out[("sumNLL", step)] = np.array(sd), np.array(sn)
    for c in range(len(N_LIST)):
        for name in NAMES:
            out[(c, name, step)] = b.download(c, name)


def run(monkeypatch, inputs, env, m, block, variant, profile=False, script=None, warm=WARM, model=None, **batch_kw):
    """Two steps of a fresh batch: every array of every chain after the first and after the second, both sums, the run counters.
    script = (tail groups, epilogue groups) for DeviceBatch.set_step_groups, set once in front of the first step; model and
    batch_kw: another model than levelTrend, arguments of DeviceBatch."""
    from consenrich_amd import _lib as L
    from consenrich_amd.batch import DeviceBatch

    set_env(monkeypatch, env, block, warm)
    what = L.EXPORT_FORWARD | L.EXPORT_SMOOTH | L.EXPORT_RESID
    flags = flags_of(variant)
    out = {}
    with DeviceBatch(0, **batch_kw) as b:
        fill(b, inputs, m, variant, model)
        if script is not None:
            b.set_step_groups(*script)
        if profile:
            b.profile(True)
        for step in range(2):
            step_outputs(b, flags, what, out, step)
        if profile:
            out["launches"] = {k: v[0] for k, v in b.kernel_times().items()}
            b.profile(False)
        out["stats"] = b.run_stats()
    return out


def assert_same(got, ref, msg):
    for key, val in ref.items():
        if key in ("stats", "launches"):
            continue
        assert np.array_equal(bits(val), bits(got[key])), (msg, key)
