"""Call sequences against one batch context and the launches each of them costs.

Shared by `make_golden.py --launches` (writes conversion_launches.json from a library built from the commit BEFORE a change of
the host layer's bookkeeping) and tests/test_gpu_residency.py (asserts that the library under test launches the same).  The
record is data only: per mode and sequence, the launch count of every profile scope of the pipeline -- the conversions between
the two layouts and, since the passes became descriptors, the chains, their fix-up and check launches, the state chain, the
E-steps and the statistics -- and the number of pipeline replays (0: a replay repeats launches)."""
from __future__ import annotations

import json
import os

import numpy as np

import cases

RECORD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "conversion_launches.json")
SCOPES = ("export_natural", "state_reblock_out", "state_records_natural", "residuals", "fwd_dstat", "chain_sums", "import_f32",
          "gain_summary", "phase_tracks",
          "stats", "fwd_chain", "fwd_fix", "fwd_cov_chain", "fwd_cov_fix", "fwd_state_chain", "fwd_state_fix", "fwd_state_seq",
          "fwd_apn_sequential", "bwd_chain", "bwd_fix", "chain_check", "estep_lambda", "estep_kappa", "ecm_commit_kappa",
          "transition_sums")
MODES = [(xtol, natin) for xtol in (0, 2) for natin in ("1", "0")]
N_LIST, M, SEED = [20000, 7000, 3001], 8, 9100
MASK = [True, False, True]
EVERY = ("D", "xf", "Pf", "pnoise", "xs", "Ps", "lag", "resid")
F = np.asarray(cases.F_TREND, np.float32)
Q0 = np.diag([1e-3, 1e-4]).astype(np.float32)


def mode_key(xtol, natin) -> str:
    return f"xtol{xtol}-natin{natin}"


def _sets():
    return [cases.synth(n, M, SEED + c, outlier_frac=0.01) for c, n in enumerate(N_LIST)]


def _kappa(b):
    for c, n in enumerate(N_LIST):
        b.upload_multipliers(c, None, cases.multipliers(n, SEED + 50 + c)[1], None)


def _step_export_twice(b, L):
    what = L.EXPORT_FORWARD | L.EXPORT_SMOOTH | L.EXPORT_RESID
    b.step(L.RETURN_NLL, what)
    b.export(what)
    b.export(what)
    for c in range(len(N_LIST)):
        for a in EVERY:
            b.download(c, a)


def _separate_calls(b, L):
    b.stats()
    b.forward(L.RETURN_NLL)
    b.backward()
    b.export(L.EXPORT_FORWARD)
    b.export(L.EXPORT_RESID)
    b.export(L.EXPORT_SMOOTH)
    b.export(L.EXPORT_SMOOTH)


def _forward_export_twice(b, L):
    b.stats()
    b.forward(L.RETURN_NLL)
    b.export(L.EXPORT_FORWARD)
    b.export(L.EXPORT_FORWARD)


def _step_forward_masked(b, L):
    b.step(L.RETURN_NLL, L.EXPORT_FORWARD | L.EXPORT_SMOOTH | L.EXPORT_RESID)
    b.forward_masked(L.RETURN_NLL, MASK)
    b.export(L.EXPORT_FORWARD)


def _step_ecm_masked(b, L):
    b.step(L.RETURN_NLL, L.EXPORT_FORWARD | L.EXPORT_SMOOTH | L.EXPORT_RESID)
    b.ecm(max_iters=1, inner_iters=2, rtol=0.0, use_kappa=True, chain_mask=MASK)
    b.export(L.EXPORT_SMOOTH | L.EXPORT_MULT)
    b.export(L.EXPORT_MULT)
    b.upload_multipliers(0, kappa=np.full(N_LIST[0], 1.5, np.float32))
    b.export(L.EXPORT_MULT)


def _step_ecm_lambda_kappa(b, L):
    # (lambda re-weighting keeps the E-steps out of the smoother chain: kernels of their own after a settle point per sweep)
    b.step(L.RETURN_NLL, L.EXPORT_FORWARD | L.EXPORT_SMOOTH | L.EXPORT_RESID)
    b.ecm(max_iters=2, inner_iters=2, rtol=0.0, use_kappa=True, use_lambda=True)


def _forward_backward_kappa(b, L):
    _kappa(b)
    b.stats()
    b.forward_backward(L.RETURN_NLL | L.USE_KAPPA)
    b.export(L.EXPORT_FORWARD)


def _chain_q_step(b, L):
    b.set_chain_q([np.diag([1e-3 * (c + 1), 1e-4]) for c in range(len(N_LIST))])
    b.step(L.RETURN_NLL, L.EXPORT_FORWARD | L.EXPORT_SMOOTH | L.EXPORT_RESID)


def _summaries_chain_by_chain(b, L):
    b.stats()
    b.forward(L.RETURN_NLL)
    b.backward()
    for _ in range(2):
        for c in range(len(N_LIST)):
            b.gain_summary(c, 1.0e-4)
            b.phase_tracks(c, 1.0e-4)


def _summaries_after_step(b, L):
    b.step(L.RETURN_NLL, L.EXPORT_FORWARD | L.EXPORT_SMOOTH | L.EXPORT_RESID)
    for _ in range(2):
        for c in range(len(N_LIST)):
            b.gain_summary(c, 1.0e-4)
            b.phase_tracks(c, 1.0e-4)


SEQUENCES = {
    "step_export_twice_download": (2, _step_export_twice),
    "separate_calls": (2, _separate_calls),
    "forward_export_twice": (2, _forward_export_twice),
    "step_forward_masked": (2, _step_forward_masked),
    "step_ecm_masked_multipliers": (2, _step_ecm_masked),
    "step_ecm_lambda_kappa": (2, _step_ecm_lambda_kappa),
    "forward_backward_kappa": (2, _forward_backward_kappa),
    "chain_q_step": (2, _chain_q_step),
    "summaries_chain_by_chain": (2, _summaries_chain_by_chain),
    "summaries_after_step": (2, _summaries_after_step),
    "level_model_step_export_twice": (1, _step_export_twice),
}


def _counts(times) -> dict:
    return {s: int(times.get(s, (0, 0.0))[0]) for s in SCOPES}


def run_mode(xtol: int) -> dict:
    """Every sequence on a batch context of its own in the validation mode `xtol`.  The caller has set CONSENRICH_AMD_NATIN and
    CONSENRICH_AMD_TAIL_SPLIT=0 (the number of tail groups of a pipelined step, hence its launch counts, depends on timing):
    a context reads them when it is created."""
    from consenrich_amd import _lib as L
    from consenrich_amd.batch import DeviceBatch, ModelParams

    sets = _sets()
    out = {}
    for name, (dim, seq) in SEQUENCES.items():
        with DeviceBatch(0, x_tol_ulps=xtol) as b:
            # (once unrecorded: a fresh context lengthens its speculation windows on first contact with the data, by replays;
            # configuring again keeps the windows and starts from a batch with nothing resident)
            for attempt in range(2):
                b.configure(ModelParams(state_dim=dim), M, N_LIST)
                for c, (d_, v_) in enumerate(sets):
                    b.upload(c, d_, v_)
                if attempt == 0:
                    seq(b, L)
                    b.synchronize()
            redos = b.run_stats()["pipeline_redos"]
            b.profile(True)
            seq(b, L)
            rec = _counts(b.kernel_times())
            b.profile(False)
            rec["pipeline_redos"] = int(b.run_stats()["pipeline_redos"] - redos)
            out[name] = rec
    out["cbackward_after_cforward"] = _per_call_backward(xtol)
    return out


def _per_call_backward(xtol: int) -> dict:
    """The per-call cbackwardPass entry on forward results the caller passes, after a per-call forward pass of the same shape left
    ITS results resident in the default context."""
    import ctypes as C

    from consenrich_amd import _lib as L
    from consenrich_amd import cconsenrich as product

    n = N_LIST[1]
    d_, v_ = cases.synth(n, M, SEED + 20)
    product.set_validation(xtol)
    try:
        xf, Pf, pn = np.zeros((n, 2), np.float32), np.zeros((n, 2, 2), np.float32), np.zeros((n, 2, 2), np.float32)
        product.cforwardPass(matrixData=d_, matrixPluginMuncInit=v_, matrixF=F, matrixQ0=Q0, intervalToBlockMap=np.zeros(n, np.int32),
                             blockCount=1, stateInit=0.0, stateCovarInit=1000.0, stateForward=xf, stateCovarForward=Pf,
                             pNoiseForward=pn, vectorD=np.zeros(n, np.float32), returnNLL=True)
        lib = L.lib()
        L.check(lib.csr_profile_enable(None, 1))
        product.cbackwardPass(matrixData=d_, matrixF=F, stateForward=xf, stateCovarForward=Pf, pNoiseForward=pn)
        buf, cnt = (L.KernelTime * 64)(), C.c_int32()
        L.check(lib.csr_profile_read(None, buf, 64, C.byref(cnt)))
        L.check(lib.csr_profile_enable(None, 0))
        times = {buf[i].name.decode(): (int(buf[i].launches), 0.0) for i in range(min(cnt.value, 64))}
    finally:
        product.set_validation(0)
    return _counts(times)       # (the default context's run statistics are not exposed: no replay count)


def load() -> dict:
    with open(RECORD) as fh:
        return json.load(fh)
